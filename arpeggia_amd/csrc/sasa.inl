// Shrake-Rupley atom SASA on the cell list (reference src/sasa.rs:174-247, rust-sasa's calculate_sasa_internal) and the SAP weight
// kernel that turns it into neighbour-sum weights (src/sap.rs:198-209).  Included by kernels.hip inside namespace arp.
//
// Contract (include/arpeggia_amd.h arp_atom_sasa, DESIGN.md "Atom SASA"): point k of atom i is buried iff some other grid atom j has
// d^2 < R_j^2, d^2 = tx^2 + ty^2 + tz^2 (left to right, f64, no FMA) with t = (c_i - c_j) + s_k R_i per axis, from the f32 values
// c (coordinates), s_k (sphere point) and R (radius + probe).  The grid is built over the f64 images of the f32 coordinates, so the
// exact-phase records (Fat::x, y, z) ARE the contract's c.  count_i = the unburied points; sasa_i = f32(4 pi R_i^2 count_i / n_points).
//
// Mapping: one wave per home slot (a grid atom).  Gather: the nine x-contiguous slot windows of the home cell's shell, 64 slots per step;
// a slot survives when its f32 distance can be below R_i + R_j (a burier of any point has |c_i - c_j| < R_i |s_k| + R_j), first against
// R_i + R_max on the prefilter record alone, then against its own R_j; survivors are compacted into the wave's LDS list (ballot + mbcnt)
// as {c_i - c_j in f32, R_j} + the slot.  Test: lanes are sphere points (passes of 64); every lane walks the same list entry at a time --
// a broadcast LDS read -- and drops out at its first burier; the walk ends when no lane of the pass is open.  The f32 test decides
// everything outside a band of +-mg around R_j^2 (mg bounds what the f32 records and arithmetic can be off by, DESIGN.md "Atom SASA:
// margin"); the few tests inside the band gather the f64 records and decide exactly, behind a wave-uniform branch.  A list that fills
// the LDS budget is tested and emptied before the gather goes on (the buried state of every point is a bit in `buried`), so no
// neighbour is ever dropped, whatever the density.  Counts are integers: the result does not depend on slot or list order.
constexpr uint32_t kSasaWaves = 4, kSasaList = 256;
constexpr double k4Pi = 4.0 * 3.141592653589793;  // (4 x the double nearest pi: exact)
constexpr uint32_t kSasaMaxPoints = 4096;  // 64 passes of 64 points: one bit per pass in `buried` (the ABI rejects more)
struct SasaWaveLds { float4 d[kSasaList]; uint32_t slot[kSasaList]; };

__global__ __launch_bounds__(kSasaWaves * 64) void k_sasa(const GridParams *gp, const uint32_t *cell_start, Sorted so, const float *R,
                                                          const float *sphere, uint32_t n_points, float r_max, float *out_sasa,
                                                          int32_t *out_count, unsigned long long *tests) {
    __shared__ SasaWaveLds wl[kSasaWaves];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    SasaWaveLds &L = wl[wave];
    const uint32_t home = blockIdx.x * kSasaWaves + wave;
    if (home >= gp->n_heavy) return;  // (wave-uniform; no block barrier below)
    const uint32_t nx = gp->nx, ny = gp->ny, nzt = gp->nzt, kx = gp->kx, sy = gp->sy_shift;
    const float4 h = so.rec[home];
    const Fat &hf = so.fat[home];
    const double cix = hf.x, ciy = hf.y, ciz = hf.z;
    const uint32_t orig_i = hf.orig, c = hf.cell, row = c / nx, cx = c - row * nx;
    uint32_t cy, cz;
    grid_row_decode(row, ny, nzt, sy, cy, cz);
    const float Ri = R[orig_i];
    // gather bounds: the grid's storage margin (grid.inl grid_setup, DESIGN.md "Prefilter margin") + 1e-5 relative for the arithmetic
    // and for |s_k| = 1 +- 2^-23 (the search radius of the grid build is 2 R_max (1 + 1e-5) >= R_i + R_j)
    const float pm = gp->prefilter_margin;
    const float thr_any = (Ri + r_max) * (Ri + r_max) * 1.00001f + pm;
    // test band: |d2_f32 - d2_f64| <= 2^-24 (7 C T + 10 T^2) with T = 2 R_i + R_max >= |t| and C >= |record coordinate|
    const double edge = gp->inv_edge > 0.0 ? 1.0 / gp->inv_edge : 0.0;
    const float C = (float)((double)(max(max((nx + kx - 1u) / kx, ny), gp->nz) + 1u) * edge);
    const float T = (2.0f * Ri + r_max) * 1.001f;
    const float mg = 0x1p-19f * (C * T + T * T) + 1e-30f;
    const uint32_t passes = (n_points + 63u) / 64u;
    unsigned long long buried = 0ull, n_tests = 0ull;

    auto test_list = [&](uint32_t cnt) {
        wave_lds_fence();  // the list entries written by the gather are visible
#pragma unroll 1
        for (uint32_t p = 0; p < passes; p++) {
            const uint32_t k = p * 64u + lane;
            bool open = k < n_points && !((buried >> p) & 1ull);
            if (!__any(open)) continue;
            const uint32_t kk = min(k, n_points - 1u);
            const float sx = sphere[3u * kk], sy_ = sphere[3u * kk + 1u], sz = sphere[3u * kk + 2u];
            const float px = sx * Ri, py = sy_ * Ri, pz = sz * Ri;
#pragma unroll 1
            for (uint32_t e = 0; e < cnt; e++) {
                const unsigned long long live = __ballot(open);
                if (live == 0ull) break;
                n_tests += (unsigned long long)__popcll(live);
                const float4 d = L.d[e];  // (the same address in every lane: a broadcast)
                const float tx = d.x + px, ty = d.y + py, tz = d.z + pz;
                const float d2 = __fmaf_rn(tx, tx, __fmaf_rn(ty, ty, tz * tz));
                const float r2 = d.w * d.w;
                bool in = open & (d2 < r2 - mg);
                const bool band = open & !in & (d2 <= r2 + mg);
                if (__any(band)) {  // rare: the f32 value cannot decide -- the contract's own test in f64
                    if (band) {
                        const Fat &fj = so.fat[L.slot[e]];
                        const double ri = (double)Ri;
                        const double ux = __dadd_rn(__dsub_rn(cix, fj.x), __dmul_rn((double)sx, ri));
                        const double uy = __dadd_rn(__dsub_rn(ciy, fj.y), __dmul_rn((double)sy_, ri));
                        const double uz = __dadd_rn(__dsub_rn(ciz, fj.z), __dmul_rn((double)sz, ri));
                        const double s2 = __dadd_rn(__dadd_rn(__dmul_rn(ux, ux), __dmul_rn(uy, uy)), __dmul_rn(uz, uz));
                        in = s2 < __dmul_rn((double)d.w, (double)d.w);  // (R_j^2 is exact in f64)
                    }
                }
                if (in) { buried |= 1ull << p; open = false; }
            }
        }
        wave_lds_fence();  // every lane is done reading before the gather overwrites the list
    };

    uint32_t cnt = 0;
    const uint32_t xlo = cx > kx ? cx - kx : 0u, xhi = min(cx + kx, nx - 1u);
#pragma unroll 1
    for (uint32_t q = 0; q < 9u; q++) {
        const int zz = (int)cz + (int)(q / 3u) - 1, yy = (int)cy + (int)(q % 3u) - 1;
        if (zz < 0 || zz >= (int)nzt || yy < 0 || yy >= (int)ny) continue;
        const uint32_t r = grid_row((uint32_t)yy, (uint32_t)zz, ny, nzt, sy) * nx;
        const uint32_t lo = cell_start[r + xlo], hi = cell_start[r + xhi + 1u];
#pragma unroll 1
        for (uint32_t s0 = lo; s0 < hi; s0 += 64u) {
            const uint32_t slot = s0 + lane;
            bool keep = slot < hi && slot != home;  // (self excluded by index)
            float dx = 0.f, dy = 0.f, dz = 0.f, Rj = 0.f;
            if (keep) {
                const float4 rj = so.rec[slot];
                dx = h.x - rj.x; dy = h.y - rj.y; dz = h.z - rj.z;
                const float d2 = __fmaf_rn(dx, dx, __fmaf_rn(dy, dy, dz * dz));
                keep = d2 <= thr_any;
                if (keep) {
                    Rj = R[so.fat[slot].orig];
                    keep = d2 <= (Ri + Rj) * (Ri + Rj) * 1.00001f + pm;
                }
            }
            const unsigned long long mask = __ballot(keep);
            const uint32_t pop = (uint32_t)__popcll(mask);
            if (cnt + pop > kSasaList) { test_list(cnt); cnt = 0; }
            if (keep) {
                const uint32_t at = cnt + mbcnt(mask);
                L.d[at] = make_float4(dx, dy, dz, Rj);
                L.slot[at] = slot;
            }
            cnt += pop;
        }
    }
    if (cnt) test_list(cnt);
    uint32_t open_count = 0;
    for (uint32_t p = 0; p < passes; p++) open_count += (uint32_t)__popcll(__ballot(p * 64u + lane < n_points && !((buried >> p) & 1ull)));
    if (lane == 0u) {
        out_count[orig_i] = (int32_t)open_count;
        // 4 pi R^2 count / n in f64, left to right, one rounding to f32 at the end
        const double ri = (double)Ri;
        out_sasa[orig_i] = (float)(__ddiv_rn(__dmul_rn(__dmul_rn(__dmul_rn(k4Pi, ri), ri), (double)open_count), (double)n_points));
        atomicAdd(tests, n_tests);
    }
}

// SAP weight of every atom of the neighbour set (src/sap.rs:198-209): hydrophobicity(resn) x clamp(sasa / max side-chain SASA(resn), 0, 1)
// of the atom-SASA row the atom's serial number maps to (src[j], -1: none -> 0), for the residue code of its name (ARP_SAP_RESIDUES order,
// >= 20: no hydrophobicity -> 0).  The operations of arp_sap_weight, in the same order: the two agree bit for bit.
#define ARP_SAP_H(n, h, a) h,
#define ARP_SAP_A(n, h, a) a,
__constant__ float kSapHydro[20] = {ARP_SAP_RESIDUES(ARP_SAP_H)};
__constant__ float kSapMaxAsa[20] = {ARP_SAP_RESIDUES(ARP_SAP_A)};
#undef ARP_SAP_H
#undef ARP_SAP_A
__global__ __launch_bounds__(256) void k_sap_weight(uint32_t n, const uint32_t *code, const int32_t *src, const float *sasa, float *w) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t r = code[j];
    const int32_t s = src[j];
    float out = 0.0f;
    if (r < 20u && s >= 0) {
        float q = sasa[s] / kSapMaxAsa[r];
        q = (0.0f < q) ? q : 0.0f;  // std::max(0.0f, q)
        q = (q < 1.0f) ? q : 1.0f;  // std::min(1.0f, q)
        out = kSapHydro[r] * q;
    }
    w[j] = out;
}

void launch_sasa(const DevAtoms &in, const Workspace &ws, double cutoff, const float *R, const float *sphere, uint32_t n_points, float r_max,
                 float *sasa, int32_t *count, hipStream_t st, Profiler *prof) {
    launch_grid(in, ws, st, prof, cutoff, /* ordered: not needed, the counts do not depend on slot order */ false);
    if (prof) prof->begin("sasa", st);
    if (in.n)
        hipLaunchKernelGGL(k_sasa, dim3((in.n + kSasaWaves - 1u) / kSasaWaves), dim3(kSasaWaves * 64), 0, st, (const GridParams *)ws.grid,
                           (const uint32_t *)ws.cell_start, ws.sorted, R, sphere, n_points, r_max, sasa, count, ws.result + kSasaTestsWord);
    if (prof) prof->end(st);
}

void launch_sap_weight(uint32_t n, const uint32_t *code, const int32_t *src, const float *sasa, float *w, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_sap_weight, dim3((n + 255u) / 256u), dim3(256), 0, st, n, code, src, sasa, w);
}
