// Shrake-Rupley atom SASA on the cell list (reference src/sasa.rs:174-247, rust-sasa's calculate_sasa_internal), its split variant that
// answers for a complex and for the atom's own group(s) in one walk (arp_atom_sasa_groups), and the SAP weight
// kernel that turns atom SASA into neighbour-sum weights (src/sap.rs:198-209).  Included by kernels.hip inside namespace arp.
//
// Contract (include/arpeggia_amd.h arp_atom_sasa, DESIGN.md "Atom SASA"): point k of atom i is buried iff some other grid atom j has
// d^2 < R_j^2, d^2 = tx^2 + ty^2 + tz^2 (left to right, f64, no FMA) with t = (c_i - c_j) + s_k R_i per axis, from the f32 values
// c (coordinates), s_k (sphere point) and R (radius + probe).  The grid is built over the f64 images of the f32 coordinates, so the
// exact-phase records (Fat::x, y, z) ARE the contract's c.  count_i = the unburied points; sasa_i = f32(4 pi R_i^2 count_i / n_points).
//
// The one variation (SPLIT, k_sasa_split): every grid atom carries a group mask g in {1, 2, 3} (bit 0: in group 1, bit 1: in group 2; the
// grid build keeps it in the pair word of the exact-phase record, Fat::pw bits 24 / 25 -- the host sets ARP_ATTR_LIGAND / ARP_ATTR_RECEPTOR;
// mask 0 = ARP_ATTR_H: not in the grid).  With the same burial test (strict, self excluded by index, same model only) atom i gets three
// open-point counts: count_c (occluders: every other grid atom), count_1 (occluders: the other grid atoms with bit 0; 0 unless g_i has bit 0)
// and count_2 (bit 1 likewise); three areas f32(4 pi R_i^2 count / n_points); and buried = [g_i & 1] count_1 + [g_i & 2] count_2 - count_c >= 0.
// count_c is the plain kernel's count on the union, count_g the plain kernel's count on group g alone.
//
// Mapping: one wave per home slot (a grid atom).  Gather: the nine x-contiguous slot windows of the home cell's shell, 64 slots per step;
// a slot survives when its f32 distance can be below R_i + R_j (a burier of any point has |c_i - c_j| < R_i |s_k| + R_j), first against
// R_i + R_max on the prefilter record alone, then against its own R_j; survivors are compacted into the wave's LDS list (ballot + mbcnt)
// as {c_i - c_j in f32, R_j} + the slot.  Test: lanes are sphere points (passes of 64); every lane walks the same list entry at a time --
// a broadcast LDS read -- and drops out at its first burier; the walk ends when no lane of the pass is open.  The f32 test decides
// everything outside a band of +-mg around R_j^2 (mg bounds what the f32 records and arithmetic can be off by, DESIGN.md "Atom SASA:
// margin"); the few tests inside the band gather the f64 records and decide exactly, behind a wave-uniform branch.  A list that fills
// the LDS budget is tested and emptied before the gather goes on (the buried state of every point is a bit in `bc`), so no
// neighbour is ever dropped, whatever the density.  Counts are integers: the result does not depend on slot or list order.
//
// SPLIT changes three things.  A list entry carries its atom's mask in bits 30 / 31 of the slot word (slots stay below 2^27).  Every lane
// keeps three words (bc: complex, b1: group 1, b2: group 2; the word of a group the home is not in starts full, so it never keeps a lane
// open): an entry that buries a point sets the complex bit always and the bit of every group it is in, and a lane is open for a pass while
// a group word of it is still clear there -- a point buried by an atom of the home's own group is buried in the complex as well, so a lane
// that walks on until its own group(s) bury it has seen everything that decides the complex count, and burial in the complex alone must
// NOT close it.  Lane 0 writes three planes (stride `plane`) of counts and areas, and `buried`.
constexpr uint32_t kSasaWaves = 4, kSasaList = 256;
constexpr double k4Pi = 4.0 * 3.141592653589793;  // (4 x the double nearest pi: exact)
constexpr uint32_t kSasaMaxPoints = 4096;  // 64 passes of 64 points: one bit per pass in a buried word (the ABI rejects more)
constexpr uint32_t kSasaMaskShift = 30, kSasaSlotMask = (1u << kSasaMaskShift) - 1u;  // SPLIT: the slot word of a list entry
struct SasaWaveLds { float4 d[kSasaList]; uint32_t slot[kSasaList]; };

template <bool SPLIT>
__device__ __forceinline__ void sasa_walk(const GridParams *gp, const uint32_t *cell_start, const Sorted &so, const float *R, const float *sphere,
                                          uint32_t n_points, float r_max, uint32_t plane, float *out_sasa, int32_t *out_count, int32_t *out_buried,
                                          unsigned long long *tests) {
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
    uint32_t gi = 3u;
    if constexpr (SPLIT) gi = (hf.pw >> 24) & 3u;
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
    // bit p of a word: the point of this lane in pass p is buried -- in the complex, by group 1, by group 2 (b1, b2: SPLIT only)
    unsigned long long bc = 0ull, b1 = (gi & 1u) ? 0ull : ~0ull, b2 = (gi & 2u) ? 0ull : ~0ull, n_tests = 0ull;

    auto test_list = [&](uint32_t cnt) {
        wave_lds_fence();  // the list entries written by the gather are visible
#pragma unroll 1
        for (uint32_t p = 0; p < passes; p++) {
            const uint32_t k = p * 64u + lane;
            bool lc = (bc >> p) & 1ull, l1 = lc, l2 = lc;  // (plain: the one word closes the lane)
            if constexpr (SPLIT) { l1 = (b1 >> p) & 1ull; l2 = (b2 >> p) & 1ull; }
            bool open = k < n_points && !(l1 & l2);
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
                uint32_t sw = 0u;
                if constexpr (SPLIT) sw = L.slot[e];
                const float tx = d.x + px, ty = d.y + py, tz = d.z + pz;
                const float d2 = __fmaf_rn(tx, tx, __fmaf_rn(ty, ty, tz * tz));
                const float r2 = d.w * d.w;
                bool in = open & (d2 < r2 - mg);
                const bool band = open & !in & (d2 <= r2 + mg);
                if (__any(band)) {  // rare: the f32 value cannot decide -- the contract's own test in f64
                    if (band) {
                        const Fat &fj = so.fat[SPLIT ? sw & kSasaSlotMask : L.slot[e]];  // (plain reads the slot word only here)
                        const double ri = (double)Ri;
                        const double ux = __dadd_rn(__dsub_rn(cix, fj.x), __dmul_rn((double)sx, ri));
                        const double uy = __dadd_rn(__dsub_rn(ciy, fj.y), __dmul_rn((double)sy_, ri));
                        const double uz = __dadd_rn(__dsub_rn(ciz, fj.z), __dmul_rn((double)sz, ri));
                        const double s2 = __dadd_rn(__dadd_rn(__dmul_rn(ux, ux), __dmul_rn(uy, uy)), __dmul_rn(uz, uz));
                        in = s2 < __dmul_rn((double)d.w, (double)d.w);  // (R_j^2 is exact in f64)
                    }
                }
                if constexpr (SPLIT) {  // (the entry's mask is wave-uniform; a word of a group the home is not in is full already)
                    lc |= in; l1 |= in & (bool)((sw >> kSasaMaskShift) & 1u); l2 |= in & (bool)(sw >> (kSasaMaskShift + 1u));
                    open &= !(l1 & l2);
                } else if (in) { bc |= 1ull << p; open = false; }
            }
            if constexpr (SPLIT) { bc |= (unsigned long long)lc << p; b1 |= (unsigned long long)l1 << p; b2 |= (unsigned long long)l2 << p; }
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
            uint32_t gj = 0u;  // (plain: stays 0, the slot word is the bare slot and Fat::pw is not read)
            if (keep) {
                const float4 rj = so.rec[slot];
                dx = h.x - rj.x; dy = h.y - rj.y; dz = h.z - rj.z;
                const float d2 = __fmaf_rn(dx, dx, __fmaf_rn(dy, dy, dz * dz));
                keep = d2 <= thr_any;
                if (keep) {
                    const Fat &fj = so.fat[slot];
                    if constexpr (SPLIT) gj = (fj.pw >> 24) & 3u;
                    Rj = R[fj.orig];
                    keep = d2 <= (Ri + Rj) * (Ri + Rj) * 1.00001f + pm;
                }
            }
            const unsigned long long mask = __ballot(keep);
            const uint32_t pop = (uint32_t)__popcll(mask);
            if (cnt + pop > kSasaList) { test_list(cnt); cnt = 0; }
            if (keep) {
                const uint32_t at = cnt + mbcnt(mask);
                L.d[at] = make_float4(dx, dy, dz, Rj);
                L.slot[at] = slot | (gj << kSasaMaskShift);
            }
            cnt += pop;
        }
    }
    if (cnt) test_list(cnt);
    uint32_t open_c = 0, open_1 = 0, open_2 = 0;
    for (uint32_t p = 0; p < passes; p++) {
        const bool valid = p * 64u + lane < n_points;
        open_c += (uint32_t)__popcll(__ballot(valid && !((bc >> p) & 1ull)));
        if constexpr (SPLIT) {
            open_1 += (uint32_t)__popcll(__ballot(valid && !((b1 >> p) & 1ull)));  // (0 for a group the home is not in: its word is full)
            open_2 += (uint32_t)__popcll(__ballot(valid && !((b2 >> p) & 1ull)));
        }
    }
    if (lane == 0u) {
        // 4 pi R^2 count / n in f64, left to right, one rounding to f32 at the end (count 0 gives +0.0f)
        const double ri = (double)Ri, a = __dmul_rn(__dmul_rn(k4Pi, ri), ri), np = (double)n_points;
        out_count[orig_i] = (int32_t)open_c;
        if constexpr (SPLIT) { out_count[plane + orig_i] = (int32_t)open_1; out_count[2u * plane + orig_i] = (int32_t)open_2; }
        out_sasa[orig_i] = (float)__ddiv_rn(__dmul_rn(a, (double)open_c), np);
        if constexpr (SPLIT) {
            out_sasa[plane + orig_i] = (float)__ddiv_rn(__dmul_rn(a, (double)open_1), np);
            out_sasa[2u * plane + orig_i] = (float)__ddiv_rn(__dmul_rn(a, (double)open_2), np);
            out_buried[orig_i] = (int32_t)(open_1 + open_2) - (int32_t)open_c;
        }
        atomicAdd(tests, n_tests);
    }
}

// The two instantiations, each with the arguments it uses (and the kernel name the profiles know).
__global__ __launch_bounds__(kSasaWaves * 64) void k_sasa(const GridParams *gp, const uint32_t *cell_start, Sorted so, const float *R,
                                                          const float *sphere, uint32_t n_points, float r_max, float *out_sasa,
                                                          int32_t *out_count, unsigned long long *tests) {
    sasa_walk<false>(gp, cell_start, so, R, sphere, n_points, r_max, 0u, out_sasa, out_count, nullptr, tests);
}
__global__ __launch_bounds__(kSasaWaves * 64) void k_sasa_split(const GridParams *gp, const uint32_t *cell_start, Sorted so, const float *R,
                                                                const float *sphere, uint32_t n_points, float r_max, uint32_t plane,
                                                                float *out_sasa, int32_t *out_count, int32_t *out_buried, unsigned long long *tests) {
    sasa_walk<true>(gp, cell_start, so, R, sphere, n_points, r_max, plane, out_sasa, out_count, out_buried, tests);
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
                 float *sasa, int32_t *count, int32_t *buried, hipStream_t st, Profiler *prof) {
    launch_grid(in, ws, st, prof, cutoff, /* ordered: not needed, the counts do not depend on slot order */ false);
    const dim3 grid((in.n + kSasaWaves - 1u) / kSasaWaves), block(kSasaWaves * 64);
    if (prof) prof->begin(buried ? "sasa_split" : "sasa", st);
    if (in.n && buried)
        hipLaunchKernelGGL(k_sasa_split, grid, block, 0, st, (const GridParams *)ws.grid, (const uint32_t *)ws.cell_start, ws.sorted, R, sphere, n_points,
                           r_max, in.n, sasa, count, buried, ws.result + kSasaTestsWord);
    else if (in.n)
        hipLaunchKernelGGL(k_sasa, grid, block, 0, st, (const GridParams *)ws.grid, (const uint32_t *)ws.cell_start, ws.sorted, R, sphere, n_points, r_max,
                           sasa, count, ws.result + kSasaTestsWord);
    if (prof) prof->end(st);
}

void launch_sap_weight(uint32_t n, const uint32_t *code, const int32_t *src, const float *sasa, float *w, hipStream_t st) {
    if (n) hipLaunchKernelGGL(k_sap_weight, dim3((n + 255u) / 256u), dim3(256), 0, st, n, code, src, sasa, w);
}
