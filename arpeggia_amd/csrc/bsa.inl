// Buried surface per atom: one Shrake-Rupley walk that answers for the complex and for the atom's own group(s) at once (DESIGN.md section
// 3.10; include/arpeggia_amd.h arp_atom_sasa_groups).  Included by kernels.hip inside namespace arp, after sasa.inl and ens.inl.
//
// Contract: every grid atom carries a group mask g in {1, 2, 3} (bit 0: in group 1, bit 1: in group 2; the grid build keeps it in the pair word
// of the exact-phase record, Fat::pw bits 24 / 25 -- the host sets ARP_ATTR_LIGAND / ARP_ATTR_RECEPTOR; mask 0 = ARP_ATTR_H: not in the grid).
// With the burial test of k_sasa (the contract at the top of sasa.inl, unchanged: d^2 < R_j^2 in f64 from the f32 values, strict, self excluded
// by index, same model only) atom i gets three open-point counts: count_c (occluders: every other grid atom), count_1 (occluders: the other
// grid atoms with bit 0; 0 unless g_i has bit 0) and count_2 (bit 1 likewise); three areas f32(4 pi R_i^2 count / n_points); and
// buried = [g_i & 1] count_1 + [g_i & 2] count_2 - count_c >= 0.  Counts are integers and depend on neither list order nor grid: count_c is
// k_sasa's count on the union, count_g is k_sasa's count on group g alone.
//
// Structure: k_sasa's -- one wave per home slot, the nine x-contiguous windows with the two-stage f32 gather, the 256-entry LDS list with flush,
// lanes = sphere points in passes of 64, the broadcast list walk, the f32 band with the f64 decision behind a wave-uniform branch.  What differs:
// a list entry carries its atom's mask (bits 30 / 31 of the slot word: slots stay below 2^27); every lane keeps three `buried` words (complex,
// group 1, group 2; the word of a group the home is not in starts full, so it never keeps a lane open); an entry that buries a point sets the
// complex bit always and the bit of every group it is in; a lane is open for a pass while a group word of it is still clear there -- a point
// buried by an atom of the home's own group is buried in the complex as well, so a lane that walks on until its own group(s) bury it has seen
// everything that decides the complex count, and burial in the complex alone must NOT close it.
constexpr uint32_t kBsaMaskShift = 30, kBsaSlotMask = (1u << kBsaMaskShift) - 1u;

__global__ __launch_bounds__(kSasaWaves * 64) void k_sasa_split(const GridParams *gp, const uint32_t *cell_start, Sorted so, const float *R,
                                                                const float *sphere, uint32_t n_points, float r_max, uint32_t plane,
                                                                float *out_sasa, int32_t *out_count, int32_t *out_buried, unsigned long long *tests) {
    __shared__ SasaWaveLds wl[kSasaWaves];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    SasaWaveLds &L = wl[wave];
    const uint32_t home = blockIdx.x * kSasaWaves + wave;
    if (home >= gp->n_heavy) return;  // (wave-uniform; no block barrier below)
    const uint32_t nx = gp->nx, ny = gp->ny, nzt = gp->nzt, kx = gp->kx, sy = gp->sy_shift;
    const float4 h = so.rec[home];
    const Fat &hf = so.fat[home];
    const double cix = hf.x, ciy = hf.y, ciz = hf.z;
    const uint32_t orig_i = hf.orig, gi = (hf.pw >> 24) & 3u, c = hf.cell, row = c / nx, cx = c - row * nx;
    uint32_t cy, cz;
    grid_row_decode(row, ny, nzt, sy, cy, cz);
    const float Ri = R[orig_i];
    // gather bounds and test band: k_sasa's (sasa.inl)
    const float pm = gp->prefilter_margin;
    const float thr_any = (Ri + r_max) * (Ri + r_max) * 1.00001f + pm;
    const double edge = gp->inv_edge > 0.0 ? 1.0 / gp->inv_edge : 0.0;
    const float C = (float)((double)(max(max((nx + kx - 1u) / kx, ny), gp->nz) + 1u) * edge);
    const float T = (2.0f * Ri + r_max) * 1.001f;
    const float mg = 0x1p-19f * (C * T + T * T) + 1e-30f;
    const uint32_t passes = (n_points + 63u) / 64u;
    // bit p of a word: the point of this lane in pass p is buried -- in the complex, by group 1, by group 2
    unsigned long long bc = 0ull, b1 = (gi & 1u) ? 0ull : ~0ull, b2 = (gi & 2u) ? 0ull : ~0ull, n_tests = 0ull;

    auto test_list = [&](uint32_t cnt) {
        wave_lds_fence();  // the list entries written by the gather are visible
#pragma unroll 1
        for (uint32_t p = 0; p < passes; p++) {
            const uint32_t k = p * 64u + lane;
            bool lc = (bc >> p) & 1ull, l1 = (b1 >> p) & 1ull, l2 = (b2 >> p) & 1ull;
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
                const uint32_t sw = L.slot[e];
                const float tx = d.x + px, ty = d.y + py, tz = d.z + pz;
                const float d2 = __fmaf_rn(tx, tx, __fmaf_rn(ty, ty, tz * tz));
                const float r2 = d.w * d.w;
                bool in = open & (d2 < r2 - mg);
                const bool band = open & !in & (d2 <= r2 + mg);
                if (__any(band)) {  // rare: the f32 value cannot decide -- the contract's own test in f64
                    if (band) {
                        const Fat &fj = so.fat[sw & kBsaSlotMask];
                        const double ri = (double)Ri;
                        const double ux = __dadd_rn(__dsub_rn(cix, fj.x), __dmul_rn((double)sx, ri));
                        const double uy = __dadd_rn(__dsub_rn(ciy, fj.y), __dmul_rn((double)sy_, ri));
                        const double uz = __dadd_rn(__dsub_rn(ciz, fj.z), __dmul_rn((double)sz, ri));
                        const double s2 = __dadd_rn(__dadd_rn(__dmul_rn(ux, ux), __dmul_rn(uy, uy)), __dmul_rn(uz, uz));
                        in = s2 < __dmul_rn((double)d.w, (double)d.w);  // (R_j^2 is exact in f64)
                    }
                }
                // (the entry's mask is wave-uniform; a word of a group the home is not in is full already)
                lc |= in; l1 |= in & (bool)((sw >> kBsaMaskShift) & 1u); l2 |= in & (bool)(sw >> (kBsaMaskShift + 1u));
                open &= !(l1 & l2);
            }
            bc |= (unsigned long long)lc << p; b1 |= (unsigned long long)l1 << p; b2 |= (unsigned long long)l2 << p;
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
            uint32_t gj = 0u;
            if (keep) {
                const float4 rj = so.rec[slot];
                dx = h.x - rj.x; dy = h.y - rj.y; dz = h.z - rj.z;
                const float d2 = __fmaf_rn(dx, dx, __fmaf_rn(dy, dy, dz * dz));
                keep = d2 <= thr_any;
                if (keep) {
                    const Fat &fj = so.fat[slot];
                    gj = (fj.pw >> 24) & 3u;
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
                L.slot[at] = slot | (gj << kBsaMaskShift);
            }
            cnt += pop;
        }
    }
    if (cnt) test_list(cnt);
    uint32_t open_c = 0, open_1 = 0, open_2 = 0;
    for (uint32_t p = 0; p < passes; p++) {
        const bool valid = p * 64u + lane < n_points;
        open_c += (uint32_t)__popcll(__ballot(valid && !((bc >> p) & 1ull)));
        open_1 += (uint32_t)__popcll(__ballot(valid && !((b1 >> p) & 1ull)));  // (0 for a group the home is not in: its word is full)
        open_2 += (uint32_t)__popcll(__ballot(valid && !((b2 >> p) & 1ull)));
    }
    if (lane == 0u) {
        // 4 pi R^2 count / n in f64, left to right, one rounding to f32 at the end (k_sasa's formula; count 0 gives +0.0f)
        const double ri = (double)Ri, a = __dmul_rn(__dmul_rn(k4Pi, ri), ri), np = (double)n_points;
        out_count[orig_i] = (int32_t)open_c; out_count[plane + orig_i] = (int32_t)open_1; out_count[2u * plane + orig_i] = (int32_t)open_2;
        out_sasa[orig_i] = (float)__ddiv_rn(__dmul_rn(a, (double)open_c), np);
        out_sasa[plane + orig_i] = (float)__ddiv_rn(__dmul_rn(a, (double)open_1), np);
        out_sasa[2u * plane + orig_i] = (float)__ddiv_rn(__dmul_rn(a, (double)open_2), np);
        out_buried[orig_i] = (int32_t)(open_1 + open_2) - (int32_t)open_c;
        atomicAdd(tests, n_tests);
    }
}

// ---- the ensemble form (arp_dsasa_ensemble): the pieces ens.inl does not have ------------------------------------------------------------
// attribute word of the packed atoms: item f * m + k gets the word of selected atom k (k_ens_tile writes everything else of the pack)
__global__ __launch_bounds__(256) void k_bsa_tile_attr(uint32_t frames, uint32_t m, const uint32_t *attr, uint32_t *out) {
    const unsigned long long total = (unsigned long long)frames * m;
    for (unsigned long long q = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (unsigned long long)gridDim.x * blockDim.x)
        out[q] = attr[(uint32_t)(q % m)];
}

// per selected atom the frames with buried > 0, over all frames so far; one thread owns one accumulator (k_ens_reduce's scheme)
__global__ __launch_bounds__(256) void k_bsa_frames_buried(uint32_t frames, uint32_t m, const int32_t *buried, uint32_t *acc, uint32_t first) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= m) return;
    uint32_t n = first ? 0u : acc[k];
    const int32_t *bp = buried + k;
#pragma unroll 4
    for (uint32_t f = 0; f < frames; f++) n += bp[(unsigned long long)f * m] > 0 ? 1u : 0u;
    acc[k] = n;
}

void launch_sasa_split(const DevAtoms &in, const Workspace &ws, double cutoff, const float *R, const float *sphere, uint32_t n_points, float r_max,
                       float *sasa3, int32_t *count3, int32_t *buried, hipStream_t st, Profiler *prof) {
    launch_grid(in, ws, st, prof, cutoff, /* ordered: not needed, the counts do not depend on slot order */ false);
    if (prof) prof->begin("sasa_split", st);
    if (in.n)
        hipLaunchKernelGGL(k_sasa_split, dim3((in.n + kSasaWaves - 1u) / kSasaWaves), dim3(kSasaWaves * 64), 0, st, (const GridParams *)ws.grid,
                           (const uint32_t *)ws.cell_start, ws.sorted, R, sphere, n_points, r_max, in.n, sasa3, count3, buried,
                           ws.result + kSasaTestsWord);
    if (prof) prof->end(st);
}

void launch_bsa_tile_attr(uint32_t frames, uint32_t m, const uint32_t *attr, uint32_t *out, hipStream_t st) {
    const unsigned long long items = (unsigned long long)frames * m;
    if (!items) return;
    hipLaunchKernelGGL(k_bsa_tile_attr, dim3((uint32_t)std::min<unsigned long long>((items + 255u) / 256u, 1u << 16)), dim3(256), 0, st, frames, m, attr, out);
}

void launch_bsa_ens_reduce(uint32_t frames, uint32_t m, const int32_t *buried, const float *sasa3, const EnsAcc &a, uint32_t *frames_buried, bool first,
                           float *const total[3], hipStream_t st) {
    if (!frames || !m) return;
    const unsigned long long plane = (unsigned long long)frames * m;
    hipLaunchKernelGGL(k_ens_reduce, dim3((m + 255u) / 256u), dim3(256), 0, st, frames, m, buried, (const float *)nullptr, a, first ? 1u : 0u);
    hipLaunchKernelGGL(k_bsa_frames_buried, dim3((m + 255u) / 256u), dim3(256), 0, st, frames, m, buried, frames_buried, first ? 1u : 0u);
    for (int g = 0; g < 3; g++)
        hipLaunchKernelGGL(k_ens_totals, dim3((frames + 3u) / 4u), dim3(256), 0, st, frames, m, sasa3 + g * plane, total[g]);
}
