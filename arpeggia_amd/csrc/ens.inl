// SASA and SAP statistics over the frames of an ensemble (arp_sasa_ensemble).  Included by kernels.hip inside
// namespace arp, after sasa.inl and sap.inl: k_sasa, k_sap_weight and k_neighbor_sum run unchanged on what k_ens_tile writes.  The dSASA form
// (arp_dsasa_ensemble) runs k_sasa_split on the same pack and adds k_bsa_tile_attr and k_bsa_frames_buried.
//
// The frames of a pass are the models of one packed input (model = frame ordinal inside the pass, DevAtoms::per_model: every frame gets its own
// z slab of the grid and its own origin, so frames never see each other and a drifting trajectory does not inflate the cell count).  Only the
// coordinates cross PCIe per pass; k_ens_tile gathers the selected atoms of every frame and writes the two coordinate sets (the f64 images of
// the f32-rounded coordinates for the SASA grid, sasa.rs:196-198; the untouched f64 coordinates for the SAP grid) and the per-frame copies of
// the topology's words.  The outputs of a pass are [frame][selected atom] arrays; k_ens_reduce folds them into per-atom accumulators that live
// on the device for the whole call, k_ens_totals sums every frame's SASA.  No atomics: every accumulator has one owner.

// (EnsTopo, EnsPack, EnsAcc: arp_internal.h)

// item q = f * m + k: selected atom k of frame f.  xyz: the pass's coordinates as they came from the host, frames x n_top x 3.
__global__ __launch_bounds__(256) void k_ens_tile(uint32_t frames, const double *xyz, EnsTopo t, EnsPack p) {
    const unsigned long long total = (unsigned long long)frames * t.m;
    for (unsigned long long q = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (unsigned long long)gridDim.x * blockDim.x) {
        const uint32_t f = (uint32_t)(q / t.m), k = (uint32_t)(q % t.m);
        const double *c = xyz + 3ull * ((unsigned long long)f * t.n_top + t.sel[k]);
        const double cx = c[0], cy = c[1], cz = c[2];
        p.x[q] = (double)__double2float_rn(cx); p.y[q] = (double)__double2float_rn(cy); p.z[q] = (double)__double2float_rn(cz);
        p.model[q] = f;
        p.R[q] = t.R[k];
        if (p.px) {
            p.px[q] = cx; p.py[q] = cy; p.pz[q] = cz;
            p.pattr[q] = t.pattr[k]; p.code[q] = t.code[k];
            p.src[q] = (int32_t)q;  // the weight of an atom comes from its own SASA of its own frame
        }
    }
}

// (dSASA form) attribute word of the packed atoms: item f * m + k gets the word of selected atom k (k_ens_tile writes everything else of the pack)
__global__ __launch_bounds__(256) void k_bsa_tile_attr(uint32_t frames, uint32_t m, const uint32_t *attr, uint32_t *out) {
    const unsigned long long total = (unsigned long long)frames * m;
    for (unsigned long long q = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (unsigned long long)gridDim.x * blockDim.x)
        out[q] = attr[(uint32_t)(q % m)];
}

// One thread per selected atom walks the frames of the pass in order (loads coalesced across atoms).  first: the call's first pass -- the
// accumulators start here, later passes carry them on, so the order of the f64 additions is frame 0 .. F - 1 whatever the pass size is.
__global__ __launch_bounds__(256) void k_ens_reduce(uint32_t frames, uint32_t m, const int32_t *count, const float *sap, EnsAcc a, uint32_t first) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= m) return;
    unsigned long long s1 = 0ull, s2 = 0ull;
    int32_t cmin = 0x7FFFFFFF, cmax = 0;
    double t1 = 0.0, t2 = 0.0;
    float pmin = INFINITY, pmax = -INFINITY;
    if (!first) {
        s1 = a.s1[k]; s2 = a.s2[k]; cmin = a.cmin[k]; cmax = a.cmax[k];
        if (sap) { t1 = a.t1[k]; t2 = a.t2[k]; pmin = a.pmin[k]; pmax = a.pmax[k]; }
    }
    const int32_t *cp = count + k;
#pragma unroll 4
    for (uint32_t f = 0; f < frames; f++) {
        const int32_t c = cp[(unsigned long long)f * m];
        s1 += (unsigned long long)c; s2 += (unsigned long long)c * (unsigned long long)c;
        cmin = min(cmin, c); cmax = max(cmax, c);
    }
    a.s1[k] = s1; a.s2[k] = s2; a.cmin[k] = cmin; a.cmax[k] = cmax;
    if (sap) {
        const float *sp = sap + k;
#pragma unroll 4
        for (uint32_t f = 0; f < frames; f++) {
            const float v = sp[(unsigned long long)f * m];
            const double d = (double)v;
            t1 = __dadd_rn(t1, d); t2 = __dadd_rn(t2, __dmul_rn(d, d));  // (d * d is exact: 24-bit factors)
            pmin = v < pmin ? v : pmin; pmax = v > pmax ? v : pmax;
        }
        a.t1[k] = t1; a.t2[k] = t2; a.pmin[k] = pmin; a.pmax[k] = pmax;
    }
}

// (dSASA form) per selected atom the frames with buried > 0, over all frames so far; one thread owns one accumulator (k_ens_reduce's scheme)
__global__ __launch_bounds__(256) void k_bsa_frames_buried(uint32_t frames, uint32_t m, const int32_t *buried, uint32_t *acc, uint32_t first) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= m) return;
    uint32_t n = first ? 0u : acc[k];
    const int32_t *bp = buried + k;
#pragma unroll 4
    for (uint32_t f = 0; f < frames; f++) n += bp[(unsigned long long)f * m] > 0 ? 1u : 0u;
    acc[k] = n;
}

// total[f] = f32 of the f64 sum of sasa[f][0 .. m) in atom order (as arp_structure_dsasa sums its totals).  One wave per frame: the lanes load
// 64 consecutive values at once, then every lane adds them up in lane order (the same uniform chain in all lanes); a lane past the end adds 0.0,
// which leaves the non-negative sum unchanged.
__global__ __launch_bounds__(256) void k_ens_totals(uint32_t frames, uint32_t m, const float *sasa, float *total) {
    const uint32_t f = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (f >= frames) return;  // (wave-uniform)
    const float *row = sasa + (unsigned long long)f * m;
    double acc = 0.0;
#pragma unroll 1
    for (uint32_t k0 = 0; k0 < m; k0 += 64u) {
        const uint32_t k = k0 + lane;
        const float v = k < m ? row[k] : 0.0f;
#pragma unroll
        for (int j = 0; j < 64; j++) acc = __dadd_rn(acc, (double)__uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), j)));
    }
    if (lane == 0u) total[f] = (float)acc;
}

void launch_ens_tile(uint32_t frames, const double *xyz, const EnsTopo &t, const EnsPack &p, hipStream_t st) {
    const unsigned long long items = (unsigned long long)frames * t.m;
    if (!items) return;
    const uint32_t blocks = (uint32_t)std::min<unsigned long long>((items + 255u) / 256u, 1u << 16);
    hipLaunchKernelGGL(k_ens_tile, dim3(blocks), dim3(256), 0, st, frames, xyz, t, p);
}

void launch_ens_reduce(uint32_t frames, uint32_t m, const int32_t *count, const float *sasa, const float *sap, const EnsAcc &a, bool first, float *total,
                       hipStream_t st) {
    if (!frames || !m) return;
    hipLaunchKernelGGL(k_ens_reduce, dim3((m + 255u) / 256u), dim3(256), 0, st, frames, m, count, sap, a, first ? 1u : 0u);
    hipLaunchKernelGGL(k_ens_totals, dim3((frames + 3u) / 4u), dim3(256), 0, st, frames, m, sasa, total);
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
