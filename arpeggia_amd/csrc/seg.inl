// Segment sums of [row][item] f32 arrays (arp_segment_sum): residue- and chain-level SASA from the per-atom values of
// k_sasa, for one structure (one row) or the frames of an ensemble pass (one row per frame).  Included by kernels.hip inside namespace arp.
//
// out[row][s] = f32 of the f64 chain acc = 0.0; acc = acc + (double)values[row][item[q]] for q = start[s] .. start[s + 1) - 1, in that order,
// one __dadd_rn per item.  The chain is serial by contract, so the parallelism is across (row, segment) pairs, never inside one:
//   k_seg_lanes  one lane per pair, for segments of at most kSegLaneItems items (a residue: 4-14 atoms).  Neighbouring lanes hold neighbouring
//                segments of one row, whose items are neighbouring atoms: the gathers of a wave fall into a few lines.
//   k_seg_waves  one wave per pair, for the longer ones (a chain: 10^2 - 10^4 atoms; the host lists them, SegCsr::long_ids).  The lanes gather
//                64 items at once (the index loads coalesced), convert them, and every lane then runs the same 64 additions in item order on
//                the values read lane by lane (k_ens_totals' chain).  A lane past the end contributes +0.0, which leaves a sum of non-negative
//                values unchanged (the accumulator is never -0.0: it starts at +0.0).
// No atomics, every output has one writer; two calls give the same bytes.

constexpr uint32_t kSegLaneItems = 64;  // longest segment the lane kernel takes; longer ones are listed for the wave kernel

__global__ __launch_bounds__(256) void k_seg_lanes(unsigned long long rows, uint32_t m, const float *values, SegCsr c, float *out) {
    const unsigned long long total = rows * c.n_seg;
    for (unsigned long long q = (unsigned long long)blockIdx.x * 256u + threadIdx.x; q < total; q += (unsigned long long)gridDim.x * 256u) {
        const unsigned long long row = q / c.n_seg;
        const uint32_t s = (uint32_t)(q % c.n_seg), k0 = c.start[s], k1 = c.start[s + 1];
        if (k1 - k0 > kSegLaneItems) continue;  // the wave kernel's
        const float *v = values + row * m;
        double acc = 0.0;
        uint32_t k = k0;
        for (; k + 4u <= k1; k += 4u) {  // four gathers in flight, then the four additions in list order
            const float a0 = v[c.item[k]], a1 = v[c.item[k + 1]], a2 = v[c.item[k + 2]], a3 = v[c.item[k + 3]];
            acc = __dadd_rn(__dadd_rn(__dadd_rn(__dadd_rn(acc, (double)a0), (double)a1), (double)a2), (double)a3);
        }
        for (; k < k1; k++) acc = __dadd_rn(acc, (double)v[c.item[k]]);
        out[q] = (float)acc;
    }
}

__global__ __launch_bounds__(256) void k_seg_waves(unsigned long long rows, uint32_t m, const float *values, SegCsr c, float *out) {
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long total = rows * c.n_long;
    // (readfirstlane: the pair is the same in all lanes of a wave; said so, the loop below runs on scalar registers)
    for (unsigned long long p = (unsigned long long)blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); p < total;
         p += (unsigned long long)gridDim.x * 4u) {
        const unsigned long long row = p / c.n_long;
        const uint32_t s = c.long_ids[(uint32_t)(p % c.n_long)], k0 = c.start[s], k1 = c.start[s + 1];
        const float *v = values + row * m;
        double acc = 0.0;
#pragma unroll 1
        for (uint32_t k = k0; k < k1; k += 64u) {
            const double d = k + lane < k1 ? (double)v[c.item[k + lane]] : 0.0;
            const int lo = __double2loint(d), hi = __double2hiint(d);
#pragma unroll
            for (int j = 0; j < 64; j++) acc = __dadd_rn(acc, __hiloint2double(__builtin_amdgcn_readlane(hi, j), __builtin_amdgcn_readlane(lo, j)));
        }
        if (lane == 0u) out[row * c.n_seg + s] = (float)acc;
    }
}

// rows x m values -> rows x c.n_seg sums.  Asynchronous on st.  The CSR has been checked by the host (seg_check): every item < m, start monotone.
void launch_segment_sum(uint64_t rows, uint32_t m, const float *values, const SegCsr &c, float *out, hipStream_t st) {
    if (!rows || !c.n_seg) return;
    if (c.n_long < c.n_seg) {
        const uint32_t blocks = (uint32_t)std::min<unsigned long long>((rows * c.n_seg + 255u) / 256u, 1u << 20);
        hipLaunchKernelGGL(k_seg_lanes, dim3(blocks), dim3(256), 0, st, (unsigned long long)rows, m, values, c, out);
    }
    if (c.n_long) {
        const uint32_t blocks = (uint32_t)std::min<unsigned long long>((rows * c.n_long + 3u) / 4u, 1u << 20);
        hipLaunchKernelGGL(k_seg_waves, dim3(blocks), dim3(256), 0, st, (unsigned long long)rows, m, values, c, out);
    }
}

// One thread per residue walks the frames of the pass in order: the SAP half of k_ens_reduce for a [frame][n_res] array.  first: the call's
// first pass -- the accumulators start here, later passes carry them on, so the f64 additions run in frame order whatever the pass size is.
__global__ __launch_bounds__(256) void k_ens_res_reduce(uint32_t frames, uint32_t n_res, const float *rs, SegAcc a, uint32_t first) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_res) return;
    double t1 = 0.0, t2 = 0.0;
    float vmin = INFINITY, vmax = -INFINITY;
    if (!first) { t1 = a.t1[r]; t2 = a.t2[r]; vmin = a.vmin[r]; vmax = a.vmax[r]; }
    const float *p = rs + r;
#pragma unroll 4
    for (uint32_t f = 0; f < frames; f++) {
        const float v = p[(unsigned long long)f * n_res];
        const double d = (double)v;
        t1 = __dadd_rn(t1, d); t2 = __dadd_rn(t2, __dmul_rn(d, d));  // (d * d is exact: 24-bit factors)
        vmin = v < vmin ? v : vmin; vmax = v > vmax ? v : vmax;
    }
    a.t1[r] = t1; a.t2[r] = t2; a.vmin[r] = vmin; a.vmax[r] = vmax;
}

void launch_ens_res_reduce(uint32_t frames, uint32_t n_res, const float *rs, const SegAcc &a, bool first, hipStream_t st) {
    if (!frames || !n_res) return;
    hipLaunchKernelGGL(k_ens_res_reduce, dim3((n_res + 255u) / 256u), dim3(256), 0, st, frames, n_res, rs, a, first ? 1u : 0u);
}
