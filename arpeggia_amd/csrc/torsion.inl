// Torsion angles, rotamer states and Ramachandran maps across the frames of an ensemble (arp_torsions).  Included by table_dev.hip
// inside namespace arp, behind rmsf.inl, whose slab sum (rmsf_slab_sum) it uses.  One torsion is torsion_eval / torsion_bin of table_dev.h, the functions the
// host twin calls.  The frames come through the upload passes of the arp_rmsd_* calls; per pass:
//   k_torsion_angle   one lane per (frame, torsion), neighbouring lanes neighbouring torsions of one frame (they share atoms: a residue's phi, psi, omega and chi1
//                     read seven atoms between them).  Writes cs[f][d][2], bin[f][d] (u16, kTorsionNoBin: undefined), the angle where it is asked for, and the
//                     state byte into the resident states[F][D]
//   k_torsion_slab    one lane per (slab of 32 frames, torsion): the pass's part of the slab added in frame order onto part[slab][d][2] -- a slab that a pass
//                     boundary cuts goes on where the pass before left it, so the sum does not depend on the pass size
//   k_torsion_hist    hist[d][bin] += 1 per defined sample: one u32 global add each.  Many rows, few hits per row and pass: nothing to aggregate
//   k_torsion_hist2<kLds>  the Ramachandran maps.  kLds: every workgroup counts its samples in a table of G B^2 words in LDS and adds the non-zero words to the
//                     global table at its end -- the route where G B^2 x 4 bytes fit kTorsionLdsBytes (four residue classes x 36 x 36: 20 KiB).  !kLds: one
//                     global add per sample, kept for measurements ("torsion_hist2_route" 3)
//   k_torsion_hist2_match  the route for tables that do not fit (one group per residue, or four classes at 72 bins and more): one wave per (pair, 64 frames of the
//                     pass); the lanes with equal (bin a, bin b) find each other by ballot and one of them adds their count: one global add per distinct bin
// and after the last pass:
//   k_torsion_sums    sums[d][2] from part: rmsf_slab_sum -- wave j of four the slabs j, j + 4, .., a fixed tree
//   k_torsion_stats   state counts, n_defined and transitions from the state bytes: lanes count runs of frames in registers and add them with u32 atomics
// The only atomics are u32 additions (exact in any order), no floating-point atomic exists: two calls give identical bytes, whatever the pass size.

constexpr uint32_t kTorsionBlock = 256;      // lanes of a workgroup of every kernel here
constexpr uint32_t kTorsionSlab = 32;        // frames of a slab of the sums (torsion_resident_bytes in table_dev.h counts on it)
constexpr uint32_t kTorsionLdsBytes = 65536; // the largest table of k_torsion_hist2<true>: what a workgroup may take of a CU's 160 KiB without an attribute
constexpr uint32_t kTorsionHist2Per = 16;    // samples per lane k_torsion_hist2 is sized for: a workgroup's table is flushed once per 4096 samples or more
constexpr uint32_t kTorsionHist2Blocks = 1024;
constexpr uint32_t kTorsionStatsFrames = 1024;  // frames of a chunk of k_torsion_stats, at least
constexpr uint64_t kTorsionPassSamples = 1ull << 27;  // (frame, torsion) samples of a pass, at most: bounds the pass buffers and every grid

// stage[fc][N][3]; quads[D][4]; cs[fc][D][2]; bins[fc][D]; angles[fc][D] (nullable); states: the pass's rows of the resident states
__global__ __launch_bounds__(kTorsionBlock) void k_torsion_angle(const double *__restrict__ stage, uint32_t N, const uint4 *__restrict__ quads, uint32_t D, uint64_t fc, uint32_t B,
                                                                 double2 *__restrict__ cs, uint16_t *__restrict__ bins, float *__restrict__ angles, uint8_t *__restrict__ states) {
    const uint64_t idx = (uint64_t)blockIdx.x * kTorsionBlock + threadIdx.x;
    if (idx >= fc * D) return;
    const uint64_t f = idx / D;
    const uint32_t d = (uint32_t)(idx % D);
    const double *x = stage + f * (uint64_t)N * 3u;
    const uint4 q = quads[d];
    const Torsion t = torsion_eval(x + (uint64_t)q.x * 3u, x + (uint64_t)q.y * 3u, x + (uint64_t)q.z * 3u, x + (uint64_t)q.w * 3u);
    cs[idx] = make_double2(t.c, t.s);
    bins[idx] = t.state && B ? (uint16_t)torsion_bin(t.a, B) : kTorsionNoBin;
    if (angles) angles[idx] = t.state ? (float)t.a : __uint_as_float(kTorsionNanBits);
    states[idx] = t.state;
}

// The frames f0 .. f0 + fc - 1 of the pass; lane (slab s of the pass, torsion d) walks the slab's frames that lie in the pass, in their order.
__global__ __launch_bounds__(kTorsionBlock) void k_torsion_slab(const double2 *__restrict__ cs, uint32_t D, uint64_t f0, uint64_t fc, uint64_t n_slabs, double2 *part) {
    const uint64_t idx = (uint64_t)blockIdx.x * kTorsionBlock + threadIdx.x;
    if (idx >= n_slabs * D) return;
    const uint64_t slab = f0 / kTorsionSlab + idx / D, d = idx % D;
    const uint64_t s0 = slab * kTorsionSlab, fa = f0 > s0 ? f0 : s0, fb = f0 + fc < s0 + kTorsionSlab ? f0 + fc : s0 + kTorsionSlab;
    double2 acc = fa == s0 ? make_double2(0.0, 0.0) : part[slab * D + d];
    for (uint64_t f = fa; f < fb; f++) {
        const double2 v = cs[(f - f0) * D + d];   // (0, 0) where undefined: adding it changes nothing
        acc.x += v.x; acc.y += v.y;
    }
    part[slab * D + d] = acc;
}

__global__ __launch_bounds__(kTorsionBlock) void k_torsion_hist(const uint16_t *__restrict__ bins, uint32_t D, uint64_t fc, uint32_t B, uint32_t *hist) {
    const uint64_t idx = (uint64_t)blockIdx.x * kTorsionBlock + threadIdx.x;
    if (idx >= fc * D) return;
    const uint16_t b = bins[idx];
    if (b != kTorsionNoBin) atomicAdd(&hist[(idx % D) * B + b], 1u);
}

// pairs[P][3]; cells = G B^2 (kLds: the words of the dynamic LDS table); the samples (frame, pair) of the pass in a grid-stride loop, pairs fastest
template <bool kLds>
__global__ __launch_bounds__(kTorsionBlock) void k_torsion_hist2(const uint16_t *__restrict__ bins, uint32_t D, uint64_t fc, const uint32_t *__restrict__ pairs, uint32_t P, uint32_t B,
                                                                 uint32_t cells, uint32_t *hist2) {
    extern __shared__ uint32_t torsion_tab[];
    if (kLds) {
        for (uint32_t i = threadIdx.x; i < cells; i += kTorsionBlock) torsion_tab[i] = 0u;
        __syncthreads();
    }
    const uint64_t n = fc * P;
    for (uint64_t idx = (uint64_t)blockIdx.x * kTorsionBlock + threadIdx.x; idx < n; idx += (uint64_t)gridDim.x * kTorsionBlock) {  // (no barrier inside)
        const uint64_t f = idx / P;
        const uint32_t *pr = pairs + (idx % P) * 3u;
        const uint16_t ba = bins[f * D + pr[0]], bb = bins[f * D + pr[1]];
        if (ba == kTorsionNoBin || bb == kTorsionNoBin) continue;
        const uint64_t cell = ((uint64_t)pr[2] * B + ba) * B + bb;   // < G B^2: group < G was checked on the host, bins < B by torsion_bin
        atomicAdd(kLds ? &torsion_tab[cell] : &hist2[cell], 1u);
    }
    if (kLds) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < cells; i += kTorsionBlock) {
            const uint32_t v = torsion_tab[i];
            if (v) atomicAdd(&hist2[i], v);
        }
    }
}

// Wave w of the grid: pair w / groups, frames 64 (w % groups) .. of the pass, one per lane.
__global__ __launch_bounds__(kTorsionBlock) void k_torsion_hist2_match(const uint16_t *__restrict__ bins, uint32_t D, uint64_t fc, const uint32_t *__restrict__ pairs, uint32_t P, uint32_t B,
                                                                       uint32_t *hist2) {
    const uint64_t wave = ((uint64_t)blockIdx.x * kTorsionBlock + threadIdx.x) >> 6, groups = (fc + 63u) / 64u;
    const uint32_t lane = threadIdx.x & 63u;
    if (wave >= (uint64_t)P * groups) return;  // (the whole wave; the kernel has no barrier)
    const uint32_t *pr = pairs + (wave / groups) * 3u;
    const uint64_t f = (wave % groups) * 64u + lane;
    bool active = f < fc;
    uint32_t key = 0u;
    if (active) {
        const uint16_t ba = bins[f * D + pr[0]], bb = bins[f * D + pr[1]];
        active = ba != kTorsionNoBin && bb != kTorsionNoBin;
        key = (uint32_t)ba * B + bb;
    }
    uint32_t *table = hist2 + (uint64_t)pr[2] * B * B;
    unsigned long long live = __ballot(active);
    while (live) {  // (live is the same in every lane: the wave makes one trip per distinct key)
        const uint32_t leader = (uint32_t)__ffsll((long long)live) - 1u;
        const uint32_t k0 = (uint32_t)__shfl((int)key, (int)leader, 64);
        const unsigned long long same = __ballot(active && key == k0);
        if (lane == leader) atomicAdd(&table[k0], (uint32_t)__popcll(same));
        live &= ~same;
    }
}

__global__ __launch_bounds__(256) void k_torsion_sums(const double *__restrict__ part, uint32_t slabs, uint32_t items, double *sums) {
    __shared__ double red[256];
    const uint32_t e = blockIdx.x * kRmsfFinish + (threadIdx.x & 63u);
    const double s = rmsf_slab_sum(part, slabs, items, e, red);
    if (threadIdx.x < kRmsfFinish && e < items) sums[e] = s;
}

// Block (x, y): the torsions 64 x .. and the frames chunk y .. chunk (y + 1) - 1; wave j of four takes the frames j, j + 4, .. of the chunk.  stats[D][6]:
// the four state counts, n_defined, n_transitions.  A transition into frame f is counted by the lane that owns f, which reads frame f - 1 as well.
__global__ __launch_bounds__(256) void k_torsion_stats(const uint8_t *__restrict__ states, uint32_t D, uint64_t F, uint64_t chunk, uint32_t *stats) {
    const uint32_t d = blockIdx.x * 64u + (threadIdx.x & 63u);
    if (d >= D) return;
    const uint64_t fa = (uint64_t)blockIdx.y * chunk, fb = F < fa + chunk ? F : fa + chunk;
    uint32_t n[4] = {0u, 0u, 0u, 0u}, tr = 0u;
    for (uint64_t f = fa + (threadIdx.x >> 6); f < fb; f += 4u) {
        const uint8_t s = states[f * D + d];
        n[0] += s == 0u; n[1] += s == 1u; n[2] += s == 2u; n[3] += s == 3u;
        if (f && s) {
            const uint8_t p = states[(f - 1u) * D + d];
            tr += p && p != s;
        }
    }
    uint32_t *o = stats + (uint64_t)d * 6u;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (n[k]) atomicAdd(&o[k], n[k]);
    if (n[1] + n[2] + n[3]) atomicAdd(&o[4], n[1] + n[2] + n[3]);
    if (tr) atomicAdd(&o[5], tr);
}

// The call on the device.  The checks, the capacity check among them, ran on the host (torsion.cpp).
arp_status device_torsions(arp_context *ctx, const TorsionJob &job, TorsionOut *out) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(context_device(ctx)));
    StreamLapTimer lap("  torsions %-10s %8.3f ms\n", st);
    const uint64_t N = job.n_atoms, F = job.n_frames, D = job.n_tors, P = job.n_pairs, B = job.n_bins, G = job.n_groups;
    const bool want_hist = out->hist != nullptr, want_hist2 = out->hist2 != nullptr;
    const uint64_t cells = want_hist2 ? G * B * B : 0u;
    // the route of the maps: LDS tables where they fit, matched global adds where not
    int route = job.hist2_route == 0 ? 1 : job.hist2_route;
    if (route == 1 && cells * 4u > kTorsionLdsBytes) route = 2;
    uint64_t per = frames_per_pass(job.chunk_atoms, N, F);
    per = std::min<uint64_t>(per, std::max<uint64_t>(1, kTorsionPassSamples / std::max(D, std::max<uint64_t>(P, 1))));
    const uint64_t slabs = (F + kTorsionSlab - 1u) / kTorsionSlab;
    const uint64_t chunk = std::max<uint64_t>(kTorsionStatsFrames, (F + 65534u) / 65535u), chunks = (F + chunk - 1u) / chunk;
    double *stage = nullptr, *sums = nullptr; uint4 *quads = nullptr; uint32_t *pairs = nullptr, *stats = nullptr, *hist = nullptr, *hist2 = nullptr;
    double2 *cs = nullptr, *part = nullptr; uint16_t *bins = nullptr; float *ang = nullptr; uint8_t *states = nullptr;
    DevBlock block;
    if (arp_status s = block.carve([&](Bump &bp) {
            stage = bp.take<double>(per * N * 3u); quads = bp.take<uint4>(D); pairs = bp.take<uint32_t>(std::max<uint64_t>(P, 1) * 3u);
            cs = bp.take<double2>(per * D); bins = bp.take<uint16_t>(per * D); ang = bp.take<float>(per * D);
            states = bp.take<uint8_t>(F * D); part = bp.take<double2>(slabs * D); sums = bp.take<double>(D * 2u);
            stats = bp.take<uint32_t>(D * 6u); hist = bp.take<uint32_t>(std::max<uint64_t>(D * B, 1)); hist2 = bp.take<uint32_t>(std::max<uint64_t>(cells, 1)); bp.take<char>(256);  // (slack)
        }); s != ARP_OK) return s;
    HIP_TRY(hipMemcpyAsync(quads, job.quads, D * 16u, hipMemcpyHostToDevice, st));
    if (want_hist2) HIP_TRY(hipMemcpyAsync(pairs, job.pairs, P * 12u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(stats, 0, D * 24u, st));
    if (want_hist) HIP_TRY(hipMemsetAsync(hist, 0, D * B * 4u, st));
    if (want_hist2) HIP_TRY(hipMemsetAsync(hist2, 0, cells * 4u, st));
    for (uint64_t f0 = 0; f0 < F; f0 += per) {
        const uint64_t fc = std::min<uint64_t>(per, F - f0), samples = fc * D;
        const dim3 per_sample((uint32_t)((samples + kTorsionBlock - 1u) / kTorsionBlock));
        HIP_TRY(hipMemcpyAsync(stage, job.xyz + f0 * N * 3u, fc * N * 24u, hipMemcpyHostToDevice, st));
        lap("upload");
        hipLaunchKernelGGL(k_torsion_angle, per_sample, dim3(kTorsionBlock), 0, st, (const double *)stage, (uint32_t)N, (const uint4 *)quads, (uint32_t)D, fc, (uint32_t)B, cs, bins,
                           out->angles ? ang : (float *)nullptr, states + f0 * D);
        const uint64_t n_slabs = (f0 + fc - 1u) / kTorsionSlab - f0 / kTorsionSlab + 1u;
        hipLaunchKernelGGL(k_torsion_slab, dim3((uint32_t)((n_slabs * D + kTorsionBlock - 1u) / kTorsionBlock)), dim3(kTorsionBlock), 0, st, (const double2 *)cs, (uint32_t)D, f0, fc, n_slabs,
                           part);
        HIP_TRY(hipGetLastError());
        lap("angle");
        if (want_hist) hipLaunchKernelGGL(k_torsion_hist, per_sample, dim3(kTorsionBlock), 0, st, (const uint16_t *)bins, (uint32_t)D, fc, (uint32_t)B, hist);
        if (want_hist2) {
            if (route == 2) {
                const uint64_t waves = P * ((fc + 63u) / 64u);
                hipLaunchKernelGGL(k_torsion_hist2_match, dim3((uint32_t)((waves + 3u) / 4u)), dim3(kTorsionBlock), 0, st, (const uint16_t *)bins, (uint32_t)D, fc, (const uint32_t *)pairs,
                                   (uint32_t)P, (uint32_t)B, hist2);
            } else {
                const uint64_t want = (fc * P + (uint64_t)kTorsionBlock * kTorsionHist2Per - 1u) / ((uint64_t)kTorsionBlock * kTorsionHist2Per);
                const dim3 grid((uint32_t)std::min<uint64_t>(std::max<uint64_t>(want, 1), kTorsionHist2Blocks));
                if (route == 1)
                    hipLaunchKernelGGL(k_torsion_hist2<true>, grid, dim3(kTorsionBlock), (size_t)(cells * 4u), st, (const uint16_t *)bins, (uint32_t)D, fc, (const uint32_t *)pairs, (uint32_t)P,
                                       (uint32_t)B, (uint32_t)cells, hist2);
                else
                    hipLaunchKernelGGL(k_torsion_hist2<false>, grid, dim3(kTorsionBlock), 0, st, (const uint16_t *)bins, (uint32_t)D, fc, (const uint32_t *)pairs, (uint32_t)P, (uint32_t)B,
                                       (uint32_t)cells, hist2);
            }
        }
        HIP_TRY(hipGetLastError());
        lap("hist");
        if (out->angles) HIP_TRY(hipMemcpyAsync(out->angles + f0 * D, ang, samples * 4u, hipMemcpyDeviceToHost, st));
        if (out->cossin) HIP_TRY(hipMemcpyAsync(out->cossin + f0 * D * 2u, cs, samples * 16u, hipMemcpyDeviceToHost, st));
        lap("download");
    }
    hipLaunchKernelGGL(k_torsion_sums, dim3((uint32_t)((2u * D + kRmsfFinish - 1u) / kRmsfFinish)), dim3(256), 0, st, (const double *)part, (uint32_t)slabs, (uint32_t)(2u * D), sums);
    hipLaunchKernelGGL(k_torsion_stats, dim3((uint32_t)((D + 63u) / 64u), (uint32_t)chunks), dim3(256), 0, st, (const uint8_t *)states, (uint32_t)D, F, chunk, stats);
    HIP_TRY(hipGetLastError());
    lap("finish");
    std::vector<uint32_t> h_stats(D * 6u);
    HIP_TRY(hipMemcpyAsync(h_stats.data(), stats, D * 24u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->sums, sums, D * 16u, hipMemcpyDeviceToHost, st));
    if (out->states) HIP_TRY(hipMemcpyAsync(out->states, states, F * D, hipMemcpyDeviceToHost, st));
    if (want_hist) HIP_TRY(hipMemcpyAsync(out->hist, hist, D * B * 4u, hipMemcpyDeviceToHost, st));
    if (want_hist2) HIP_TRY(hipMemcpyAsync(out->hist2, hist2, cells * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint64_t d = 0; d < D; d++) {
        for (int k = 0; k < 4; k++) out->state_counts[4u * d + k] = h_stats[6u * d + k];
        out->n_defined[d] = h_stats[6u * d + 4u];
        out->n_transitions[d] = h_stats[6u * d + 5u];
    }
    lap("download");
    return ARP_OK;
}
