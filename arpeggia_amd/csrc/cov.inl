// Covariance, DCCM and projection of an ensemble's motions (arp_covariance, arp_project).
// Included by table_dev.hip inside namespace arp, behind rmsf.inl, whose resident state it reads: the packed measured atoms XM[F][3][m_pad], the last
// rotations R[F][9] and the finished mean of the measured atoms.
//   k_cov_dev          D[F][3][m_pad] = R_f XM_f - mean, the pads zero: the deviations, written once and read by both ends of the Gram
//   k_cov_gram<kEnd>   tiles over the upper triangle of D^T D on v_mfma_f64_16x16x4_f64, the contraction split into slabs of frames: partial[slab][tile][32][32]
//                      kCovFull  D as F rows of 3 m_pad coordinates: the coordinates' second moments
//                      kCovDccm  D as 3 F rows of m_pad atoms: the atoms' dot products, the contraction running over (frame, component)
//   k_cov_finish       per entry of a tile the slabs, four interleaved runs in their order and a fixed tree, / F, the tile and its mirror in atom-major
//                      order (a = 3 i + k)
//   k_dccm_var         v_i = t_ii: the slabs of the diagonal entries likewise, / F
//   k_dccm_finish      per entry the slabs likewise, / F, t_ij / sqrt(v_i v_j), the clamp, one rounding to f32, the tile and its mirror
//   k_project          per (sixteen frames, sixteen modes): R_f p + t_f - mean of the measured atoms gathered from the staged pass, the dot products in the
//                      order of the coordinate index
// A product's terms are summed in the order of the frames within a slab, four per MFMA, and the slabs in a fixed interleave; the slab count depends on (F, m)
// alone (table_dev.h cov_plan) and no floating-point atomic exists: two calls give identical bytes, whatever the upload pass size.

constexpr uint32_t kCovLds = 48;  // LDS stride in doubles of one contraction row (32 coordinates and 16 of padding): 48 = 16 mod 32, so the sixteen coordinates x two
                                  // contraction rows that one half of a wave reads (ds_read_b64 serves lanes 0-31, then 32-63) fall on all 32 eight-byte slots
                                  // of the 64 four-byte banks once; the staging writes, 32 consecutive coordinates of two rows, do the same
constexpr int kCovFull = 0, kCovDccm = 1;
static_assert(kCovTile == 32 && kCovChunk % 4 == 0 && kCovSlabMin % kCovChunk == 0 && kCovLds % 32 == 16, "two by two waves of 16 x 16, whole MFMA steps per chunk, whole chunks per slab");

__global__ __launch_bounds__(256) void k_cov_dev(const double *__restrict__ XM, const double *__restrict__ R, const double *__restrict__ mean, uint64_t F, uint32_t m, uint32_t m_pad,
                                                 double *D) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= F * m_pad) return;
    const uint64_t f = idx / m_pad;
    const uint32_t i = (uint32_t)(idx % m_pad);
    const double *x = XM + f * 3u * m_pad + i, *r = R + f * 9u;
    const double x0 = x[0], x1 = x[m_pad], x2 = x[2u * (size_t)m_pad];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double y = (r[3 * k] * x0 + r[3 * k + 1] * x1) + r[3 * k + 2] * x2;  // (k_rmsf_sweep's expression: the same bits)
        D[(f * 3u + k) * m_pad + i] = i < m ? y - mean[(size_t)k * m_pad + i] : 0.0;
    }
}

// Block b: tile b % tri of the upper triangle of the L x L product, slab b / tri of the K contraction rows of D[K][L].  Wave (wi, wj) of the 2 x 2 owns the
// 16 x 16 entries (16 wi + r, 16 wj + c); its accumulator holds entry (r = (lane >> 4) + 4 reg, c = lane & 15).  The contraction rows go through LDS in
// chunks of kCovChunk, the next chunk fetched into registers while the current one is consumed; a row past the slab or past K and a column past L are
// staged as zeros.  The two ends share the loop: kCovFull reads D as F rows of L = 3 m_pad coordinates, kCovDccm as 3 F rows of L = m_pad atoms, so a slab
// of slab_frames frames is three times as many contraction rows there.
template <int kEnd>
__global__ __launch_bounds__(256) void k_cov_gram(const double *__restrict__ D, uint64_t F, uint32_t slab_frames, uint32_t L, uint32_t T, uint32_t tri, double *part) {
    __shared__ __attribute__((aligned(16))) double lds[2u * kCovChunk * kCovLds];
    constexpr uint32_t kRows = kEnd == kCovDccm ? 3u : 1u;  // contraction rows of a frame
    const uint64_t K = F * kRows;
    const uint32_t slab = blockIdx.x / tri, tile = blockIdx.x % tri, slab_rows = slab_frames * kRows;
    uint32_t t = tile, ti = 0;
    while (t >= T - ti) { t -= T - ti; ti++; }
    const uint32_t tj = ti + t, row0 = ti * kCovTile, col0 = tj * kCovTile;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, wi = wave >> 1, wj = wave & 1u, c = lane & 15u, h = lane >> 4;
    double *sA = lds, *sB = lds + kCovChunk * kCovLds;
    const uint32_t lc = threadIdx.x & 31u, lr = threadIdx.x >> 5;  // staging: coordinate lc of the contraction rows lr and lr + 8 of the chunk
    const uint64_t k_begin = (uint64_t)slab * slab_rows, k_end = min(K, k_begin + slab_rows);
    double ra[2], rb[2];
    auto fetch = [&](uint64_t k0) {
#pragma unroll
        for (uint32_t i = 0; i < 2u; i++) {
            const uint64_t k = k0 + lr + 8u * i;
            ra[i] = (k < k_end && row0 + lc < L) ? D[k * L + row0 + lc] : 0.0;
            rb[i] = (k < k_end && col0 + lc < L) ? D[k * L + col0 + lc] : 0.0;
        }
    };
    rmsd_acc acc = rmsd_acc{0.0, 0.0, 0.0, 0.0};
    fetch(k_begin);
    for (uint64_t k0 = k_begin; k0 < k_end; k0 += kCovChunk) {
#pragma unroll
        for (uint32_t i = 0; i < 2u; i++) {
            sA[(lr + 8u * i) * kCovLds + lc] = ra[i];
            sB[(lr + 8u * i) * kCovLds + lc] = rb[i];
        }
        __syncthreads();
        if (k0 + kCovChunk < k_end) fetch(k0 + kCovChunk);
#pragma unroll
        for (uint32_t kk = 0; kk < kCovChunk; kk += 4u) {
            const double a = sA[(kk + h) * kCovLds + 16u * wi + c], b = sB[(kk + h) * kCovLds + 16u * wj + c];
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);  // (a chunk's rows past k_end are zeros: they add +0.0)
        }
        __syncthreads();
    }
    double *out = part + ((size_t)slab * tri + tile) * (kCovTile * kCovTile);
#pragma unroll
    for (int reg = 0; reg < 4; reg++) out[(16u * wi + h + 4u * (uint32_t)reg) * kCovTile + 16u * wj + c] = acc[reg];
}

constexpr uint32_t kCovFinish = 64;                                       // entries of a workgroup of the finish kernels
constexpr uint32_t kCovFinishGroups = kCovTile * kCovTile / kCovFinish;   // such workgroups per tile
constexpr uint32_t kCovFinishLanes = 4;                                   // waves of such a workgroup: wave j sums the slabs j, j + 4, .. of its entries

// Entry e of tile t for the workgroup's 64 entries (rmsf_slab_sum's scheme): wave j sums the slabs j, j + 4, .. in that order, the four waves meet in a fixed
// tree; an entry that is not `wanted` reads nothing.  The whole workgroup calls this; the first wave holds the result.
__device__ __forceinline__ double cov_slab_sum(const double *__restrict__ part, uint32_t slabs, uint32_t tri, uint32_t t, uint32_t e, bool wanted, double *red) {
    double s = 0.0;
    if (wanted)
        for (uint32_t b = threadIdx.x >> 6; b < slabs; b += kCovFinishLanes) s += part[((size_t)b * tri + t) * (kCovTile * kCovTile) + e];
    red[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t off = 128u; off >= kCovFinish; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    return red[threadIdx.x & 63u];
}

// Block 16 t + g: entries 64 g .. of tile t = (ti, tj).  Device coordinate a' = k m_pad + i (component-major) goes to a = 3 i + k of cov[3 m][3 m]; of a
// diagonal tile the entries on and above the diagonal are taken, and every value is written to (a, b) and (b, a).
__global__ __launch_bounds__(256) void k_cov_finish(const double *__restrict__ part, uint32_t slabs, uint32_t T, uint32_t tri, uint64_t F, uint32_t m, uint32_t m_pad, double *cov) {
    __shared__ double red[256];
    const uint32_t tile = blockIdx.x / kCovFinishGroups;
    uint32_t t = tile, ti = 0;
    while (t >= T - ti) { t -= T - ti; ti++; }
    const uint32_t tj = ti + t, L = 3u * m_pad;
    const uint32_t e = (blockIdx.x % kCovFinishGroups) * kCovFinish + (threadIdx.x & 63u), r = e >> 5, c = e & 31u, ap = ti * kCovTile + r, bp = tj * kCovTile + c;
    const bool wanted = ap < L && bp < L && !(ti == tj && c < r) && ap % m_pad < m && bp % m_pad < m;
    const double s = cov_slab_sum(part, slabs, tri, tile, e, wanted, red);
    if (threadIdx.x >= kCovFinish || !wanted) return;
    const double v = s / (double)F;
    const uint64_t ld = 3u * (uint64_t)m, a = 3u * (uint64_t)(ap % m_pad) + ap / m_pad, b = 3u * (uint64_t)(bp % m_pad) + bp / m_pad;
    cov[a * ld + b] = v;
    cov[b * ld + a] = v;
}

// Block g: atoms 64 g ..; v_i is the diagonal entry (i % 32, i % 32) of tile (i / 32, i / 32)
__global__ __launch_bounds__(256) void k_dccm_var(const double *__restrict__ part, uint32_t slabs, uint32_t T, uint32_t tri, uint64_t F, uint32_t m_pad, double *var) {
    __shared__ double red[256];
    const uint32_t i = blockIdx.x * kCovFinish + (threadIdx.x & 63u);
    const bool wanted = i < m_pad;
    const uint32_t tt = wanted ? i / kCovTile : 0u, l = i % kCovTile;
    const uint32_t t = (uint32_t)((uint64_t)tt * T - (uint64_t)tt * (tt ? tt - 1u : 0u) / 2u);  // tile (tt, tt): the T + (T - 1) + .. tiles of the rows before it
    const double s = cov_slab_sum(part, slabs, tri, t, l * kCovTile + l, wanted, red);
    if (threadIdx.x < kCovFinish && wanted) var[i] = s / (double)F;
}

__global__ __launch_bounds__(256) void k_dccm_finish(const double *__restrict__ part, const double *__restrict__ var, uint32_t slabs, uint32_t T, uint32_t tri, uint64_t F, uint32_t m,
                                                     float *dccm) {
    __shared__ double red[256];
    const uint32_t tile = blockIdx.x / kCovFinishGroups;
    uint32_t t = tile, ti = 0;
    while (t >= T - ti) { t -= T - ti; ti++; }
    const uint32_t tj = ti + t;
    const uint32_t e = (blockIdx.x % kCovFinishGroups) * kCovFinish + (threadIdx.x & 63u), r = e >> 5, c = e & 31u, i = ti * kCovTile + r, j = tj * kCovTile + c;
    const bool inside = i < m && j < m && !(ti == tj && c < r);
    const double vi = inside ? var[i] : 0.0, vj = inside ? var[j] : 0.0;
    const bool wanted = inside && i != j && vi != 0.0 && vj != 0.0;
    const double s = cov_slab_sum(part, slabs, tri, tile, e, wanted, red);
    if (threadIdx.x >= kCovFinish || !inside) return;
    const float v = i == j ? 1.0f : wanted ? (float)fmin(1.0, fmax(-1.0, (s / (double)F) / sqrt(vi * vj))) : 0.0f;
    dccm[(size_t)i * m + j] = v;
    dccm[(size_t)j * m + i] = v;
}

// cov and dccm of the resident superposition, behind the deviations of device_rmsf (which calls this when either output is asked for).  The block of its own
// holds D, the slab partials of one end at a time and the outputs; the capacity checks ran on the host (cov.cpp).
arp_status device_cov(hipStream_t st, StreamLapTimer &lap, const double *XM, const double *R, const double *mean_m, uint64_t F, uint64_t m, uint64_t m_pad, RmsfOut *out) {
    const CovPlan full = cov_plan(F, 3u * m_pad), atoms = cov_plan(F, m_pad);
    if ((out->cov && full.tri * std::max<uint64_t>(full.slabs, kCovFinishGroups) >= (1ull << 31)) ||
        (out->dccm && atoms.tri * std::max<uint64_t>(atoms.slabs, kCovFinishGroups) >= (1ull << 31))) {
        set_error("covariance: %llu frames x %llu atoms are more than one launch covers", (unsigned long long)F, (unsigned long long)m);
        return ARP_ERR_CAPACITY;
    }
    const uint64_t part_items = std::max(out->cov ? full.part_items() : 0u, out->dccm ? atoms.part_items() : 0u);
    const uint64_t cov_bytes = out->cov ? 9u * m_pad * m_pad * 8u : 0u, dccm_bytes = out->dccm ? m_pad * m_pad * 4u : 0u;
    double *D = nullptr, *part = nullptr, *d_cov = nullptr, *var = nullptr; float *d_dccm = nullptr;
    DevBlock block;
    if (arp_status s = block.carve([&](Bump &bp) {
            D = bp.take<double>(F * 3u * m_pad); part = bp.take<double>(part_items); d_cov = reinterpret_cast<double *>(bp.take<char>(cov_bytes));
            d_dccm = reinterpret_cast<float *>(bp.take<char>(dccm_bytes)); var = bp.take<double>(m_pad); bp.take<char>(256);  // (slack)
        }); s != ARP_OK) return s;
    hipLaunchKernelGGL(k_cov_dev, dim3((uint32_t)((F * m_pad + 255u) / 256u)), dim3(256), 0, st, XM, R, mean_m, F, (uint32_t)m, (uint32_t)m_pad, D);
    HIP_TRY(hipGetLastError());
    lap("cov_dev");
    if (out->cov) {
        hipLaunchKernelGGL(k_cov_gram<kCovFull>, dim3((uint32_t)(full.tri * full.slabs)), dim3(256), 0, st, (const double *)D, F, (uint32_t)full.slab_frames, (uint32_t)full.L,
                           (uint32_t)full.T, (uint32_t)full.tri, part);
        HIP_TRY(hipGetLastError());
        lap("cov_gram");
        hipLaunchKernelGGL(k_cov_finish, dim3((uint32_t)(full.tri * kCovFinishGroups)), dim3(256), 0, st, (const double *)part, (uint32_t)full.slabs, (uint32_t)full.T, (uint32_t)full.tri, F, (uint32_t)m,
                           (uint32_t)m_pad, d_cov);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out->cov, d_cov, 9u * m * m * 8u, hipMemcpyDeviceToHost, st));
        lap("cov_finish");
    }
    if (out->dccm) {
        hipLaunchKernelGGL(k_cov_gram<kCovDccm>, dim3((uint32_t)(atoms.tri * atoms.slabs)), dim3(256), 0, st, (const double *)D, F, (uint32_t)atoms.slab_frames, (uint32_t)atoms.L,
                           (uint32_t)atoms.T, (uint32_t)atoms.tri, part);
        HIP_TRY(hipGetLastError());
        lap("dccm_gram");
        hipLaunchKernelGGL(k_dccm_var, dim3((uint32_t)((m_pad + kCovFinish - 1u) / kCovFinish)), dim3(256), 0, st, (const double *)part, (uint32_t)atoms.slabs, (uint32_t)atoms.T, (uint32_t)atoms.tri, F,
                           (uint32_t)m_pad, var);
        hipLaunchKernelGGL(k_dccm_finish, dim3((uint32_t)(atoms.tri * kCovFinishGroups)), dim3(256), 0, st, (const double *)part, (const double *)var, (uint32_t)atoms.slabs, (uint32_t)atoms.T,
                           (uint32_t)atoms.tri, F, (uint32_t)m, d_dccm);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out->dccm, d_dccm, m * m * 4u, hipMemcpyDeviceToHost, st));
        lap("dccm_finish");
    }
    HIP_TRY(hipStreamSynchronize(st));  // (the block is freed on return)
    return ARP_OK;
}

constexpr uint32_t kProjTile = 16;   // frames and modes of a workgroup of k_project: thread (frame t >> 4, mode t & 15) owns one projection
constexpr uint32_t kProjAtoms = 16;  // atoms (48 coordinates) of one step of its loop: thread (frame t >> 4, atom t & 15) forms that atom's deviation
constexpr uint32_t kProjLds = 49;    // LDS stride in doubles of a frame's deviations and of a mode's entries: sixteen rows 49 doubles apart start on sixteen different
                                     // even banks, so the sixteen modes one quarter wave reads at the same coordinate do not collide (a frame's value is a broadcast)

// Block (bx, by): frames 16 bx .. of the pass against modes 16 by ..  stage[fc][N][3] are the pass's absolute coordinates, tr[fc][12] its transforms (R
// row-major, then t), mean[m][3] and modes[k][3 m] atom-major.  A frame past fc, a mode past k and an atom past m are staged as zeros.  Plain f64
// multiply-adds, one accumulator per projection, in the order of the coordinate index a = 3 i + c: the sum's order is the definition's.
__global__ __launch_bounds__(256) void k_project(const double *__restrict__ stage, uint32_t N, uint64_t fc, const uint32_t *__restrict__ msel, uint32_t m, const double *__restrict__ tr,
                                                 const double *__restrict__ mean, const double *__restrict__ modes, uint32_t k, double *proj) {
    __shared__ double sd[kProjTile * kProjLds], sv[kProjTile * kProjLds];
    const uint32_t hi = threadIdx.x >> 4, lo = threadIdx.x & 15u;
    const uint64_t f = (uint64_t)blockIdx.x * kProjTile + hi;  // the frame of this thread, in both roles
    const uint32_t j = blockIdx.y * kProjTile + lo;
    double rt[12];
#pragma unroll
    for (int q = 0; q < 12; q++) rt[q] = f < fc ? tr[f * 12u + q] : 0.0;
    double acc = 0.0;
    for (uint32_t i0 = 0; i0 < m; i0 += kProjAtoms) {
        const uint32_t i = i0 + lo;
        double d[3] = {0.0, 0.0, 0.0};
        if (f < fc && i < m) {
            const double *p = stage + (f * N + msel[i]) * 3u;
            const double p0 = p[0], p1 = p[1], p2 = p[2];
#pragma unroll
            for (int c = 0; c < 3; c++) d[c] = (((rt[3 * c] * p0 + rt[3 * c + 1] * p1) + rt[3 * c + 2] * p2) + rt[9 + c]) - mean[3u * (size_t)i + c];
        }
#pragma unroll
        for (uint32_t c = 0; c < 3u; c++) sd[hi * kProjLds + 3u * lo + c] = d[c];
#pragma unroll
        for (uint32_t q = 0; q < 3u; q++) {  // mode hi of the tile, entries lo, lo + 16, lo + 32 of the step
            const uint32_t a = lo + 16u * q, jm = blockIdx.y * kProjTile + hi;
            sv[hi * kProjLds + a] = (jm < k && 3u * i0 + a < 3u * m) ? modes[(size_t)jm * 3u * m + 3u * i0 + a] : 0.0;
        }
        __syncthreads();
#pragma unroll 8
        for (uint32_t a = 0; a < 3u * kProjAtoms; a++) acc += sd[hi * kProjLds + a] * sv[lo * kProjLds + a];
        __syncthreads();
    }
    if (f < fc && j < k) proj[f * k + j] = acc;
}

// arp_project on the device: the frames go up in the passes of the rmsd calls, every pass is projected where it is staged.  The checks ran on the host.
arp_status device_project(arp_context *ctx, const ProjectJob &job, double *proj) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(context_device(ctx)));
    StreamLapTimer lap("  project %-10s %8.3f ms\n", st);
    const uint64_t N = job.n_atoms, F = job.n_frames, m = job.n_msel, k = job.k;
    if ((k + kProjTile - 1u) / kProjTile > 65535u) { set_error("project: %llu modes are more than one launch covers", (unsigned long long)k); return ARP_ERR_CAPACITY; }
    const uint64_t per = frames_per_pass(job.chunk_atoms, N, F);
    double *stage = nullptr, *tr = nullptr, *mean = nullptr, *modes = nullptr, *d_proj = nullptr; uint32_t *msel = nullptr;
    DevBlock block;
    if (arp_status s = block.carve([&](Bump &bp) {
            stage = bp.take<double>(per * N * 3u); tr = bp.take<double>(F * 12u); msel = bp.take<uint32_t>(m);
            mean = bp.take<double>(m * 3u); modes = bp.take<double>(k * 3u * m); d_proj = bp.take<double>(F * k); bp.take<char>(256);  // (slack)
        }); s != ARP_OK) return s;
    std::vector<double> identity;
    if (!job.transforms) {
        identity.assign(F * 12u, 0.0);
        for (uint64_t f = 0; f < F; f++) identity[f * 12u] = identity[f * 12u + 4u] = identity[f * 12u + 8u] = 1.0;
    }
    HIP_TRY(hipMemcpyAsync(tr, job.transforms ? job.transforms : identity.data(), F * 96u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(msel, job.msel, m * 4u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(mean, job.mean, m * 24u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(modes, job.modes, k * 3u * m * 8u, hipMemcpyHostToDevice, st));
    const uint32_t mode_tiles = (uint32_t)((k + kProjTile - 1u) / kProjTile);
    for (uint64_t f0 = 0; f0 < F; f0 += per) {
        const uint64_t fc = std::min<uint64_t>(per, F - f0);
        HIP_TRY(hipMemcpyAsync(stage, job.xyz + f0 * N * 3u, fc * N * 24u, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_project, dim3((uint32_t)((fc + kProjTile - 1u) / kProjTile), mode_tiles), dim3(256), 0, st, (const double *)stage, (uint32_t)N, fc, (const uint32_t *)msel,
                           (uint32_t)m, (const double *)tr + f0 * 12u, (const double *)mean, (const double *)modes, (uint32_t)k, d_proj + f0 * k);
        HIP_TRY(hipGetLastError());
    }
    lap("project");
    HIP_TRY(hipMemcpyAsync(proj, d_proj, F * k * 8u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lap("download");
    return ARP_OK;
}
