// RMSF and the mean structure: the frames of an ensemble superposed on a reference or on their own iterated mean (arp_rmsf).
// Included by table_dev.hip inside namespace arp, behind rmsd.inl, whose pack (k_rmsd_pack<true>: X[F][3][n_pad] of the fit atoms, XM[F][3][m_pad] of the
// measured atoms centred on the same centroid, C[F][3] the centroids), block sum and K(S) it uses.
//   k_rmsf_fit         per frame, one wave: the nine sums of S_f = sum_i x_f,i T_i^T against the resident target, cyclic Jacobi on K(S_f) with the
//                      eigenvectors accumulated (rmsd_jacobi_vec), the rotation R_f of the top eigenvector
//   k_rmsf_sweep       atom tiles x frame slabs: per atom the sum over the slab's frames, in their order, of R_f x_f,i (the mean) or of |R_f x_f,i - mean_i|^2
//   k_rmsf_mean_finish per (component, atom) the slabs, four interleaved runs in their order and a fixed tree, / F: M; per block the sum of (M - T)^2
//   k_rmsf_change      the blocks in a fixed tree: change = sqrt(sum / n), the one scalar the host reads per round
//   k_rmsf_dev_finish  per measured atom the slabs in the same order: rmsf, one rounding to f32
//   k_rmsf_frame       per frame, one wave: sqrt((1 / n) sum_i |R_f x_f,i - M_i|^2) over the fit atoms
//   k_rmsf_aligned     R_f x_f,i + c_T of the measured atoms of one download pass, atom-major
// These are F x 1 products: each frame meets one target, so a 16 x 16 MFMA tile would carry one useful column in sixteen; the sums are plain f64 FMA-free
// multiply-adds (the library is built with -ffp-contract=off) whose order depends on (F, n, m) alone -- lane strides, a fixed butterfly, slabs in order --
// and no floating-point atomic exists: two calls give identical bytes, whatever the upload pass size.

constexpr uint32_t kRmsfLanes = 64;      // lanes of a frame in k_rmsf_fit and k_rmsf_frame: one wave; lane l sums the atoms l, l + 64, ..
constexpr uint32_t kRmsfFitFrames = 4;   // frames (waves) of a workgroup of those two kernels
constexpr uint32_t kRmsfTile = 64;       // atoms of a tile of k_rmsf_sweep: one per lane of its one wave
constexpr uint32_t kRmsfSlab = 32;       // frames of a slab of k_rmsf_sweep
constexpr uint32_t kRmsfFinish = 64;     // items of a workgroup of the finish kernels: (component, atom) pairs of the mean, atoms of the deviations
constexpr uint32_t kRmsfFinishLanes = 4; // waves of such a workgroup: wave j sums the slabs j, j + 4, .. of its items
constexpr int kRmsfMean = 0, kRmsfDev = 1;

// the wave's sum in every lane: a butterfly of six exchanges, the same tree for every lane count (a + b and b + a are the same bits)
__device__ __forceinline__ double rmsf_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// rmsd_jacobi_top with the eigenvectors: the same sweeps, the rotations accumulated in v (columns).  Returns the column of the largest diagonal entry, the
// lowest index on ties: a unit top eigenvector, a deterministic one where the top eigenvalue is double.
__device__ __forceinline__ void rmsd_jacobi_vec(double (&a)[4][4], double (&q)[4]) {
    double v[4][4];
#pragma unroll
    for (int p = 0; p < 4; p++)
#pragma unroll
        for (int k = 0; k < 4; k++) v[p][k] = p == k ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 32; sweep++) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[0][3]) + fabs(a[1][2]) + fabs(a[1][3]) + fabs(a[2][3]);
        const double diag = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]) + fabs(a[3][3]);
        if (off <= 1e-300 || off <= 1e-19 * diag) break;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q2 = p + 1; q2 < 4; q2++) {
                const double apq = a[p][q2];
                if (fabs(apq) <= 1e-300) continue;
                const double theta = (a[q2][q2] - a[p][p]) / (2.0 * apq);
                const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                a[p][p] -= t * apq; a[q2][q2] += t * apq; a[p][q2] = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const double vx = v[k][p], vy = v[k][q2];
                    v[k][p] = cs * vx - sn * vy;
                    v[k][q2] = sn * vx + cs * vy;
                    if (k == p || k == q2) continue;
                    double &akp = k < p ? a[k][p] : a[p][k], &akq = k < q2 ? a[k][q2] : a[q2][k];
                    const double x = akp, y = akq;
                    akp = cs * x - sn * y;
                    akq = sn * x + cs * y;
                }
            }
    }
    int top = 0;
#pragma unroll
    for (int p = 1; p < 4; p++)
        if (a[p][p] > a[top][top]) top = p;
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = top == 0 ? v[k][0] : top == 1 ? v[k][1] : top == 2 ? v[k][2] : v[k][3];
}

// The proper rotation of the top eigenvector of K(S), S = sum_i x_i T_i^T: the R that minimises sum_i |R x_i - T_i|^2 (Horn 1987), row-major.
__device__ __forceinline__ void rmsf_rotation(const double (&s)[3][3], double (&r)[9]) {
    double a[4][4], q[4];
    a[0][0] = (s[0][0] + s[1][1]) + s[2][2];
    a[1][1] = (s[0][0] - s[1][1]) - s[2][2];
    a[2][2] = (-s[0][0] + s[1][1]) - s[2][2];
    a[3][3] = (-s[0][0] - s[1][1]) + s[2][2];
    a[0][1] = s[1][2] - s[2][1]; a[0][2] = s[2][0] - s[0][2]; a[0][3] = s[0][1] - s[1][0];
    a[1][2] = s[0][1] + s[1][0]; a[1][3] = s[2][0] + s[0][2]; a[2][3] = s[1][2] + s[2][1];
    rmsd_jacobi_vec(a, q);
    const double norm = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    const double w = q[0] / norm, x = q[1] / norm, y = q[2] / norm, z = q[3] / norm;
    r[0] = ((w * w + x * x) - y * y) - z * z; r[1] = 2.0 * (x * y - w * z);                r[2] = 2.0 * (x * z + w * y);
    r[3] = 2.0 * (y * x + w * z);               r[4] = ((w * w - x * x) + y * y) - z * z;  r[5] = 2.0 * (y * z - w * x);
    r[6] = 2.0 * (z * x - w * y);               r[7] = 2.0 * (z * y + w * x);              r[8] = ((w * w - x * x) - y * y) + z * z;
}

// Wave w of the block: frame f = 4 block + w against the target T[3][n_pad] (padding: zeros in both).  Every lane ends with the same nine sums and runs the
// same eigen-solve; lane 0 writes R[f][9].
__global__ __launch_bounds__(256) void k_rmsf_fit(const double *__restrict__ X, const double *__restrict__ T, uint32_t F, uint32_t n_pad, double *R) {
    const uint32_t lane = threadIdx.x & 63u, f = blockIdx.x * kRmsfFitFrames + (threadIdx.x >> 6);
    if (f >= F) return;  // (the whole wave; the kernel has no barrier)
    const double *x = X + (size_t)f * 3u * n_pad;
    double s[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    for (uint32_t i = lane; i < n_pad; i += kRmsfLanes) {
        const double a[3] = {x[i], x[(size_t)n_pad + i], x[2u * (size_t)n_pad + i]};
        const double b[3] = {T[i], T[(size_t)n_pad + i], T[2u * (size_t)n_pad + i]};
#pragma unroll
        for (int u = 0; u < 3; u++)
#pragma unroll
            for (int v = 0; v < 3; v++) s[u][v] += a[u] * b[v];
    }
#pragma unroll
    for (int u = 0; u < 3; u++)
#pragma unroll
        for (int v = 0; v < 3; v++) s[u][v] = rmsf_wave_sum(s[u][v]);
    double r[9];
    rmsf_rotation(s, r);
    if (lane == 0u)
#pragma unroll
        for (int k = 0; k < 9; k++) R[(size_t)f * 9u + k] = r[k];
}

// Block b: tile b % tiles of the atoms, slab b / tiles of the frames.  Lane i of the tile walks the slab's frames in their order.
//   kRmsfMean  part[slab][3][n_pad] = sum_f R_f x_f,i
//   kRmsfDev   part[slab][n_pad]    = sum_f |R_f x_f,i - mean_i|^2, mean[3][n_pad]
template <int kOp>
__global__ __launch_bounds__(64) void k_rmsf_sweep(const double *__restrict__ X, const double *__restrict__ R, const double *__restrict__ mean, uint32_t F, uint32_t n_pad,
                                                  uint32_t tiles, double *part) {
    const uint32_t slab = blockIdx.x / tiles, i = (blockIdx.x % tiles) * kRmsfTile + threadIdx.x;
    if (i >= n_pad) return;
    const uint32_t f0 = slab * kRmsfSlab, f1 = min(F, f0 + kRmsfSlab);
    double acc[3] = {0.0, 0.0, 0.0}, mu[3] = {0.0, 0.0, 0.0};
    if (kOp == kRmsfDev)
        for (int k = 0; k < 3; k++) mu[k] = mean[(size_t)k * n_pad + i];
    for (uint32_t f = f0; f < f1; f++) {
        const double *x = X + (size_t)f * 3u * n_pad + i, *r = R + (size_t)f * 9u;
        const double x0 = x[0], x1 = x[n_pad], x2 = x[2u * (size_t)n_pad];
        double y[3];
#pragma unroll
        for (int k = 0; k < 3; k++) y[k] = (r[3 * k] * x0 + r[3 * k + 1] * x1) + r[3 * k + 2] * x2;
        if (kOp == kRmsfMean) {
#pragma unroll
            for (int k = 0; k < 3; k++) acc[k] += y[k];
        } else {
            const double d0 = y[0] - mu[0], d1 = y[1] - mu[1], d2 = y[2] - mu[2];
            acc[0] += (d0 * d0 + d1 * d1) + d2 * d2;
        }
    }
    if (kOp == kRmsfMean) {
#pragma unroll
        for (int k = 0; k < 3; k++) part[((size_t)slab * 3u + k) * n_pad + i] = acc[k];
    } else {
        part[(size_t)slab * n_pad + i] = acc[0];
    }
}

// Wave j of a finish workgroup sums, for each of the workgroup's 64 items, the slabs j, j + 4, .. in that order; the four waves meet in a fixed tree.
__device__ __forceinline__ double rmsf_slab_sum(const double *__restrict__ part, uint32_t slabs, uint64_t items, uint32_t e, double *red) {
    double s = 0.0;
    if (e < items)
        for (uint32_t b = threadIdx.x >> 6; b < slabs; b += kRmsfFinishLanes) s += part[(size_t)b * items + e];
    red[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t off = 128u; off >= kRmsfFinish; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    return red[threadIdx.x & 63u];  // (read by the first wave only)
}

// M[3][n_pad] = the slabs of part, / F; an item is one (component, atom), 3 n_pad of them.  T given: block_d2[block] = the sum over the block's items of the
// squares of M - T, padding left out, in a fixed tree (M and T are two buffers).
__global__ __launch_bounds__(256) void k_rmsf_mean_finish(const double *__restrict__ part, uint32_t slabs, uint32_t F, uint32_t n, uint32_t n_pad, const double *__restrict__ T,
                                                          double *M, double *block_d2) {
    __shared__ double red[256];
    const uint32_t items = 3u * n_pad, e = blockIdx.x * kRmsfFinish + (threadIdx.x & 63u);
    const double s = rmsf_slab_sum(part, slabs, items, e, red);
    double d2 = 0.0;
    if (threadIdx.x < kRmsfFinish && e < items) {
        const double mk = s / (double)F;
        M[e] = mk;
        if (T && e % n_pad < n) {
            const double d = mk - T[e];
            d2 = d * d;
        }
    }
    if (!T) return;  // (the whole block)
    __syncthreads();
    if (threadIdx.x < kRmsfFinish) red[threadIdx.x] = d2;
    __syncthreads();
    for (uint32_t off = kRmsfFinish / 2u; off; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0u) block_d2[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void k_rmsf_change(const double *__restrict__ block_d2, uint32_t blocks, uint32_t n, double *change) {
    __shared__ double red[256];
    double v = 0.0;
    for (uint32_t b = threadIdx.x; b < blocks; b += 256u) v += block_d2[b];
    v = rmsd_block_sum(v, red);
    if (threadIdx.x == 0u) *change = sqrt(v / (double)n);
}

// rmsf[i] of the m measured atoms (the items) from part[slab][m_pad]
__global__ __launch_bounds__(256) void k_rmsf_dev_finish(const double *__restrict__ part, uint32_t slabs, uint32_t F, uint32_t m, uint32_t m_pad, float *rmsf) {
    __shared__ double red[256];
    const uint32_t e = blockIdx.x * kRmsfFinish + (threadIdx.x & 63u);
    const double s = rmsf_slab_sum(part, slabs, m_pad, e, red);
    if (threadIdx.x < kRmsfFinish && e < m) rmsf[e] = (float)sqrt(s / (double)F);
}

__global__ __launch_bounds__(256) void k_rmsf_frame(const double *__restrict__ X, const double *__restrict__ R, const double *__restrict__ M, uint32_t F, uint32_t n, uint32_t n_pad,
                                                    float *out) {
    const uint32_t lane = threadIdx.x & 63u, f = blockIdx.x * kRmsfFitFrames + (threadIdx.x >> 6);
    if (f >= F) return;  // (the whole wave)
    const double *x = X + (size_t)f * 3u * n_pad, *r = R + (size_t)f * 9u;
    double s = 0.0;
    for (uint32_t i = lane; i < n; i += kRmsfLanes) {
        const double x0 = x[i], x1 = x[(size_t)n_pad + i], x2 = x[2u * (size_t)n_pad + i];
        double d[3];
#pragma unroll
        for (int k = 0; k < 3; k++) d[k] = ((r[3 * k] * x0 + r[3 * k + 1] * x1) + r[3 * k + 2] * x2) - M[(size_t)k * n_pad + i];
        s += (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    }
    s = rmsf_wave_sum(s);
    if (lane == 0u) out[f] = (float)sqrt(s / (double)n);
}

// out[fc][m][3] of the frames f0 .. f0 + fc - 1 (XM and R already offset to f0): R_f x_f,i + c_T, which is R_f (absolute) + t_f
__global__ __launch_bounds__(256) void k_rmsf_aligned(const double *__restrict__ XM, const double *__restrict__ R, const double *__restrict__ c_t, uint64_t fc, uint32_t m, uint32_t m_pad,
                                                      double *out) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= fc * m) return;
    const uint64_t f = idx / m;
    const uint32_t i = (uint32_t)(idx % m);
    const double *x = XM + f * 3u * m_pad + i, *r = R + f * 9u;
    const double x0 = x[0], x1 = x[m_pad], x2 = x[2u * (size_t)m_pad];
#pragma unroll
    for (int k = 0; k < 3; k++) out[idx * 3u + k] = ((r[3 * k] * x0 + r[3 * k + 1] * x1) + r[3 * k + 2] * x2) + c_t[k];
}

arp_status device_cov(hipStream_t st, StreamLapTimer &lap, const double *XM, const double *R, const double *mean_m, uint64_t F, uint64_t m, uint64_t m_pad, RmsfOut *out);  // cov.inl

// The call on the device.  Upload and pack as device_rmsd does; X, XM, C and the rotations stay resident.  Then the rounds -- fit, sweep, finish, change, one
// 8-byte read-back -- the measured atoms' mean and deviations under the last rotations, and the downloads; aligned goes through the staging buffer in the
// upload passes' sizes.  The capacity checks ran on the host (rmsf.cpp) before this is called.
arp_status device_rmsf(arp_context *ctx, const RmsfJob &job, RmsfOut *out) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(context_device(ctx)));
    StreamLapTimer lap("  rmsf %-10s %8.3f ms\n", st);
    const uint64_t N = job.n_atoms, F = job.n_frames, n = job.n_sel, n_pad = rmsd_n_pad(n);
    const bool own = job.msel != nullptr;  // a measured set of its own
    const uint64_t m = own ? job.n_msel : n, m_pad = rmsd_n_pad(m), w_pad = std::max(n_pad, m_pad);
    const uint64_t per = frames_per_pass(job.chunk_atoms, N, F);
    const uint64_t slabs = (F + kRmsfSlab - 1u) / kRmsfSlab, fin_n = (3u * n_pad + kRmsfFinish - 1u) / kRmsfFinish, fin_m = (3u * m_pad + kRmsfFinish - 1u) / kRmsfFinish,
                   fin_dev = (m_pad + kRmsfFinish - 1u) / kRmsfFinish;
    const uint64_t tiles_n = (n_pad + kRmsfTile - 1u) / kRmsfTile, tiles_m = (m_pad + kRmsfTile - 1u) / kRmsfTile;
    if (slabs * std::max(tiles_n, tiles_m) >= (1ull << 31)) { set_error("rmsf: %llu frames x %llu atoms are more than one launch covers", (unsigned long long)F, (unsigned long long)std::max(n, m)); return ARP_ERR_CAPACITY; }
    double *X = nullptr, *G = nullptr, *XM = nullptr, *C = nullptr, *stage = nullptr, *XR = nullptr, *GR = nullptr, *CR = nullptr, *R = nullptr, *M2[2] = {nullptr, nullptr};
    double *MM = nullptr, *part = nullptr, *block_d2 = nullptr, *d_change = nullptr; uint32_t *sel = nullptr, *msel = nullptr; float *d_rmsf = nullptr, *d_frame = nullptr;
    DevBlock block;
    if (arp_status s = block.carve([&](Bump &bp) {
            X = bp.take<double>(F * 3u * n_pad); G = bp.take<double>(F); sel = bp.take<uint32_t>(n); msel = bp.take<uint32_t>(m);
            XM = own ? bp.take<double>(F * 3u * m_pad) : X; C = bp.take<double>(F * 3u);
            stage = bp.take<double>(per * N * 3u); XR = bp.take<double>(3u * n_pad); GR = bp.take<double>(1); CR = bp.take<double>(3); R = bp.take<double>(F * 9u);
            for (double *&p : M2) p = bp.take<double>(3u * n_pad);
            MM = bp.take<double>(3u * m_pad); part = bp.take<double>(slabs * 3u * w_pad); block_d2 = bp.take<double>(fin_n); d_change = bp.take<double>(1);
            d_rmsf = bp.take<float>(m); d_frame = bp.take<float>(F); bp.take<char>(256);  // (slack)
        }); s != ARP_OK) return s;
    HIP_TRY(hipMemcpyAsync(sel, job.sel, n * 4u, hipMemcpyHostToDevice, st));
    if (own) HIP_TRY(hipMemcpyAsync(msel, job.msel, m * 4u, hipMemcpyHostToDevice, st));
    for (uint64_t f0 = 0; f0 < F; f0 += per) {
        const uint64_t fc = std::min<uint64_t>(per, F - f0);
        HIP_TRY(hipMemcpyAsync(stage, job.xyz + f0 * N * 3u, fc * N * 24u, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_rmsd_pack<true>, dim3((uint32_t)fc), dim3(256), 0, st, (const double *)stage, (uint32_t)N, (const uint32_t *)sel, (uint32_t)n, (uint32_t)n_pad,
                           X + f0 * 3u * n_pad, G + f0, (const uint32_t *)msel, own ? (uint32_t)m : 0u, own ? (uint32_t)m_pad : 0u, own ? XM + f0 * 3u * m_pad : (double *)nullptr,
                           C + f0 * 3u);
        HIP_TRY(hipGetLastError());
    }
    if (job.ref_xyz) {
        HIP_TRY(hipMemcpyAsync(stage, job.ref_xyz, N * 24u, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_rmsd_pack<true>, dim3(1), dim3(256), 0, st, (const double *)stage, (uint32_t)N, (const uint32_t *)sel, (uint32_t)n, (uint32_t)n_pad, XR, GR,
                           (const uint32_t *)msel, 0u, 0u, (double *)nullptr, CR);
        HIP_TRY(hipGetLastError());
    }
    lap("pack");
    const double *T = job.ref_xyz ? XR : X + job.ref_frame * 3u * n_pad, *c_t = job.ref_xyz ? CR : C + job.ref_frame * 3u;
    const dim3 per_frame((uint32_t)((F + kRmsfFitFrames - 1u) / kRmsfFitFrames));
    double *M = nullptr, change = 0.0;
    uint32_t round = 0;
    for (;;) {
        round++;
        M = M2[round & 1u];
        hipLaunchKernelGGL(k_rmsf_fit, per_frame, dim3(256), 0, st, (const double *)X, T, (uint32_t)F, (uint32_t)n_pad, R);
        lap("fit");  // (a lap drains the stream only with the `timing` knob on; the laps of every round carry the same names)
        hipLaunchKernelGGL(k_rmsf_sweep<kRmsfMean>, dim3((uint32_t)(slabs * tiles_n)), dim3(64), 0, st, (const double *)X, (const double *)R, (const double *)nullptr, (uint32_t)F,
                           (uint32_t)n_pad, (uint32_t)tiles_n, part);
        lap("sweep");
        hipLaunchKernelGGL(k_rmsf_mean_finish, dim3((uint32_t)fin_n), dim3(256), 0, st, (const double *)part, (uint32_t)slabs, (uint32_t)F, (uint32_t)n, (uint32_t)n_pad, T, M, block_d2);
        hipLaunchKernelGGL(k_rmsf_change, dim3(1), dim3(256), 0, st, (const double *)block_d2, (uint32_t)fin_n, (uint32_t)n, d_change);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&change, d_change, 8u, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        lap("finish");
        if (round == job.max_rounds || change <= job.tol) break;
        T = M;
    }
    const double *mean_m = M;
    if (own) {
        hipLaunchKernelGGL(k_rmsf_sweep<kRmsfMean>, dim3((uint32_t)(slabs * tiles_m)), dim3(64), 0, st, (const double *)XM, (const double *)R, (const double *)nullptr, (uint32_t)F,
                           (uint32_t)m_pad, (uint32_t)tiles_m, part);
        hipLaunchKernelGGL(k_rmsf_mean_finish, dim3((uint32_t)fin_m), dim3(256), 0, st, (const double *)part, (uint32_t)slabs, (uint32_t)F, (uint32_t)m, (uint32_t)m_pad,
                           (const double *)nullptr, MM, (double *)nullptr);
        mean_m = MM;
    }
    hipLaunchKernelGGL(k_rmsf_sweep<kRmsfDev>, dim3((uint32_t)(slabs * tiles_m)), dim3(64), 0, st, (const double *)XM, (const double *)R, mean_m, (uint32_t)F, (uint32_t)m_pad,
                       (uint32_t)tiles_m, part);
    hipLaunchKernelGGL(k_rmsf_dev_finish, dim3((uint32_t)fin_dev), dim3(256), 0, st, (const double *)part, (uint32_t)slabs, (uint32_t)F, (uint32_t)m, (uint32_t)m_pad, d_rmsf);
    hipLaunchKernelGGL(k_rmsf_frame, per_frame, dim3(256), 0, st, (const double *)X, (const double *)R, (const double *)M, (uint32_t)F, (uint32_t)n, (uint32_t)n_pad, d_frame);
    HIP_TRY(hipGetLastError());
    lap("deviation");
    if (out->cov || out->dccm) {  // arp_covariance: the second moments of the same deviations (cov.inl)
        const arp_status cs = device_cov(st, lap, XM, R, mean_m, F, m, m_pad, out);
        if (cs != ARP_OK) return cs;
    }
    std::vector<double> h_mean(3u * m_pad), h_c(F * 3u), h_r(out->transforms ? F * 9u : 0u);
    double h_ct[3];
    HIP_TRY(hipMemcpyAsync(h_mean.data(), mean_m, 3u * m_pad * 8u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_ct, c_t, 24u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->rmsf, d_rmsf, m * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->frame_rmsd, d_frame, F * 4u, hipMemcpyDeviceToHost, st));
    if (out->transforms) {
        HIP_TRY(hipMemcpyAsync(h_c.data(), C, F * 24u, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h_r.data(), R, F * 72u, hipMemcpyDeviceToHost, st));
    }
    if (out->aligned)
        for (uint64_t f0 = 0; f0 < F; f0 += per) {  // stage holds per x N x 3 doubles, m <= N
            const uint64_t fc = std::min<uint64_t>(per, F - f0);
            hipLaunchKernelGGL(k_rmsf_aligned, dim3((uint32_t)((fc * m + 255u) / 256u)), dim3(256), 0, st, (const double *)XM + f0 * 3u * m_pad, (const double *)R + f0 * 9u, c_t, fc,
                               (uint32_t)m, (uint32_t)m_pad, stage);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(out->aligned + f0 * m * 3u, stage, fc * m * 24u, hipMemcpyDeviceToHost, st));
        }
    HIP_TRY(hipStreamSynchronize(st));
    for (uint64_t i = 0; i < m; i++)
        for (int k = 0; k < 3; k++) out->mean[3u * i + k] = h_mean[(size_t)k * m_pad + i] + h_ct[k];
    if (out->transforms)
        for (uint64_t f = 0; f < F; f++) {
            double *t = out->transforms + f * 12u;
            const double *r = h_r.data() + f * 9u, *c = h_c.data() + f * 3u;
            for (int k = 0; k < 9; k++) t[k] = r[k];
            for (int k = 0; k < 3; k++) t[9 + k] = h_ct[k] - ((r[3 * k] * c[0] + r[3 * k + 1] * c[1]) + r[3 * k + 2] * c[2]);
        }
    out->n_rounds = round;
    out->last_change = change;
    lap("download");
    return ARP_OK;
}
