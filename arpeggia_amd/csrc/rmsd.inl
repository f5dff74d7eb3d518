// RMSD between the frames of an ensemble after optimal superposition (arp_rmsd_matrix, arp_rmsd_reference, arp_rmsd_clusters).
// Included by table_dev.hip inside namespace arp, behind cluster.inl.
//
// For a pair of frames (f, g) the 3 x 3 cross-covariance S = sum_i x_f,i x_g,i^T of the centred selected atoms is one 3 x 3 block of the f64 product
// (3F x n) . (n x 3F); the rmsd follows from the largest eigenvalue of Horn's 4 x 4 matrix K(S) (include/arpeggia_amd.h):
//   k_rmsd_pack        per frame of an upload pass: gather the selection, f64 centroid, centre, G_f = sum |x|^2, X[F][3][n_pad] component-major, zero padded
//   k_rmsd_gram        the tile loop over the upper triangle of F x F on v_mfma_f64_16x16x4_f64, the eigenvalue per pair in registers, and one of three ends:
//                      the f32 matrix and its mirror; the neighbour bits adj[F][ceil(F / 32)] of rmsd <= cutoff in k_bit_adjacency's layout; one row against a
//                      packed reference
//   k_rmsd_to_centre   after the rounds of cluster.inl on those neighbour bits: rmsd(f, centre of f's cluster), the matrix entry's bits
// A pair's products are summed in the order of the atoms, four per MFMA, whatever tile, pass or kernel the pair falls in; a step of padding adds zeros.  The
// bit-equalities between the three calls rest on that, and on the eigenvalue iteration being an odd function of the antisymmetric part of S (S^T for S).

constexpr uint32_t kRmsdTile = 32;    // frames of a workgroup tile edge: 2 x 2 waves of 16 x 16 pairs each; a tile row is one word of neighbour bits
constexpr uint32_t kRmsdStep = 4;     // atoms per MFMA (the K of 16x16x4); n_pad is n rounded up to it (table_dev.h rmsd_n_pad)
constexpr uint32_t kRmsdChunk = 16;   // atoms staged through LDS per step of the tile loop
constexpr uint32_t kRmsdLds = 20;     // LDS stride in doubles of one (frame, component) row: a frame's stride is 60 = -4 mod 32, so the sixteen frames x four atoms
                                      // of one operand read fall on all 32 eight-byte slots of the bank row, twice
constexpr uint32_t kRmsdRows = 3u * kRmsdTile;  // (frame, component) rows of one operand of a tile
constexpr uint32_t kRmsdMirror = kRmsdTile + 1u;  // row stride of the epilogue's tile image: its transposed reads walk the banks
constexpr int kRmsdMatrix = 0, kRmsdAdjacency = 1, kRmsdRow = 2;  // the three ends of k_rmsd_gram
static_assert(rmsd_n_pad(1) == kRmsdStep && kRmsdChunk % kRmsdStep == 0, "n_pad is a multiple of the MFMA step, the chunk a whole number of steps");

typedef double rmsd_acc __attribute__((ext_vector_type(4)));  // the four f64 results of a lane: C/D col = lane & 15, row = (lane >> 4) + 4 reg

// Block f: frame f of the pass, N atoms x 3 doubles at xyz.  Every lane sums its atoms i = lane, lane + 256, .. in that order, the 256 partial sums meet in
// a fixed tree: the centroid, G and X do not depend on which pass the frame was uploaded in.
__device__ inline double rmsd_block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t off = 128u; off; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}
// kMeasured (rmsf.inl): the centring is refined (below), the frame's centroid goes to C[f][3] as well, and the m atoms of msel, centred on that same
// centroid of the fit atoms, to XM[F][3][m_pad].  The arp_rmsd_* calls instantiate kMeasured = false: nothing of theirs changes.
template <bool kMeasured>
__global__ __launch_bounds__(256) void k_rmsd_pack(const double *xyz, uint32_t N, const uint32_t *__restrict__ sel, uint32_t n, uint32_t n_pad, double *X, double *G,
                                                   const uint32_t *__restrict__ msel, uint32_t m, uint32_t m_pad, double *XM, double *C) {
    __shared__ double red[256];
    const double *frame = xyz + (size_t)blockIdx.x * N * 3u;
    double *out = X + (size_t)blockIdx.x * 3u * n_pad;
    double c[3] = {0.0, 0.0, 0.0};
    for (uint32_t i = threadIdx.x; i < n; i += 256u) {
        const double *p = frame + (size_t)sel[i] * 3u;
        c[0] += p[0]; c[1] += p[1]; c[2] += p[2];
    }
    for (int k = 0; k < 3; k++) c[k] = rmsd_block_sum(c[k], red) / (double)n;
    double g = 0.0;
    for (uint32_t i = threadIdx.x; i < n_pad; i += 256u) {
        double d[3] = {0.0, 0.0, 0.0};
        if (i < n) {
            const double *p = frame + (size_t)sel[i] * 3u;
            for (int k = 0; k < 3; k++) d[k] = p[k] - c[k];
        }
        g += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        for (int k = 0; k < 3; k++) out[(size_t)k * n_pad + i] = d[k];
    }
    g = rmsd_block_sum(g, red);
    if (threadIdx.x == 0u) G[blockIdx.x] = g;
    if (kMeasured) {
        // A second centring: c carries the rounding of a sum of absolute coordinates (10^-11 A for a frame 10^5 A from the origin), which would move the
        // whole frame against the others.  r = the centroid of the centred atoms is that error, known to the rounding of the small x; the frame's centroid
        // is c + r and x - r is centred to eps |x|.  (Each lane rereads what it wrote itself.)
        double r[3];
        for (int k = 0; k < 3; k++) {
            double s = 0.0;
            for (uint32_t i = threadIdx.x; i < n; i += 256u) s += out[(size_t)k * n_pad + i];
            r[k] = rmsd_block_sum(s, red) / (double)n;
        }
        g = 0.0;
        for (uint32_t i = threadIdx.x; i < n; i += 256u) {
            double d[3];
            for (int k = 0; k < 3; k++) out[(size_t)k * n_pad + i] = d[k] = out[(size_t)k * n_pad + i] - r[k];
            g += d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        }
        g = rmsd_block_sum(g, red);
        if (threadIdx.x == 0u) G[blockIdx.x] = g;
        if (threadIdx.x == 0u)
            for (int k = 0; k < 3; k++) C[(size_t)blockIdx.x * 3u + k] = c[k] + r[k];
        double *outm = XM + (size_t)blockIdx.x * 3u * m_pad;
        for (uint32_t i = threadIdx.x; i < m_pad; i += 256u) {
            double d[3] = {0.0, 0.0, 0.0};
            if (i < m) {
                const double *p = frame + (size_t)msel[i] * 3u;
                for (int k = 0; k < 3; k++) d[k] = (p[k] - c[k]) - r[k];
            }
            for (int k = 0; k < 3; k++) outm[(size_t)k * m_pad + i] = d[k];
        }
    }
}

// The largest eigenvalue of the symmetric 4 x 4 matrix a (its upper triangle) by cyclic Jacobi rotations: every rotation is backward stable whatever the gaps
// between the eigenvalues, so a double top eigenvalue (planar, collinear, mirror-image and n <= 3 selections) costs no accuracy.  Negating a[0][1 .. 3] (K of
// S^T) negates those entries in every later step and leaves the diagonal's bits alone.
__device__ __forceinline__ double rmsd_jacobi_top(double (&a)[4][4]) {
    for (int sweep = 0; sweep < 32; sweep++) {
        const double off = fabs(a[0][1]) + fabs(a[0][2]) + fabs(a[0][3]) + fabs(a[1][2]) + fabs(a[1][3]) + fabs(a[2][3]);
        const double diag = fabs(a[0][0]) + fabs(a[1][1]) + fabs(a[2][2]) + fabs(a[3][3]);
        if (off <= 1e-300 || off <= 1e-19 * diag) break;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                const double apq = a[p][q];
                if (fabs(apq) <= 1e-300) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                a[p][p] -= t * apq; a[q][q] += t * apq; a[p][q] = 0.0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (k == p || k == q) continue;
                    double &akp = k < p ? a[k][p] : a[p][k], &akq = k < q ? a[k][q] : a[q][k];
                    const double x = akp, y = akq;
                    akp = cs * x - sn * y;
                    akq = sn * x + cs * y;
                }
            }
    }
    return fmax(fmax(a[0][0], a[1][1]), fmax(a[2][2], a[3][3]));
}

// rmsd of one pair from its S (s[a][b] = sum_i x_f,a x_g,b), G_f + G_g and n: Horn's K(S) as the header writes it out, its top eigenvalue, one rounding to f32
__device__ __forceinline__ float rmsd_of_pair(const double (&s)[3][3], double g_sum, uint32_t n) {
    double a[4][4];
    a[0][0] = (s[0][0] + s[1][1]) + s[2][2];
    a[1][1] = (s[0][0] - s[1][1]) - s[2][2];
    a[2][2] = (-s[0][0] + s[1][1]) - s[2][2];
    a[3][3] = (-s[0][0] - s[1][1]) + s[2][2];
    a[0][1] = s[1][2] - s[2][1]; a[0][2] = s[2][0] - s[0][2]; a[0][3] = s[0][1] - s[1][0];
    a[1][2] = s[0][1] + s[1][0]; a[1][3] = s[2][0] + s[0][2]; a[2][3] = s[1][2] + s[2][1];
    const double lambda = rmsd_jacobi_top(a);
    const double msd = fmax(0.0, (g_sum - 2.0 * lambda) / (double)n);
    return (float)sqrt(msd);
}

// Tile (ti, tj) of the upper triangle as in k_bit_gram (kRmsdRow: the tiles of one row, ti = 0): frames row0 .. of XA against frames col0 .. of XB.  Wave
// (wi, wj) of the 2 x 2 owns the pairs (16 wi + r, 16 wj + c); with the rows of both operands ordered component-major the nine accumulators acc[a][b] hold
// S_ab of pair (r = (lane >> 4) + 4 reg, c = lane & 15) in the same lane and register: the epilogue runs per lane on its four pairs, without a shuffle.  The
// 96 + 96 (frame, component) rows go through LDS in chunks of kRmsdChunk atoms; the next chunk is fetched into registers while the current one is consumed.
// Frames past MA / MB and atoms past n_pad are staged as zeros.
//   kRmsdMatrix     out[MA x MB] (MA = MB, XA = XB): the tile, and off the diagonal its mirror through an LDS image; the diagonal is written 0.0f
//   kRmsdAdjacency  adj[MA][KA]: bit c of word tj of row r <=> rmsd <= cutoff (f32, inclusive; the diagonal set, pairs past MA clear), and the mirror word
//   kRmsdRow        out[MB]: row 0 of the tile (MA = 1: XA is one packed reference); out[self] = 0.0f when the reference is frame `self`, ARP_NONE: none is
template <int kEnd>
__global__ __launch_bounds__(256) void k_rmsd_gram(const double *__restrict__ XA, const double *__restrict__ GA, uint32_t MA, const double *__restrict__ XB,
                                                   const double *__restrict__ GB, uint32_t MB, uint32_t n, uint32_t n_pad, uint32_t T, float cutoff, uint32_t self, float *out,
                                                   uint32_t *adj, uint64_t KA) {
    static_assert(2u * kRmsdRows * kRmsdLds * 8u >= kRmsdTile * kRmsdMirror * 4u, "the epilogue's tile image reuses the staging buffer");
    __shared__ __attribute__((aligned(16))) double lds[2u * kRmsdRows * kRmsdLds];
    uint32_t t = blockIdx.x, ti = 0;
    if (kEnd != kRmsdRow)
        while (t >= T - ti) { t -= T - ti; ti++; }
    const uint32_t tj = ti + t;
    const uint32_t row0 = ti * kRmsdTile, col0 = tj * kRmsdTile;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, wi = wave >> 1, wj = wave & 1u;
    const uint32_t c = lane & 15u, h = lane >> 4;
    double *sA = lds, *sB = lds + kRmsdRows * kRmsdLds;
    const uint32_t lk = threadIdx.x & 15u, lr = threadIdx.x >> 4;  // staging: atom lk of rows lr, lr + 16, ..
    double ra[6], rb[6];
    auto fetch = [&](uint32_t k0) {
        const uint32_t k = k0 + lk;
#pragma unroll
        for (uint32_t i = 0; i < 6u; i++) {
            const uint32_t r = lr + 16u * i;  // row r: frame r / 3, component r % 3 -- row 3 frame + component of X
            ra[i] = (row0 + r / 3u < MA && k < n_pad) ? XA[((size_t)row0 * 3u + r) * n_pad + k] : 0.0;
            rb[i] = (col0 + r / 3u < MB && k < n_pad) ? XB[((size_t)col0 * 3u + r) * n_pad + k] : 0.0;
        }
    };
    rmsd_acc acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) acc[a][b] = rmsd_acc{0.0, 0.0, 0.0, 0.0};
    fetch(0);
    for (uint32_t k0 = 0; k0 < n_pad; k0 += kRmsdChunk) {
#pragma unroll
        for (uint32_t i = 0; i < 6u; i++) {
            sA[(lr + 16u * i) * kRmsdLds + lk] = ra[i];
            sB[(lr + 16u * i) * kRmsdLds + lk] = rb[i];
        }
        __syncthreads();
        if (k0 + kRmsdChunk < n_pad) fetch(k0 + kRmsdChunk);
#pragma unroll
        for (uint32_t kk = 0; kk < kRmsdChunk; kk += kRmsdStep) {
            if (k0 + kk >= n_pad) break;  // (the whole block)
            double a[3], b[3];
#pragma unroll
            for (uint32_t x = 0; x < 3u; x++) {
                a[x] = sA[((16u * wi + c) * 3u + x) * kRmsdLds + kk + h];
                b[x] = sB[((16u * wj + c) * 3u + x) * kRmsdLds + kk + h];
            }
#pragma unroll
            for (int x = 0; x < 3; x++)
#pragma unroll
                for (int y = 0; y < 3; y++) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b[y], acc[x][y], 0, 0, 0);
        }
        __syncthreads();
    }
    // the epilogue: pair (fr, gc) of register reg
    const uint32_t gc = col0 + 16u * wj + c;
    const double g_col = gc < MB ? GB[gc] : 0.0;
    float v[4];
    bool inside[4];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const uint32_t fr = row0 + 16u * wi + h + 4u * (uint32_t)reg;
        inside[reg] = fr < MA && gc < MB;
        v[reg] = 0.0f;
        const bool same = kEnd == kRmsdRow ? gc == self : fr == gc;
        if (kEnd == kRmsdRow && fr != 0u) inside[reg] = false;
        if (inside[reg] && !same) {
            double s[3][3];
#pragma unroll
            for (int x = 0; x < 3; x++)
#pragma unroll
                for (int y = 0; y < 3; y++) s[x][y] = acc[x][y][reg];
            v[reg] = rmsd_of_pair(s, GA[fr] + g_col, n);
        }
    }
    if (kEnd == kRmsdRow) {
        if (inside[0]) out[gc] = v[0];
        return;
    }
    if (kEnd == kRmsdMatrix) {
        float *image = reinterpret_cast<float *>(lds);  // [kRmsdTile][kRmsdMirror]
#pragma unroll
        for (int reg = 0; reg < 4; reg++) {
            const uint32_t rl = 16u * wi + h + 4u * (uint32_t)reg;
            if (inside[reg]) out[(size_t)(row0 + rl) * MB + gc] = v[reg];
            image[rl * kRmsdMirror + 16u * wj + c] = v[reg];
        }
        if (ti != tj) {
            __syncthreads();
            const uint32_t rr = threadIdx.x & 31u;
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++) {
                const uint32_t cc = (threadIdx.x >> 5) + 8u * i;
                if (col0 + cc < MB && row0 + rr < MA) out[(size_t)(col0 + cc) * MB + row0 + rr] = image[rr * kRmsdMirror + cc];
            }
        }
        return;
    }
    // kRmsdAdjacency: the ballot of register reg carries, in bits 16 h .. 16 h + 15, the sixteen columns of row 4 reg + h of the wave; the two waves of a
    // row put the halves of its word together in LDS
    uint16_t *half = reinterpret_cast<uint16_t *>(lds);  // [kRmsdTile][2]
    const uint32_t *image = reinterpret_cast<const uint32_t *>(lds);
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const uint32_t fr = row0 + 16u * wi + h + 4u * (uint32_t)reg;
        const bool pass = inside[reg] && (fr == gc || v[reg] <= cutoff);
        const unsigned long long votes = __ballot(pass);
        if (c == 0u) half[(16u * wi + h + 4u * (uint32_t)reg) * 2u + wj] = (uint16_t)(votes >> (16u * h));
    }
    __syncthreads();
    if (threadIdx.x < kRmsdTile) {
        const uint32_t r = threadIdx.x;
        if (row0 + r < MA) adj[(size_t)(row0 + r) * KA + tj] = image[r];
        if (ti != tj && col0 + r < MA) {  // column r of the tile is row col0 + r of the mirror tile
            uint32_t m = 0;
#pragma unroll 8
            for (uint32_t k = 0; k < kRmsdTile; k++) m |= (image[k] >> r & 1u) << k;
            adj[(size_t)(col0 + r) * KA + ti] = m;
        }
    }
}

// One wave per sixteen frames: pair c of the wave is (f = 16 block + c, the centre of f's cluster), operand row c of A is frame f, operand column c of B its
// centre, and the same MFMA steps in the same order as k_rmsd_gram leave the pair's S on the diagonal of the nine blocks: lane (c, h) with (c & 3) == h holds
// it in register c >> 2.  A centre gets 0.0f; a frame max_clusters left over keeps the NaN bits k_cluster_init wrote.
__global__ __launch_bounds__(64) void k_rmsd_to_centre(const double *__restrict__ X, const double *__restrict__ G, uint32_t M, uint32_t n, uint32_t n_pad,
                                                       const uint32_t *__restrict__ cluster, const unsigned long long *__restrict__ best, uint32_t *sim) {
    const uint32_t c = threadIdx.x & 15u, h = threadIdx.x >> 4;
    const uint32_t f = blockIdx.x * 16u + c;
    const uint32_t fa = f < M ? f : M - 1u;
    const uint32_t k = f < M ? cluster[f] : ARP_NONE;
    const uint32_t centre = k != ARP_NONE ? 0xFFFFFFFFu - (uint32_t)best[k] : fa;
    const double *pa = X + (size_t)fa * 3u * n_pad, *pb = X + (size_t)centre * 3u * n_pad;
    rmsd_acc acc[3][3];
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) acc[a][b] = rmsd_acc{0.0, 0.0, 0.0, 0.0};
    for (uint32_t k0 = 0; k0 < n_pad; k0 += kRmsdStep) {
        double a[3], b[3];
#pragma unroll
        for (uint32_t x = 0; x < 3u; x++) {
            a[x] = pa[(size_t)x * n_pad + k0 + h];
            b[x] = pb[(size_t)x * n_pad + k0 + h];
        }
#pragma unroll
        for (int x = 0; x < 3; x++)
#pragma unroll
            for (int y = 0; y < 3; y++) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b[y], acc[x][y], 0, 0, 0);
    }
    if ((c & 3u) != h || k == ARP_NONE) return;
    if (centre == f) { sim[f] = 0u; return; }
    double s[3][3];
#pragma unroll
    for (int x = 0; x < 3; x++)
#pragma unroll
        for (int y = 0; y < 3; y++) {
            const rmsd_acc r = acc[x][y];
            const uint32_t reg = c >> 2;
            s[x][y] = reg == 0u ? r[0] : reg == 1u ? r[1] : reg == 2u ? r[2] : r[3];
        }
    sim[f] = __float_as_uint(rmsd_of_pair(s, G[f] + G[centre], n));
}

// The call on the device.  Upload in passes of whole frames (the atom budget of the frequency path: the knob's, else kFreqAutoAtoms) and pack; X and G stay
// resident.  Then by kind: the matrix; one row against frame `ref_frame` or the packed ref_xyz; neighbour bits, the rounds of cluster.inl and the distances
// to the centres.  The capacity checks ran on the host (rmsd.cpp) before this is called.
arp_status device_rmsd(arp_context *ctx, const RmsdJob &job, float *out, ClustersHost *clusters) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(context_device(ctx)));
    StreamLapTimer lap("  rmsd %-10s %8.3f ms\n", st);
    const uint64_t N = job.n_atoms, F = job.n_frames, n = job.n_sel, n_pad = rmsd_n_pad(n);
    const uint64_t per = frames_per_pass(job.chunk_atoms, N, F);
    const bool ext_ref = job.kind == RmsdJob::kReference && job.ref_xyz;
    const uint64_t out_bytes = job.kind == RmsdJob::kMatrix ? F * F * 4u : job.kind == RmsdJob::kReference ? F * 4u : 0u;
    double *X = nullptr, *G = nullptr, *stage = nullptr, *XR = nullptr, *GR = nullptr; uint32_t *sel = nullptr; float *d_out = nullptr;
    DevBlock block;
    if (arp_status s = block.carve([&](Bump &bp) {
            X = bp.take<double>(F * 3u * n_pad); G = bp.take<double>(F); sel = bp.take<uint32_t>(n);
            stage = bp.take<double>(per * N * 3u); XR = bp.take<double>(3u * n_pad); GR = bp.take<double>(1);
            d_out = reinterpret_cast<float *>(bp.take<char>(out_bytes)); bp.take<char>(256);  // (slack)
        }); s != ARP_OK) return s;
    HIP_TRY(hipMemcpyAsync(sel, job.sel, n * 4u, hipMemcpyHostToDevice, st));
    for (uint64_t f0 = 0; f0 < F; f0 += per) {
        const uint64_t fc = std::min<uint64_t>(per, F - f0);
        HIP_TRY(hipMemcpyAsync(stage, job.xyz + f0 * N * 3u, fc * N * 24u, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_rmsd_pack<false>, dim3((uint32_t)fc), dim3(256), 0, st, (const double *)stage, (uint32_t)N, (const uint32_t *)sel, (uint32_t)n, (uint32_t)n_pad,
                           X + f0 * 3u * n_pad, G + f0, (const uint32_t *)nullptr, 0u, 0u, (double *)nullptr, (double *)nullptr);
        HIP_TRY(hipGetLastError());
    }
    if (ext_ref) {
        HIP_TRY(hipMemcpyAsync(stage, job.ref_xyz, N * 24u, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_rmsd_pack<false>, dim3(1), dim3(256), 0, st, (const double *)stage, (uint32_t)N, (const uint32_t *)sel, (uint32_t)n, (uint32_t)n_pad, XR, GR,
                           (const uint32_t *)nullptr, 0u, 0u, (double *)nullptr, (double *)nullptr);
        HIP_TRY(hipGetLastError());
    }
    lap("pack");
    const uint32_t T = (uint32_t)((F + kRmsdTile - 1u) / kRmsdTile);
    const uint32_t tri = (uint32_t)((uint64_t)T * (T + 1u) / 2u);
    if (job.kind == RmsdJob::kMatrix) {
        hipLaunchKernelGGL(k_rmsd_gram<kRmsdMatrix>, dim3(tri), dim3(256), 0, st, (const double *)X, (const double *)G, (uint32_t)F, (const double *)X, (const double *)G, (uint32_t)F,
                           (uint32_t)n, (uint32_t)n_pad, T, 0.0f, ARP_NONE, d_out, (uint32_t *)nullptr, (uint64_t)0);
        HIP_TRY(hipGetLastError());
        lap("gram");
    } else if (job.kind == RmsdJob::kReference) {
        const double *xa = ext_ref ? XR : X + job.ref_frame * 3u * n_pad, *ga = ext_ref ? GR : G + job.ref_frame;
        hipLaunchKernelGGL(k_rmsd_gram<kRmsdRow>, dim3(T), dim3(256), 0, st, xa, ga, 1u, (const double *)X, (const double *)G, (uint32_t)F, (uint32_t)n, (uint32_t)n_pad, T, 0.0f,
                           ext_ref ? ARP_NONE : (uint32_t)job.ref_frame, d_out, (uint32_t *)nullptr, (uint64_t)0);
        HIP_TRY(hipGetLastError());
        lap("gram");
    }
    if (job.kind != RmsdJob::kClusters) {
        HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        lap("download");
        return ARP_OK;
    }
    *clusters = ClustersHost{};
    ClusterDev dv;
    ClusterBufs cb;
    arp_status s = cluster_alloc(st, F, job.max_clusters, &dv, &cb);
    if (s != ARP_OK) return s;
    hipLaunchKernelGGL(k_rmsd_gram<kRmsdAdjacency>, dim3(tri), dim3(256), 0, st, (const double *)X, (const double *)G, (uint32_t)F, (const double *)X, (const double *)G, (uint32_t)F,
                       (uint32_t)n, (uint32_t)n_pad, T, job.cutoff, ARP_NONE, (float *)nullptr, cb.adj, cb.KA);
    HIP_TRY(hipGetLastError());
    lap("gram");
    if ((s = cluster_rounds<false>(st, cb, F, nullptr, 0, job.max_clusters, lap, &dv)) != ARP_OK) return s;
    hipLaunchKernelGGL(k_rmsd_to_centre, dim3((uint32_t)((F + 15u) / 16u)), dim3(64), 0, st, (const double *)X, (const double *)G, (uint32_t)F, (uint32_t)n, (uint32_t)n_pad,
                       (const uint32_t *)dv.cluster, (const unsigned long long *)cb.best, dv.sim);
    HIP_TRY(hipGetLastError());
    const uint64_t C = dv.best.size();
    clusters->m = F; clusters->n_clusters = C;
    clusters->cluster.resize(F); clusters->sim.resize(F); clusters->n_neighbours.resize(F);
    clusters->centre.resize(C); clusters->cluster_size.resize(C);
    for (uint64_t k = 0; k < C; k++) { clusters->centre[k] = ~(uint32_t)dv.best[k]; clusters->cluster_size[k] = (uint32_t)(dv.best[k] >> 32); }
    HIP_TRY(hipMemcpyAsync(clusters->cluster.data(), dv.cluster, F * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(clusters->sim.data(), dv.sim, F * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(clusters->n_neighbours.data(), dv.n_neighbours, F * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lap("download");
    return cluster_verify(*clusters, 0, nullptr);
}
