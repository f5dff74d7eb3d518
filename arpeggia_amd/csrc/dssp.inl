// Secondary structure by the rules of Kabsch & Sander 1983, per frame and across the frames of an ensemble (arp_dssp).  Included by
// table_dev.hip inside namespace arp.  The frames come through the upload passes of the arp_rmsd_* calls; per pass:
//   k_dssp_pack    per (frame, residue): N, CA, C, O gathered by bb from the staged frame into acceptor records A[f][r] = (CA, C, O) and donor records
//                  D[f][r] = (N, H); bits[f][r]: bit 0 brk, bit 1 the residue donates (H exists)
//   k_dssp_sweep   the hot kernel.  Block b: donor tile b % tiles of frame b / tiles, one lane per donor j with N, H, CA in registers; the frame's acceptors go
//                  through LDS in tiles of kDsspTile records.  Per tile, first the squared CA distance of every acceptor, read at the same address by every lane (a
//                  broadcast), against a bound that is certain to hold every pair within the cut; then, per lane, those it is near to (a 64-bit mask): the CA test
//                  as defined and the four distances; the two best in registers.  Writes acc[f][j][2] (ARP_NONE: none), en[f][j][2] (f32) and ok[f][j] (bit k:
//                  entry k is a bond, E < -0.5 in f64)
//   k_dssp_assign  one workgroup per frame.  Everything is a function of the two-best lists, hb(a, b) = a in best[b]: the bridge partners of i are looked up
//                  forwards from best[i] and best[i + 1] (eight candidates), no R x R matrix exists.  Phases B/E/H -> G -> I -> T/S with block barriers between
//                  them; then the frame's histogram (LDS) and counts[r][code] += 1 (u32 atomics: the only atomics, exact in any order)
// All arithmetic is f64 in the order of the definition (the library is built with -ffp-contract=off); nothing depends on another frame or on the pass size.

constexpr uint32_t kDsspTile = 64;        // donors of a workgroup of k_dssp_sweep (one wave, one donor per lane) = acceptors of an LDS tile = bits of a lane's mask
constexpr uint32_t kDsspAssign = 256;     // lanes of a workgroup of k_dssp_assign
constexpr uint32_t kDsspPack = 256;       // lanes of a workgroup of k_dssp_pack
constexpr uint8_t kDsspBrk = 1, kDsspDonor = 2;
constexpr double kDsspFar2 = 82.0;        // A^2: d^2 at or above it has sqrt(d^2) >= 9.05 > kDsspCaCut whatever the rounding -- rejected without the square root

__device__ __forceinline__ double dssp_dist(const double *a, double bx, double by, double bz) {
    const double dx = a[0] - bx, dy = a[1] - by, dz = a[2] - bz;
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// stage[fc][N][3]; bb[R][4]; A[fc][R][9]; D[fc][R][6]; bits[fc][R]
__global__ __launch_bounds__(kDsspPack) void k_dssp_pack(const double *__restrict__ stage, uint32_t N, const uint32_t *__restrict__ bb, const uint8_t *__restrict__ flags, uint32_t R,
                                                         uint64_t fc, double *__restrict__ A, double *__restrict__ D, uint8_t *__restrict__ bits) {
    const uint64_t idx = (uint64_t)blockIdx.x * kDsspPack + threadIdx.x;
    if (idx >= fc * R) return;
    const uint64_t f = idx / R;
    const uint32_t r = (uint32_t)(idx % R);
    const double *x = stage + f * (uint64_t)N * 3u;
    const double *n = x + (uint64_t)bb[4u * r] * 3u, *ca = x + (uint64_t)bb[4u * r + 1u] * 3u, *c = x + (uint64_t)bb[4u * r + 2u] * 3u, *o = x + (uint64_t)bb[4u * r + 3u] * 3u;
    double *a = A + idx * 9u, *d = D + idx * 6u;
#pragma unroll
    for (int k = 0; k < 3; k++) { a[k] = ca[k]; a[3 + k] = c[k]; a[6 + k] = o[k]; d[k] = n[k]; }
    const uint8_t fl = flags[r];
    bool brk = r == 0u || (fl & ARP_DSSP_CHAIN_START);
    double h[3] = {0.0, 0.0, 0.0};
    bool donor = false;
    if (!brk) {
        const double *cp = x + (uint64_t)bb[4u * (r - 1u) + 2u] * 3u, *op = x + (uint64_t)bb[4u * (r - 1u) + 3u] * 3u;
        brk = dssp_dist(cp, n[0], n[1], n[2]) > kDsspBreak;
        donor = !brk && !(fl & ARP_DSSP_NO_H);
        if (donor) {
            const double len = dssp_dist(cp, op[0], op[1], op[2]);
#pragma unroll
            for (int k = 0; k < 3; k++) h[k] = n[k] + (cp[k] - op[k]) / len;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) d[3 + k] = h[k];
    bits[idx] = (uint8_t)((brk ? kDsspBrk : 0u) | (donor ? kDsspDonor : 0u));
}

__global__ __launch_bounds__(kDsspTile) void k_dssp_sweep(const double *__restrict__ A, const double *__restrict__ D, const uint8_t *__restrict__ bits, uint32_t R, uint32_t tiles,
                                                          uint32_t *__restrict__ acc, float *__restrict__ en, uint8_t *__restrict__ ok) {
    __shared__ double tile[kDsspTile * 9u];
    const uint64_t f = blockIdx.x / tiles;
    const uint32_t j = (blockIdx.x % tiles) * kDsspTile + threadIdx.x;
    const double *Af = A + f * (uint64_t)R * 9u;
    const bool donor = j < R && (bits[f * R + j] & kDsspDonor);
    double n[3] = {0.0, 0.0, 0.0}, h[3] = {0.0, 0.0, 0.0}, ca[3] = {0.0, 0.0, 0.0};
    if (donor) {
        const double *d = D + (f * R + j) * 6u, *a = Af + (uint64_t)j * 9u;
#pragma unroll
        for (int k = 0; k < 3; k++) { n[k] = d[k]; h[k] = d[3 + k]; ca[k] = a[k]; }
    }
    double e0 = INFINITY, e1 = INFINITY;
    uint32_t i0 = ARP_NONE, i1 = ARP_NONE;
    for (uint32_t t0 = 0; t0 < R; t0 += kDsspTile) {
        const uint32_t tn = min(kDsspTile, R - t0);
        __syncthreads();  // (the previous tile has been read)
        for (uint32_t k = threadIdx.x; k < tn * 9u; k += kDsspTile) tile[k] = Af[(uint64_t)t0 * 9u + k];
        __syncthreads();
        if (!donor) continue;  // (the barriers are outside: every lane of the block makes the same trips)
        // 1: every acceptor of the tile against the lane's CA, the wave in step (every lane reads the same address: a broadcast); the few that may be within
        //    the cut set their bit in the lane's mask
        unsigned long long near = 0ull;
        for (uint32_t t = 0; t < tn; t++) {
            const double *a = tile + t * 9u;
            const double dx = a[0] - ca[0], dy = a[1] - ca[1], dz = a[2] - ca[2];
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            const uint32_t i = t0 + t;
            if (d2 < kDsspFar2 && i != j && i + 1u != j) near |= 1ull << t;
        }
        // 2: the lane's own bits, lowest first: the definition's CA test and the energy.  The wave makes as many trips as its fullest mask has bits, not
        //    one per acceptor that any lane is near to
        while (near) {
            const uint32_t t = (uint32_t)__ffsll(near) - 1u, i = t0 + t;
            near &= near - 1ull;
            const double *a = tile + t * 9u;
            if (!(dssp_dist(a, ca[0], ca[1], ca[2]) < kDsspCaCut)) continue;
            const double d_on = dssp_dist(a + 6, n[0], n[1], n[2]), d_ch = dssp_dist(a + 3, h[0], h[1], h[2]), d_oh = dssp_dist(a + 6, h[0], h[1], h[2]),
                         d_cn = dssp_dist(a + 3, n[0], n[1], n[2]);
            double e = kDsspCoupling * (((1.0 / d_on + 1.0 / d_ch) - 1.0 / d_oh) - 1.0 / d_cn);
            if (d_on < kDsspMinDist || d_ch < kDsspMinDist || d_oh < kDsspMinDist || d_cn < kDsspMinDist) e = kDsspMinEnergy;
            if (e < e0) { e1 = e0; i1 = i0; e0 = e; i0 = i; }
            else if (e < e1) { e1 = e; i1 = i; }
        }
    }
    if (j >= R) return;
    const uint64_t o = (f * R + j) * 2u;
    acc[o] = i0; acc[o + 1u] = i1;
    en[o] = i0 == ARP_NONE ? 0.0f : (float)e0;
    en[o + 1u] = i1 == ARP_NONE ? 0.0f : (float)e1;
    ok[f * R + j] = (uint8_t)((e0 < kDsspHbond ? 1u : 0u) | (e1 < kDsspHbond ? 2u : 0u));
}

// one frame's lists, as the assignment reads them
struct DsspLists {
    const uint8_t *bits, *ok;
    const uint32_t *acc;
    int64_t R;
    __device__ __forceinline__ bool cont(int64_t a, int64_t b) const {
        if (a < 0 || b >= R) return false;
        for (int64_t r = a + 1; r <= b; r++)
            if (bits[r] & kDsspBrk) return false;
        return true;
    }
    __device__ __forceinline__ bool hb(int64_t i, int64_t j) const {
        if (i < 0 || j < 0 || i >= R || j >= R) return false;
        const uint8_t k = ok[j];
        return ((k & 1u) && acc[2 * j] == (uint32_t)i) || ((k & 2u) && acc[2 * j + 1] == (uint32_t)i);
    }
    __device__ __forceinline__ bool turn(int n, int64_t i) const { return cont(i, i + n) && hb(i, i + n); }
    __device__ __forceinline__ bool pairable(int64_t i, int64_t j) const {
        return i >= 0 && j >= 0 && i < R && j < R && (i - j >= 3 || j - i >= 3) && cont(i - 1, i + 1) && cont(j - 1, j + 1);
    }
    __device__ __forceinline__ bool par(int64_t i, int64_t j) const { return pairable(i, j) && ((hb(i - 1, j) && hb(j, i + 1)) || (hb(j - 1, i) && hb(i, j + 1))); }
    __device__ __forceinline__ bool anti(int64_t i, int64_t j) const { return pairable(i, j) && ((hb(i, j) && hb(j, i)) || (hb(i - 1, j + 1) && hb(j - 1, i + 1))); }
};

// G (n = 3) or I (n = 5): mark[k] = some i in k - n + 1 .. k has turn_n(i - 1), turn_n(i) and i .. i + n - 1 all '-' before the phase.  In the definition's
// ascending walk a residue can only have turned into this phase's own state, which the walk lets pass: the test on the states before the phase is the same.
__device__ __forceinline__ void dssp_helix_phase(const DsspLists &L, int n, uint8_t state, uint8_t *code, uint8_t *mark) {
    for (int64_t k = threadIdx.x; k < L.R; k += kDsspAssign) {
        bool hit = false;
        for (int64_t i = k - n + 1; i <= k && !hit; i++) {
            if (!(L.turn(n, i - 1) && L.turn(n, i))) continue;  // (turn_n(i): i + n < R)
            bool open = true;
            for (int64_t q = i; q < i + n; q++) open = open && code[q] == 0u;
            hit = open;
        }
        mark[k] = hit ? 1u : 0u;
    }
    __syncthreads();
    for (int64_t k = threadIdx.x; k < L.R; k += kDsspAssign)
        if (mark[k]) code[k] = state;
    __syncthreads();
}

// Block f: frame f of the pass.  code[fc][R] (the output rows), mark[fc][R] scratch, counts[R][8] (accumulated over the passes), frame_counts[fc][8].
__global__ __launch_bounds__(kDsspAssign) void k_dssp_assign(const double *__restrict__ A, const uint8_t *__restrict__ bits, const uint32_t *__restrict__ acc, const uint8_t *__restrict__ ok,
                                                            uint32_t R, uint8_t *code_all, uint8_t *mark_all, uint32_t *counts, uint32_t *frame_counts) {
    __shared__ uint32_t hist[8];
    const uint64_t f = blockIdx.x;
    const DsspLists L{bits + f * R, ok + f * R, acc + f * (uint64_t)R * 2u, (int64_t)R};
    uint8_t *code = code_all + f * R, *mark = mark_all + f * R;
    const double *Af = A + f * (uint64_t)R * 9u;
    if (threadIdx.x < 8u) hist[threadIdx.x] = 0u;
    // B, E, H: each lane writes its own residues from the lists alone
    for (int64_t i = threadIdx.x; i < L.R; i += kDsspAssign) {
        bool bridge = false, ladder = false;
        for (int c = 0; c < 4; c++) {  // best[i][0], best[i][1], best[i + 1][0], best[i + 1][1]
            const int64_t d = i + (c >> 1);
            if (d >= L.R) continue;
            const uint32_t a = L.acc[2 * d + (c & 1)];
            if (a == ARP_NONE) continue;
            for (int64_t j = a; j <= (int64_t)a + 1; j++) {
                const bool p = L.par(i, j), q = L.anti(i, j);
                bridge = bridge || p || q;
                ladder = ladder || (p && (L.par(i - 1, j - 1) || L.par(i + 1, j + 1))) || (q && (L.anti(i - 1, j + 1) || L.anti(i + 1, j - 1)));
            }
        }
        bool helix = false;
        for (int64_t s = i - 3; s <= i; s++) helix = helix || (L.turn(4, s - 1) && L.turn(4, s));
        code[i] = helix ? 1u : ladder ? 3u : bridge ? 2u : 0u;
    }
    __syncthreads();
    dssp_helix_phase(L, 3, 4u, code, mark);
    dssp_helix_phase(L, 5, 5u, code, mark);
    // T, S, and the statistics: own residues only
    for (int64_t k = threadIdx.x; k < L.R; k += kDsspAssign) {
        uint8_t s = code[k];
        if (s == 0u) {
            bool t = false;
            for (int n = 3; n <= 5; n++)
                for (int64_t i = k - n + 1; i < k; i++) t = t || L.turn(n, i);
            if (t) s = 6u;
            else if (L.cont(k - 2, k + 2)) {
                const double *a = Af + (k - 2) * 9, *b = Af + k * 9, *c = Af + (k + 2) * 9;
                const double ux = b[0] - a[0], uy = b[1] - a[1], uz = b[2] - a[2], vx = c[0] - b[0], vy = c[1] - b[1], vz = c[2] - b[2];
                const double dot = (ux * vx + uy * vy) + uz * vz;
                const double lu = sqrt((ux * ux + uy * uy) + uz * uz), lv = sqrt((vx * vx + vy * vy) + vz * vz);
                if (dot / (lu * lv) < kDsspCos70) s = 7u;
            }
            code[k] = s;
        }
        atomicAdd(&hist[s], 1u);
        atomicAdd(&counts[(uint64_t)k * 8u + s], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 8u) frame_counts[f * 8u + threadIdx.x] = hist[threadIdx.x];
}

// The call on the device.  The checks ran on the host (dssp.cpp).  Per upload pass: copy, pack, sweep, assign, and the pass's rows of every requested output
// back; counts accumulate on the device and come back once.
arp_status device_dssp(arp_context *ctx, const DsspJob &job, DsspOut *out) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(context_device(ctx)));
    StreamLapTimer lap("  dssp %-10s %8.3f ms\n", st);
    const uint64_t N = job.n_atoms, F = job.n_frames, R = job.n_res;
    const uint64_t tiles = (R + kDsspTile - 1u) / kDsspTile;
    uint64_t per = frames_per_pass(job.chunk_atoms, N, F);
    per = std::min<uint64_t>(per, std::max<uint64_t>(1, ((1ull << 31) - 1u) / std::max(tiles, (R + kDsspPack - 1u) / kDsspPack)));  // one launch covers a pass
    double *stage = nullptr, *A = nullptr, *D = nullptr; uint32_t *bb = nullptr, *acc = nullptr, *counts = nullptr, *fcounts = nullptr; float *en = nullptr;
    uint8_t *flags = nullptr, *bits = nullptr, *ok = nullptr, *code = nullptr, *mark = nullptr;
    DevBlock block;
    if (arp_status s = block.carve([&](Bump &bp) {
            stage = bp.take<double>(per * N * 3u); bb = bp.take<uint32_t>(R * 4u); flags = bp.take<uint8_t>(R);
            A = bp.take<double>(per * R * 9u); D = bp.take<double>(per * R * 6u);
            bits = bp.take<uint8_t>(per * R); ok = bp.take<uint8_t>(per * R); code = bp.take<uint8_t>(per * R);
            acc = bp.take<uint32_t>(per * R * 2u); en = bp.take<float>(per * R * 2u); mark = bp.take<uint8_t>(per * R);
            counts = bp.take<uint32_t>(R * 8u); fcounts = bp.take<uint32_t>(per * 8u); bp.take<char>(256);  // (slack)
        }); s != ARP_OK) return s;
    HIP_TRY(hipMemcpyAsync(bb, job.bb, R * 16u, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(flags, job.flags, R, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(counts, 0, R * 32u, st));
    for (uint64_t f0 = 0; f0 < F; f0 += per) {
        const uint64_t fc = std::min<uint64_t>(per, F - f0);
        HIP_TRY(hipMemcpyAsync(stage, job.xyz + f0 * N * 3u, fc * N * 24u, hipMemcpyHostToDevice, st));
        lap("upload");
        hipLaunchKernelGGL(k_dssp_pack, dim3((uint32_t)((fc * R + kDsspPack - 1u) / kDsspPack)), dim3(kDsspPack), 0, st, (const double *)stage, (uint32_t)N, (const uint32_t *)bb,
                           (const uint8_t *)flags, (uint32_t)R, fc, A, D, bits);
        lap("pack");
        hipLaunchKernelGGL(k_dssp_sweep, dim3((uint32_t)(fc * tiles)), dim3(kDsspTile), 0, st, (const double *)A, (const double *)D, (const uint8_t *)bits, (uint32_t)R, (uint32_t)tiles,
                           acc, en, ok);
        lap("sweep");
        hipLaunchKernelGGL(k_dssp_assign, dim3((uint32_t)fc), dim3(kDsspAssign), 0, st, (const double *)A, (const uint8_t *)bits, (const uint32_t *)acc, (const uint8_t *)ok, (uint32_t)R,
                           code, mark, counts, fcounts);
        HIP_TRY(hipGetLastError());
        lap("assign");
        if (out->codes) HIP_TRY(hipMemcpyAsync(out->codes + f0 * R, code, fc * R, hipMemcpyDeviceToHost, st));
        if (out->frame_counts) HIP_TRY(hipMemcpyAsync(out->frame_counts + f0 * 8u, fcounts, fc * 32u, hipMemcpyDeviceToHost, st));
        if (out->hb_acceptor) HIP_TRY(hipMemcpyAsync(out->hb_acceptor + f0 * R * 2u, acc, fc * R * 8u, hipMemcpyDeviceToHost, st));
        if (out->hb_energy) HIP_TRY(hipMemcpyAsync(out->hb_energy + f0 * R * 2u, en, fc * R * 8u, hipMemcpyDeviceToHost, st));
        lap("download");
    }
    HIP_TRY(hipMemcpyAsync(out->counts, counts, R * 32u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return ARP_OK;
}
