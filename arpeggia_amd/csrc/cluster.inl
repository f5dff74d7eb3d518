// Clustering the frames of an ensemble by their contacts (arp_contact_clusters, arp_bit_cluster).  Included by table_dev.hip
// inside namespace arp, behind similarity.inl.
//
// The bit-rows of A[M][K words] (similarity.inl: the transposed timeline bitmap on axis "frames", the bitmap itself on axis "rows") are clustered by the
// gromos method on the neighbour relation adj[f][g] <=> tanimoto(f, g) >= min_similarity:
//   k_bit_adjacency   the tile loop of k_bit_gram with a threshold epilogue: adj[M][ceil(M / 32)], one bit per pair, never the f32 matrix
//   k_cluster_round   launch r applies cluster r - 1 (its centre is the argmax that launch r - 1 left in best[r - 1]) and counts the neighbours of every
//                     frame that is still alive: best[r] = max over them of (count << 32 | ~index), one unsigned maximum for "largest count, smallest index"
//   k_cluster_tail    once the largest count is 1, the frames left are singletons in index order: one launch instead of one each
//   k_cluster_counts  cluster_counts[r][k] = the frames of cluster k in which row r is present, by an LDS histogram over the row's set bits
// A round is a launch: its workgroups meet nowhere but in best[r] (atomicMax) and in the kernel boundary.  Launches behind the last round find a count <= 1
// in best[r - 1] and return.  Integer work and the one IEEE divide of the Tanimoto value: the bytes do not depend on scheduling.

constexpr uint32_t kClusterRows = 64;            // frames of one block of k_cluster_round: two words of the alive set, sixteen frames per wave
constexpr uint32_t kClusterCountTile = 4096;     // clusters of one histogram sweep of k_cluster_counts (16 KiB of LDS)
constexpr uint32_t kClusterNaN = 0x7FC00000u;    // similarity_to_centre of a frame that max_clusters left over
constexpr uint32_t kClusterBatch0 = 16, kClusterBatchMax = 256;  // launches between two host looks at best[]: 16, 32, .. 256

// the f32 Tanimoto value of k_bit_gram<true>, bit for bit
__device__ inline uint32_t tanimoto_bits(uint32_t inter, uint32_t size_a, uint32_t size_b) {
    const unsigned long long uni = (unsigned long long)size_a + size_b - inter;
    return uni ? __float_as_uint((float)((double)inter / (double)uni)) : 0x3F800000u;
}

// The tile loop of k_bit_gram, word for word (a sibling, so that k_bit_gram compiles to what it was: its two instantiations came out with other registers when
// they shared this function): acc[i][j] = |row (row0 + ty + 16 i) AND row (col0 + tx + 16 j)| of A.  The 64 rows of the tile's rows and the 64 of its columns go
// through LDS (2 x kSimTile x kSimLds words) in chunks of kSimChunk words; the next chunk is fetched into registers while the current one is consumed.  Rows
// past M and words past K are staged as zeros.  Every lane of the block calls it; the staging buffer is free again when it returns.
__device__ __forceinline__ void bit_adjacency_tile(const uint32_t *A, uint32_t M, uint64_t K, uint64_t stride, uint32_t row0, uint32_t col0, uint32_t *lds,
                                                   uint32_t (&acc)[kSimReg][kSimReg]) {
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint32_t lk = threadIdx.x & 31u, lr = threadIdx.x >> 5;  // staging: word lk of rows lr, lr + 8, ..
    uint32_t *sA = lds, *sB = lds + kSimTile * kSimLds;
    uint32_t ra[8], rb[8];
    auto fetch = [&](uint64_t k0) {
        const uint64_t k = k0 + lk;
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++) {
            const uint32_t r = row0 + lr + 8u * i, c = col0 + lr + 8u * i;
            ra[i] = (r < M && k < K) ? A[(size_t)r * stride + k] : 0u;
            rb[i] = (c < M && k < K) ? A[(size_t)c * stride + k] : 0u;
        }
    };
    fetch(0);
    for (uint64_t k0 = 0; k0 < K; k0 += kSimChunk) {
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++) {
            sA[(lr + 8u * i) * kSimLds + lk] = ra[i];
            sB[(lr + 8u * i) * kSimLds + lk] = rb[i];
        }
        __syncthreads();
        if (k0 + kSimChunk < K) fetch(k0 + kSimChunk);
#pragma unroll
        for (uint32_t kk = 0; kk < kSimChunk; kk += 4u) {
            uint4 a[kSimReg], b[kSimReg];
#pragma unroll
            for (uint32_t i = 0; i < kSimReg; i++) a[i] = *reinterpret_cast<const uint4 *>(sA + (ty + 16u * i) * kSimLds + kk);
#pragma unroll
            for (uint32_t j = 0; j < kSimReg; j++) b[j] = *reinterpret_cast<const uint4 *>(sB + (tx + 16u * j) * kSimLds + kk);
#pragma unroll
            for (uint32_t i = 0; i < kSimReg; i++)
#pragma unroll
                for (uint32_t j = 0; j < kSimReg; j++)
                    acc[i][j] += (uint32_t)(__popc(a[i].x & b[j].x) + __popc(a[i].y & b[j].y) + __popc(a[i].z & b[j].z) + __popc(a[i].w & b[j].w));
        }
        __syncthreads();
    }
}

// Tile (ti, tj) of the upper triangle as in k_bit_gram; lane (tx, ty) holds the counts of outputs (ty + 16 i, tx + 16 j).  A wave holds four rows ty of
// sixteen columns tx, so the ballot of element (i, j) carries bits 16 j .. 16 j + 15 of the rows 16 i + 4 wave .. + 3: lanes tx = 0 / 1 of a row put its two
// words together and write them.  Rows and columns past M fail the test: their bits are zero.  Off the diagonal the 64 x 2 words go through LDS and lane c
// of the first wave gathers column c, which is row col0 + c of the mirror tile.
__global__ __launch_bounds__(256) void k_bit_adjacency(const uint32_t *A, uint32_t M, uint64_t K, uint64_t stride, const uint32_t *sizes, uint32_t T, float min_similarity,
                                                       uint32_t *adj, uint64_t KA) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[2u * kSimTile * kSimLds];
    uint32_t t = blockIdx.x, ti = 0;
    while (t >= T - ti) { t -= T - ti; ti++; }
    const uint32_t tj = ti + t;
    const uint32_t row0 = ti * kSimTile, col0 = tj * kSimTile;
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    uint32_t acc[kSimReg][kSimReg] = {};
    bit_adjacency_tile(A, M, K, stride, row0, col0, lds, acc);
    uint32_t sa[kSimReg], sb[kSimReg];
#pragma unroll
    for (uint32_t i = 0; i < kSimReg; i++) {
        const uint32_t r = row0 + ty + 16u * i, c = col0 + tx + 16u * i;
        sa[i] = r < M ? sizes[r] : 0u;
        sb[i] = c < M ? sizes[c] : 0u;
    }
    uint32_t *image = lds;  // [kSimTile][2]
#pragma unroll
    for (uint32_t i = 0; i < kSimReg; i++) {
        const uint32_t r = row0 + ty + 16u * i;
        uint32_t seg[kSimReg];
#pragma unroll
        for (uint32_t j = 0; j < kSimReg; j++) {
            const uint32_t c = col0 + tx + 16u * j;
            const bool pass = r < M && c < M && __uint_as_float(tanimoto_bits(acc[i][j], sa[i], sb[j])) >= min_similarity;
            seg[j] = (uint32_t)(__ballot(pass) >> (16u * (ty & 3u))) & 0xFFFFu;
        }
        if (tx < 2u) {
            const uint32_t w = tx ? (seg[2] | seg[3] << 16) : (seg[0] | seg[1] << 16);
            const uint64_t wi = col0 / 32u + tx;
            image[(ty + 16u * i) * 2u + tx] = w;
            if (r < M && wi < KA) adj[(size_t)r * KA + wi] = w;
        }
    }
    if (ti != tj) {
        __syncthreads();
        if (threadIdx.x < kSimTile) {
            const uint32_t c = threadIdx.x, cw = c >> 5, cb = c & 31u;
            uint32_t m0 = 0, m1 = 0;
#pragma unroll 8
            for (uint32_t r = 0; r < 32u; r++) {
                m0 |= (image[r * 2u + cw] >> cb & 1u) << r;
                m1 |= (image[(r + 32u) * 2u + cw] >> cb & 1u) << r;
            }
            const uint64_t wi = row0 / 32u;  // (row0 < M: the word exists)
            if (col0 + c < M) {
                adj[(size_t)(col0 + c) * KA + wi] = m0;
                if (wi + 1u < KA) adj[(size_t)(col0 + c) * KA + wi + 1u] = m1;
            }
        }
    }
}

// every frame unassigned, the alive set full: the M low bits of alive[KA]
__global__ __launch_bounds__(256) void k_cluster_init(uint32_t M, uint64_t KA, uint32_t *cluster, uint32_t *sim, uint32_t *alive) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < M) { cluster[i] = ARP_NONE; sim[i] = kClusterNaN; }
    if (i < KA) alive[i] = (i + 1u) * 32u <= M ? 0xFFFFFFFFu : (1u << (M & 31u)) - 1u;
}

// the sum of v over the wave, in lane 0
__device__ inline uint32_t wave_sum(uint32_t v) {
    for (uint32_t off = 32u; off; off >>= 1) v += (uint32_t)__shfl_down((int)v, off);
    return v;
}

// Launch `round`.  alive_prev is the alive set before cluster round - 1 was taken out; its centre c is in best[round - 1].  The set after it,
// alive_prev AND NOT adj[c], is formed on the fly, and the block writes its own two words of it to alive_next (the two buffers swap roles from launch to
// launch).  A wave takes sixteen frames, one after the other, the lanes share the words of a row:
//   a member of cluster round - 1 (alive before, neighbour of c) gets its cluster and tanimoto(f, c) from the two bit-rows of A and the sizes;
//   a frame that stays alive gets n[f] = popcount(adj[f] AND alive) -- in round 0, with every frame alive, popcount(adj[f]) = n_neighbours[f]: a set bit past
//   M would be a phantom neighbour there -- and offers (n << 32 | ~f) to best[round].
// round == max_clusters: the last cluster is applied, nothing is counted, best[round] stays 0.
// kTanimoto false (rmsd.inl: the neighbour bits come from coordinates, there are no bit-rows): a member gets its cluster only, A, K and sizes are not read and
// sim is left to the caller's own kernel.
template <bool kTanimoto>
__global__ __launch_bounds__(256) void k_cluster_round(uint32_t round, uint32_t max_clusters, const uint32_t *adj, uint32_t M, uint64_t KA, const uint32_t *A, uint64_t K,
                                                       const uint32_t *sizes, unsigned long long *best, const uint32_t *alive_prev, uint32_t *alive_next, uint32_t *cluster,
                                                       uint32_t *sim, uint32_t *n_neighbours) {
    __shared__ unsigned long long s_best[4];
    const uint32_t *adj_c = nullptr;
    uint32_t c = 0;
    if (round) {
        const unsigned long long prev = best[round - 1u];
        if ((prev >> 32) <= 1u) return;  // (the whole grid) nothing was alive, max_clusters was reached, or only singletons are left: k_cluster_tail's
        c = ~(uint32_t)prev;
        adj_c = adj + (size_t)c * KA;
    }
    const bool counting = round < max_clusters;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x < 2u) {
        const uint64_t w = (uint64_t)blockIdx.x * 2u + threadIdx.x;
        if (w < KA) alive_next[w] = alive_prev[w] & ~(adj_c ? adj_c[w] : 0u);
    }
    unsigned long long mine = 0ull;
    for (uint32_t i = 0; i < kClusterRows / 4u; i++) {
        const uint32_t f = blockIdx.x * kClusterRows + wave * (kClusterRows / 4u) + i;
        if (f >= M) break;  // (the whole wave)
        const uint32_t bit = 1u << (f & 31u);
        const bool was = (alive_prev[f >> 5] & bit) != 0u;
        const bool member = was && adj_c && (adj_c[f >> 5] & bit) != 0u;
        if (member && !kTanimoto) {
            if (lane == 0u) cluster[f] = round - 1u;
        } else if (member) {
            const uint32_t *a = A + (size_t)f * K, *b = A + (size_t)c * K;
            uint32_t inter = 0;
            for (uint64_t w = lane; w < K; w += 64u) inter += (uint32_t)__popc(a[w] & b[w]);
            inter = wave_sum(inter);
            if (lane == 0u) { cluster[f] = round - 1u; sim[f] = tanimoto_bits(inter, sizes[f], sizes[c]); }
        }
        if (!was || member || !counting) continue;
        const uint32_t *row = adj + (size_t)f * KA;
        uint32_t n = 0;
        if (round == 0u)  // every frame is alive and the neighbour words have no bit past M: the row's own popcount, without a load of the alive set
            for (uint64_t w = lane; w < KA; w += 64u) n += (uint32_t)__popc(row[w]);
        else
            for (uint64_t w = lane; w < KA; w += 64u) n += (uint32_t)__popc(row[w] & alive_prev[w] & ~adj_c[w]);
        n = wave_sum(n);
        if (lane == 0u) {
            if (round == 0u) n_neighbours[f] = n;
            const unsigned long long key = (unsigned long long)n << 32 | (0xFFFFFFFFu - f);
            if (key > mine) mine = key;
        }
    }
    if (lane == 0u) s_best[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0u) {
        unsigned long long m = s_best[0];
        for (uint32_t k = 1; k < 4u; k++) if (s_best[k] > m) m = s_best[k];
        if (m) atomicMax(best + round, m);
    }
}

// One block.  The frames of `alive` become the clusters base, base + 1, .. in index order, each its own centre, as far as max_clusters allows: best[k]
// gets the key a round would have left there.  The rank of a frame is the exclusive prefix of the words' popcounts, 256 words per step.
__global__ __launch_bounds__(256) void k_cluster_tail(uint32_t base, uint32_t max_clusters, const uint32_t *alive, uint64_t KA, unsigned long long *best, uint32_t *cluster,
                                                      uint32_t *sim) {
    __shared__ uint32_t s_scan[256];
    uint32_t carry = base;
    for (uint64_t w0 = 0; w0 < KA; w0 += 256u) {
        const uint64_t w = w0 + threadIdx.x;
        uint32_t x = w < KA ? alive[w] : 0u;
        s_scan[threadIdx.x] = (uint32_t)__popc(x);
        __syncthreads();
        for (uint32_t off = 1; off < 256u; off <<= 1) {
            const uint32_t v = threadIdx.x >= off ? s_scan[threadIdx.x - off] : 0u;
            __syncthreads();
            s_scan[threadIdx.x] += v;
            __syncthreads();
        }
        uint32_t k = carry + s_scan[threadIdx.x] - (uint32_t)__popc(x);
        carry += s_scan[255];
        for (; x; x &= x - 1u, k++) {
            const uint32_t f = (uint32_t)(w * 32u) + (uint32_t)__ffs((int)x) - 1u;
            if (k >= max_clusters) break;
            cluster[f] = k;
            sim[f] = 0x3F800000u;
            best[k] = 1ull << 32 | (0xFFFFFFFFu - f);
        }
        __syncthreads();
    }
}

// Block r: row r of words[R][W] (bit f of the row: row r is present in frame f; the bits past F are zero).  Per sweep of kClusterCountTile clusters the block
// zeroes its histogram, walks the row's set bits -- a lane takes every 256th word -- and adds one to the cluster of each bit's frame when it lies in the sweep
// (a left-over frame, ARP_NONE, lies in none); the histogram is then the row's slice of counts[R][C].
__global__ __launch_bounds__(256) void k_cluster_counts(const uint32_t *__restrict__ words, uint64_t W, const uint32_t *__restrict__ cluster, uint32_t C, uint32_t *counts) {
    __shared__ uint32_t hist[kClusterCountTile];
    const uint32_t *row = words + (size_t)blockIdx.x * W;
    for (uint32_t c0 = 0; c0 < C; c0 += kClusterCountTile) {
        const uint32_t n = min(kClusterCountTile, C - c0);
        for (uint32_t i = threadIdx.x; i < n; i += 256u) hist[i] = 0u;
        __syncthreads();
        for (uint64_t w = threadIdx.x; w < W; w += 256u)
            for (uint32_t x = row[w]; x; x &= x - 1u) {
                const uint32_t k = cluster[w * 32u + (uint32_t)__ffs((int)x) - 1u] - c0;
                if (k < n) atomicAdd(&hist[k], 1u);
            }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += 256u) counts[(size_t)blockIdx.x * C + c0 + i] = hist[i];
        __syncthreads();
    }
}

namespace {
arp_status cluster_cap_check(uint64_t M, bool by_rows, uint64_t cap_bytes) {
    constexpr uint64_t kMaxEdge = 1ull << 21;  // (the tile triangle of one launch)
    const uint64_t need = M >= kMaxEdge ? ~0ull : M * ((M + 31u) / 32u) * 4u;
    if (need > cap_bytes) {
        set_error("contact clusters: the neighbour bits of %llu %s need %llu bytes, the limit is %llu (cluster_cap_bytes)", (unsigned long long)M, by_rows ? "rows" : "frames (F)",
                  (unsigned long long)need, (unsigned long long)cap_bytes);
        return ARP_ERR_CAPACITY;
    }
    return ARP_OK;
}

// The device buffers of one clustering.  best[k], k < n_clusters, holds cluster k's (size << 32 | ~centre).
struct ClusterDev {
    DevBlock block, counts_block;
    uint32_t *sizes = nullptr, *cluster = nullptr, *sim = nullptr, *n_neighbours = nullptr, *counts = nullptr;
    std::vector<unsigned long long> best;  // the host's copy, n_clusters entries
};

// The buffers of the rounds inside dv->block: the neighbour bits, the two alive sets and best[] (zeroed), with every frame unassigned and alive[1] full
struct ClusterBufs { uint32_t *adj = nullptr, *alive[2] = {nullptr, nullptr}; unsigned long long *best = nullptr; uint64_t KA = 0, last = 0; };
arp_status cluster_alloc(hipStream_t st, uint64_t M, uint32_t max_clusters, ClusterDev *dv, ClusterBufs *b) {
    const uint64_t KA = (M + 31u) / 32u, last = std::min<uint64_t>(M, max_clusters);  // launch `last` applies the last cluster there can be
    b->KA = KA; b->last = last;
    if (arp_status s = dv->block.carve([&](Bump &bp) {
            b->adj = bp.take<uint32_t>(M * KA);
            dv->sizes = bp.take<uint32_t>(M); dv->cluster = bp.take<uint32_t>(M); dv->sim = bp.take<uint32_t>(M); dv->n_neighbours = bp.take<uint32_t>(M);
            b->alive[0] = bp.take<uint32_t>(KA); b->alive[1] = bp.take<uint32_t>(KA);
            b->best = bp.take<unsigned long long>(last + 2u); bp.take<char>(256);  // (slack)
        }); s != ARP_OK) return s;
    HIP_TRY(hipMemsetAsync(b->best, 0, (last + 2u) * 8u, st));
    hipLaunchKernelGGL(k_cluster_init, dim3((uint32_t)((M + 255u) / 256u)), dim3(256), 0, st, (uint32_t)M, KA, dv->cluster, dv->sim, b->alive[1]);
    HIP_TRY(hipGetLastError());
    return ARP_OK;
}

// Rounds and tail on the neighbour bits b.adj (M > 0).  The host looks at best[] once per batch of launches; the launches of a batch that lie behind the last
// round are no-ops.  kTanimoto: k_cluster_round's mode (false: A, K and dv->sizes are not read).
template <bool kTanimoto>
arp_status cluster_rounds(hipStream_t st, const ClusterBufs &b, uint64_t M, const uint32_t *A, uint64_t K, uint32_t max_clusters, StreamLapTimer &lap, ClusterDev *dv) {
    const uint64_t KA = b.KA, last = b.last;
    uint32_t *const adj = b.adj, *const alive[2] = {b.alive[0], b.alive[1]};
    unsigned long long *const best = b.best;
    dv->best.assign(last + 1u, 0ull);
    uint64_t next = 0, stop = last + 1u;  // stop: the first launch index whose best[] has a count <= 1
    for (uint64_t batch = kClusterBatch0; next <= last; batch = std::min<uint64_t>(batch * 2u, kClusterBatchMax)) {
        const uint64_t r0 = next, r1 = std::min(last + 1u, next + batch);
        for (uint64_t r = r0; r < r1; r++) {
            hipLaunchKernelGGL(k_cluster_round<kTanimoto>, dim3((uint32_t)((M + kClusterRows - 1u) / kClusterRows)), dim3(256), 0, st, (uint32_t)r, max_clusters, (const uint32_t *)adj,
                               (uint32_t)M, KA, A, K, (const uint32_t *)dv->sizes, best, (const uint32_t *)alive[(r + 1u) & 1u], alive[r & 1u], dv->cluster, dv->sim,
                               dv->n_neighbours);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(dv->best.data() + r0, best + r0, (r1 - r0) * 8u, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        next = r1;
        for (uint64_t r = r0; r < r1 && stop > last; r++)
            if ((dv->best[r] >> 32) <= 1u) stop = r;
        if (stop <= last) break;
    }
    if (stop > last) { set_error("internal error: the cluster rounds did not end after %llu launches", (unsigned long long)(last + 1u)); return ARP_ERR_HIP; }
    uint64_t C = stop;
    if (dv->best[stop] >> 32) {  // singletons from here on: alive[stop & 1] is the set launch `stop` wrote
        hipLaunchKernelGGL(k_cluster_tail, dim3(1), dim3(256), 0, st, (uint32_t)stop, max_clusters, (const uint32_t *)alive[stop & 1u], KA, best, dv->cluster, dv->sim);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(dv->best.data() + stop, best + stop, (last + 1u - stop) * 8u, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        while (C < last && dv->best[C]) C++;
    }
    dv->best.resize(C);
    lap("rounds");
    return ARP_OK;
}

// sizes, adjacency, rounds and tail for the bit-rows A[M][K] on the device (M > 0, K > 0)
arp_status cluster_launch(hipStream_t st, const uint32_t *A, uint64_t M, uint64_t K, float min_similarity, uint32_t max_clusters, StreamLapTimer &lap, ClusterDev *dv) {
    ClusterBufs b;
    arp_status s = cluster_alloc(st, M, max_clusters, dv, &b);
    if (s != ARP_OK) return s;
    hipLaunchKernelGGL(k_bit_sizes, dim3((uint32_t)((M + 3u) / 4u)), dim3(256), 0, st, A, (uint32_t)M, K, K, dv->sizes);
    HIP_TRY(hipGetLastError());
    const uint32_t T = (uint32_t)((M + kSimTile - 1u) / kSimTile);
    hipLaunchKernelGGL(k_bit_adjacency, dim3((uint32_t)((uint64_t)T * (T + 1u) / 2u)), dim3(256), 0, st, A, (uint32_t)M, K, K, (const uint32_t *)dv->sizes, T, min_similarity, b.adj, b.KA);
    HIP_TRY(hipGetLastError());
    lap("adjacency");
    return cluster_rounds<true>(st, b, M, A, K, max_clusters, lap, dv);
}

// cluster_counts[R][C] on the device, from the bitmap words[R][W] and the finished assignment (R > 0, C > 0)
arp_status cluster_counts_launch(hipStream_t st, const uint32_t *words, uint64_t R, uint64_t W, uint64_t C, uint64_t cap_bytes, ClusterDev *dv) {
    if (R * C * 4u > cap_bytes) {
        set_error("contact clusters: the counts of %llu rows x %llu clusters need %llu bytes, the limit is %llu (cluster_cap_bytes)", (unsigned long long)R, (unsigned long long)C,
                  (unsigned long long)(R * C * 4u), (unsigned long long)cap_bytes);
        return ARP_ERR_CAPACITY;
    }
    if (arp_status s = dv->counts_block.carve([&](Bump &bp) { dv->counts = bp.take<uint32_t>(R * C); }); s != ARP_OK) return s;
    hipLaunchKernelGGL(k_cluster_counts, dim3((uint32_t)R), dim3(256), 0, st, words, W, (const uint32_t *)dv->cluster, (uint32_t)C, dv->counts);
    HIP_TRY(hipGetLastError());
    return ARP_OK;
}

// host memory for the counts that the result then owns: a pooled pinned block when it is large
arp_status cluster_counts_host(uint64_t R, uint64_t C, ClustersHost *out) {
    const size_t bytes = std::max<size_t>((size_t)(R * C * 4u), 4u);
    if (bytes >= (1u << 20)) {
        out->owner = pinned_block(bytes);
        if (!out->owner) { set_error("out of pinned host memory for the cluster counts"); return ARP_ERR_OOM; }
    } else {
        char *heap = (char *)malloc(bytes);
        if (!heap) { set_error("out of host memory"); return ARP_ERR_OOM; }
        out->owner = std::shared_ptr<char>(heap, [](char *q) { free(q); });
    }
    out->counts = reinterpret_cast<uint32_t *>(out->owner.get());
    return ARP_OK;
}

// the O(M) and O(C) vectors and the counts, queued on the stream (the caller synchronises); centre and cluster_size come out of best[] afterwards
arp_status cluster_download(hipStream_t st, const ClusterDev &dv, uint64_t M, uint64_t R, ClustersHost *out) {
    const uint64_t C = dv.best.size();
    out->m = M; out->n_clusters = C;
    out->cluster.resize(M); out->sim.resize(M); out->n_neighbours.resize(M); out->sizes.resize(M);
    out->centre.resize(C); out->cluster_size.resize(C);
    for (uint64_t k = 0; k < C; k++) { out->centre[k] = ~(uint32_t)dv.best[k]; out->cluster_size[k] = (uint32_t)(dv.best[k] >> 32); }
    HIP_TRY(hipMemcpyAsync(out->cluster.data(), dv.cluster, M * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->sim.data(), dv.sim, M * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->n_neighbours.data(), dv.n_neighbours, M * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->sizes.data(), dv.sizes, M * 4u, hipMemcpyDeviceToHost, st));
    if (dv.counts) HIP_TRY(hipMemcpyAsync(out->counts, dv.counts, R * C * 4u, hipMemcpyDeviceToHost, st));
    return ARP_OK;
}

// what the host verifies of a finished clustering (an "internal error" otherwise): the cluster sizes add up to the assigned frames, and, with every frame
// assigned, a row's counts add up to its frames
arp_status cluster_verify(const ClustersHost &c, uint64_t R, const uint32_t *row_frames) {
    uint64_t assigned = 0, sized = 0;
    for (uint32_t k : c.cluster) assigned += k != ARP_NONE;
    for (uint32_t n : c.cluster_size) sized += n;
    if (assigned != sized) { set_error("internal error: the cluster sizes add up to %llu, %llu frames are assigned", (unsigned long long)sized, (unsigned long long)assigned); return ARP_ERR_HIP; }
    if (!c.counts || assigned != c.m) return ARP_OK;
    for (uint64_t r = 0; r < R; r++) {
        uint64_t sum = 0;
        for (uint64_t k = 0; k < c.n_clusters; k++) sum += c.counts[r * c.n_clusters + k];
        if (sum != row_frames[r]) {
            set_error("internal error: the cluster counts of row %llu add up to %llu, the frequency table counts %u", (unsigned long long)r, (unsigned long long)sum, row_frames[r]);
            return ARP_ERR_HIP;
        }
    }
    return ARP_OK;
}
}  // namespace

arp_status device_clusters(arp_context *ctx, const FreqJob &job, float min_similarity, uint32_t max_clusters, bool want_counts, uint64_t timeline_cap_bytes, uint64_t cap_bytes,
                           FreqRowsHost *rows, ClustersHost *out) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(context_device(ctx)));
    StreamLapTimer lap("  clusters %-10s %8.3f ms\n", st);
    *out = ClustersHost{};
    // 1. + 2. rows and marks (timeline.inl); the neighbour bits are refused as soon as R is known (their size depends on F alone)
    TimelineDev dev;
    const uint64_t F = job.n_frames;
    arp_status s = timeline_device(ctx, job, timeline_cap_bytes, rows, &dev, lap, [&](uint64_t) { return cluster_cap_check(F, false, cap_bytes); });
    if (s != ARP_OK) return s;
    const uint64_t R = rows->key.size(), W = (F + 31u) / 32u, WR = (R + 31u) / 32u;
    out->has_counts = want_counts;
    if (R == 0) {  // no contact in any frame: F empty sets, all mutual neighbours at any threshold -- one cluster around frame 0
        out->m = F; out->n_clusters = 1;
        out->cluster.assign(F, 0u); out->sim.assign(F, 0x3F800000u); out->n_neighbours.assign(F, (uint32_t)F); out->sizes.assign(F, 0u);
        out->centre.assign(1, 0u); out->cluster_size.assign(1, (uint32_t)F);
        return want_counts ? cluster_counts_host(0, 1, out) : ARP_OK;
    }
    // 3. the bit transpose: frames become the bit-rows
    uint32_t *wordsT = nullptr;
    DevBlock block;
    if ((s = block.carve([&](Bump &bp) { wordsT = bp.take<uint32_t>(F * WR); })) != ARP_OK) return s;
    if ((s = bit_transpose_launch(st, dev.words, R, W, F, wordsT, WR)) != ARP_OK) return s;
    lap("transpose");
    // 4. neighbour bits, rounds, counts
    ClusterDev dv;
    if ((s = cluster_launch(st, wordsT, F, WR, min_similarity, max_clusters, lap, &dv)) != ARP_OK) return s;
    const uint64_t C = dv.best.size();
    if (want_counts) {
        if ((s = cluster_counts_launch(st, dev.words, R, W, C, cap_bytes, &dv)) != ARP_OK || (s = cluster_counts_host(R, C, out)) != ARP_OK) return s;
        lap("counts");
    }
    // 5. download: the vectors, the counts, the rows' popcounts of k_timeline_stats and the error word of the marks -- no F x F anything
    uint32_t h_err = 0;
    std::vector<uint32_t> count(R);
    HIP_TRY(hipMemcpyAsync(&h_err, dev.err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(count.data(), dev.stat[4], R * 4, hipMemcpyDeviceToHost, st));
    if ((s = cluster_download(st, dv, F, R, out)) != ARP_OK) return s;
    HIP_TRY(hipStreamSynchronize(st));
    lap("download");
    if (h_err) { set_error(h_err & 1u ? "internal error: timeline item without a row" : "internal error: timeline item outside the frames"); return ARP_ERR_HIP; }
    for (uint64_t r = 0; r < R; r++)
        if (count[r] != rows->count[r]) {
            set_error("internal error: timeline row %llu has %u frames marked, the frequency table counts %u", (unsigned long long)r, count[r], rows->count[r]);
            return ARP_ERR_HIP;
        }
    return cluster_verify(*out, R, rows->count.data());
}

// a host bitmap through the same kernels: upload, clear the bits past n_bits, (transpose,) neighbour bits, rounds, (counts,) download (rows > 0, n_bits > 0)
arp_status device_bit_cluster(arp_context *ctx, uint64_t rows, uint64_t n_bits, const uint32_t *words, bool by_rows, float min_similarity, uint32_t max_clusters, bool want_counts,
                              uint64_t cap_bytes, ClustersHost *out) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(context_device(ctx)));
    StreamLapTimer lap("  bit cluster %-10s %8.3f ms\n", st);
    *out = ClustersHost{};
    const uint64_t W = (n_bits + 31u) / 32u, WR = (rows + 31u) / 32u, M = by_rows ? rows : n_bits;
    arp_status s = cluster_cap_check(M, by_rows, cap_bytes);
    if (s != ARP_OK) return s;
    if (rows * W * 4u > (1ull << 31)) { set_error("bit cluster: a bitmap of %llu rows x %llu bits is more than 2^31 bytes", (unsigned long long)rows, (unsigned long long)n_bits); return ARP_ERR_CAPACITY; }
    uint32_t *d_words = nullptr, *wordsT = nullptr;
    DevBlock block;
    if ((s = block.carve([&](Bump &bp) {
            d_words = bp.take<uint32_t>(rows * W);
            if (!by_rows) wordsT = bp.take<uint32_t>(n_bits * WR);
        })) != ARP_OK) return s;
    HIP_TRY(hipMemcpyAsync(d_words, words, rows * W * 4u, hipMemcpyHostToDevice, st));
    if (n_bits & 31u) {
        hipLaunchKernelGGL(k_bit_mask_tail, dim3((uint32_t)((rows + 255u) / 256u)), dim3(256), 0, st, d_words, rows, W, (1u << (n_bits & 31u)) - 1u);
        HIP_TRY(hipGetLastError());
    }
    const uint32_t *A = d_words;
    uint64_t K = W;
    if (!by_rows) {
        if ((s = bit_transpose_launch(st, d_words, rows, W, n_bits, wordsT, WR)) != ARP_OK) return s;
        A = wordsT;
        K = WR;
    }
    ClusterDev dv;
    if ((s = cluster_launch(st, A, M, K, min_similarity, max_clusters, lap, &dv)) != ARP_OK) return s;
    out->has_counts = want_counts;
    if (want_counts && ((s = cluster_counts_launch(st, d_words, rows, W, dv.best.size(), cap_bytes, &dv)) != ARP_OK || (s = cluster_counts_host(rows, dv.best.size(), out)) != ARP_OK))
        return s;
    if ((s = cluster_download(st, dv, M, rows, out)) != ARP_OK) return s;
    HIP_TRY(hipStreamSynchronize(st));
    return cluster_verify(*out, 0, nullptr);
}
