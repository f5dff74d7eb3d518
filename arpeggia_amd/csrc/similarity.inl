// Frame-by-frame contact similarity and contact co-occurrence (arp_contact_similarity, arp_bit_gram).  Included by
// table_dev.hip inside namespace arp, behind timeline.inl.
//
// Both questions are the Gram matrix of a bit matrix A[M][K words]: inter[a][b] = sum over words of popcount(A[a][w] & A[b][w]).
//   axis "rows"    A = the timeline bitmap words[R][W] as it is: M = R bit-rows of F bits
//   axis "frames"  A = its bit transpose wordsT[F][WR] (k_bit_transpose): M = F bit-rows of R bits
// k_bit_sizes counts every bit-row, k_bit_gram computes the upper tile triangle and writes every tile and its mirror, as counts or as
// Tanimoto values f32((double)inter / (double)(size_a + size_b - inter)), 1.0f for an empty union.  Integer sums and one IEEE divide per
// element: the bytes do not depend on the tile schedule.

constexpr uint32_t kSimTile = 64;                // output tile edge of k_bit_gram: 16 x 16 lanes, 4 x 4 accumulators each
constexpr uint32_t kSimChunk = 32;               // words of K staged through LDS per step
constexpr uint32_t kSimReg = kSimTile / 16u;     // register tile edge
constexpr uint32_t kSimLds = kSimChunk + 4u;     // LDS row stride in words: 144 bytes, so 16 rows' 16-byte reads fall into 16 different slots of the 256-byte bank row
constexpr uint32_t kSimMirror = kSimTile + 1u;   // row stride of the epilogue's tile image: its transposed reads walk the banks

// bits past n_bits in every row's last word are cleared in place (a host bitmap may carry anything there; the table's own bitmaps carry zeros)
__global__ __launch_bounds__(256) void k_bit_mask_tail(uint32_t *words, uint64_t rows, uint64_t W, uint32_t mask) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) words[r * W + (W - 1u)] &= mask;
}

// words[R][W] (frame f = bit f & 31 of word f >> 5) -> wordsT[F][WR] (row r = bit r & 31 of word r >> 5), WR = ceil(R / 32).  A half wave takes one
// tile of 32 rows x 32 frames: lane l holds the word of row 32 rt + l, ballot b collects bit b of all 32 rows, which is the output word of frame
// 32 wt + b, and lane b keeps it.  The two halves of a wave and the four waves of a block take eight neighbouring words of the same 32 rows.
// Rows past R read as zero (the unused high bits of an output row's last word); frames past F are not written.
__global__ __launch_bounds__(256) void k_bit_transpose(const uint32_t *words, uint32_t R, uint64_t W, uint32_t F, uint32_t *wordsT, uint64_t WR, uint32_t n_wblocks) {
    const uint32_t lane = threadIdx.x & 63u, half = lane >> 5, l = lane & 31u;
    const uint32_t rt = blockIdx.x / n_wblocks;
    const uint64_t wt = (uint64_t)(blockIdx.x % n_wblocks) * 8u + (threadIdx.x >> 6) * 2u + half;
    const uint64_t r = (uint64_t)rt * 32u + l;
    const uint32_t v = (r < R && wt < W) ? words[r * W + wt] : 0u;
    uint32_t mine = 0u;
    for (uint32_t b = 0; b < 32u; b++) {
        const unsigned long long m = __ballot((v >> b) & 1u);
        if ((lane & 31u) == b) mine = (uint32_t)(m >> (half * 32u));
    }
    const uint64_t f = wt * 32u + l;
    if (f < F) wordsT[f * WR + rt] = mine;  // (f < F implies wt < W)
}

// one wave per bit-row: its number of set bits
__global__ __launch_bounds__(256) void k_bit_sizes(const uint32_t *A, uint32_t M, uint64_t K, uint64_t stride, uint32_t *sizes) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= M) return;  // (the whole wave)
    const uint32_t *row = A + (size_t)r * stride;
    uint32_t c = 0;
    for (uint64_t w = lane; w < K; w += 64u) c += (uint32_t)__popc(row[w]);
    for (uint32_t off = 32u; off; off >>= 1) c += (uint32_t)__shfl_down((int)c, off);
    if (lane == 0u) sizes[r] = c;
}

// Block t of the upper tile triangle (T tiles per edge, row by row: (0, 0) .. (0, T - 1), (1, 1) ..) computes tile (ti, tj), tj >= ti.  The 64 A rows
// of ti and the 64 of tj go through LDS in chunks of kSimChunk words, row-major with stride kSimLds; the words of the next chunk are fetched into
// registers while the current one is consumed.  Lane (tx, ty) owns outputs (ty + 16 i, tx + 16 j) and reads its rows four words at a time.  Rows past
// M and words past K are staged as zeros.  The epilogue writes the tile from registers and, off the diagonal, its mirror through an LDS image so
// that both are written along output rows.  out: u32 counts, or the bits of the f32 Tanimoto values.
template <bool TANIMOTO>
__global__ __launch_bounds__(256) void k_bit_gram(const uint32_t *A, uint32_t M, uint64_t K, uint64_t stride, const uint32_t *sizes, uint32_t T, uint32_t *out) {
    static_assert(2u * kSimTile * kSimLds >= kSimTile * kSimMirror, "the epilogue's tile image reuses the staging buffer");
    __shared__ __attribute__((aligned(16))) uint32_t lds[2u * kSimTile * kSimLds];
    uint32_t t = blockIdx.x, ti = 0;
    while (t >= T - ti) { t -= T - ti; ti++; }
    const uint32_t tj = ti + t;
    const uint32_t row0 = ti * kSimTile, col0 = tj * kSimTile;
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;
    const uint32_t lk = threadIdx.x & 31u, lr = threadIdx.x >> 5;  // staging: word lk of rows lr, lr + 8, ..
    uint32_t *sA = lds, *sB = lds + kSimTile * kSimLds;
    uint32_t acc[kSimReg][kSimReg] = {};
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
    // the tile, from registers
    uint32_t sa[kSimReg], sb[kSimReg];
#pragma unroll
    for (uint32_t i = 0; i < kSimReg; i++) {
        const uint32_t r = row0 + ty + 16u * i, c = col0 + tx + 16u * i;
        sa[i] = (TANIMOTO && r < M) ? sizes[r] : 0u;
        sb[i] = (TANIMOTO && c < M) ? sizes[c] : 0u;
    }
#pragma unroll
    for (uint32_t i = 0; i < kSimReg; i++)
#pragma unroll
        for (uint32_t j = 0; j < kSimReg; j++) {
            if constexpr (TANIMOTO) {
                const unsigned long long uni = (unsigned long long)sa[i] + sb[j] - acc[i][j];
                acc[i][j] = uni ? __float_as_uint((float)((double)acc[i][j] / (double)uni)) : 0x3F800000u;  // (an empty union: two identical sets)
            }
            const uint32_t r = row0 + ty + 16u * i, c = col0 + tx + 16u * j;
            if (r < M && c < M) out[(size_t)r * M + c] = acc[i][j];
        }
    // its mirror (a diagonal tile is its own): element (r, c) of the tile is element (c, r) of tile (tj, ti)
    if (ti != tj) {
#pragma unroll
        for (uint32_t i = 0; i < kSimReg; i++)
#pragma unroll
            for (uint32_t j = 0; j < kSimReg; j++) lds[(ty + 16u * i) * kSimMirror + tx + 16u * j] = acc[i][j];
        __syncthreads();
#pragma unroll
        for (uint32_t i = 0; i < kSimReg; i++)
#pragma unroll
            for (uint32_t j = 0; j < kSimReg; j++) {
                const uint32_t c = ty + 16u * i, r = tx + 16u * j;
                if (col0 + c < M && row0 + r < M) out[(size_t)(col0 + c) * M + row0 + r] = lds[r * kSimMirror + c];
            }
    }
}

namespace {
// sizes and the matrix of A[M][K words] (row stride `stride`), both on the device
arp_status bit_gram_launch(hipStream_t st, const uint32_t *A, uint64_t M, uint64_t K, uint64_t stride, bool counts, uint32_t *d_sizes, uint32_t *d_out) {
    if (!M) return ARP_OK;
    hipLaunchKernelGGL(k_bit_sizes, dim3((uint32_t)((M + 3u) / 4u)), dim3(256), 0, st, A, (uint32_t)M, K, stride, d_sizes);
    HIP_TRY(hipGetLastError());
    const uint32_t T = (uint32_t)((M + kSimTile - 1u) / kSimTile);
    const auto kernel = counts ? k_bit_gram<false> : k_bit_gram<true>;
    hipEvent_t ev[2] = {nullptr, nullptr};  // the knob "timing": the kernel alone, from events
    if (g_debug.timing) { HIP_TRY(hipEventCreate(&ev[0])); HIP_TRY(hipEventCreate(&ev[1])); HIP_TRY(hipEventRecord(ev[0], st)); }
    hipLaunchKernelGGL(kernel, dim3((uint32_t)((uint64_t)T * (T + 1u) / 2u)), dim3(256), 0, st, A, (uint32_t)M, K, stride, (const uint32_t *)d_sizes, T, d_out);
    HIP_TRY(hipGetLastError());
    if (ev[0]) {
        float ms = 0.f;
        HIP_TRY(hipEventRecord(ev[1], st));
        HIP_TRY(hipEventSynchronize(ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        fprintf(stderr, "  similarity k_bit_gram %8.3f ms  (M %llu, K %llu words)\n", ms, (unsigned long long)M, (unsigned long long)K);
        (void)hipEventDestroy(ev[0]); (void)hipEventDestroy(ev[1]);
    }
    return ARP_OK;
}
arp_status bit_transpose_launch(hipStream_t st, const uint32_t *words, uint64_t R, uint64_t W, uint64_t F, uint32_t *wordsT, uint64_t WR) {
    const uint64_t n_wblocks = (W + 7u) / 8u;
    if (n_wblocks * WR > 0x7FFFFFFFull) { set_error("bit transpose: %llu rows x %llu bits are more tiles than one launch takes", (unsigned long long)R, (unsigned long long)F); return ARP_ERR_CAPACITY; }
    hipLaunchKernelGGL(k_bit_transpose, dim3((uint32_t)(n_wblocks * WR)), dim3(256), 0, st, words, (uint32_t)R, W, (uint32_t)F, wordsT, WR, (uint32_t)n_wblocks);
    HIP_TRY(hipGetLastError());
    return ARP_OK;
}
arp_status similarity_cap_check(uint64_t M, bool by_rows, uint64_t cap_bytes) {
    constexpr uint64_t kMaxEdge = 1ull << 21;  // (the tile triangle of one launch; such a matrix is 16 TB)
    if (M >= kMaxEdge || M * M * 4u > cap_bytes) {
        set_error("contact similarity: the matrix of axis %s, M = %llu, needs %llu bytes, the limit is %llu (similarity_cap_bytes)", by_rows ? "rows" : "frames",
                  (unsigned long long)M, (unsigned long long)(M >= (1ull << 31) ? ~0ull : M * M * 4u), (unsigned long long)cap_bytes);
        return ARP_ERR_CAPACITY;
    }
    return ARP_OK;
}
}  // namespace

arp_status device_similarity(arp_context *ctx, const FreqJob &job, bool by_rows, bool counts, uint64_t timeline_cap_bytes, uint64_t cap_bytes, FreqRowsHost *rows,
                             SimilarityHost *out) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(context_device(ctx)));
    StreamLapTimer lap("  similarity %-10s %8.3f ms\n", st);
    *out = SimilarityHost{};
    // 1. + 2. rows and marks (timeline.inl); the matrix is refused as soon as its edge is known
    TimelineDev dev;
    const uint64_t F = job.n_frames;
    arp_status s = timeline_device(ctx, job, timeline_cap_bytes, rows, &dev, lap,
                                   [&](uint64_t R) { return similarity_cap_check(by_rows ? R : F, by_rows, cap_bytes); });
    if (s != ARP_OK) return s;
    const uint64_t R = rows->key.size(), W = (F + 31u) / 32u, WR = (R + 31u) / 32u, M = by_rows ? R : F;
    out->m = M;
    out->sizes.assign(M, 0u);
    // the matrix lands in host memory that the table then owns: a pooled pinned block when it is large (the copy is most of the call at 10^4 frames)
    const size_t bytes = std::max<size_t>((size_t)(M * M * 4u), 4u);
    if (bytes >= (1u << 20)) {
        out->owner = pinned_block(bytes);
        if (!out->owner) { set_error("out of pinned host memory for the similarity matrix"); return ARP_ERR_OOM; }
    } else {
        char *heap = (char *)malloc(bytes);
        if (!heap) { set_error("out of host memory"); return ARP_ERR_OOM; }
        out->owner = std::shared_ptr<char>(heap, [](char *q) { free(q); });
    }
    out->matrix = reinterpret_cast<uint32_t *>(out->owner.get());
    if (R == 0) {  // no contact in any frame: F empty sets (identical: 1.0), or no rows at all
        for (uint64_t k = 0; k < M * M; k++) out->matrix[k] = counts ? 0u : 0x3F800000u;
        return ARP_OK;
    }
    uint32_t *d_out = nullptr, *d_sizes = nullptr, *wordsT = nullptr;
    DevBlock block;
    if ((s = block.carve([&](Bump &bp) {
            d_out = bp.take<uint32_t>(M * M); d_sizes = bp.take<uint32_t>(M);
            if (!by_rows) wordsT = bp.take<uint32_t>(F * WR);
        })) != ARP_OK) return s;
    const uint32_t *A = dev.words;
    uint64_t K = W;
    if (!by_rows) {  // 3. the bit transpose: frames become the bit-rows
        if ((s = bit_transpose_launch(st, dev.words, R, W, F, wordsT, WR)) != ARP_OK) return s;
        A = wordsT;
        K = WR;
    }
    lap("transpose");
    // 4. sizes and the matrix
    if ((s = bit_gram_launch(st, A, M, K, K, counts, d_sizes, d_out)) != ARP_OK) return s;
    lap("gram");
    // 5. download: the matrix, the sizes, the rows' popcounts of k_timeline_stats and the error word of the marks
    uint32_t h_err = 0;
    std::vector<uint32_t> count(R);
    HIP_TRY(hipMemcpyAsync(&h_err, dev.err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(count.data(), dev.stat[4], R * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->sizes.data(), d_sizes, M * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->matrix, d_out, M * M * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lap("download");
    if (h_err) { set_error(h_err & 1u ? "internal error: timeline item without a row" : "internal error: timeline item outside the frames"); return ARP_ERR_HIP; }
    for (uint64_t r = 0; r < R; r++)
        if (count[r] != rows->count[r] || (by_rows && out->sizes[r] != rows->count[r])) {
            set_error("internal error: timeline row %llu has %u frames marked (sizes: %u), the frequency table counts %u", (unsigned long long)r, count[r],
                      by_rows ? out->sizes[r] : count[r], rows->count[r]);
            return ARP_ERR_HIP;
        }
    return ARP_OK;
}

// a host bitmap through the same kernels: upload, clear the bits past n_bits, (transpose,) sizes, matrix, download
arp_status device_bit_gram(arp_context *ctx, uint64_t rows, uint64_t n_bits, const uint32_t *words, bool by_rows, bool counts, uint64_t cap_bytes, void *out, uint32_t *sizes) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(context_device(ctx)));
    const uint64_t W = (n_bits + 31u) / 32u, WR = (rows + 31u) / 32u, M = by_rows ? rows : n_bits;
    arp_status s = similarity_cap_check(M, by_rows, cap_bytes);
    if (s != ARP_OK) return s;
    if (rows * W * 4u > (1ull << 31)) { set_error("bit gram: a bitmap of %llu rows x %llu bits is more than 2^31 bytes", (unsigned long long)rows, (unsigned long long)n_bits); return ARP_ERR_CAPACITY; }
    uint32_t *d_words = nullptr, *d_out = nullptr, *d_sizes = nullptr, *wordsT = nullptr;
    DevBlock block;
    if ((s = block.carve([&](Bump &bp) {
            d_words = bp.take<uint32_t>(rows * W); d_out = bp.take<uint32_t>(M * M); d_sizes = bp.take<uint32_t>(M);
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
    if ((s = bit_gram_launch(st, A, M, K, K, counts, d_sizes, d_out)) != ARP_OK) return s;
    HIP_TRY(hipMemcpyAsync(sizes, d_sizes, M * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out, d_out, M * M * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return ARP_OK;
}
