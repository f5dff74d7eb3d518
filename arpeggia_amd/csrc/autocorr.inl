// Contact autocorrelation and survival curves across frames (arp_contact_autocorrelation, arp_bit_autocorr).  Included by
// table_dev.hip inside namespace arp, behind similarity.inl.
//
// Per row r of the timeline bitmap words[R][W] (F bits, the bits past F zero) and per lag t = 0 .. L:
//   intermittent  acf[r][t] = #{ f < F - t : bit f and bit f + t }                    k_acf_intermittent: AND + popcount over a shifted copy of the row
//   continuous    acf[r][t] = #{ f < F - t : bits f .. f + t } = sum over the row's maximal runs of max(0, length - t)
//                                                                                     k_acf_runs lists the run lengths, k_acf_continuous sums them
// Both kernels give one lane one lag of one row and end in acf_epilogue: the count goes to the matrix (unless ARP_ACF_NO_MATRIX), lag 0 to lag0[r], the
// smallest lag that passes the half-life predicate to half[r] (atomicMin) and the count into sums[group of r][t] (u64 atomicAdd).  Integer sums and
// minima only: the bytes do not depend on scheduling.

constexpr uint32_t kAcfLagsPerWave = 64;                      // a lane owns one lag
constexpr uint32_t kAcfLagsPerBlock = 256;                    // the lag tile of a workgroup: four waves
constexpr uint32_t kAcfOverlap = kAcfLagsPerBlock / 32u;      // words the shifted operand of a tile's last lag lies past its first lag's
constexpr uint32_t kAcfChunkWords = 512;                      // words of a row staged through LDS per step (2 KiB + the shifted window)
constexpr uint32_t kAcfRowsPerBlock = 4;                      // k_acf_runs: one wave per row
constexpr uint32_t kAcfRunChunk = 1024;                       // run lengths of a row staged through LDS per step (k_acf_continuous)
constexpr uint64_t kAcfMaxBlocks = (1ull << 24) - 1u;         // blocks of one launch: 256 lanes each, and fewer than 2^32 threads in all

// 2 acf F <= n0 (F - t), the window-corrected estimator at or below one half.  Both products are below 2^64 and the left one is an integer, so
// comparing it with the halved right one is the same test without the factor's overflow.
__device__ inline bool acf_half_passed(uint32_t acf, uint32_t n0, uint32_t F, uint32_t t) {
    return (unsigned long long)acf * F <= (((unsigned long long)n0 * (F - t)) >> 1);
}

struct AcfOut {
    uint32_t L, F, n_groups;
    const uint32_t *n0;                   // per row: its set bits (k_timeline_stats)
    const unsigned long long *row_keys;   // the group of a row is the code in its key's low bits ...
    const uint32_t *group;                // ... or, when given, group[r]; neither: no sums
    uint32_t *matrix;                     // R x (L + 1), or nullptr
    uint32_t *lag0, *half;                // per row; half starts as ARP_NONE
    unsigned long long *sums;             // n_groups x (L + 1), zeroed
};

// every lane of the block calls this with its lag t (lanes of a wave hold consecutive lags) and its count
__device__ inline void acf_epilogue(const AcfOut &o, uint32_t r, uint32_t t, uint32_t acf) {
    const bool mine = t <= o.L;
    if (mine) {
        if (o.matrix) o.matrix[(size_t)r * (o.L + 1u) + t] = acf;
        if (t == 0u) o.lag0[r] = acf;
        if (acf && (o.group || o.row_keys)) {
            const uint32_t g = o.group ? o.group[r] : (uint32_t)(o.row_keys[r] & ((1ull << kFreqCodeBits) - 1ull));
            if (g < o.n_groups) atomicAdd(o.sums + (size_t)g * (o.L + 1u) + t, (unsigned long long)acf);
        }
    }
    const unsigned long long passed = __ballot(mine && t >= 1u && acf_half_passed(acf, o.n0[r], o.F, t));
    if (passed && (threadIdx.x & (kAcfLagsPerWave - 1u)) == 0u) atomicMin(o.half + r, t + (uint32_t)__ffsll((long long)passed) - 1u);
}

// Block b: row b / n_tiles, lags t0 = 256 (b % n_tiles) .. t0 + 255.  Lane t = t0 + tid shifts by q = t >> 5 words and s = t & 31 bits: bit f + t of the
// row is bit s of word (f >> 5) + q for the first bit of a word, so the word that lines up with row[w] is the funnel shift of row[w + q + 1] : row[w + q]
// by s.  Window A holds row[c0 ..] (the same address for every lane: a broadcast), window B holds row[c0 + (t0 >> 5) ..] with kAcfOverlap words more,
// which is as far as the tile's last lag reaches; words past W are staged as zeros, and words from W - (t0 >> 5) on meet only zeros, so the chunks end there.
__global__ __launch_bounds__(kAcfLagsPerBlock) void k_acf_intermittent(const uint32_t *__restrict__ words, uint64_t W, uint32_t n_tiles, AcfOut o) {
    __shared__ uint32_t sA[kAcfChunkWords], sB[kAcfChunkWords + kAcfOverlap];
    const uint32_t r = blockIdx.x / n_tiles, t0 = (blockIdx.x % n_tiles) * kAcfLagsPerBlock;
    const uint32_t tid = threadIdx.x, q = tid >> 5, s = tid & 31u;
    const uint32_t *row = words + (size_t)r * W;
    const uint64_t q0 = t0 >> 5, Wt = W - q0;  // (t0 <= L < F, so q0 < W)
    uint32_t acc = 0;
    for (uint64_t c0 = 0; c0 < Wt; c0 += kAcfChunkWords) {
        for (uint32_t i = tid; i < kAcfChunkWords + kAcfOverlap; i += kAcfLagsPerBlock) {
            if (i < kAcfChunkWords) sA[i] = c0 + i < W ? row[c0 + i] : 0u;
            sB[i] = c0 + q0 + i < W ? row[c0 + q0 + i] : 0u;
        }
        __syncthreads();
        const uint32_t nw = (uint32_t)min((uint64_t)kAcfChunkWords, Wt - c0);
        uint32_t lo = sB[q];
#pragma unroll 4
        for (uint32_t w = 0; w < nw; w++) {
            const uint32_t hi = sB[w + q + 1u];
            const uint32_t shifted = (uint32_t)((((unsigned long long)hi << 32) | lo) >> s);
            acc += (uint32_t)__popc(sA[w] & shifted);
            lo = hi;
        }
        __syncthreads();
    }
    acf_epilogue(o, r, t0 + tid, acc);
}

// One wave per row lists the lengths of the row's maximal runs in runs[off[r] ..], 64 words per step, lane l the word step + l.  A run is filed by the
// lane in whose word it ends (bit set, next bit of the row clear); its length is counted inside that word down to the nearest zero, and when there is
// none, the run came in from the words before: `entering` is the run of ones that ends with the previous word, from a scan over the lanes of
// (ones at the top of the word, word all ones) and the carry of the steps before.  The place of a lane's runs is the exclusive prefix of the lanes' end
// counts.  off comes from the rows' n_events (k_timeline_stats): a row has exactly off[r + 1] - off[r] ends, and nothing is written past them.
__global__ __launch_bounds__(64 * kAcfRowsPerBlock) void k_acf_runs(const uint32_t *__restrict__ words, uint32_t n_rows, uint64_t W, const unsigned long long *__restrict__ off,
                                                                    uint32_t *runs) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * kAcfRowsPerBlock + (threadIdx.x >> 6);
    if (r >= n_rows) return;  // (the whole wave)
    const uint32_t *row = words + (size_t)r * W;
    unsigned long long at = off[r];
    const unsigned long long end = off[r + 1u];
    uint32_t carry = 0;  // the run of ones that ends with the last word of the steps so far
    for (uint64_t step = 0; step < W; step += 64u) {
        const uint64_t w = step + lane;
        const uint32_t x = w < W ? row[w] : 0u;
        uint32_t next = (uint32_t)__shfl_down((int)x, 1);
        if (lane == 63u) next = step + 64u < W ? row[step + 64u] : 0u;
        const uint32_t ends = x & ~((x >> 1) | (next << 31));
        const uint32_t n_ends = (uint32_t)__popc(ends);
        uint32_t before = n_ends;  // inclusive prefix of the end counts, made exclusive below
        uint32_t top = x == 0xFFFFFFFFu ? 32u : (uint32_t)__clz((int)~x), all = x == 0xFFFFFFFFu ? 1u : 0u;  // of the span of words that ends with this lane's
        for (uint32_t o = 1; o < 64u; o <<= 1) {
            const uint32_t b_o = (uint32_t)__shfl_up((int)before, o), top_o = (uint32_t)__shfl_up((int)top, o), all_o = (uint32_t)__shfl_up((int)all, o);
            if (lane >= o) {
                before += b_o;
                if (all) top += top_o;
                all &= all_o;
            }
        }
        const uint32_t total = (uint32_t)__shfl((int)before, 63);
        before -= n_ends;
        uint32_t entering = (uint32_t)__shfl_up((int)(top + (all ? carry : 0u)), 1);
        if (lane == 0u) entering = carry;
        carry = (uint32_t)__shfl((int)(top + (all ? carry : 0u)), 63);
        uint32_t k = 0;
        for (uint32_t b = ends; b; b &= b - 1u, k++) {
            const uint32_t e = (uint32_t)__ffs((int)b) - 1u;
            const uint32_t zeros_below = ~x & ((1u << e) - 1u);
            const uint32_t len = zeros_below ? e - (31u - (uint32_t)__clz((int)zeros_below)) : e + 1u + entering;
            const unsigned long long p = at + before + k;
            if (p < end) runs[p] = len;
        }
        at += total;
    }
}

// Block b: row b / n_tiles, lags t0 .. t0 + 255 as above; the row's run lengths go through LDS in chunks and lane t adds max(0, length - t).  A tile
// whose first lag is not below the row's longest run has nothing to add.
__global__ __launch_bounds__(kAcfLagsPerBlock) void k_acf_continuous(const uint32_t *__restrict__ runs, const unsigned long long *__restrict__ off, const uint32_t *__restrict__ longest,
                                                                     uint32_t n_tiles, AcfOut o) {
    __shared__ uint32_t sR[kAcfRunChunk];
    const uint32_t r = blockIdx.x / n_tiles, t0 = (blockIdx.x % n_tiles) * kAcfLagsPerBlock;
    const uint32_t tid = threadIdx.x, t = t0 + tid;
    uint32_t acc = 0;
    if (t0 < longest[r]) {  // (the whole block)
        const unsigned long long a = off[r], b = off[r + 1u];
        for (unsigned long long c0 = a; c0 < b; c0 += kAcfRunChunk) {
            const uint32_t n = (uint32_t)min((unsigned long long)kAcfRunChunk, b - c0);
            for (uint32_t i = tid; i < n; i += kAcfLagsPerBlock) sR[i] = runs[c0 + i];
            __syncthreads();
            for (uint32_t i = 0; i < n; i++) { const uint32_t len = sR[i]; acc += len > t ? len - t : 0u; }
            __syncthreads();
        }
    }
    acf_epilogue(o, r, t, acc);
}

namespace {
arp_status autocorr_cap_check(uint64_t R, uint64_t L, uint64_t cap_bytes) {
    const uint64_t cells = R * (L + 1u);  // (rows and lags are at most 2^32 each: their product fits, four times it may not)
    const uint64_t need = cells > (~0ull >> 2) ? ~0ull : cells * 4u;
    if (need > cap_bytes) {
        set_error("contact autocorrelation: the matrix of %llu rows x %llu lags needs %llu bytes, the limit is %llu (autocorr_cap_bytes)", (unsigned long long)R,
                  (unsigned long long)(L + 1u), (unsigned long long)need, (unsigned long long)cap_bytes);
        return ARP_ERR_CAPACITY;
    }
    return ARP_OK;
}

// The device buffers of one autocorrelation and the kernels on a device bitmap with its k_timeline_stats results (n_events, longest, count).
struct AcfDev {
    DevBlock block, runs;
    uint32_t *matrix = nullptr, *lag0 = nullptr, *half = nullptr, *group = nullptr;
    unsigned long long *sums = nullptr;
};
// group_host: nullable; row_keys (device): nullable.  want_matrix false: no R x (L + 1) buffer exists.
arp_status acf_launch(hipStream_t st, const uint32_t *words, uint64_t R, uint64_t W, uint64_t F, uint64_t L, bool continuous, bool want_matrix, const unsigned long long *row_keys,
                      const uint32_t *group_host, uint64_t n_groups, const uint32_t *d_events, const uint32_t *d_longest, const uint32_t *d_count, AcfDev *dv) {
    const uint64_t n_lags = L + 1u, n_tiles = (n_lags + kAcfLagsPerBlock - 1u) / kAcfLagsPerBlock;
    // one launch: a block per row and lag tile, and the runtime takes fewer than 2^32 threads per launch
    if (R * n_tiles > kAcfMaxBlocks) {
        set_error("contact autocorrelation: %llu rows x %llu lags are %llu lag tiles, one launch takes %llu (lower max_lag, or cut the rows)", (unsigned long long)R,
                  (unsigned long long)n_lags, (unsigned long long)(R * n_tiles), (unsigned long long)kAcfMaxBlocks);
        return ARP_ERR_CAPACITY;
    }
    const bool with_sums = (row_keys || group_host) && n_groups;
    if (with_sums && n_groups * n_lags * 8u > (1ull << 31)) { set_error("contact autocorrelation: the sums of %llu groups x %llu lags are more than 2^31 bytes", (unsigned long long)n_groups, (unsigned long long)n_lags); return ARP_ERR_CAPACITY; }
    arp_status s;
    if ((s = dv->block.carve([&](Bump &bp) {
            dv->matrix = want_matrix ? bp.take<uint32_t>(R * n_lags) : nullptr;
            dv->lag0 = bp.take<uint32_t>(R); dv->half = bp.take<uint32_t>(R); dv->group = bp.take<uint32_t>(R);
            dv->sums = with_sums ? bp.take<unsigned long long>(n_groups * n_lags) : nullptr; bp.take<char>(256);  // (slack)
        })) != ARP_OK) return s;
    HIP_TRY(hipMemsetAsync(dv->half, 0xFF, R * 4u, st));
    if (with_sums) HIP_TRY(hipMemsetAsync(dv->sums, 0, n_groups * n_lags * 8u, st));
    if (group_host) HIP_TRY(hipMemcpyAsync(dv->group, group_host, R * 4u, hipMemcpyHostToDevice, st));
    AcfOut o{(uint32_t)L, (uint32_t)F, with_sums ? (uint32_t)n_groups : 0u, d_count, with_sums && !group_host ? row_keys : nullptr, with_sums && group_host ? dv->group : nullptr,
             dv->matrix, dv->lag0, dv->half, dv->sums};
    struct Events {  // the knob "timing": the kernels alone, from events (destroyed on every way out)
        hipEvent_t ev[2] = {nullptr, nullptr};
        ~Events() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
    } events_owner;
    hipEvent_t(&ev)[2] = events_owner.ev;
    auto stamp = [&](int k) -> arp_status { if (g_debug.timing) { if (!ev[k]) HIP_TRY(hipEventCreate(&ev[k])); HIP_TRY(hipEventRecord(ev[k], st)); } return ARP_OK; };
    if (!continuous) {
        if ((s = stamp(0)) != ARP_OK) return s;
        hipLaunchKernelGGL(k_acf_intermittent, dim3((uint32_t)(R * n_tiles)), dim3(kAcfLagsPerBlock), 0, st, words, W, (uint32_t)n_tiles, o);
        HIP_TRY(hipGetLastError());
    } else {
        // the rows' run lists: offsets from the rows' n_events (one small round trip), lengths by k_acf_runs
        std::vector<uint32_t> events(R);
        HIP_TRY(hipMemcpyAsync(events.data(), d_events, R * 4u, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        std::vector<unsigned long long> off(R + 1u, 0ull);
        for (uint64_t r = 0; r < R; r++) off[r + 1u] = off[r] + events[r];
        const uint64_t total = off[R];
        if (total * 4u > (1ull << 31)) { set_error("contact autocorrelation: the run list of %llu runs is more than 2^31 bytes", (unsigned long long)total); return ARP_ERR_CAPACITY; }
        unsigned long long *d_off = nullptr; uint32_t *d_runs = nullptr;
        if ((s = dv->runs.carve([&](Bump &rp) {
                d_off = rp.take<unsigned long long>(R + 1u); d_runs = rp.take<uint32_t>(total); rp.take<char>(256);  // (slack)
            })) != ARP_OK) return s;
        HIP_TRY(hipMemcpyAsync(d_off, off.data(), (R + 1u) * 8u, hipMemcpyHostToDevice, st));
        if ((s = stamp(0)) != ARP_OK) return s;
        hipLaunchKernelGGL(k_acf_runs, dim3((uint32_t)((R + kAcfRowsPerBlock - 1u) / kAcfRowsPerBlock)), dim3(64 * kAcfRowsPerBlock), 0, st, words, (uint32_t)R, W,
                           (const unsigned long long *)d_off, d_runs);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_acf_continuous, dim3((uint32_t)(R * n_tiles)), dim3(kAcfLagsPerBlock), 0, st, (const uint32_t *)d_runs, (const unsigned long long *)d_off, d_longest,
                           (uint32_t)n_tiles, o);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st));  // (off is the host's: it must outlive its copy)
    }
    if (ev[0]) {
        float ms = 0.f;
        if ((s = stamp(1)) != ARP_OK) return s;
        HIP_TRY(hipEventSynchronize(ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        fprintf(stderr, "  autocorr %s %8.3f ms  (rows %llu, words %llu, lags %llu)\n", continuous ? "k_acf_runs+k_acf_continuous" : "k_acf_intermittent", ms, (unsigned long long)R,
                (unsigned long long)W, (unsigned long long)n_lags);
    }
    return ARP_OK;
}
}  // namespace

arp_status device_autocorrelation(arp_context *ctx, const FreqJob &job, bool continuous, bool want_matrix, uint64_t L, uint64_t timeline_cap_bytes, uint64_t cap_bytes,
                                  FreqRowsHost *rows, AutocorrHost *out) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(context_device(ctx)));
    StreamLapTimer lap("  autocorr %-10s %8.3f ms\n", st);
    *out = AutocorrHost{};
    // 1. + 2. rows and marks (timeline.inl); the matrix is refused as soon as its height is known
    TimelineDev dev;
    const uint64_t F = job.n_frames, n_lags = L + 1u, G = ARP_N_INTERACTIONS;
    arp_status s = timeline_device(ctx, job, timeline_cap_bytes, rows, &dev, lap, [&](uint64_t R) { return want_matrix ? autocorr_cap_check(R, L, cap_bytes) : ARP_OK; });
    if (s != ARP_OK) return s;
    const uint64_t R = rows->key.size(), W = (F + 31u) / 32u;
    out->n_lags = n_lags; out->n_groups = (uint32_t)G; out->has_matrix = want_matrix;
    out->sums.assign(G * n_lags, 0ull);
    out->half_life.assign(R, ARP_NONE);
    if (R == 0) return ARP_OK;  // no contact in any frame: a 0 x (L + 1) matrix, zero sums
    // the matrix lands in host memory that the table then owns: a pooled pinned block when it is large
    if (want_matrix) {
        const size_t bytes = (size_t)(R * n_lags * 4u);
        if (bytes >= (1u << 20)) {
            out->owner = pinned_block(bytes);
            if (!out->owner) { set_error("out of pinned host memory for the autocorrelation matrix"); return ARP_ERR_OOM; }
        } else {
            char *heap = (char *)malloc(bytes);
            if (!heap) { set_error("out of host memory"); return ARP_ERR_OOM; }
            out->owner = std::shared_ptr<char>(heap, [](char *q) { free(q); });
        }
        out->matrix = reinterpret_cast<uint32_t *>(out->owner.get());
    }
    // 3. the curves
    AcfDev dv;
    if ((s = acf_launch(st, dev.words, R, W, F, L, continuous, want_matrix, dev.row_keys, nullptr, G, dev.stat[2], dev.stat[3], dev.stat[4], &dv)) != ARP_OK) return s;
    lap("curves");
    // 4. download: the matrix, the sums, the half-lives, lag 0, the rows' popcounts of k_timeline_stats and the error word of the marks
    uint32_t h_err = 0;
    std::vector<uint32_t> count(R), lag0(R);
    HIP_TRY(hipMemcpyAsync(&h_err, dev.err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(count.data(), dev.stat[4], R * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(lag0.data(), dv.lag0, R * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->half_life.data(), dv.half, R * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->sums.data(), dv.sums, G * n_lags * 8u, hipMemcpyDeviceToHost, st));
    if (want_matrix) HIP_TRY(hipMemcpyAsync(out->matrix, dv.matrix, R * n_lags * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    lap("download");
    if (h_err) { set_error(h_err & 1u ? "internal error: timeline item without a row" : "internal error: timeline item outside the frames"); return ARP_ERR_HIP; }
    for (uint64_t r = 0; r < R; r++)
        if (count[r] != rows->count[r] || lag0[r] != rows->count[r] || (want_matrix && out->matrix[r * n_lags] != rows->count[r])) {
            set_error("internal error: timeline row %llu has %u frames marked (lag 0: %u), the frequency table counts %u", (unsigned long long)r, count[r], lag0[r], rows->count[r]);
            return ARP_ERR_HIP;
        }
    return ARP_OK;
}

// a host bitmap through the same kernels: upload, clear the bits past n_bits, k_timeline_stats, the curves, download (rows > 0, max_lag < n_bits)
arp_status device_bit_autocorr(arp_context *ctx, uint64_t rows, uint64_t n_bits, const uint32_t *words, bool continuous, uint64_t L, const uint32_t *group, uint64_t n_groups,
                               uint64_t cap_bytes, uint32_t *acf, unsigned long long *sums, uint32_t *half_life) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(context_device(ctx)));
    const uint64_t W = (n_bits + 31u) / 32u, n_lags = L + 1u;
    arp_status s;
    if (acf && (s = autocorr_cap_check(rows, L, cap_bytes)) != ARP_OK) return s;
    if (rows * W * 4u > (1ull << 31)) { set_error("bit autocorrelation: a bitmap of %llu rows x %llu bits is more than 2^31 bytes", (unsigned long long)rows, (unsigned long long)n_bits); return ARP_ERR_CAPACITY; }
    uint32_t *d_words = nullptr, *stat[5];
    DevBlock block;
    if ((s = block.carve([&](Bump &bp) {
            d_words = bp.take<uint32_t>(rows * W);
            for (uint32_t *&p : stat) p = bp.take<uint32_t>(rows); bp.take<char>(256);  // (slack)
        })) != ARP_OK) return s;
    HIP_TRY(hipMemcpyAsync(d_words, words, rows * W * 4u, hipMemcpyHostToDevice, st));
    if (n_bits & 31u) {
        hipLaunchKernelGGL(k_bit_mask_tail, dim3((uint32_t)((rows + 255u) / 256u)), dim3(256), 0, st, d_words, rows, W, (1u << (n_bits & 31u)) - 1u);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_timeline_stats, dim3((uint32_t)((rows + 3u) / 4u)), dim3(256), 0, st, (uint32_t)rows, W, (const uint32_t *)d_words, stat[0], stat[1], stat[2], stat[3], stat[4]);
    HIP_TRY(hipGetLastError());
    AcfDev dv;
    const bool with_sums = group && sums && n_groups;
    if ((s = acf_launch(st, d_words, rows, W, n_bits, L, continuous, acf != nullptr, nullptr, with_sums ? group : nullptr, n_groups, stat[2], stat[3], stat[4], &dv)) != ARP_OK) return s;
    if (acf) HIP_TRY(hipMemcpyAsync(acf, dv.matrix, rows * n_lags * 4u, hipMemcpyDeviceToHost, st));
    if (with_sums) HIP_TRY(hipMemcpyAsync(sums, dv.sums, n_groups * n_lags * 8u, hipMemcpyDeviceToHost, st));
    if (half_life) HIP_TRY(hipMemcpyAsync(half_life, dv.half, rows * 4u, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return ARP_OK;
}
