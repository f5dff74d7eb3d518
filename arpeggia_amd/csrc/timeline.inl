// Contact timelines over the frames of an ensemble (arp_contact_timelines).  Included by table_dev.hip inside namespace
// arp, behind freq_rings.inl.
//
// present[r][f] = 1 iff frame f contributes at least one item to row r of the frequency table.  Two sweeps over the frames:
//   rows   device_frequencies as it is: its table is the call's frequency columns, its sorted row keys go back to the device;
//   marks  freq_sweep runs the same passes again (upload, k_freq_tile, contacts-only pair pass, ring fit); timeline_mark_pass finds every item's
//          row by binary search and ORs bit f & 31 into words[r][f >> 5].  Atom pairs are read straight from the pair list (no expand, no sort,
//          no item buffer); ring items come from k_freq_ring_rows, water bridges from k_freq_water_rows, into a small buffer of their own.
// OR is idempotent and order-free: the bitmap does not depend on the pass size or on the order of pairs, and two passes may share a word.
// k_timeline_stats then folds each row's words, one wave per row, into {first, last, events, longest run, popcount}.
//
// Row keys are the host's form, without a frame tag: i << 34 | j << 5 | code (atom level), A << (res_bits + 5) | B << 5 | code (residue level).

struct TimelineMarks {
    const unsigned long long *row_keys;  // sorted ascending, n_rows
    uint32_t n_rows, n_frames;
    uint32_t *words;                     // n_rows x W, zeroed
    uint64_t W;
    uint32_t *err;                       // device error word: 1 = an item without a row, 2 = a frame outside the call
    // the ring and water-bridge items of one pass (allocated by the first pass with either, grown when a pass has more)
    DevBlock items;
    uint64_t items_cap = 0;
};

// the row of `key` (lower bound in the sorted keys), or n_rows
__device__ inline uint32_t timeline_row(const unsigned long long *row_keys, uint32_t n_rows, unsigned long long key) {
    uint32_t lo = 0, hi = n_rows;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (row_keys[mid] < key) lo = mid + 1u; else hi = mid;
    }
    return (lo < n_rows && row_keys[lo] == key) ? lo : n_rows;
}
// nothing is written for an item without a row or a frame outside the call: the error word is raised instead
__device__ inline void timeline_mark(const unsigned long long *row_keys, uint32_t n_rows, uint32_t n_frames, uint32_t *words, uint64_t W, uint32_t *err,
                                     unsigned long long key, uint32_t f) {
    const uint32_t r = timeline_row(row_keys, n_rows, key);
    if (r >= n_rows) { atomicOr(err, 1u); return; }
    if (f >= n_frames) { atomicOr(err, 2u); return; }
    uint32_t *w = words + (size_t)r * W + (f >> 5);
    const uint32_t bit = 1u << (f & 31u);
    // (bits are only ever set: a stale read costs one redundant OR; at residue level most items of a frame find their bit already there)
    if (!(__atomic_load_n(w, __ATOMIC_RELAXED) & bit)) atomicOr(w, bit);
}

// pair p of the pass's list: frame f0 + i / n, one key per set bit of its kind word (k_freq_expand's items, without the buffer)
template <bool RES>
__global__ __launch_bounds__(256) void k_timeline_mark_pairs(const arp_pair *pairs, uint32_t n_pairs, uint32_t n, uint32_t f0, const uint32_t *res_of, uint32_t res_bits,
                                                             const unsigned long long *row_keys, uint32_t n_rows, uint32_t n_frames, uint32_t *words, uint64_t W, uint32_t *err) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_pairs) return;
    const arp_pair q = pairs[p];
    const uint32_t kind = q.kind & ((1u << ARP_N_INTERACTIONS) - 1u);
    const uint32_t f = f0 + q.i / n;
    unsigned long long ij;
    if constexpr (RES) ij = ((unsigned long long)res_of[q.i % n] << (res_bits + kFreqCodeBits)) | ((unsigned long long)res_of[q.j % n] << kFreqCodeBits);
    else ij = ((unsigned long long)(q.i % n) << kFreqKeyShiftI) | ((unsigned long long)(q.j % n) << kFreqKeyShiftJ);
    for (uint32_t b = kind; b; b &= b - 1u) timeline_mark(row_keys, n_rows, n_frames, words, W, err, ij | (unsigned long long)(__ffs((int)b) - 1), f);
}

// item t of k_freq_ring_rows: item_frame given (atom level): the key is a row key, the frame inside the pass is item_frame[t]; nullptr (residue
// level): the key's low tag_bits hold the frame inside the pass + 1, the rest is the row key
__global__ __launch_bounds__(256) void k_timeline_mark_items(uint32_t m, const unsigned long long *keys, const uint32_t *item_frame, uint32_t tag_bits, uint32_t f0,
                                                             const unsigned long long *row_keys, uint32_t n_rows, uint32_t n_frames, uint32_t *words, uint64_t W, uint32_t *err) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    unsigned long long key = keys[t];
    uint32_t f;
    if (item_frame) f = f0 + item_frame[t];
    else {
        const uint32_t tag = (uint32_t)(key & ((1ull << tag_bits) - 1ull));
        if (!tag) { atomicOr(err, 2u); return; }
        f = f0 + tag - 1u;
        key >>= tag_bits;
    }
    timeline_mark(row_keys, n_rows, n_frames, words, W, err, key, f);
}

// The summary of a stretch of frames (a whole number of words), associative under tl_join: its length in frames, the run of set bits it starts
// with (lead == len: every bit is set), the run it ends with, its longest run, its number of maximal runs, its first and last set frame, its
// set bits.  A word of zeros is the neutral stretch, so lanes past the row's end and the frames past F in the last word need no special case.
struct TlSum { uint32_t len, lead, trail, best, events, first, last, count; };
__device__ inline TlSum tl_word(uint32_t w, uint32_t frame0) {
    TlSum s;
    s.len = 32u;
    s.lead = w == 0xFFFFFFFFu ? 32u : (uint32_t)__ffs((int)~w) - 1u;
    s.trail = w == 0xFFFFFFFFu ? 32u : (uint32_t)__clz((int)~w);
    s.events = (uint32_t)__popc(w & ~(w << 1));
    s.count = (uint32_t)__popc(w);
    uint32_t best = 0;
    for (uint32_t x = w; x; x &= x << 1) best++;
    s.best = best;
    s.first = w ? frame0 + (uint32_t)__ffs((int)w) - 1u : 0xFFFFFFFFu;
    s.last = w ? frame0 + 31u - (uint32_t)__clz((int)w) : 0u;
    return s;
}
// a = the stretch in front, b = the one behind it.  A run continues across the boundary when a's trailing run and b's leading run touch.
__device__ inline TlSum tl_join(const TlSum &a, const TlSum &b) {
    TlSum s;
    s.len = a.len + b.len;
    s.lead = a.lead == a.len ? a.len + b.lead : a.lead;
    s.trail = b.trail == b.len ? b.len + a.trail : b.trail;
    s.best = max(max(a.best, b.best), a.trail + b.lead);
    s.events = a.events + b.events - ((a.trail && b.lead) ? 1u : 0u);
    s.first = min(a.first, b.first);
    s.last = max(a.last, b.last);
    s.count = a.count + b.count;
    return s;
}
__device__ inline TlSum tl_shfl_down(const TlSum &s, uint32_t off) {
    TlSum o;
    o.len = (uint32_t)__shfl_down((int)s.len, off); o.lead = (uint32_t)__shfl_down((int)s.lead, off); o.trail = (uint32_t)__shfl_down((int)s.trail, off);
    o.best = (uint32_t)__shfl_down((int)s.best, off); o.events = (uint32_t)__shfl_down((int)s.events, off); o.first = (uint32_t)__shfl_down((int)s.first, off);
    o.last = (uint32_t)__shfl_down((int)s.last, off); o.count = (uint32_t)__shfl_down((int)s.count, off);
    return o;
}

// one wave per row: lane l takes word step + l of the row; after the step with offset `off` lane l holds the stretch of lanes l .. l + 2 off - 1
// (a lane whose partner is past lane 63 joins the neutral stretch), so lane 0 ends with the 64 words in order and joins them behind what the
// earlier 64-word steps carried.
__global__ __launch_bounds__(256) void k_timeline_stats(uint32_t n_rows, uint64_t W, const uint32_t *words, uint32_t *first, uint32_t *last, uint32_t *events, uint32_t *longest,
                                                        uint32_t *count) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= n_rows) return;  // (the whole wave)
    const uint32_t *row = words + (size_t)r * W;
    const TlSum zero = tl_word(0u, 0u);
    TlSum carry = zero;
    for (uint64_t step = 0; step < W; step += 64u) {
        const uint64_t w = step + lane;
        TlSum s = tl_word(w < W ? row[w] : 0u, (uint32_t)(w << 5));
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            TlSum o = tl_shfl_down(s, off);
            if (lane + off >= 64u) o = zero;
            s = tl_join(s, o);
        }
        carry = tl_join(carry, s);  // (lane 0's is the row's)
    }
    if (lane == 0u) {
        first[r] = carry.first; last[r] = carry.events ? carry.last : 0xFFFFFFFFu; events[r] = carry.events; longest[r] = carry.best; count[r] = carry.count;
    }
}

namespace {
// the ring and water items' buffers inside marks->items
struct TimelineItems { unsigned long long *keys; FreqVal *vals; uint32_t *frame, *counter; };
arp_status timeline_items(TimelineMarks *mk, uint64_t cap, TimelineItems *it) {
    auto layout = [&](Bump &bp) {
        it->keys = bp.take<unsigned long long>(mk->items_cap); it->vals = bp.take<FreqVal>(mk->items_cap); it->frame = bp.take<uint32_t>(mk->items_cap);
        it->counter = bp.take<uint32_t>(64);
    };
    if (cap <= mk->items_cap) return carve_block(mk->items.p, planned_bytes(layout), layout);  // the block as it is
    if (cap > 0x7FFFFFF0ull) { set_error("contact timelines: more than 2^31 ring and water items in one pass (lower freq_chunk_atoms)"); return ARP_ERR_CAPACITY; }
    mk->items_cap = cap;
    const arp_status s = mk->items.carve(layout);
    if (s != ARP_OK) mk->items_cap = 0;
    return s;
}
}  // namespace

arp_status timeline_mark_pass(hipStream_t st, TimelineMarks *mk, const FreqPassView &v) {
    if (v.n_pairs) {
        const auto kernel = v.residue ? k_timeline_mark_pairs<true> : k_timeline_mark_pairs<false>;
        hipLaunchKernelGGL(kernel, dim3(freq_blocks(v.n_pairs)), dim3(256), 0, st, v.pairs, v.n_pairs, v.n, v.f0, v.res_of, v.res_bits, mk->row_keys, mk->n_rows, mk->n_frames,
                           mk->words, mk->W, mk->err);
        HIP_TRY(hipGetLastError());
    }
    if (!v.fr.n_rings && !v.fw.n_water) return ARP_OK;
    const auto ring_rows_kernel = v.residue ? k_freq_ring_rows<true> : k_freq_ring_rows<false>;
    TimelineItems it;
    // (the knob freq_cap_items sizes this first buffer too, so that tests make it grow)
    arp_status s = timeline_items(mk, std::max<uint64_t>(mk->items_cap, g_debug.freq_cap_items > 0 ? (uint64_t)g_debug.freq_cap_items : 1u << 14), &it);
    if (s != ARP_OK) return s;
    uint32_t counted[2] = {0u, 0u};  // {items, the water kernel's error word}
    const size_t counted_bytes = v.fw.n_water ? 8 : 4;
    uint32_t n_items = 0;
    for (int attempt = 0;; attempt++) {  // grown and repeated when the items do not fit, as in device_frequencies
        HIP_TRY(hipMemsetAsync(it.counter, 0, counted_bytes, st));
        if (v.fr.n_rings) {
            hipLaunchKernelGGL(ring_rows_kernel, dim3(v.frames * v.ring_tiles), dim3(256), 0, st, v.ring_tiles, v.n, v.fr, v.attr, v.res_ord, v.chain_rank, v.x, v.y, v.z, v.planes,
                               v.cutoff, it.keys, it.vals, 0u, (uint32_t)mk->items_cap, it.counter, v.rk, v.residue ? (uint32_t *)nullptr : it.frame);
            HIP_TRY(hipGetLastError());
        }
        if (v.fw.n_water) {  // (residue level only: the water items carry their frame in the key's tag, like the ring items of that level)
            hipLaunchKernelGGL(k_freq_water_rows<false>, dim3(v.frames * v.water_tiles), dim3(256), 0, st, v.water_tiles, v.n, v.fw, v.attr, v.res_ord, v.chain_rank, v.x, v.y, v.z,
                               it.keys, it.vals, (WaterTriple *)nullptr, 0u, 0u, (uint32_t)mk->items_cap, it.counter, it.counter + 1, v.rk);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(counted, it.counter, counted_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (counted[1]) return water_capacity_error();
        n_items = counted[0];
        if (n_items <= mk->items_cap) break;
        if (attempt) { set_error("internal error: the item count changed between passes"); return ARP_ERR_HIP; }
        if ((s = timeline_items(mk, (uint64_t)n_items + n_items / 4u, &it)) != ARP_OK) return s;
    }
    if (n_items) {
        hipLaunchKernelGGL(k_timeline_mark_items, dim3(freq_blocks(n_items)), dim3(256), 0, st, n_items, (const unsigned long long *)it.keys,
                           v.residue ? (const uint32_t *)nullptr : (const uint32_t *)it.frame, v.rk.frame_bits, v.f0, mk->row_keys, mk->n_rows, mk->n_frames, mk->words, mk->W, mk->err);
        HIP_TRY(hipGetLastError());
    }
    return ARP_OK;
}

// The device block of a timeline: the row keys, the bitmap, the five per-row results of k_timeline_stats and the error word of the marks.  It lives as
// long as this object, so that a follower (similarity.inl) can go on from the bitmap.  block == nullptr: the job has no rows.
struct TimelineDev {
    DevBlock block;
    unsigned long long *row_keys = nullptr;
    uint32_t *words = nullptr, *stat[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}, *err = nullptr;
};

// rows sweep, marks sweep, statistics: everything of a timeline up to its download.  lap is called after "rows" and "marks" (the statistics kernel is
// the caller's to lap, alone or with what it launches next); after_rows (nullable) sees the number of rows before anything is allocated and may refuse the job.
arp_status timeline_device(arp_context *ctx, const FreqJob &job, uint64_t cap_bytes, FreqRowsHost *rows, TimelineDev *dev, StreamLapTimer &lap,
                           const std::function<arp_status(uint64_t)> &after_rows) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    // 1. rows: the frequency table as the frequency call computes it
    arp_status s = device_frequencies(ctx, job, rows);
    if (s != ARP_OK) return s;
    lap("rows");
    const uint64_t R = rows->key.size(), F = job.n_frames, W = (F + 31u) / 32u;
    if (after_rows && (s = after_rows(R)) != ARP_OK) return s;
    if (R == 0) return ARP_OK;
    if (F > 0xFFFFFFF0ull) { set_error("contact timelines: more than 2^32 frames"); return ARP_ERR_BAD_INPUT; }
    const uint64_t need = R * W * 4u;
    if (need > cap_bytes) {
        set_error("contact timelines: the bitmap of %llu rows x %llu frames needs %llu bytes of device memory, the limit is %llu (timeline_cap_bytes)", (unsigned long long)R,
                  (unsigned long long)F, (unsigned long long)need, (unsigned long long)cap_bytes);
        return ARP_ERR_CAPACITY;
    }
    // 2. marks: the row keys back on the device, the zeroed bitmap, the five per-row results, the error word
    if ((s = dev->block.carve([&](Bump &bp) {
            dev->row_keys = bp.take<unsigned long long>(R);
            dev->words = bp.take<uint32_t>(R * W);
            for (uint32_t *&p : dev->stat) p = bp.take<uint32_t>(R);
            dev->err = bp.take<uint32_t>(64);
        })) != ARP_OK) return s;
    HIP_TRY(hipMemcpyAsync(dev->row_keys, rows->key.data(), R * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(dev->words, 0, need, st));
    HIP_TRY(hipMemsetAsync(dev->err, 0, 4, st));
    TimelineMarks mk{dev->row_keys, (uint32_t)R, (uint32_t)F, dev->words, W, dev->err};
    FreqRowsHost none;
    if ((s = freq_sweep(ctx, job, &none, &mk)) != ARP_OK) return s;
    lap("marks");
    // 3. statistics: one wave per row
    hipLaunchKernelGGL(k_timeline_stats, dim3((uint32_t)((R + 3u) / 4u)), dim3(256), 0, st, (uint32_t)R, W, (const uint32_t *)dev->words, dev->stat[0], dev->stat[1], dev->stat[2],
                       dev->stat[3], dev->stat[4]);
    HIP_TRY(hipGetLastError());
    return ARP_OK;
}

arp_status device_timelines(arp_context *ctx, const FreqJob &job, bool want_bitmap, uint64_t cap_bytes, FreqRowsHost *rows, TimelineHost *out) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(context_device(ctx)));
    StreamLapTimer lap("  timeline %-10s %8.3f ms\n", st);
    *out = TimelineHost{};
    TimelineDev dev;
    arp_status s = timeline_device(ctx, job, cap_bytes, rows, &dev, lap, nullptr);
    if (s != ARP_OK) return s;
    const uint64_t R = rows->key.size(), F = job.n_frames, W = (F + 31u) / 32u, need = R * W * 4u;
    if (R) lap("stats");
    out->words_per_row = W;
    out->has_bitmap = want_bitmap;
    out->first.resize(R); out->last.resize(R); out->n_events.resize(R); out->longest.resize(R);
    if (R == 0) return ARP_OK;
    // 4. download
    uint32_t h_err = 0;
    std::vector<uint32_t> count(R);
    HIP_TRY(hipMemcpyAsync(&h_err, dev.err, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->first.data(), dev.stat[0], R * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->last.data(), dev.stat[1], R * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->n_events.data(), dev.stat[2], R * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(out->longest.data(), dev.stat[3], R * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(count.data(), dev.stat[4], R * 4, hipMemcpyDeviceToHost, st));
    if (want_bitmap) {
        out->words.resize(R * W);
        HIP_TRY(hipMemcpyAsync(out->words.data(), dev.words, need, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    lap("download");
    if (h_err) { set_error(h_err & 1u ? "internal error: timeline item without a row" : "internal error: timeline item outside the frames"); return ARP_ERR_HIP; }
    for (uint64_t r = 0; r < R; r++) {
        uint64_t pop = count[r];
        if (want_bitmap) { pop = 0; for (uint64_t w = 0; w < W; w++) pop += (uint64_t)__builtin_popcount(out->words[r * W + w]); }
        if (pop != rows->count[r] || count[r] != rows->count[r]) {
            set_error("internal error: timeline row %llu has %llu frames marked, the frequency table counts %u", (unsigned long long)r, (unsigned long long)pop, rows->count[r]);
            return ARP_ERR_HIP;
        }
    }
    return ARP_OK;
}
