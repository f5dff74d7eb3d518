// Contact frequencies over the frames of an ensemble (arp_contact_frequencies).  Included by table_dev.hip inside
// namespace arp, after the table kernels (k_iota is shared).
//
// F frames of one topology run as F models of one packed input: every model owns its own z slab of the grid, so no pair crosses frames
// (batch.inl makes the same argument for packed structures).  Only the coordinates cross PCIe per frame; k_freq_tile writes the per-frame
// copies of the topology's arrays on the device with the index offsets of frame f and model ordinal f.  The pair list of a chunk of frames
// becomes (key, value) items -- key = i_top << 34 | j_top << 5 | code, value = {1 frame, distance, distance} -- which are appended to the
// running aggregate (one item per distinct key so far), sorted by key and reduced run by run.  Memory stays bounded by the distinct rows and
// one chunk's items, whatever F is, and only the aggregate comes back.
//
// Residue level (arp_residue_contact_frequencies): the same items under the key
// res(from) << (rb + 5 + fb) | res(to) << (5 + fb) | code << fb | tag, rb = bits of a residue ordinal, tag = the item's frame inside the pass + 1
// in fb bits (an entry of the aggregate has tag 0).  One sort by the whole key puts every (row, frame) sub-run together; the reduction by
// (key, tag) gives each sub-run's closest approach, k_freq_collapse turns it into {1 frame, c_f, c_f} and strips the tag, and a second
// reduction of the already sorted array by the row key merges the frames with the aggregate.

constexpr uint32_t kFreqKeyShiftI = 34, kFreqKeyShiftJ = 5;
constexpr uint32_t kFreqCodeBits = 5, kFreqFrameBitsMax = 17;  // residue level: the code's bits, and the most tag bits a key gets
constexpr uint64_t kFreqAutoAtoms = 1u << 21;  // atoms per pass when the knob freq_chunk_atoms is 0: 1ubq x 3000 frames, 6bft x 230
// the frames of an upload pass of the calls that stage whole frames of N atoms (rmsd.inl and behind): the knob's atom budget, else kFreqAutoAtoms; 1 <= it <= F
inline uint64_t frames_per_pass(uint64_t chunk_atoms, uint64_t N, uint64_t F) {
    return std::min<uint64_t>(F, std::max<uint64_t>(1, (chunk_atoms ? chunk_atoms : kFreqAutoAtoms) / std::max<uint64_t>(N, 1)));
}

// {frames, min, max} of one key; min / max are order-preserving codes of the f32 distances, so that unsigned atomics order them like floats
struct FreqVal { uint32_t count, mn, mx; };
__device__ inline uint32_t freq_code(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// topology arrays (device, frame 0) and the packed arrays of a chunk of `frames` frames
struct FreqTopo {
    uint32_t n, n_res, n_h;
    const uint32_t *attr, *res_ord, *chain_rank, *res_id, *res_h_ptr, *res_h_idx, *res_cb, *res_sg;
};
struct FreqPack {
    double *x, *y, *z;
    uint32_t *attr, *res_ord, *chain_rank, *model, *res_id, *res_h_ptr, *res_h_idx, *res_cb, *res_sg;
};

// item t = (frame f, entry k) of W = max(n, n_res + 1, n_h) entries per frame: atom k, residue k, hydrogen-list entry k of frame f.
// xyz: the chunk's coordinates as they came from the host, frames x n x 3.
__global__ __launch_bounds__(256) void k_freq_tile(uint32_t frames, uint32_t W, const double *xyz, FreqTopo t, FreqPack p) {
    const unsigned long long total = (unsigned long long)frames * W;
    for (unsigned long long q = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (unsigned long long)gridDim.x * blockDim.x) {
        const uint32_t f = (uint32_t)(q / W), k = (uint32_t)(q % W);
        const uint32_t atom0 = f * t.n, res0 = f * t.n_res, h0 = f * t.n_h;  // (frames x n < 2^32: checked by the host)
        if (k < t.n) {
            const uint32_t a = atom0 + k;
            const double *c = xyz + 3ull * a;
            p.x[a] = c[0]; p.y[a] = c[1]; p.z[a] = c[2];
            p.attr[a] = t.attr[k]; p.res_ord[a] = t.res_ord[k]; p.chain_rank[a] = t.chain_rank[k];
            p.model[a] = f;
            if (t.n_res) p.res_id[a] = t.res_id[k] + res0;
        }
        if (k < t.n_res) {
            const uint32_t r = res0 + k;
            p.res_h_ptr[r] = t.res_h_ptr[k] + h0;
            const uint32_t cb = t.res_cb[k], sg = t.res_sg[k];
            p.res_cb[r] = cb == ARP_NONE ? ARP_NONE : cb + atom0;
            p.res_sg[r] = sg == ARP_NONE ? ARP_NONE : sg + atom0;
        }
        if (t.n_res && k == t.n_res && f + 1u == frames) p.res_h_ptr[frames * t.n_res] = frames * t.n_h;
        if (k < t.n_h) p.res_h_idx[h0 + k] = t.res_h_idx[k] + atom0;
    }
}

// residue level: the residue of a topology atom and where the key's fields start (freq_rings.inl takes a ring's residue from its slot)
struct FreqResKey { const uint32_t *res_of; uint32_t shift_a, shift_b, frame_bits; };

// one item per set bit of a pair's kind word, appended at base + (a place reserved with one atomic per wave); nothing is written at or past
// cap, but *counter still counts every item (the host then grows the buffers and runs this again on the same pair list).
// RES: the residue-level key; the pair's frame inside the pass is its packed index / n.
template <bool RES>
__global__ __launch_bounds__(256) void k_freq_expand(const arp_pair *pairs, uint32_t n_pairs, uint32_t n, unsigned long long *keys, FreqVal *vals, uint32_t base,
                                                     uint32_t cap, uint32_t *counter, FreqResKey rk) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
    arp_pair q = {0u, 0u, 0.0f, 0u};
    if (p < n_pairs) q = pairs[p];
    const uint32_t kind = q.kind & ((1u << ARP_N_INTERACTIONS) - 1u);
    const uint32_t cnt = (uint32_t)__popc(kind);
    uint32_t incl = cnt;  // inclusive prefix over the wave
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, off);
        if (lane >= off) incl += v;
    }
    const uint32_t wave_total = (uint32_t)__shfl((int)incl, 63);
    uint32_t at = 0;
    if (lane == 63u && wave_total) at = atomicAdd(counter, wave_total);
    at = (uint32_t)__shfl((int)at, 63);
    if (!cnt) return;
    // i and j are atoms of the same frame: their topology indices are the packed indices modulo n
    unsigned long long ij;
    uint32_t code_shift = 0;
    if constexpr (RES) {
        ij = ((unsigned long long)rk.res_of[q.i % n] << rk.shift_a) | ((unsigned long long)rk.res_of[q.j % n] << rk.shift_b) | (unsigned long long)(q.i / n + 1u);
        code_shift = rk.frame_bits;
    } else {
        ij = ((unsigned long long)(q.i % n) << kFreqKeyShiftI) | ((unsigned long long)(q.j % n) << kFreqKeyShiftJ);
    }
    const uint32_t d = freq_code(q.dist);
    unsigned long long o = (unsigned long long)base + at + (incl - cnt);
    for (uint32_t b = kind; b; b &= b - 1u, ++o) {
        if (o >= cap) break;
        keys[o] = ij | ((unsigned long long)(__ffs((int)b) - 1) << code_shift);
        vals[o] = FreqVal{1u, d, d};
    }
}

// sorted items: flag the first item of every key
__global__ __launch_bounds__(256) void k_freq_heads(uint32_t m, const unsigned long long *keys, uint32_t *head) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m) head[t] = (t == 0u || keys[t] != keys[t - 1u]) ? 1u : 0u;
}
__global__ __launch_bounds__(256) void k_freq_init(uint32_t m, FreqVal *out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m) out[t] = FreqVal{0u, 0xFFFFFFFFu, 0u};
}
// run r (run = inclusive scan of the heads - 1): the wave first combines its items per run (runs are contiguous), then the first lane of each
// run in the wave adds the run's share with one atomic per field -- integer sums, minima and maxima, so the result is the same in any order
__global__ __launch_bounds__(256) void k_freq_reduce(uint32_t m, const unsigned long long *keys, const uint32_t *idx, const FreqVal *vals, const uint32_t *run_incl,
                                                     unsigned long long *out_keys, FreqVal *out) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
    const bool have = t < m;
    uint32_t r = 0xFFFFFFFFu;
    FreqVal v{0u, 0xFFFFFFFFu, 0u};
    if (have) { r = run_incl[t] - 1u; v = vals[idx[t]]; }
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const uint32_t r2 = (uint32_t)__shfl_down((int)r, off);
        const uint32_t c2 = (uint32_t)__shfl_down((int)v.count, off), mn2 = (uint32_t)__shfl_down((int)v.mn, off), mx2 = (uint32_t)__shfl_down((int)v.mx, off);
        if (lane + off < 64u && r2 == r) { v.count += c2; v.mn = min(v.mn, mn2); v.mx = max(v.mx, mx2); }
    }
    const uint32_t r_prev = (uint32_t)__shfl_up((int)r, 1);
    if (!have || (lane != 0u && r_prev == r)) return;
    atomicAdd(&out[r].count, v.count);
    atomicMin(&out[r].mn, v.mn);
    atomicMax(&out[r].mx, v.mx);
    if (t == 0u || keys[t - 1u] != keys[t]) out_keys[r] = keys[t];
}

// residue level, between the two reductions: entry t is one (row, tag) sub-run.  A frame's sub-run (tag >= 1) becomes {1 frame, c_f, c_f}, c_f its
// smallest distance, and loses its tag; an entry of the aggregate (tag 0) stays as it is.
__global__ __launch_bounds__(256) void k_freq_collapse(uint32_t m, unsigned long long tag_mask, unsigned long long *keys, FreqVal *vals) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const unsigned long long k = keys[t];
    if (!(k & tag_mask)) return;
    keys[t] = k & ~tag_mask;
    const uint32_t mn = vals[t].mn;
    vals[t] = FreqVal{1u, mn, mn};
}

// the ring items of a pass (ARP_FREQ_RINGS): the kernels are in freq_rings.inl, behind this file.  The topology's rings on the device: one plane
// per ring residue (slot), one RingEnt per entity (src_res = slot; every altloc of a residue is an entity of its own that shares the residue's
// plane), and the atoms a CationPi row can name.
struct FreqRings {
    uint32_t n_rings, n_slots, n_cand;
    const uint32_t *res_atom_ptr, *res_atom_idx, *slot_res, *cand;
    const uint8_t *plane_bits;
    const RingEnt *rings;
};
constexpr uint32_t kFreqRingTile = 64;  // ring entities per workgroup of k_freq_ring_rows
__global__ __launch_bounds__(128) void k_freq_ring_fit(uint32_t frames, uint32_t n, FreqRings r, const double *x, const double *y, const double *z, PlaneD *planes);
template <bool RES>
__global__ __launch_bounds__(256) void k_freq_ring_rows(uint32_t n_tiles, uint32_t n, FreqRings r, const uint32_t *attr, const uint32_t *res_ord, const uint32_t *chain_rank, const double *x,
                                 const double *y, const double *z, const PlaneD *planes, double cutoff, unsigned long long *keys, FreqVal *vals, uint32_t base, uint32_t cap,
                                 uint32_t *counter, FreqResKey rk, uint32_t *item_frame);

// the water-bridge items of a pass (ARP_FREQ_WATERS): the kernel is in freq_water.inl, behind freq_rings.inl.  The topology's water atoms and polar
// atoms on the device; a water keeps at most kFreqWaterPartners polar atoms within 3.5 A (more fail the call: water_capacity_error).
struct FreqWaters {
    uint32_t n_water, n_polar;
    const uint32_t *water, *polar;
};
constexpr uint32_t kFreqWaterTile = 64, kFreqWaterPartners = 32;  // waters per workgroup of k_freq_water_rows; list entries per water
template <bool TRIPLES>
__global__ __launch_bounds__(256) void k_freq_water_rows(uint32_t n_tiles, uint32_t n, FreqWaters w, const uint32_t *attr, const uint32_t *res_ord, const uint32_t *chain_rank,
                                                         const double *x, const double *y, const double *z, unsigned long long *keys, FreqVal *vals, WaterTriple *triples,
                                                         uint32_t f0, uint32_t base, uint32_t cap, uint32_t *counter, uint32_t *err, FreqResKey rk);
inline arp_status water_capacity_error() {
    set_error("water bridges: a water has more than %u polar atoms within 3.5 A in some frame (the per-water partner list is full)", kFreqWaterPartners);
    return ARP_ERR_CAPACITY;
}

// the mark sweep of arp_contact_timelines (timeline.inl, behind freq_rings.inl): the same passes -- upload, k_freq_tile, pair pass, ring fit -- but
// every item ORs its frame's bit into its row of a bitmap instead of joining the aggregate.  What a pass hands over:
struct TimelineMarks;
struct FreqPassView {
    uint32_t n, f0, frames, n_pairs;  // topology atoms; the pass's first frame and frame count; its listed pairs
    const arp_pair *pairs;
    bool residue;
    uint32_t res_bits;                // residue level: bits of a residue ordinal in a row key
    const uint32_t *res_of;
    FreqRings fr;                     // n_rings > 0: what k_freq_ring_rows takes
    uint32_t ring_tiles;
    const uint32_t *attr, *res_ord, *chain_rank;
    const double *x, *y, *z;
    const PlaneD *planes;
    double cutoff;
    FreqResKey rk;
    FreqWaters fw;                    // n_water > 0: what k_freq_water_rows takes
    uint32_t water_tiles;
};
arp_status timeline_mark_pass(hipStream_t st, TimelineMarks *marks, const FreqPassView &v);

namespace {
uint32_t freq_blocks(unsigned long long items) { return (uint32_t)std::max<unsigned long long>(1ull, (items + 255u) / 256u); }  // (items < 2^32: one thread each)

// the aggregate and one chunk's items: kin / vin hold the aggregate (first n_agg) + the new items; the sort and the reduction write the other set
struct FreqBufs {
    DevBlock block;
    uint64_t cap = 0;  // items
    unsigned long long *kin = nullptr, *ks = nullptr, *kout = nullptr;
    FreqVal *vin = nullptr, *vout = nullptr;
    uint32_t *iota = nullptr, *is = nullptr, *head = nullptr, *scan = nullptr, *counter = nullptr;
    void *tmp = nullptr; size_t tmp_bytes = 0;
    void layout(Bump &bp) {  // cap and tmp_bytes are set
        kin = bp.take<unsigned long long>(cap); ks = bp.take<unsigned long long>(cap); kout = bp.take<unsigned long long>(cap);
        vin = bp.take<FreqVal>(cap); vout = bp.take<FreqVal>(cap);
        iota = bp.take<uint32_t>(cap); is = bp.take<uint32_t>(cap); head = bp.take<uint32_t>(cap); scan = bp.take<uint32_t>(cap);
        counter = bp.take<uint32_t>(64); tmp = bp.take<char>(tmp_bytes);
    }
};
arp_status freq_alloc(FreqBufs *b, uint64_t cap, uint64_t keep, hipStream_t st) {
    if (cap > 0x7FFFFFF0ull) { set_error("contact frequencies: more than 2^31 items in one pass (lower freq_chunk_atoms)"); return ARP_ERR_CAPACITY; }
    size_t sort_bytes = 0, scan_bytes = 0;
    HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const unsigned long long *)nullptr, (unsigned long long *)nullptr, (const uint32_t *)nullptr,
                                               (uint32_t *)nullptr, (int)cap, 0, 64, st));
    HIP_TRY(hipcub::DeviceScan::InclusiveSum(nullptr, scan_bytes, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)cap, st));
    const size_t tmp = std::max(sort_bytes, scan_bytes);
    FreqBufs nb;
    nb.cap = cap; nb.tmp_bytes = tmp;
    if (arp_status s = nb.block.carve([&](Bump &bp) { nb.layout(bp); }); s != ARP_OK) return s;
    if (keep && b->block.p) {  // the aggregate moves into the new block
        HIP_TRY(hipMemcpyAsync(nb.kin, b->kin, keep * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(nb.vin, b->vin, keep * sizeof(FreqVal), hipMemcpyDeviceToDevice, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    *b = std::move(nb);  // (frees the old block)
    return ARP_OK;
}
}  // namespace

// marks == nullptr: the frequency table of the job.  Otherwise the mark sweep of timeline.inl: every pass ends in timeline_mark_pass and *out stays empty.
arp_status freq_sweep(arp_context *ctx, const FreqJob &job, FreqRowsHost *out, TimelineMarks *marks) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(context_device(ctx)));
    StreamLapTimer lap("    frequencies %-24s %8.3f ms\n", st);
    *out = FreqRowsHost{};
    const uint64_t n = job.n, nr = job.n_res, nh = job.n_h, F = job.n_frames;
    const uint64_t n_rings = job.n_rings, n_slots = job.n_slots, n_cand = job.n_cand, n_ra = n_rings ? job.res_atom_ptr[nr] : 0;
    const uint64_t n_water = job.residue ? job.n_water : 0, n_polar = n_water ? job.n_polar : 0, water_tiles = (n_water + kFreqWaterTile - 1) / kFreqWaterTile;
    if (n == 0 || F == 0) return ARP_OK;
    // frames per pass: the knob's atom budget, else kFreqAutoAtoms; never more frames than fit 32-bit packed indices
    const uint64_t budget = job.chunk_atoms ? job.chunk_atoms : kFreqAutoAtoms;
    uint64_t per = std::max<uint64_t>(1, budget / n);
    per = std::min<uint64_t>({per, F, 0x7FFFFFF0ull / std::max<uint64_t>({n, nr + 1, nh, 1}), 65535});
    // residue level: rb bits per residue ordinal, the tag gets what is left of the key (at most kFreqFrameBitsMax, or the knob's fewer), and a
    // pass has at most 2^fb - 1 frames (tag 0 is the aggregate's)
    uint32_t rb = 1, fbits = 0;
    if (job.residue) {
        if (nr == 0) { set_error("residue contact frequencies: the topology has no residue table"); return ARP_ERR_BAD_INPUT; }
        while (rb < 29u && (1ull << rb) < nr) rb++;
        fbits = std::min<uint32_t>(kFreqFrameBitsMax, 64u - kFreqCodeBits - 2u * rb);
        if (job.frame_bits) fbits = std::min<uint32_t>(fbits, job.frame_bits);
        per = std::min<uint64_t>(per, (1ull << fbits) - 1u);
    }
    if (n_rings) per = std::min<uint64_t>(per, std::max<uint64_t>(1, 0x7FFFFFF0ull / std::max<uint64_t>({n_slots, (n_rings + kFreqRingTile - 1) / kFreqRingTile, 1})));  // (one thread per (frame, slot), one workgroup per (frame, tile))
    if (n_water) per = std::min<uint64_t>(per, std::max<uint64_t>(1, 0x7FFFFFF0ull / water_tiles));  // (one workgroup per (frame, tile))
    if (per == 0) { set_error("contact frequencies: one frame exceeds 32-bit indices"); return ARP_ERR_BAD_INPUT; }
    // topology (once) and the packed arrays of one pass
    struct Seg { const void *src; uint64_t bytes; };
    const Seg topo_seg[16] = {{job.attr, n * 4}, {job.res_ord, n * 4}, {job.chain_rank, n * 4}, {nr ? job.res_id : nullptr, nr ? n * 4 : 0},
                             {nr ? job.res_h_ptr : nullptr, nr ? (nr + 1) * 4 : 0}, {nh ? job.res_h_idx : nullptr, nh * 4}, {nr ? job.res_cb : nullptr, nr * 4},
                             {nr ? job.res_sg : nullptr, nr * 4},
                             // the rings of the topology (ARP_FREQ_RINGS; nothing otherwise)
                             {job.rings, n_rings * sizeof(RingEnt)}, {job.slot_res, n_slots * 4}, {job.res_atom_ptr, n_rings ? (nr + 1) * 4 : 0}, {job.res_atom_idx, n_ra * 4},
                             {job.cand, n_cand * 4}, {job.plane_bits, n_rings ? n : 0},
                             // the water and polar atoms of the topology (ARP_FREQ_WATERS; nothing otherwise)
                             {job.water, n_water * 4}, {job.polar, n_polar * 4}};
    const uint64_t pn = per * n, pr = per * nr, ph = per * nh;
    char *topo_dev[16];
    double *xyz = nullptr; FreqPack pk; PlaneD *planes = nullptr;  // planes: one pass's ring planes, frames x slots
    DevBlock block;
    if (arp_status s = block.carve([&](Bump &bp) {
            for (int k = 0; k < 16; k++) topo_dev[k] = bp.take<char>(topo_seg[k].bytes);
            xyz = bp.take<double>(pn * 3);
            pk.x = bp.take<double>(pn); pk.y = bp.take<double>(pn); pk.z = bp.take<double>(pn);
            pk.attr = bp.take<uint32_t>(pn); pk.res_ord = bp.take<uint32_t>(pn); pk.chain_rank = bp.take<uint32_t>(pn); pk.model = bp.take<uint32_t>(pn);
            pk.res_id = bp.take<uint32_t>(pn); pk.res_h_ptr = bp.take<uint32_t>(pr + 1); pk.res_cb = bp.take<uint32_t>(pr); pk.res_sg = bp.take<uint32_t>(pr);
            pk.res_h_idx = bp.take<uint32_t>(ph); planes = bp.take<PlaneD>(per * n_slots); bp.take<char>(256);  // (slack)
        }); s != ARP_OK) return s;
    for (int k = 0; k < 16; k++)
        if (topo_seg[k].bytes) HIP_TRY(hipMemcpyAsync(topo_dev[k], topo_seg[k].src, topo_seg[k].bytes, hipMemcpyHostToDevice, st));
    FreqTopo tp{(uint32_t)n, (uint32_t)nr, (uint32_t)nh, (const uint32_t *)topo_dev[0], (const uint32_t *)topo_dev[1], (const uint32_t *)topo_dev[2],
                (const uint32_t *)topo_dev[3], (const uint32_t *)topo_dev[4], (const uint32_t *)topo_dev[5], (const uint32_t *)topo_dev[6], (const uint32_t *)topo_dev[7]};
    const FreqRings fr{(uint32_t)n_rings, (uint32_t)n_slots, (uint32_t)n_cand, (const uint32_t *)topo_dev[10], (const uint32_t *)topo_dev[11], (const uint32_t *)topo_dev[9],
                       (const uint32_t *)topo_dev[12], (const uint8_t *)topo_dev[13], (const RingEnt *)topo_dev[8]};
    const uint32_t ring_tiles = (uint32_t)((n_rings + kFreqRingTile - 1) / kFreqRingTile);
    const FreqWaters fw{(uint32_t)n_water, (uint32_t)n_polar, (const uint32_t *)topo_dev[14], (const uint32_t *)topo_dev[15]};
    lap("topology upload");
    arp_params prm;
    arp_default_params(&prm);
    prm.vdw_comp = job.vdw_comp; prm.dist_cutoff = job.dist_cutoff;
    prm.flags |= ARP_FLAG_CONTACTS_ONLY;
    // key bits: j in bits 5.., i in bits 34..; only the bits an index of n atoms + n_rings rings can set are sorted
    int ibits = 1;
    while (ibits < 29 && (1ull << ibits) < n + n_rings) ibits++;
    const int end_bit = job.residue ? (int)(2u * rb + kFreqCodeBits + fbits) : (int)kFreqKeyShiftI + ibits;
    const FreqResKey rk{tp.res_id, rb + kFreqCodeBits + fbits, kFreqCodeBits + fbits, fbits};
    const unsigned long long tag_mask = (1ull << fbits) - 1ull;
    const auto expand_kernel = job.residue ? k_freq_expand<true> : k_freq_expand<false>;
    const auto ring_rows_kernel = job.residue ? k_freq_ring_rows<true> : k_freq_ring_rows<false>;
    FreqBufs fb;
    uint64_t n_agg = 0;
    for (uint64_t f0 = 0; f0 < F; f0 += per) {
        const uint64_t fc = std::min<uint64_t>(per, F - f0);
        // 1. upload: the chunk's coordinates only; the tiling kernel writes the per-frame arrays
        HIP_TRY(hipMemcpyAsync(xyz, job.xyz + f0 * n * 3, fc * n * 24, hipMemcpyHostToDevice, st));
        const uint64_t W = std::max<uint64_t>({n, nr ? nr + 1 : 0, nh});
        hipLaunchKernelGGL(k_freq_tile, dim3(std::min<uint32_t>(freq_blocks(fc * W), 1u << 16)), dim3(256), 0, st, (uint32_t)fc, (uint32_t)W, (const double *)xyz, tp, pk);
        HIP_TRY(hipGetLastError());
        // 2. the pair pass over the packed frames (contacts only: what arp_get_contacts turns into rows)
        arp_atoms av{};
        av.n = fc * n; av.x = pk.x; av.y = pk.y; av.z = pk.z; av.attr = pk.attr; av.res_ord = pk.res_ord; av.chain_rank = pk.chain_rank; av.model = pk.model;
        av.res_id = nr ? pk.res_id : nullptr; av.n_res = fc * nr; av.res_h_ptr = nr ? pk.res_h_ptr : nullptr; av.res_h_idx = pk.res_h_idx;
        av.res_cb = nr ? pk.res_cb : nullptr; av.res_sg = nr ? pk.res_sg : nullptr;
        av.location = ARP_MEM_DEVICE;
        const arp_pair *pairs = nullptr;
        uint64_t n_pairs = 0;
        arp_status s = contacts_atomic_view(ctx, &av, &prm, &pairs, &n_pairs);
        if (s != ARP_OK) return s;
        lap("pair pass");
        if (n_pairs > 0xFFFFFFF0ull) { set_error("contact frequencies: more than 2^32 pairs in one pass (lower freq_chunk_atoms)"); return ARP_ERR_CAPACITY; }
        if (n_pairs == 0 && !n_rings && !n_water) continue;  // (ring - ring items and water bridges need no atom pair: with either no pass is skipped here)
        if (n_rings) {  // the frames' ring planes
            hipLaunchKernelGGL(k_freq_ring_fit, dim3((uint32_t)((fc * n_slots + 127u) / 128u)), dim3(128), 0, st, (uint32_t)fc, (uint32_t)n, fr, (const double *)pk.x, (const double *)pk.y,
                               (const double *)pk.z, planes);
            HIP_TRY(hipGetLastError());
            lap("ring fit");
        }
        if (marks) {
            const FreqPassView view{(uint32_t)n, (uint32_t)f0, (uint32_t)fc, (uint32_t)n_pairs, pairs, job.residue, rb, tp.res_id, fr, ring_tiles, tp.attr, tp.res_ord, tp.chain_rank,
                                    pk.x, pk.y, pk.z, planes, job.dist_cutoff, rk, fw, (uint32_t)water_tiles};
            if ((s = timeline_mark_pass(st, marks, view)) != ARP_OK) return s;
            lap("marks");
            continue;
        }
        // 3. expand into (key, value) items behind the aggregate, the ring items behind the atom items, the water bridges behind both; grown and
        // repeated when they do not fit
        if (!fb.block.p && (s = freq_alloc(&fb, g_debug.freq_cap_items > 0 ? (uint64_t)g_debug.freq_cap_items : std::max<uint64_t>(1u << 16, 2 * n_pairs), 0, st)) != ARP_OK) return s;
        uint32_t counted[2] = {0u, 0u};  // {items, the water kernel's error word}
        const size_t counted_bytes = n_water ? 8 : 4;
        for (int attempt = 0;; attempt++) {
            HIP_TRY(hipMemsetAsync(fb.counter, 0, counted_bytes, st));
            if (n_pairs) hipLaunchKernelGGL(expand_kernel, dim3(freq_blocks(n_pairs)), dim3(256), 0, st, pairs, (uint32_t)n_pairs,
                                            (uint32_t)n, fb.kin, fb.vin, (uint32_t)n_agg, (uint32_t)fb.cap, fb.counter, rk);
            HIP_TRY(hipGetLastError());
            if (n_rings) {
                lap("expand");
                hipLaunchKernelGGL(ring_rows_kernel, dim3((uint32_t)fc * ring_tiles), dim3(256), 0, st, ring_tiles, (uint32_t)n, fr,
                                   tp.attr, tp.res_ord, tp.chain_rank, (const double *)pk.x, (const double *)pk.y, (const double *)pk.z, (const PlaneD *)planes, job.dist_cutoff,
                                   fb.kin, fb.vin, (uint32_t)n_agg, (uint32_t)fb.cap, fb.counter, rk, (uint32_t *)nullptr);
                HIP_TRY(hipGetLastError());
            }
            if (n_water) {
                lap(n_rings ? "ring rows" : "expand");
                hipLaunchKernelGGL(k_freq_water_rows<false>, dim3((uint32_t)(fc * water_tiles)), dim3(256), 0, st, (uint32_t)water_tiles, (uint32_t)n, fw, tp.attr, tp.res_ord,
                                   tp.chain_rank, (const double *)pk.x, (const double *)pk.y, (const double *)pk.z, fb.kin, fb.vin, (WaterTriple *)nullptr, 0u, (uint32_t)n_agg,
                                   (uint32_t)fb.cap, fb.counter, fb.counter + 1, rk);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipMemcpyAsync(counted, fb.counter, counted_bytes, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (counted[1]) return water_capacity_error();
            const uint32_t n_items = counted[0];
            if (n_agg + n_items <= fb.cap) break;
            if (attempt) { set_error("internal error: the item count changed between passes"); return ARP_ERR_HIP; }
            const uint64_t want = n_agg + n_items;
            if ((s = freq_alloc(&fb, want + want / 4, n_agg, st)) != ARP_OK) return s;
        }
        lap(n_water ? "water bridges" : n_rings ? "ring rows" : "expand");
        const uint32_t n_items = counted[0];
        if (n_items == 0) continue;
        // 4. + 5. sort the aggregate and the new items together, reduce every run of equal keys to one
        const uint32_t m = (uint32_t)(n_agg + n_items);
        size_t tb = fb.tmp_bytes;
        hipLaunchKernelGGL(k_iota, dim3(freq_blocks(m)), dim3(256), 0, st, m, fb.iota);
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(fb.tmp, tb, (const unsigned long long *)fb.kin, fb.ks, (const uint32_t *)fb.iota, fb.is, (int)m, 0, end_bit, st));
        hipLaunchKernelGGL(k_freq_heads, dim3(freq_blocks(m)), dim3(256), 0, st, m, (const unsigned long long *)fb.ks, fb.head);
        tb = fb.tmp_bytes;
        HIP_TRY(hipcub::DeviceScan::InclusiveSum(fb.tmp, tb, (const uint32_t *)fb.head, fb.scan, (int)m, st));
        hipLaunchKernelGGL(k_freq_init, dim3(freq_blocks(m)), dim3(256), 0, st, m, fb.vout);
        hipLaunchKernelGGL(k_freq_reduce, dim3(freq_blocks(m)), dim3(256), 0, st, m, (const unsigned long long *)fb.ks, (const uint32_t *)fb.is, (const FreqVal *)fb.vin,
                           (const uint32_t *)fb.scan, fb.kout, fb.vout);
        HIP_TRY(hipGetLastError());
        uint32_t runs = 0;
        HIP_TRY(hipMemcpyAsync(&runs, fb.scan + (m - 1u), 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        lap("sort + reduce");
        if (job.residue) {
            // 5b. kout / vout hold one entry per (row, tag) sub-run, still sorted: collapse each frame's sub-run to {1, c_f, c_f}, strip the tags and
            // reduce again by the row key -- no second sort; the next aggregate goes to kin / vin, whose items are spent
            hipLaunchKernelGGL(k_freq_collapse, dim3(freq_blocks(runs)), dim3(256), 0, st, runs, tag_mask, fb.kout, fb.vout);
            hipLaunchKernelGGL(k_freq_heads, dim3(freq_blocks(runs)), dim3(256), 0, st, runs, (const unsigned long long *)fb.kout, fb.head);
            tb = fb.tmp_bytes;
            HIP_TRY(hipcub::DeviceScan::InclusiveSum(fb.tmp, tb, (const uint32_t *)fb.head, fb.scan, (int)runs, st));
            hipLaunchKernelGGL(k_freq_init, dim3(freq_blocks(runs)), dim3(256), 0, st, runs, fb.vin);
            hipLaunchKernelGGL(k_freq_reduce, dim3(freq_blocks(runs)), dim3(256), 0, st, runs, (const unsigned long long *)fb.kout, (const uint32_t *)fb.iota, (const FreqVal *)fb.vout,
                               (const uint32_t *)fb.scan, fb.kin, fb.vin);
            HIP_TRY(hipGetLastError());
            uint32_t rows = 0;
            HIP_TRY(hipMemcpyAsync(&rows, fb.scan + (runs - 1u), 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            n_agg = rows;
            lap("collapse + reduce");
        } else {
            std::swap(fb.kin, fb.kout); std::swap(fb.vin, fb.vout);
            n_agg = runs;
        }
    }
    if (marks) return ARP_OK;
    // 6. only the aggregate comes back
    out->key.resize(n_agg); out->count.resize(n_agg); out->mn.resize(n_agg); out->mx.resize(n_agg);
    if (n_agg) {
        std::vector<FreqVal> v(n_agg);
        HIP_TRY(hipMemcpyAsync(out->key.data(), fb.kin, n_agg * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(v.data(), fb.vin, n_agg * sizeof(FreqVal), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        auto decode = [](uint32_t c) { const uint32_t b = (c & 0x80000000u) ? (c & 0x7FFFFFFFu) : ~c; float f; memcpy(&f, &b, 4); return f; };
        for (uint64_t r = 0; r < n_agg; r++) { out->count[r] = v[r].count; out->mn[r] = decode(v[r].mn); out->mx[r] = decode(v[r].mx); }
        if (job.residue) for (uint64_t r = 0; r < n_agg; r++) out->key[r] >>= fbits;  // (the aggregate's tags are 0)
    }
    out->res_bits = job.residue ? rb : 0u;
    lap("download");
    return ARP_OK;
}
arp_status device_frequencies(arp_context *ctx, const FreqJob &job, FreqRowsHost *out) { return freq_sweep(ctx, job, out, nullptr); }
