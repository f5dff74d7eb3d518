// Exclusive scans of device arrays whose length lives on the device.  Included by kernels.hip inside namespace arp, ahead of grid.inl; needs
// arp_internal.h (GridParams, the kRes* / kStat* words) and DEVFN only, so a test library can include it alone (tests/scan_unit).
//
//   k_scan_reduce + k_scan_apply   the pair-count scan: per-block totals, then carry + apply (pairs.inl launch_scan)
//   k_scan_single                  the cell scan in one launch: chunk totals published as {1, total} words, a block looks back at the blocks before it
//   k_scan_one                     the cell scan of inputs whose cells fit one workgroup's registers
// kScanBlocks x kScanThreads: the launch shape of k_scan_reduce / k_scan_apply, and of k_scan_single on packs and on inputs beyond 2^20 atoms;
// kScanPartAt: k_scan_single's published chunk totals live behind the 32 result words (Workspace::result + kScanPartAt, kScanBlocks of them)
constexpr uint32_t kScanBlocks = 1024, kScanThreads = 256, kScanPartAt = 32;
constexpr uint32_t kScanSingleBlocks = kScanThreads;  // one published word per thread of a later block: a single round of device-scope loads

DEVFN uint32_t wave_inclusive_add_u32(uint32_t v) {  // (the scan wave_reduce_u32 is the last lane of)
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
    return v;
}

// ---------------------------------------------------------------------------------------------- scan
// Exclusive scan of in[0..n) (n read from device memory) into out[0..n], out[n] = total, over a fixed 1024-block
// decomposition so that no host knowledge of n is needed.  Two launches (pairs.inl launch_scan): the per-block sums, then the
// per-block scans, whose blocks add up the raw sums of the blocks before them themselves (k_scan_tmp, the sums' scan as a launch
// of its own, is kept but no longer launched; a fused arrival-ticket variant was measured slower).  ZERO_IN clears the input
// behind itself; FINISH also publishes the pair total and the status flags.
template <typename TOut>
DEVFN TOut block_exclusive_scan(TOut v, TOut *total, TOut *lds /* [kScanThreads/64 + 1] */) {
    TOut inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        TOut t = __shfl_up(inc, off);
        if ((threadIdx.x & 63) >= (uint32_t)off) inc += t;
    }
    uint32_t w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 63) lds[w] = inc;
    __syncthreads();
    TOut wave_off = 0, tot = 0;
    for (uint32_t k = 0; k < kScanThreads / 64; k++) { TOut s = lds[k]; if (k < w) wave_off += s; tot += s; }
    *total = tot;
    return wave_off + inc - v;
}

template <typename TOut>
__global__ __launch_bounds__(kScanThreads) void k_scan_reduce(const uint32_t *in, const uint32_t *n_ptr, TOut *tmp) {
    __shared__ TOut lds[kScanThreads / 64 + 1];
    const uint32_t n = *n_ptr;
    const uint32_t chunk = (n + kScanBlocks - 1) / kScanBlocks;
    const uint32_t lo = min(n, blockIdx.x * chunk), hi = min(n, lo + chunk);
    TOut s = 0;
    for (uint32_t i = lo + threadIdx.x; i < hi; i += kScanThreads) s += in[i];
    TOut tot;
    block_exclusive_scan<TOut>(s, &tot, lds);
    if (threadIdx.x == 0) tmp[blockIdx.x] = tot;
}
template <typename TOut>
__global__ __launch_bounds__(kScanThreads) void k_scan_tmp(TOut *tmp) {  // tmp[kScanBlocks] receives the grand total
    __shared__ TOut lds[kScanThreads / 64 + 1];
    TOut carry = 0;
    for (uint32_t base = 0; base < kScanBlocks; base += kScanThreads) {
        TOut v = tmp[base + threadIdx.x], tot;
        TOut ex = block_exclusive_scan<TOut>(v, &tot, lds);
        tmp[base + threadIdx.x] = carry + ex;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) tmp[kScanBlocks] = carry;
}

template <typename TOut, bool ZERO_IN, bool FINISH>
__global__ __launch_bounds__(kScanThreads) void k_scan_apply(uint32_t *in, const uint32_t *n_ptr, const TOut *tmp, TOut *out, const GridParams *g,
                                                             unsigned long long *result, unsigned long long capacity, int have_out) {
    __shared__ TOut lds[kScanThreads / 64 + 1];
    const uint32_t n = *n_ptr;
    const uint32_t chunk = (n + kScanBlocks - 1) / kScanBlocks;
    const uint32_t lo = min(n, blockIdx.x * chunk), hi = min(n, lo + chunk);
    // carry = sum of the partial totals of the blocks before this one, recomputed here from the kScanBlocks raw totals
    // (4-8 KB out of L2): one launch less than scanning them in a kernel of their own
    TOut part = 0, all = 0;
    for (uint32_t k = threadIdx.x; k < kScanBlocks; k += kScanThreads) { const TOut v = tmp[k]; all += v; if (k < blockIdx.x) part += v; }
    TOut carry, grand = 0;
    block_exclusive_scan<TOut>(part, &carry, lds);
    __syncthreads();
    if (blockIdx.x == 0) { block_exclusive_scan<TOut>(all, &grand, lds); __syncthreads(); }
    for (uint32_t base = lo; base < hi; base += kScanThreads) {
        const uint32_t i = base + threadIdx.x;
        TOut v = (i < hi) ? (TOut)in[i] : (TOut)0, tot;
        TOut ex = block_exclusive_scan<TOut>(v, &tot, lds);
        if (i < hi) { out[i] = carry + ex; if (ZERO_IN) in[i] = 0; }
        carry += tot;
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const TOut total = grand;
        out[n] = total;
        if (FINISH) {  // the pair-count scan also publishes the result word and the status flags
            result[kResPairs] = (unsigned long long)total;
            if (have_out && (unsigned long long)total > capacity) result[kResFlags] |= kStatCapacity;
            if (g->bad & 1u) result[kResFlags] |= kStatNonFinite;
            if (g->bad & 2u) result[kResFlags] |= kStatSparseModels;
        }
    }
}

// The cell scan of larger inputs in ONE launch (round 5; two before: per-block totals, then carry + apply): every block adds up its chunk and
// publishes the total as one 64-bit word {1, total}; a block's carry is the sum of the words of the blocks before it, read with device-scope
// loads as they appear (the words are zeroed by the grid sizing of the same call, a kernel earlier on the stream).  A block only ever waits
// for blocks with a smaller index -- dispatched before it -- so the wait ends whatever else shares the device; value and flag travel in
// one atomic word, so nothing else has to become visible with it.
//
// How a block touches memory: its chunk is a multiple of four cells, read and written as 16-byte words in tiles of kScanThreads x kScanTile of
// them -- wave w owns kScanTile x 256 consecutive cells of a tile, and all loads of a tile are issued before the first is waited for.  A chunk
// of one tile (the usual case: the grid sizing allows 0.35 cells per atom, 1 434 cells per block at 2^20 atoms) stays in registers across the
// look-back: one load trip, publish + look-back, one store trip.  A chunk of several tiles (a sparse input, a pack's 8 M cells on 1 024 blocks)
// is read twice, once for the total and once for the scan.  Inside a wave the scan runs on the DPP row shifts; one barrier per tile exchanges
// the four wave totals.  (Before: one dword per lane and trip, each waited for, and a two-barrier block scan per trip -- nine or ten dependent
// round trips to memory for 1.1 MB of cells.)
constexpr uint32_t kScanTile = 4, kScanTileCells = kScanThreads * kScanTile * 4u;
// Trip j of a lane covers the cells i = w0 + 256 j .. + 3 (i is a multiple of four; only the chunk that ends at n can end inside a 16-byte word).
// Called with hi > 0.  Every load is a whole word from a clamped address -- a word past the chunk reads the chunk's last one instead -- and the
// cells at or past hi are zeroed afterwards: a branch around a load, or around the single cells of a ragged end, makes hipcc wait for each
// load before it issues the next (grid.inl box_accumulate).  `in` is therefore READ up to the end of the 16-byte word that holds cell n - 1,
// i.e. up to cell ((n + 3) & ~3) - 1; nothing past n - 1 is ever written.  The caller's invariant that keeps this read inside the array: the
// array holds at least n rounded up to a multiple of four words.  For the workspace that is n <= ncells_cap with ncells_cap a multiple of
// four (engine.cpp ensure_workspace: ccap = 8 cap + 65536, or 0xFFFFFFF0; ccap + 1 words allocated) -- a capacity that is no multiple of
// four would have to allocate up to the next one.
DEVFN void scan_tile_load(const uint32_t *in, uint32_t w0, uint32_t hi, uint4 (&v)[kScanTile]) {
    const uint32_t last_word = (hi - 1u) & ~3u;
#pragma unroll
    for (uint32_t j = 0; j < kScanTile; j++) v[j] = *reinterpret_cast<const uint4 *>(in + min(w0 + j * 256u, last_word));
#pragma unroll
    for (uint32_t j = 0; j < kScanTile; j++) {
        const uint32_t i = w0 + j * 256u;
        v[j].x = i < hi ? v[j].x : 0u; v[j].y = i + 1u < hi ? v[j].y : 0u; v[j].z = i + 2u < hi ? v[j].z : 0u; v[j].w = i + 3u < hi ? v[j].w : 0u;
    }
}
// ex[j]: cells before this lane's four of trip j, inside the wave's stretch; returns the stretch's total (every lane)
DEVFN uint32_t scan_tile_wave(const uint4 (&v)[kScanTile], uint32_t (&ex)[kScanTile]) {
    uint32_t run = 0;
#pragma unroll
    for (uint32_t j = 0; j < kScanTile; j++) {
        const uint32_t s = v[j].x + v[j].y + v[j].z + v[j].w, inc = wave_inclusive_add_u32(s);
        ex[j] = run + inc - s;
        run += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    }
    return run;
}
// out = before + the exclusive scan, and zeroes behind it in `in` (cell_count is ready for the next call); nothing at or past hi is written
DEVFN void scan_tile_store(uint32_t *in, uint32_t *out, uint32_t w0, uint32_t hi, const uint4 (&v)[kScanTile], const uint32_t (&ex)[kScanTile], uint32_t before) {
#pragma unroll
    for (uint32_t j = 0; j < kScanTile; j++) {
        const uint32_t i = w0 + j * 256u, o = before + ex[j];
        const uint4 r = make_uint4(o, o + v[j].x, o + v[j].x + v[j].y, o + v[j].x + v[j].y + v[j].z);
        if (i + 4u <= hi) {
            *reinterpret_cast<uint4 *>(out + i) = r;
            *reinterpret_cast<uint4 *>(in + i) = make_uint4(0u, 0u, 0u, 0u);
        } else if (i < hi) {
            out[i] = r.x; in[i] = 0u;
            if (i + 1u < hi) { out[i + 1u] = r.y; in[i + 1u] = 0u; }
            if (i + 2u < hi) { out[i + 2u] = r.z; in[i + 2u] = 0u; }
        }
    }
}
__global__ __launch_bounds__(kScanThreads) void k_scan_single(uint32_t *in, const uint32_t *n_ptr, unsigned long long *part, uint32_t *out) {
    constexpr uint32_t kWaves = kScanThreads / 64u;
    __shared__ uint32_t wave_total[2][kWaves], look[kWaves];
    const uint32_t n = *n_ptr, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    // (gridDim.x: kScanSingleBlocks, or kScanBlocks for the cell counts of packs and of inputs beyond 2^20 atoms)
    const uint32_t chunk = ((n + gridDim.x - 1u) / gridDim.x + 3u) & ~3u;  // every block starts on a 16-byte word; the blocks past the end have empty chunks
    const uint32_t lo = min(n, blockIdx.x * chunk), hi = min(n, lo + chunk);
    const uint32_t w_off = wave * (kScanTile * 256u) + lane * 4u;
    const bool one_tile = chunk <= kScanTileCells, last_block = blockIdx.x == gridDim.x - 1u;
    uint4 v[kScanTile];
    uint32_t ex[kScanTile], mine;  // mine: this wave's share of the chunk total
    if (one_tile) {
#pragma unroll
        for (uint32_t j = 0; j < kScanTile; j++) v[j] = make_uint4(0u, 0u, 0u, 0u);
        if (lo < hi) scan_tile_load(in, lo + w_off, hi, v);  // (an empty chunk -- a block past the end, n == 0 -- reads nothing)
        mine = scan_tile_wave(v, ex);
    } else {
        uint32_t s = 0;
        for (uint32_t base = lo; base < hi; base += kScanTileCells) {
            scan_tile_load(in, base + w_off, hi, v);
#pragma unroll
            for (uint32_t j = 0; j < kScanTile; j++) s += v[j].x + v[j].y + v[j].z + v[j].w;
        }
        mine = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_add_u32(s), 63);
    }
    if (lane == 0u) wave_total[0][wave] = mine;
    __syncthreads();
    uint32_t own = 0, before_wave = 0;
#pragma unroll
    for (uint32_t k = 0; k < kWaves; k++) { const uint32_t t = wave_total[0][k]; if (k < wave) before_wave += t; own += t; }
    if (threadIdx.x == 0) __hip_atomic_store(&part[blockIdx.x], (1ull << 32) | own, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (lo >= hi && !last_block) return;  // an empty chunk: nothing to write (the last block still writes the total)
    // thread t waits for the words of blocks t, t + 256, ... (blocks with a smaller index were dispatched earlier); the loads of a round are in
    // flight together, and only the words that had not appeared yet are asked for again
    constexpr uint32_t kWordsPer = kScanBlocks / kScanThreads;
    unsigned long long w[kWordsPer];
    bool pending = false;
#pragma unroll
    for (uint32_t j = 0; j < kWordsPer; j++) {
        const uint32_t k = threadIdx.x + j * kScanThreads;
        w[j] = k < blockIdx.x ? __hip_atomic_load(&part[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (1ull << 32);
    }
#pragma unroll
    for (uint32_t j = 0; j < kWordsPer; j++) pending |= (w[j] >> 32) == 0ull;
    while (pending) {
        pending = false;
#pragma unroll
        for (uint32_t j = 0; j < kWordsPer; j++)
            if ((w[j] >> 32) == 0ull) { w[j] = __hip_atomic_load(&part[threadIdx.x + j * kScanThreads], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); pending |= (w[j] >> 32) == 0ull; }
    }
    uint32_t before = 0, carry = 0;
#pragma unroll
    for (uint32_t j = 0; j < kWordsPer; j++) before += (uint32_t)w[j];
    before = (uint32_t)__builtin_amdgcn_readlane((int)wave_inclusive_add_u32(before), 63);
    if (lane == 0u) look[wave] = before;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < kWaves; k++) carry += look[k];
    if (last_block && threadIdx.x == 0) out[n] = carry + own;  // (no chunk reaches past the last block's: the grand total)
    if (one_tile) {
        scan_tile_store(in, out, lo + w_off, hi, v, ex, carry + before_wave);
        return;
    }
    uint32_t buf = 1u;  // (wave_total[0] held the chunk totals; the two halves alternate so that one barrier per tile is enough)
    for (uint32_t base = lo; base < hi; base += kScanTileCells, buf ^= 1u) {
        scan_tile_load(in, base + w_off, hi, v);
        mine = scan_tile_wave(v, ex);
        if (lane == 0u) wave_total[buf][wave] = mine;
        __syncthreads();
        uint32_t tile = 0;
        before_wave = 0;
#pragma unroll
        for (uint32_t k = 0; k < kWaves; k++) { const uint32_t t = wave_total[buf][k]; if (k < wave) before_wave += t; tile += t; }
        scan_tile_store(in, out, base + w_off, hi, v, ex, carry + before_wave);
        carry += tile;
    }
}

// The cell scan in ONE launch for inputs whose cells fit one workgroup's registers (launch_grid: up to kScanOneAtoms atoms, i.e. <= 65536
// cells at the 0.35 cells per atom the grid sizing allows): wave w owns 4096 consecutive cells per pass -- 16 coalesced 16-byte loads per
// lane, all in flight together --, scans them with the DPP row shifts (no LDS round trips), and one barrier exchanges the 16 wave totals.
// A sparse input with more cells than that takes further passes (correct, just slower than the two-launch scan the launcher would have
// picked had it known: the cell count only exists on the device).
constexpr uint32_t kScanOneThreads = 1024, kScanOnePer = 16, kScanOneCells = kScanOneThreads * kScanOnePer * 4u, kScanOneAtoms = 180000;
// Round 5: launched with kScanOneBlocks blocks.  Block b takes the passes b, b + kScanOneBlocks, ...: the usual input is one pass,
// which block 0 runs exactly as before while the other blocks read the cell count and leave; a sparse or many-model input of the same atom
// count (up to 8 n + 64 K cells: ~23 passes at 180 000 atoms) no longer runs them one after the other on one CU.  A pass publishes its total
// as one word {1, total} (the words k_scan_single uses, zeroed by the grid sizing) and adds up the words of the passes before it.
constexpr uint32_t kScanOneBlocks = 32;  // >= ceil((8 * kScanOneAtoms + 65536 + 1) / kScanOneCells) = 23 passes
template <bool ZERO_IN>
__global__ __launch_bounds__(kScanOneThreads) void k_scan_one(uint32_t *in, const uint32_t *n_ptr, unsigned long long *part, uint32_t *out) {
    __shared__ uint32_t wave_total[kScanOneThreads / 64];
    __shared__ uint32_t s_carry;
    const uint32_t n = *n_ptr, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t n_pass = (n + kScanOneCells - 1u) / kScanOneCells;
    if (blockIdx.x == 0u && n_pass == 0u && threadIdx.x == 0u) out[0] = 0u;  // (no cells: the total)
    for (uint32_t ps = blockIdx.x; ps < n_pass; ps += gridDim.x) {
        const uint32_t base = ps * kScanOneCells;
        const uint32_t w0 = base + wave * (kScanOnePer * 256u) + lane * 4u;
        uint4 v[kScanOnePer];
#pragma unroll
        for (uint32_t j = 0; j < kScanOnePer; j++) {
            const uint32_t i = w0 + j * 256u;
            v[j] = make_uint4(0u, 0u, 0u, 0u);
            if (i + 4u <= n) v[j] = *reinterpret_cast<const uint4 *>(in + i);
            else if (i < n) { v[j].x = in[i]; if (i + 1u < n) v[j].y = in[i + 1u]; if (i + 2u < n) v[j].z = in[i + 2u]; }
        }
        uint32_t ex[kScanOnePer], run = 0;  // ex[j]: cells before this lane's four of trip j, inside the wave's stretch
#pragma unroll
        for (uint32_t j = 0; j < kScanOnePer; j++) {
            const uint32_t s = v[j].x + v[j].y + v[j].z + v[j].w, inc = wave_inclusive_add_u32(s);
            ex[j] = run + inc - s;
            run += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
        }
        __syncthreads();  // (the previous pass of this block is done with wave_total / s_carry)
        if (lane == 0u) wave_total[wave] = run;
        __syncthreads();
        uint32_t before = 0, pass = 0;
        for (uint32_t k = 0; k < kScanOneThreads / 64u; k++) { const uint32_t t = wave_total[k]; if (k < wave) before += t; pass += t; }
        // the passes before this one (none for the usual single pass): their published totals, read as they appear
        if (n_pass > 1u) {
            if (threadIdx.x == 0u) __hip_atomic_store(&part[ps], (1ull << 32) | pass, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (wave == 0u) {
                uint32_t c = 0;
                for (uint32_t k = lane; k < ps; k += 64u) {
                    unsigned long long w;
                    do { w = __hip_atomic_load(&part[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); } while ((w >> 32) == 0ull);
                    c += (uint32_t)w;
                }
                c = wave_inclusive_add_u32(c);
                if (lane == 63u) s_carry = c;
            }
            __syncthreads();
            before += s_carry;
        }
#pragma unroll
        for (uint32_t j = 0; j < kScanOnePer; j++) {
            const uint32_t i = w0 + j * 256u, o = before + ex[j];
            const uint4 r = make_uint4(o, o + v[j].x, o + v[j].x + v[j].y, o + v[j].x + v[j].y + v[j].z);
            if (i + 4u <= n) {
                *reinterpret_cast<uint4 *>(out + i) = r;
                if (ZERO_IN) *reinterpret_cast<uint4 *>(in + i) = make_uint4(0u, 0u, 0u, 0u);
            } else if (i < n) {
                out[i] = r.x; if (i + 1u < n) out[i + 1u] = r.y; if (i + 2u < n) out[i + 2u] = r.z;
                if (ZERO_IN) { in[i] = 0u; if (i + 1u < n) in[i + 1u] = 0u; if (i + 2u < n) in[i + 2u] = 0u; }
            }
        }
        if (ps + 1u == n_pass && threadIdx.x == 0u) out[n] = (n_pass > 1u ? s_carry : 0u) + pass;  // the last pass holds the grand total
    }
}
