// Water bridges (ARP_FREQ_WATERS on the residue frequency and timeline calls, and arp_water_bridges).  Included by
// table_dev.hip inside namespace arp, behind freq_rings.inl.
// (FreqWaters, kFreqWaterTile, kFreqWaterPartners and WaterTriple: freq.inl, whose freq_sweep launches this kernel.)
//
// In frame f a water atom w and a polar atom p form a LEG iff dx*dx + dy*dy + dz*dz <= 12.25 in f64 (3.5 A, the PolarContact distance, inclusive).
// (p, w, q) is a BRIDGE iff p != q, both legs hold, p is in the ligand set, q in the receptor set and compare_residues_d(key(p), key(q), true) --
// the table path's own residue rule, so a residue pair has one orientation.  The water's own chain and groups play no part, nor do vdw_comp and
// dist_cutoff.  The sweep is brute force, every water against every polar atom of its frame, as freq_rings.inl sweeps rings against candidates: exact
// and independent of the pair pass's cell list.
// Items: key = res(p) << shift_a | res(q) << shift_b | 19 << frame_bits | (frame inside the pass + 1), the residue-level key of freq.inl, value =
// the longer leg as f32, so that a frame's closest approach is its tightest bridge.  TRIPLES: one {frame, p, q, w, leg p, leg q} record per bridge.

// One workgroup = (frame f, tile of kFreqWaterTile waters).  The tile's coordinates sit in LDS as separate arrays (one word per array and water, the
// same address on every lane: a broadcast), and every water has a count and kFreqWaterPartners list entries there (partner atom, f64 d^2).
// Sweep 1: the lanes stride over the polar atoms; per (water, sweep step) the hits of a wave take consecutive list slots from ONE LDS atomic.  A slot
// at or past kFreqWaterPartners is not written: bit 0 of *err is raised instead and the host fails the call (ARP_ERR_CAPACITY).
// Sweep 2: the waves take the tile's waters round-robin, the lanes the ordered partner pairs (i, j) of the water's list; hits are appended with the
// protocol of k_freq_ring_rows -- one ballot, one atomic on the counter, nothing written at or past cap, the counter counts every item.
// TRIPLES: xyz holds the frames as they came from the host (frames x n x 3), y and z are unused; otherwise x / y / z are the pass's packed arrays.
template <bool TRIPLES>
__global__ __launch_bounds__(256) void k_freq_water_rows(uint32_t n_tiles, uint32_t n, FreqWaters w, const uint32_t *attr, const uint32_t *res_ord, const uint32_t *chain_rank,
                                                         const double *x, const double *y, const double *z, unsigned long long *keys, FreqVal *vals, WaterTriple *triples,
                                                         uint32_t f0, uint32_t base, uint32_t cap, uint32_t *counter, uint32_t *err, FreqResKey rk) {
    __shared__ double s_w[3][kFreqWaterTile];
    __shared__ uint32_t s_cnt[kFreqWaterTile];
    __shared__ uint32_t s_pa[kFreqWaterTile][kFreqWaterPartners];
    __shared__ double s_pd[kFreqWaterTile][kFreqWaterPartners];
    const uint32_t f = blockIdx.x / n_tiles, w0 = (blockIdx.x % n_tiles) * kFreqWaterTile, lane = threadIdx.x & 63u;
    const uint32_t n_tile = min(kFreqWaterTile, w.n_water - w0);
    const size_t at0 = (size_t)f * n;  // (frames x n < 2^32: checked by the host)
    auto coord = [&](uint32_t a, double *c) {
        if constexpr (TRIPLES) { const double *q = x + 3u * (at0 + a); c[0] = q[0]; c[1] = q[1]; c[2] = q[2]; }
        else { c[0] = x[at0 + a]; c[1] = y[at0 + a]; c[2] = z[at0 + a]; }
    };
    if (threadIdx.x < n_tile) {
        double c[3];
        coord(w.water[w0 + threadIdx.x], c);
        for (int a = 0; a < 3; a++) s_w[a][threadIdx.x] = c[a];
        s_cnt[threadIdx.x] = 0u;
    }
    __syncthreads();
    // sweep 1: the legs
    for (uint32_t o0 = 0; o0 < w.n_polar; o0 += blockDim.x) {
        const uint32_t c = o0 + threadIdx.x;
        const bool have = c < w.n_polar;
        uint32_t a = 0;
        double q[3] = {0, 0, 0};
        if (have) { a = w.polar[c]; coord(a, q); }
        for (uint32_t t = 0; t < n_tile; t++) {  // (the same on every lane)
            const double dx = q[0] - s_w[0][t], dy = q[1] - s_w[1][t], dz = q[2] - s_w[2][t];
            const double d2 = dx * dx + dy * dy + dz * dz;
            const bool hit = have && d2 <= 12.25;
            const unsigned long long mask = __ballot(hit);
            if (!mask) continue;
            uint32_t at = 0;
            if (lane == 0u) at = atomicAdd(&s_cnt[t], (uint32_t)__popcll(mask));
            at = (uint32_t)__shfl((int)at, 0);
            const uint32_t slot = at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (!hit) continue;
            if (slot < kFreqWaterPartners) { s_pa[t][slot] = a; s_pd[t][slot] = d2; }
            else atomicOr(err, 1u);
        }
    }
    __syncthreads();
    // sweep 2: the bridges
    for (uint32_t t = threadIdx.x >> 6; t < n_tile; t += blockDim.x >> 6) {
        const uint32_t cnt = min(s_cnt[t], kFreqWaterPartners), n_cand = cnt * cnt;  // (the same on every lane of the wave)
        for (uint32_t o0 = 0; o0 < n_cand; o0 += 64u) {
            const uint32_t k = o0 + lane;
            bool hit = false;
            uint32_t p = 0, q = 0;
            double d2p = 0.0, d2q = 0.0;
            if (k < n_cand && k / cnt != k % cnt) {
                p = s_pa[t][k / cnt]; q = s_pa[t][k % cnt];
                d2p = s_pd[t][k / cnt]; d2q = s_pd[t][k % cnt];
                const uint32_t ap = attr[p], aq = attr[q];
                if ((ap & ARP_ATTR_LIGAND) && (aq & ARP_ATTR_RECEPTOR)) {
                    const ResKeyD pk{0, chain_rank[p], res_ord[p], (ap & ARP_ATTR_LIGAND) != 0u, (ap & ARP_ATTR_RECEPTOR) != 0u};
                    const ResKeyD qk{0, chain_rank[q], res_ord[q], (aq & ARP_ATTR_LIGAND) != 0u, (aq & ARP_ATTR_RECEPTOR) != 0u};
                    hit = compare_residues_d(pk, qk, true);
                }
            }
            const unsigned long long mask = __ballot(hit);
            if (!mask) continue;
            uint32_t at = 0;
            if (lane == 0u) at = atomicAdd(counter, (uint32_t)__popcll(mask));
            at = (uint32_t)__shfl((int)at, 0);
            const unsigned long long o = (unsigned long long)base + at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (!hit || o >= cap) continue;
            if constexpr (TRIPLES) {
                triples[o] = WaterTriple{f0 + f, p, q, w.water[w0 + t], (float)sqrt(d2p), (float)sqrt(d2q)};
            } else {
                const uint32_t d = freq_code((float)sqrt(fmax(d2p, d2q)));  // the longer leg
                keys[o] = ((unsigned long long)rk.res_of[p] << rk.shift_a) | ((unsigned long long)rk.res_of[q] << rk.shift_b) |
                          ((unsigned long long)ARP_WaterBridge << rk.frame_bits) | (unsigned long long)(f + 1u);
                vals[o] = FreqVal{1u, d, d};
            }
        }
    }
}

// arp_water_bridges: the triples of every frame, ordered by (frame, p, q, w).  No pair pass: the frames go to the device chunk by chunk as they came
// from the host, and the kernel reads them in place.
arp_status device_water_bridges(arp_context *ctx, const FreqJob &job, std::vector<WaterTriple> *out) {
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(context_device(ctx)));
    StreamLapTimer lap("    water bridges %-22s %8.3f ms\n", st);
    out->clear();
    const uint64_t n = job.n, F = job.n_frames, nw = job.n_water, np = job.n_polar;
    if (n == 0 || F == 0 || nw == 0 || np < 2) return ARP_OK;
    const uint64_t tiles = (nw + kFreqWaterTile - 1) / kFreqWaterTile;
    const uint64_t budget = job.chunk_atoms ? job.chunk_atoms : kFreqAutoAtoms;
    const uint64_t per = std::min<uint64_t>({std::max<uint64_t>(1, budget / n), F, 0x7FFFFFF0ull / std::max<uint64_t>(n, tiles)});
    if (per == 0) { set_error("water bridges: one frame exceeds 32-bit indices"); return ARP_ERR_BAD_INPUT; }
    uint32_t *attr = nullptr, *res_ord = nullptr, *chain_rank = nullptr, *water = nullptr, *polar = nullptr, *counter = nullptr; double *xyz = nullptr;
    DevBlock block;
    arp_status s;
    if ((s = block.carve([&](Bump &bp) {
            attr = bp.take<uint32_t>(n); res_ord = bp.take<uint32_t>(n); chain_rank = bp.take<uint32_t>(n); water = bp.take<uint32_t>(nw); polar = bp.take<uint32_t>(np);
            xyz = bp.take<double>(per * n * 3); counter = bp.take<uint32_t>(64);
        })) != ARP_OK) return s;
    HIP_TRY(hipMemcpyAsync(attr, job.attr, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(res_ord, job.res_ord, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(chain_rank, job.chain_rank, n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(water, job.water, nw * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(polar, job.polar, np * 4, hipMemcpyHostToDevice, st));
    lap("topology upload");
    const FreqWaters fw{(uint32_t)nw, (uint32_t)np, water, polar};
    WaterTriple *rec = nullptr;
    uint64_t rec_cap = 0;
    struct FreeRec { WaterTriple **p; ~FreeRec() { if (*p) (void)hipFree(*p); } } rec_owner{&rec};
    auto rec_alloc = [&](uint64_t cap) -> arp_status {
        if (cap > 0x7FFFFFF0ull) { set_error("water bridges: more than 2^31 bridges in one pass (lower freq_chunk_atoms)"); return ARP_ERR_CAPACITY; }
        if (rec) { (void)hipFree(rec); rec = nullptr; rec_cap = 0; }
        HIP_TRY(hipMalloc((void **)&rec, cap * sizeof(WaterTriple)));
        rec_cap = cap;
        return ARP_OK;
    };
    s = rec_alloc(g_debug.freq_cap_items > 0 ? (uint64_t)g_debug.freq_cap_items : std::max<uint64_t>(1u << 14, 4 * nw));
    if (s != ARP_OK) return s;
    for (uint64_t f0 = 0; f0 < F; f0 += per) {
        const uint64_t fc = std::min<uint64_t>(per, F - f0);
        HIP_TRY(hipMemcpyAsync(xyz, job.xyz + f0 * n * 3, fc * n * 24, hipMemcpyHostToDevice, st));
        uint32_t h[2] = {0u, 0u};  // {bridges, error word}
        for (int attempt = 0;; attempt++) {  // grown and repeated when the bridges do not fit, as in freq_sweep
            HIP_TRY(hipMemsetAsync(counter, 0, 8, st));
            hipLaunchKernelGGL(k_freq_water_rows<true>, dim3((uint32_t)(fc * tiles)), dim3(256), 0, st, (uint32_t)tiles, (uint32_t)n, fw, (const uint32_t *)attr,
                               (const uint32_t *)res_ord, (const uint32_t *)chain_rank, (const double *)xyz, (const double *)nullptr, (const double *)nullptr,
                               (unsigned long long *)nullptr, (FreqVal *)nullptr, rec, (uint32_t)f0, 0u, (uint32_t)rec_cap, counter, counter + 1, FreqResKey{nullptr, 0u, 0u, 0u});
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h, counter, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (h[1]) return water_capacity_error();
            if (h[0] <= rec_cap) break;
            if (attempt) { set_error("internal error: the item count changed between passes"); return ARP_ERR_HIP; }
            if ((s = rec_alloc((uint64_t)h[0] + h[0] / 4u)) != ARP_OK) return s;
        }
        if (out->size() + h[0] > 0x7FFFFFFFull) { set_error("water bridges: more than 2^31 rows"); return ARP_ERR_CAPACITY; }
        const size_t had = out->size();
        out->resize(had + h[0]);
        if (h[0]) {
            HIP_TRY(hipMemcpyAsync(out->data() + had, rec, (size_t)h[0] * sizeof(WaterTriple), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        lap("sweep");
    }
    // (the order in which waves take their places is not fixed: the rows' order is the host's)
    std::sort(out->begin(), out->end(), [](const WaterTriple &a, const WaterTriple &b) {
        if (a.frame != b.frame) return a.frame < b.frame;
        if (a.p != b.p) return a.p < b.p;
        if (a.q != b.q) return a.q < b.q;
        return a.w < b.w;
    });
    lap("sort");
    return ARP_OK;
}
