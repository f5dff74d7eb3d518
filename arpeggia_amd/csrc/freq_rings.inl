// Ring rows (CationPi, the six Pi* stackings) of contact frequencies over frames (arp_contact_frequencies_ex with ARP_FREQ_RINGS; DESIGN.md
// section 3.11).  Included by table_dev.hip inside namespace arp, behind freq.inl.
// (FreqRings and kFreqRingTile: freq.inl, whose device_frequencies launches these kernels.)
//
// Frame f's ring rows are, by definition, the ring rows of the single-model structure that holds model 0's atoms with frame f's coordinates.
// The kernels here therefore call the table path's own device code -- fit_plane_dev, compare_residues_d, cation_pi_d, pi_stacking_d -- on the
// pass's packed coordinates: k_freq_ring_fit is k_fit_planes with the frame as an offset, k_freq_ring_rows is k_ring_ring plus a brute-force
// k_ring_atom (every ring against every candidate atom of its frame, no cell list).  Their items join the atom items of the pass in the same
// key / value buffers: key = (n + e1) << 34 | (n + e2 or atom) << 5 | code with ring entity e as entity n + e, so all ring rows sort behind
// all atom rows.
// RES (arp_residue_contact_frequencies): the same items under the residue-level key of freq.inl -- a ring entity's
// residue is the residue of its slot, an atom's comes from the topology, the frame is the workgroup's.

// thread t = (frame f of the pass, slot k): the ring plane of residue slot_res[k] from frame f's coordinates, atoms in k_fit_planes' order
__global__ __launch_bounds__(128) void k_freq_ring_fit(uint32_t frames, uint32_t n, FreqRings r, const double *x, const double *y, const double *z, PlaneD *planes) {
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (unsigned long long)frames * r.n_slots) return;
    const uint32_t f = (uint32_t)(t / r.n_slots), k = (uint32_t)(t % r.n_slots), res = r.slot_res[k];
    const size_t at = (size_t)f * n;  // (frames x n < 2^32: checked by the host)
    PlaneD pl;
    if (!fit_plane_dev(x + at, y + at, z + at, r.res_atom_idx, r.res_atom_ptr[res], r.res_atom_ptr[res + 1u], r.plane_bits, 1u, &pl)) pl = PlaneD{{0, 0, 0}, {0, 0, 1}};  // (a slot has >= 3 ring atoms)
    planes[t] = pl;
}

// One workgroup = (frame f, tile of kFreqRingTile ring entities).  The tile's planes and residue keys sit in LDS as separate arrays, so that the
// inner loops read one word per array and ring, the same address on every lane (a broadcast: no bank conflict whatever the record size).  The
// lanes sweep first the frame's rings (k_ring_ring: e1 in the ligand set, e2 in the receptor set, centres within 6 A first), then the topology's
// candidate atoms (k_ring_atom: d^2 <= cutoff^2 in f64, the residue rule, then the plane arithmetic).  A hit is rare; the waves stay converged
// around it, and per (tile ring, sweep step) the hits of a wave take their places with ONE atomic on the pass's item counter (k_freq_expand's
// counter).  Nothing is written at or past cap; the counter counts every item.  item_frame (nullable): the item's frame inside the pass, at the key's place.
template <bool RES>
__global__ __launch_bounds__(256) void k_freq_ring_rows(uint32_t n_tiles, uint32_t n, FreqRings r, const uint32_t *attr, const uint32_t *res_ord, const uint32_t *chain_rank,
                                                        const double *x, const double *y, const double *z, const PlaneD *planes, double cutoff,
                                                        unsigned long long *keys, FreqVal *vals, uint32_t base, uint32_t cap, uint32_t *counter, FreqResKey rk, uint32_t *item_frame) {
    __shared__ double s_c[3][kFreqRingTile], s_n[3][kFreqRingTile];
    __shared__ uint32_t s_chain[kFreqRingTile], s_ord[kFreqRingTile], s_flags[kFreqRingTile], s_res[RES ? kFreqRingTile : 1];
    const uint32_t f = blockIdx.x / n_tiles, e0 = (blockIdx.x % n_tiles) * kFreqRingTile, lane = threadIdx.x & 63u;
    const uint32_t n_tile = min(kFreqRingTile, r.n_rings - e0);
    const PlaneD *fp = planes + (size_t)f * r.n_slots;
    if (threadIdx.x < n_tile) {
        const RingEnt k = r.rings[e0 + threadIdx.x];
        const PlaneD pl = fp[k.src_res];
        for (int a = 0; a < 3; a++) { s_c[a][threadIdx.x] = pl.c[a]; s_n[a][threadIdx.x] = pl.n[a]; }
        s_chain[threadIdx.x] = k.chain_rank; s_ord[threadIdx.x] = k.ord; s_flags[threadIdx.x] = k.flags;
        if constexpr (RES) s_res[threadIdx.x] = r.slot_res[k.src_res];
    }
    __syncthreads();
    // every lane of the wave calls this at the same point: the hits take consecutive places from one atomic
    auto append = [&](bool hit, unsigned long long key, double dist) {
        const unsigned long long mask = __ballot(hit);
        if (!mask) return;
        uint32_t at = 0;
        if (lane == 0u) at = atomicAdd(counter, (uint32_t)__popcll(mask));
        at = (uint32_t)__shfl((int)at, 0);
        const unsigned long long o = (unsigned long long)base + at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
        if (hit && o < cap) {
            const uint32_t d = freq_code((float)dist);  // (narrowed to f32 where the table path narrows it: append_row)
            keys[o] = key;
            vals[o] = FreqVal{1u, d, d};
            if (item_frame) item_frame[o] = f;  // (the mark sweep of timeline.inl: an atom-level key does not hold the frame)
        }
    };
    // the item's key: from tile ring t to ring entity e2 (to_ring) or to topology atom `to`
    auto item_key = [&](uint32_t t, bool to_ring, uint32_t to, uint32_t to_res, uint32_t code) {
        if constexpr (RES)
            return ((unsigned long long)s_res[t] << rk.shift_a) | ((unsigned long long)to_res << rk.shift_b) | ((unsigned long long)code << rk.frame_bits) | (unsigned long long)(f + 1u);
        else
            return ((unsigned long long)(n + e0 + t) << kFreqKeyShiftI) | ((unsigned long long)(to_ring ? n + to : to) << kFreqKeyShiftJ) | (unsigned long long)code;
    };
    auto tile_plane = [&](uint32_t t) { return PlaneD{{s_c[0][t], s_c[1][t], s_c[2][t]}, {s_n[0][t], s_n[1][t], s_n[2][t]}}; };
    auto tile_key = [&](uint32_t t) { return ResKeyD{0, s_chain[t], s_ord[t], (s_flags[t] & 1u) != 0u, (s_flags[t] & 2u) != 0u}; };
    // ring - ring
    for (uint32_t o0 = 0; o0 < r.n_rings; o0 += blockDim.x) {
        const uint32_t e2 = o0 + threadIdx.x;
        const bool have = e2 < r.n_rings;
        RingEnt k2{};
        PlaneD p2{};
        uint32_t res2 = 0;
        if (have) { k2 = r.rings[e2]; p2 = fp[k2.src_res]; if constexpr (RES) res2 = r.slot_res[k2.src_res]; }
        const bool ok2 = have && (k2.flags & 4u) && (k2.flags & 2u);
        const ResKeyD r2k{0, k2.chain_rank, k2.ord, (k2.flags & 1u) != 0u, (k2.flags & 2u) != 0u};
        for (uint32_t t = 0; t < n_tile; t++) {
            const uint32_t fl = s_flags[t];
            if (!(fl & 4u) || !(fl & 1u)) continue;  // (the same on every lane)
            bool hit = false;
            int code = -1;
            double dist = 0.0;
            if (ok2) {
                const PlaneD p1 = tile_plane(t);
                const double v[3] = {p1.c[0] - p2.c[0], p1.c[1] - p2.c[1], p1.c[2] - p2.c[2]};
                dist = norm3d(v);
                if (dist <= 6.0 && compare_residues_d(tile_key(t), r2k, true)) {
                    code = pi_stacking_d(p1, p2, dist);
                    hit = code >= 0;
                }
            }
            append(hit, item_key(t, true, e2, res2, (uint32_t)(hit ? code : 0)), dist);
        }
    }
    // ring - cation
    const double r2 = cutoff * cutoff;  // (k_ring_atom: only ever the square)
    const size_t at0 = (size_t)f * n;
    for (uint32_t o0 = 0; o0 < r.n_cand; o0 += blockDim.x) {
        const uint32_t c = o0 + threadIdx.x;
        const bool have = c < r.n_cand;
        uint32_t a = 0, aw = 0, res_a = 0;
        double q[3] = {0, 0, 0};
        ResKeyD yk{0, 0u, 0u, false, false};
        if (have) {
            a = r.cand[c]; aw = attr[a];
            if constexpr (RES) res_a = rk.res_of[a];
            q[0] = x[at0 + a]; q[1] = y[at0 + a]; q[2] = z[at0 + a];
            yk = ResKeyD{0, chain_rank[a], res_ord[a], (aw & ARP_ATTR_LIGAND) != 0u, (aw & ARP_ATTR_RECEPTOR) != 0u};
        }
        for (uint32_t t = 0; t < n_tile; t++) {
            if (!(s_flags[t] & 4u)) continue;  // (the same on every lane)
            bool hit = false;
            double dist = 0.0;
            if (have) {
                const double dx = q[0] - s_c[0][t], dy = q[1] - s_c[1][t], dz = q[2] - s_c[2][t];
                if (dx * dx + dy * dy + dz * dz <= r2 && compare_residues_d(tile_key(t), yk, false)) hit = cation_pi_d(tile_plane(t), q, &dist);
            }
            append(hit, item_key(t, false, a, res_a, (uint32_t)ARP_CationPi), dist);
        }
    }
}
