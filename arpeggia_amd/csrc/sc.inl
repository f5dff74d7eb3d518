// Shape complementarity (Lawrence & Colman 1993; reference src/sc/surface_generator.rs, src/sc/sc_calculator.rs).  Included by kernels.hip
// inside namespace arp; the host side (stage order, cell geometry, medians) is sc.cpp, the contract is DESIGN.md section 3.6.
//
// Every rule is the reference's, in f64, with its operation order (no contraction: the build's -ffp-contract=off; division and square
// root correctly rounded; sin / cos / atan2 / acos / exp from the device library, a few ulps from glibc's):
//   atoms      sc_calculator.rs:40-111 + surface_generator.rs:145-215: Buried iff an atom of the other molecule has d^2 < sep^2; the
//              same-molecule neighbours are those with d^2 <= sep^2 (rstar's inclusive query) and d^2 < (r_i + r_j + 2 rp)^2, sorted by
//              d^2 and then by atom index (the reference's sort is unstable); a same-molecule pair with d^2 <= 1e-4 is the Coincident error.
//   pairs      :375-688: probes (:442-545, the sin_wedge <= 0 `return` kept) and toroidal dots (:547-688, atom j's arc only when j is Far).
//   contact    :217-373: north / south from neighbour 0, collision with neighbours 1.. on the distance with <=.
//   concave    :713-880: nears = the other low probes (height < rp) with d^2 <= 4 rp^2; one burial decision per probe (its centre).
//   burial     add_dot :882-915 and :332-344 / :842-854: d^2(pcen, b) <= (r_b + rp)^2 for some atom b of the other molecule.
//   trim / nn  sc_calculator.rs:221-347: trimmed = buried with no non-buried dot of its surface within d^2 <= band^2; nearest trimmed dot
//              of the other surface (lower index on a tie), r = clamp(n1.n2 exp(-d^2 w), -0.999, 0.999), score = -r.
//
// Mapping: every stage is a count pass, a scan and a fill pass that runs the same code again and writes at the scanned offset, so every
// output lands in the reference's sequential order and no capacity is fixed.  Atoms, pairs (i, j), trim and nearest neighbour run one
// thread per item; the contact and concave stages run one wave per atom / probe with the lanes over its latitudes (sc_wave_lats).  A
// sampling angle is the result of k sequential additions (`a += delta`): a lane replays them up to its own sample, which gives the
// reference's values bit for bit.  Neighbour searches use uniform cell lists (ScCells) whose edge is at least the search radius, so a
// 27-cell visit is exhaustive; burial tests walk the atom's candidate list (other-molecule atoms within r_i + r_b + 2 rp + kScBurMargin),
// which holds every atom that can bury a point at distance r_i + rp of atom i.
//
// Every kernel with relations between items is a template on ENS.  ENS = false is the single-frame path of launch_sc below, which passes an empty
// ScEns and compiles to the code it had before the parameter existed; ENS = true takes many frames of one topology at once (sc_ens.inl).

constexpr double kScBurMargin = 0.01;  // A: slack of the burial candidate lists over r_i + r_b + 2 rp (positions are within ~1e-12 A of their sphere)
constexpr uint32_t kScDotConvex = ARP_SC_DOT_CONVEX, kScDotToroidal = ARP_SC_DOT_TOROIDAL, kScDotConcave = ARP_SC_DOT_CONCAVE, kScDotBuried = ARP_SC_DOT_BURIED,
                   kScDotTrimmed = ARP_SC_DOT_TRIMMED;

struct ScCells {      // uniform cell list over a point set (sc.cpp sc_cells): start[ncells + 1], item[] = point indices
    double ox, oy, oz, inv;
    int nx, ny, nz;
    const uint32_t *start, *item;
    const double *org;  // ensemble (sc_ens.inl): one slab of nx ny nz cells per frame, frame f's origin at org[3 f]; the single-frame path leaves it unset
};
// What the frame-aware instantiations (ENS) of the kernels below need; the single-frame launches pass ScEns{} and never read it (sc_ens.inl)
struct ScEns {
    uint32_t n_per;              // atoms per frame: the frame of any item is (its owner atom) / n_per
    unsigned long long *coinc;   // [B] the coincident-pair word of each frame (minimum over its pairs, atoms local to the frame)
    uint32_t *subdiv;            // [B] the subdivision flag of each frame
    const uint32_t *adj[2];      // [B] added to a fill offset: moves a frame's run of this kind into the frame's segment of the surface
    const uint32_t *other;       // [B + 1] trim: the segment starts of the other surface (a frame without dots there is not trimmed)
};
struct ScAtoms {
    uint32_t n;
    const double4 *c;       // x, y, z, radius
    const uint32_t *mol;
    const long long *serial;
    double rp, density, sep, r_max;
};

struct DV { double x, y, z; };
__device__ inline DV v3(double x, double y, double z) { return DV{x, y, z}; }
__device__ inline DV vadd(DV a, DV b) { return v3(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ inline DV vsub(DV a, DV b) { return v3(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ inline DV vmul(DV a, double s) { return v3(a.x * s, a.y * s, a.z * s); }
__device__ inline DV vdiv(DV a, double s) { return v3(__ddiv_rn(a.x, s), __ddiv_rn(a.y, s), __ddiv_rn(a.z, s)); }
__device__ inline double vdot(DV a, DV b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ inline DV vcross(DV a, DV b) { return v3(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
__device__ inline DV vnorm(DV a) {
    const double m2 = vdot(a, a), m = __dsqrt_rn(m2 > 0.0 ? m2 : 0.0);
    return m > 0.0 ? vdiv(a, m) : a;
}
__device__ inline double vd2(DV a, DV b) { const DV d = vsub(a, b); return vdot(d, d); }
__device__ inline DV catom(const ScAtoms &A, uint32_t i) { const double4 c = A.c[i]; return v3(c.x, c.y, c.z); }
__device__ inline DV dp3(const double *p) { return v3(p[0], p[1], p[2]); }

// the cell of p; returns the first cell of the slab it lies in (0 unless ENS: the slab of frame f, around that frame's own origin)
template <bool ENS = false>
__device__ inline uint32_t cell_of(const ScCells &g, DV p, int &cx, int &cy, int &cz, uint32_t f = 0) {
    const double ox = ENS ? g.org[3u * f] : g.ox, oy = ENS ? g.org[3u * f + 1u] : g.oy, oz = ENS ? g.org[3u * f + 2u] : g.oz;
    cx = (int)floor((p.x - ox) * g.inv); cy = (int)floor((p.y - oy) * g.inv); cz = (int)floor((p.z - oz) * g.inv);
    cx = min(max(cx, 0), g.nx - 1); cy = min(max(cy, 0), g.ny - 1); cz = min(max(cz, 0), g.nz - 1);
    return ENS ? f * ((uint32_t)g.nx * (uint32_t)g.ny * (uint32_t)g.nz) : 0u;
}
// f(item) over the items of the cells within `reach` cells of p's cell; stops when f returns true
template <bool ENS = false, class F>
__device__ inline bool cells_visit(const ScCells &g, DV p, int reach, F &&f, uint32_t frame = 0) {
    int cx, cy, cz;
    const uint32_t slab = cell_of<ENS>(g, p, cx, cy, cz, frame);
    for (int z = max(cz - reach, 0); z <= min(cz + reach, g.nz - 1); z++)
        for (int y = max(cy - reach, 0); y <= min(cy + reach, g.ny - 1); y++) {
            const uint32_t row = slab + ((uint32_t)z * (uint32_t)g.ny + (uint32_t)y) * (uint32_t)g.nx;
            const uint32_t lo = g.start[row + (uint32_t)max(cx - reach, 0)], hi = g.start[row + (uint32_t)min(cx + reach, g.nx - 1) + 1u];
            for (uint32_t s = lo; s < hi; s++) if (f(g.item[s])) return true;
        }
    return false;
}

// ---- cell lists: count, (scan on the host side), fill.  Point k of a strided f64 array is included by `mode`.
enum : uint32_t { kScPtAll = 0, kScPtDotOpen = 1, kScPtDotTrimmed = 2, kScPtLowProbe = 3 };
__device__ inline bool sc_pt(uint32_t mode, const double *base, uint32_t stride, uint32_t k, double rp, DV &p) {
    const double *q = base + (size_t)k * stride;
    p = dp3(q);
    if (mode == kScPtDotOpen) return !(((const ScDot *)q)->flags & kScDotBuried);
    if (mode == kScPtDotTrimmed) return (((const ScDot *)q)->flags & kScDotTrimmed) != 0u;
    if (mode == kScPtLowProbe) return ((const ScProbe *)q)->height < rp;
    return true;
}
__global__ __launch_bounds__(256) void k_sc_cell_count(const double *base, uint32_t stride, uint32_t n, uint32_t mode, double rp, ScCells g,
                                                       uint32_t *count, uint32_t *rank) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    DV p;
    if (!sc_pt(mode, base, stride, k, rp, p)) { rank[k] = ~0u; return; }
    int cx, cy, cz;
    cell_of(g, p, cx, cy, cz);
    const uint32_t c = ((uint32_t)cz * (uint32_t)g.ny + (uint32_t)cy) * (uint32_t)g.nx + (uint32_t)cx;
    rank[k] = atomicAdd(&count[c], 1u);
}
__global__ __launch_bounds__(256) void k_sc_cell_fill(const double *base, uint32_t stride, uint32_t n, double rp, ScCells g, const uint32_t *rank,
                                                      uint32_t *item) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n || rank[k] == ~0u) return;
    const DV p = dp3(base + (size_t)k * stride);
    int cx, cy, cz;
    cell_of(g, p, cx, cy, cz);
    const uint32_t c = ((uint32_t)cz * (uint32_t)g.ny + (uint32_t)cy) * (uint32_t)g.nx + (uint32_t)cx;
    item[g.start[c] + rank[k]] = k;
}

// ---- exclusive scan of n + 1 uint32 (in[n] = 0 gives out[n] = the total): 1024 per block, block sums scanned by the host recursion
constexpr uint32_t kScScanBlock = 1024;
__global__ __launch_bounds__(256) void k_sc_scan_block(const uint32_t *in, uint32_t *out, uint32_t *bsum, uint32_t n) {
    __shared__ uint32_t wsum[4];
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6, base = blockIdx.x * kScScanBlock + t * 4u;
    uint32_t v[4], s = 0;
    for (int k = 0; k < 4; k++) { v[k] = base + k < n ? in[base + k] : 0u; s += v[k]; }
    uint32_t inc = s;  // inclusive scan over the wave
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    if (lane == 63u) wsum[w] = inc;
    __syncthreads();
    uint32_t off = 0;
    for (uint32_t k = 0; k < w; k++) off += wsum[k];
    uint32_t run = off + inc - s;
    for (int k = 0; k < 4; k++) { if (base + k < n) out[base + k] = run; run += v[k]; }
    if (t == 255u) bsum[blockIdx.x] = off + inc;
}
__global__ __launch_bounds__(256) void k_sc_scan_add(uint32_t *out, const uint32_t *boff, uint32_t n) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n) out[k] += boff[k / kScScanBlock];
}

// ---- (a) atoms: attention, neighbour lists (CSR, sorted by (d^2, index)), burial candidate lists, coincidence
template <bool FILL, bool ENS = false>
__global__ __launch_bounds__(256) void k_sc_atoms(ScAtoms A, ScCells g, uint32_t *nb_cnt, uint32_t *bur_cnt, uint32_t *att, uint32_t *acc, unsigned long long *err,
                                                  const uint32_t *nb_off, uint32_t *nb_idx, double *nb_d2, uint32_t *nb_own, const uint32_t *bur_off,
                                                  uint32_t *bur_idx, ScEns E) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= A.n) return;
    const uint32_t fr = ENS ? i / E.n_per : 0u, a0 = fr * (ENS ? E.n_per : 0u);  // the frame and its first atom
    if (ENS && FILL && E.coinc[fr] != ~0ull) return;  // a frame with a coincident pair has no lists (its counts were zeroed)
    const double4 ci4 = A.c[i];
    const DV ci = v3(ci4.x, ci4.y, ci4.z);
    const double ri = ci4.w, s2 = A.sep * A.sep;
    const uint32_t mi = A.mol[i];
    double best = INFINITY;
    uint32_t m = 0, b = 0;
    const uint32_t nb0 = FILL ? nb_off[i] : 0u, bur0 = FILL ? bur_off[i] : 0u;
    cells_visit<ENS>(g, ci, 1, [&](uint32_t j) {
        const double4 cj = A.c[j];
        const double d2 = vd2(ci, v3(cj.x, cj.y, cj.z));
        if (A.mol[j] != mi) {
            const double reach = ri + cj.w + 2.0 * A.rp + kScBurMargin;
            if (d2 <= reach * reach) { if (FILL) bur_idx[bur0 + b] = j; b++; }
            if (d2 <= s2 && d2 < best) best = d2;
            return false;
        }
        if (!(d2 <= s2) || A.serial[j] == A.serial[i]) return false;
        if (!FILL && d2 <= 0.0001) atomicMin(ENS ? E.coinc + fr : err, ((unsigned long long)(i - a0) << 32) | (j - a0));
        const double bridge = ri + cj.w + 2.0 * A.rp;
        if (d2 < bridge * bridge) {
            if (FILL) {  // insertion into this atom's segment by (d^2, index)
                uint32_t k = m;
                while (k > 0 && (nb_d2[nb0 + k - 1] > d2 || (nb_d2[nb0 + k - 1] == d2 && nb_idx[nb0 + k - 1] > j))) {
                    nb_d2[nb0 + k] = nb_d2[nb0 + k - 1]; nb_idx[nb0 + k] = nb_idx[nb0 + k - 1]; k--;
                }
                nb_d2[nb0 + k] = d2; nb_idx[nb0 + k] = j; nb_own[nb0 + m] = i;
            }
            m++;
        }
        return false;
    }, fr);
    if (!FILL) { nb_cnt[i] = m; bur_cnt[i] = b; att[i] = best < s2 ? 1u : 0u; acc[i] = m == 0u ? 1u : 0u; }
}

// ---- sampling (surface_generator.rs:918-1091).  emit(k, point) for each sample; returns false on TooManySubdivisions.
template <class F>
__device__ inline bool sc_segment(DV cen, double rad, DV x, DV y, double angle, double density, uint32_t &n, double &ps, F &&emit) {
    n = 0;
    if (rad <= 0.0) { ps = 0.0; return true; }
    const double delta = __ddiv_rn(1.0, __dsqrt_rn(density) * rad);
    double a = __ddiv_rn(-delta, 2.0);
    for (int it = 0; it < 100000; it++) {
        a += delta;
        if (a > angle) break;
        const double c = rad * cos(a), s = rad * sin(a);
        emit(n, vadd(vadd(cen, vmul(x, c)), vmul(y, s)));
        n++;
    }
    if (a + delta < angle) return false;
    ps = n == 0 ? 0.0 : __ddiv_rn(rad * angle, (double)n);
    return true;
}
template <class F>
__device__ inline bool sc_arc(DV cen, double rad, DV axis, double density, DV x, DV v, uint32_t &n, double &ps, F &&emit) {
    const DV y = vcross(axis, x);
    double angle = atan2(vdot(v, y), vdot(v, x));
    if (angle < 0.0) angle += 2.0 * M_PI;
    return sc_segment(cen, rad, x, y, angle, density, n, ps, emit);
}
template <class F>
__device__ inline bool sc_circle(DV cen, double rad, DV axis, double density, uint32_t &n, double &ps, F &&emit) {
    DV v1 = vnorm(v3(axis.y * axis.y + axis.z * axis.z, axis.x * axis.x + axis.z * axis.z, axis.x * axis.x + axis.y * axis.y));
    if (fabs(vdot(v1, axis)) > 0.99) v1 = v3(1.0, 0.0, 0.0);
    const DV v2 = vnorm(vcross(axis, v1));
    const DV x = vnorm(vcross(axis, v2));
    const DV y = vcross(axis, x);
    return sc_segment(cen, rad, x, y, 2.0 * M_PI, density, n, ps, emit);
}
__device__ inline bool sc_buried(const ScAtoms &A, const uint32_t *bur_off, const uint32_t *bur_idx, uint32_t owner, DV pcen) {
    for (uint32_t e = bur_off[owner]; e < bur_off[owner + 1]; e++) {
        const double4 b = A.c[bur_idx[e]];
        const double erl = b.w + A.rp;
        if (vd2(pcen, v3(b.x, b.y, b.z)) <= erl * erl) return true;
    }
    return false;
}
__device__ inline void sc_put(ScDot *d, DV p, DV nml, double area, uint32_t atom, uint32_t flags) {
    d->p[0] = p.x; d->p[1] = p.y; d->p[2] = p.z; d->n[0] = nml.x; d->n[1] = nml.y; d->n[2] = nml.z;
    d->area = area; d->nn_dist = 0.0; d->score = 0.0; d->atom = atom; d->flags = flags;
}

// ---- (b) one item per neighbour-list entry (i, j): build_probes' body (:389-438), build_probe_triplets, emit_reentrant_surface
struct ScPairOut { uint32_t *p_cnt, *t_cnt[2], *acc; unsigned long long *err; const uint32_t *p_off, *t_off[2]; ScProbe *probes; ScDot *tor[2]; };
template <bool FILL, bool ENS = false>
__global__ __launch_bounds__(256) void k_sc_pairs(ScAtoms A, uint32_t n_items, const uint32_t *nb_off, const uint32_t *nb_idx, const double *nb_d2,
                                                  const uint32_t *nb_own, const uint32_t *att, const uint32_t *bur_off, const uint32_t *bur_idx, ScPairOut o,
                                                  ScEns E) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    if (e >= n_items) return;
    const uint32_t i = nb_own[e], j = nb_idx[e], mi = A.mol[i];
    uint32_t np = 0, nt = 0;
    const double rp = A.rp;
    auto finish = [&]() {
        if (!FILL) { o.p_cnt[e] = np; o.t_cnt[mi][e] = nt; o.t_cnt[1u - mi][e] = 0u; }
    };
    if (att[i] == 0u || A.serial[j] <= A.serial[i]) { finish(); return; }
    const uint32_t nb0 = nb_off[i], nb1 = nb_off[i + 1], num = nb1 - nb0;
    const DV ci = catom(A, i), cj = catom(A, j);
    const double ri = A.c[i].w, rj = A.c[j].w, ei = ri + rp, ej = rj + rp;
    const double d2 = nb_d2[e], dij = __dsqrt_rn(d2);
    const DV ua = vdiv(vsub(cj, ci), dij);
    const double asym = __ddiv_rn(ei * ei - ej * ej, dij);
    const DV mid = vadd(vmul(vadd(ci, cj), 0.5), vmul(ua, asym * 0.5));
    double far = (ei + ej) * (ei + ej) - d2;
    if (far <= 0.0) { finish(); return; }
    far = __dsqrt_rn(far);
    const double dr = ri - rj;
    double contain = d2 - dr * dr;
    if (contain <= 0.0) { finish(); return; }
    contain = __dsqrt_rn(contain);
    const double ring_r = __ddiv_rn(0.5 * far * contain, dij);
    if (num <= 1u) {  // (:418-422: both accessible, and the loop ends -- there is no other j)
        if (!FILL) { atomicOr(&o.acc[i], 1u); atomicOr(&o.acc[j], 1u); }
        finish();
        return;
    }
    // build_probe_triplets (:442-545)
    bool made = false;
    for (uint32_t q = nb0; q < nb1; q++) {
        const uint32_t k = nb_idx[q];
        if (A.serial[k] <= A.serial[j]) continue;
        const DV ck = catom(A, k);
        const double ek = A.c[k].w + rp;
        const double djk2 = vd2(cj, ck);
        if (!(djk2 <= A.sep * A.sep)) continue;  // k is not in j's map
        if (__dsqrt_rn(djk2) >= ej + ek) continue;
        const double dik = __dsqrt_rn(nb_d2[q]);
        if (dik >= ei + ek) continue;
        if (att[i] == 0u && att[j] == 0u && att[k] == 0u) continue;
        const DV uik = vdiv(vsub(ck, ci), dik);
        const double sw = sin(acos(vdot(ua, uik)));
        if (sw <= 0.0) {
            const double dtijk2 = __dsqrt_rn(vd2(mid, ck));
            const double rkp2 = ek * ek - ring_r * ring_r;
            if (dtijk2 < rkp2) { made = false; break; }  // (:494-496 returns: no accessible update from this pair's probes)
            continue;
        }
        const DV an = vdiv(vcross(ua, uik), sw);
        const DV perp = vcross(an, ua);
        const double asym_ik = __ddiv_rn(ei * ei - ek * ek, dik);
        const DV mid_ik = vadd(vmul(vadd(ci, ck), 0.5), vmul(uik, asym_ik * 0.5));
        DV cw = vsub(mid_ik, mid);
        cw = v3(uik.x * cw.x, uik.y * cw.y, uik.z * cw.z);
        const double csum = cw.x + cw.y + cw.z;
        const DV tc = vadd(mid, vmul(perp, __ddiv_rn(csum, sw)));
        double h = ei * ei - vd2(tc, ci);
        if (h <= 0.0) continue;
        h = __dsqrt_rn(h);
        for (int is0 = 1; is0 <= 2; is0++) {
            const int sign = 3 - 2 * is0;
            const DV pc = vadd(tc, vmul(an, h * (double)sign));
            bool coll = false;  // check_atom_collision2_idx (:690-711)
            for (uint32_t u = nb0; u < nb1 && !coll; u++) {
                const uint32_t ni = nb_idx[u];
                if (A.serial[ni] == A.serial[j] || A.serial[ni] == A.serial[k]) continue;
                const double4 c = A.c[ni];
                const double er = c.w + rp;
                coll = vd2(pc, v3(c.x, c.y, c.z)) <= er * er;
            }
            if (coll) continue;
            if (FILL) {
                ScProbe &P = o.probes[o.p_off[e] + np];
                P.p[0] = pc.x; P.p[1] = pc.y; P.p[2] = pc.z;
                const DV alt = vmul(an, (double)sign);
                P.alt[0] = alt.x; P.alt[1] = alt.y; P.alt[2] = alt.z;
                P.height = h;
                P.a[0] = sign > 0 ? i : j; P.a[1] = sign > 0 ? j : i; P.a[2] = k; P.i = i;
            }
            np++;
            made = true;
        }
    }
    if (made && !FILL) atomicOr(&o.acc[i], 1u);
    // emit_reentrant_surface (:547-688); (:426-428: i is never Far here, so the surface is always emitted)
    const bool point_cusp = fabs(asym) < dij;
    const double density = __ddiv_rn(A.density + A.density, 2.0);
    const double rri = __ddiv_rn(ring_r * ri, ei), rrj = __ddiv_rn(ring_r * rj, ej);
    double belt = ring_r - rp;
    if (belt <= 0.0) belt = 0.0;
    const double mean_r = __ddiv_rn(rri + 2.0 * belt + rrj, 4.0);
    const double ecc = __ddiv_rn(mean_r, ring_r);
    const double eff = ecc * ecc * density;
    ScDot *out = FILL ? o.tor[mi] + o.t_off[mi][e] : nullptr;
    uint32_t n_sub;
    double ts;
    bool ok = true;
    // ts is known only once the ring is sampled (and the reference samples it before its loop): a first pass sizes it
    bool ring_ok = sc_circle(mid, ring_r, ua, eff, n_sub, ts, [](uint32_t, DV) {});
    if (ring_ok) sc_circle(mid, ring_r, ua, eff, n_sub, ts, [&](uint32_t, DV rpnt) {
        if (!ok || (nt & 0x80000000u)) return;  // an earlier ring point ended the pair (or failed)
        for (uint32_t u = nb0; u < nb1; u++) {
            const uint32_t ni = nb_idx[u];
            if (A.serial[ni] == A.serial[j]) continue;
            const double4 c = A.c[ni];
            const double er = c.w + rp;
            if (vd2(rpnt, v3(c.x, c.y, c.z)) < er * er) return;
        }
        if (!FILL) { atomicOr(&o.acc[i], 1u); atomicOr(&o.acc[j], 1u); }
        const DV vpi = vdiv(vsub(ci, rpnt), ei), vpj = vdiv(vsub(cj, rpnt), ej);
        const DV tax = vnorm(vcross(vpi, vpj));
        double cusp = rp * rp - ring_r * ring_r;
        DV arc_i, arc_j;
        if (cusp > 0.0 && point_cusp) {
            cusp = __dsqrt_rn(cusp);
            const DV qij = vsub(mid, vmul(ua, cusp));
            arc_i = vdiv(vsub(qij, rpnt), rp);
            arc_j = v3(0.0, 0.0, 0.0);
        } else {
            arc_i = arc_j = vnorm(vadd(vpi, vpj));
        }
        double dt = vdot(arc_i, vpi);
        if (dt >= 1.0 || dt <= -1.0) { nt |= 0x80000000u; return; }
        dt = vdot(arc_j, vpj);
        if (dt >= 1.0 || dt <= -1.0) { nt |= 0x80000000u; return; }
        const bool buried = sc_buried(A, bur_off, bur_idx, i, rpnt);
        const uint32_t fl = kScDotToroidal | (buried ? kScDotBuried : 0u);
        uint32_t na;
        double ps;
        auto arc_emit = [&](uint32_t atom) {
            return [&, atom](uint32_t, DV pt) {
                if (FILL) {
                    const DV v = vsub(pt, mid);
                    const double t = vdot(v, ua);
                    double q2 = vdot(v, v) - t * t;
                    if (q2 < 0.0) q2 = 0.0;
                    const double area = __ddiv_rn(ps * ts * __dsqrt_rn(q2), ring_r);
                    sc_put(out + (nt & 0x7FFFFFFFu), pt, vdiv(vsub(rpnt, pt), rp), area, atom, fl);
                }
                nt++;
            };
        };
        // the areas need ps, known only after the arc: sample once to count, then again to write (FILL)
        if (!sc_arc(rpnt, rp, tax, density, vpi, arc_i, na, ps, [](uint32_t, DV) {})) { ok = false; return; }
        if (!sc_arc(rpnt, rp, tax, density, vpi, arc_i, na, ps, arc_emit(i))) { ok = false; return; }
        if (att[j] != 0u) return;
        if (!sc_arc(rpnt, rp, tax, density, arc_j, vpj, na, ps, [](uint32_t, DV) {})) { ok = false; return; }
        if (!sc_arc(rpnt, rp, tax, density, arc_j, vpj, na, ps, arc_emit(j))) { ok = false; return; }
    });
    // (a ring point with |dot| >= 1 ends the pair: its flag bit stops the remaining points, the dots before it stay)
    nt &= 0x7FFFFFFFu;
    if (!(ok && ring_ok) && !FILL) {
        if (ENS) atomicOr(&E.subdiv[i / E.n_per], 1u);
        else atomicOr(o.err, (unsigned long long)kScErrSubdiv);
    }
    finish();
}

// ---- (c) and (d): one wave per atom / probe, the lanes over its latitudes.  Lane l replays the latitude arc's angle accumulation up to
// sample l (the same IEEE additions as one sequential walk: the reference's values), then walks that latitude's circle: its points
// stay in the reference's order inside the lane, and the lanes' counts, scanned across the wave, place each latitude after the ones
// before it.  A wave takes 64 latitudes at a time.
__device__ inline uint32_t sc_wave_excl(uint32_t v, uint32_t &total) {  // exclusive prefix of v over the wave; total = the sum
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t inc = v;
    for (uint32_t d = 1; d < 64; d <<= 1) { const uint32_t o = __shfl_up(inc, d, 64); if (lane >= d) inc += o; }
    total = __shfl(inc, 63, 64);
    return inc - v;
}
// work(lat, dst, nd): the dots of one latitude (written from dst when dst != nullptr), false when its circle fails.  Returns the item's
// dot count, 0 when any circle failed (`.ok()?` drops the whole atom or probe).  Wave-uniform arguments.
template <bool FILL, class W>
__device__ inline uint32_t sc_wave_lats(double rad, DV axis, double density, DV from, DV to, uint32_t nl, ScDot *out, W &&work) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t total = 0;
    bool fail = false;
    for (uint32_t c0 = 0; c0 < nl; c0 += 64u) {
        const uint32_t l = c0 + lane;
        DV lat = v3(0.0, 0.0, 0.0);
        uint32_t nn;
        double cc;
        if (l < nl) sc_arc(v3(0.0, 0.0, 0.0), rad, axis, density, from, to, nn, cc, [&](uint32_t k, DV p) { if (k == l) lat = p; });
        uint32_t nd = 0;
        const bool ok = l >= nl || work(lat, (ScDot *)nullptr, nd);
        if (__any(!ok)) fail = true;
        uint32_t tot;
        const uint32_t pre = sc_wave_excl(nd, tot);
        if (FILL && l < nl && nd) { uint32_t n2 = 0; work(lat, out + total + pre, n2); }
        total += tot;
    }
    return fail ? 0u : total;
}

// (c) contact dots (:217-373), one wave per atom; out[m] + off[m][i] receives atom i's dots (m = its molecule)
constexpr uint32_t kScWaves = 4;
template <bool FILL, bool ENS = false>
__global__ __launch_bounds__(kScWaves * 64) void k_sc_contact(ScAtoms A, const uint32_t *nb_off, const uint32_t *nb_idx, const uint32_t *att,
                                                              const uint32_t *acc, const uint32_t *bur_off, const uint32_t *bur_idx, uint32_t *cnt0,
                                                              uint32_t *cnt1, const uint32_t *off0, const uint32_t *off1, ScDot *out0, ScDot *out1, ScEns E) {
    const uint32_t i = blockIdx.x * kScWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= A.n) return;  // (wave-uniform, as every return below)
    const uint32_t mi = A.mol[i];
    uint32_t nd = 0;
    auto finish = [&]() { if (!FILL && lane == 0u) { cnt0[i] = mi == 0u ? nd : 0u; cnt1[i] = mi == 1u ? nd : 0u; } };
    if (att[i] == 0u || acc[i] == 0u || (FILL && off0[i + 1] + off1[i + 1] == off0[i] + off1[i])) { finish(); return; }
    const double rp = A.rp;
    const DV ci = catom(A, i);
    const double ri = A.c[i].w, ei = ri + rp;
    const uint32_t nb0 = nb_off[i], nb1 = nb_off[i + 1];
    DV north = v3(0.0, 0.0, 1.0), south = v3(0.0, 0.0, -1.0), eq = v3(1.0, 0.0, 0.0);
    if (nb1 > nb0) {
        const uint32_t m = nb_idx[nb0];
        const DV cn = catom(A, m);
        north = vnorm(vsub(ci, cn));
        DV t = vnorm(v3(north.y * north.y + north.z * north.z, north.x * north.x + north.z * north.z, north.x * north.x + north.y * north.y));
        if (fabs(vdot(t, north)) > 0.99) t = v3(1.0, 0.0, 0.0);
        eq = vnorm(vcross(north, t));
        const double rn = A.c[m].w, en = rn + rp;
        const double dij = __dsqrt_rn(vd2(ci, cn));
        const DV ua = vdiv(vsub(cn, ci), dij);
        const double asym = __ddiv_rn(ei * ei - en * en, dij);
        const DV mid = vadd(vmul(vadd(ci, cn), 0.5), vmul(ua, asym * 0.5));
        double far = (ei + en) * (ei + en) - dij * dij;
        if (far <= 0.0) { finish(); return; }
        far = __dsqrt_rn(far);
        const double dr = ri - rn;
        double contain = dij * dij - dr * dr;
        if (contain <= 0.0) { finish(); return; }
        contain = __dsqrt_rn(contain);
        const double ring_r = __ddiv_rn(0.5 * far * contain, dij);
        const DV rpnt = vadd(mid, vmul(vcross(eq, north), ring_r));
        south = vdiv(vsub(rpnt, ci), ei);
        if (vdot(vcross(north, south), eq) <= 0.0) { finish(); return; }
    }
    ScDot *out = FILL ? (mi == 0u ? out0 + off0[i] : out1 + off1[i]) : nullptr;
    if (FILL && ENS) out += E.adj[mi][i / E.n_per];
    uint32_t nl;
    double cs;
    // the latitudes first: their count and cs (a failure drops the atom, `.ok()?`)
    if (!sc_arc(v3(0.0, 0.0, 0.0), ri, eq, A.density, north, south, nl, cs, [](uint32_t, DV) {})) { finish(); return; }
    nd = sc_wave_lats<FILL>(ri, eq, A.density, north, south, nl, out, [&](DV lat, ScDot *dst, uint32_t &n) {
        const double dt = vdot(lat, north);
        const DV cen = vadd(ci, vmul(north, dt));
        double rad = ri * ri - dt * dt;
        if (rad <= 0.0) return true;
        rad = __dsqrt_rn(rad);
        uint32_t np;
        double ps;
        if (!sc_circle(cen, rad, north, A.density, np, ps, [](uint32_t, DV) {})) return false;
        const double area = ps * cs;
        sc_circle(cen, rad, north, A.density, np, ps, [&](uint32_t, DV p) {
            const DV pcen = vadd(ci, vmul(vsub(p, ci), __ddiv_rn(ei, ri)));
            for (uint32_t q = nb0 + 1u; q < nb1; q++) {
                const double4 c = A.c[nb_idx[q]];
                if (__dsqrt_rn(vd2(pcen, v3(c.x, c.y, c.z))) <= c.w + rp) return;
            }
            if (dst) {
                const bool buried = sc_buried(A, bur_off, bur_idx, i, pcen);
                sc_put(dst + n, p, vdiv(vsub(pcen, p), rp), area, i, kScDotConvex | (buried ? kScDotBuried : 0u));
            }
            n++;
        });
        return true;
    });
    finish();
}

// (d) concave dots (:713-880), one wave per probe; all three atoms of a probe are of one molecule (same-molecule neighbours)
template <bool FILL, bool ENS = false>
__global__ __launch_bounds__(kScWaves * 64) void k_sc_concave(ScAtoms A, const ScProbe *probes, uint32_t n_probes, ScCells low, const uint32_t *bur_off,
                                                              const uint32_t *bur_idx, uint32_t *cnt0, uint32_t *cnt1, const uint32_t *off0,
                                                              const uint32_t *off1, ScDot *out0, ScDot *out1, ScEns E) {
    const uint32_t pi = blockIdx.x * kScWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (pi >= n_probes) return;  // (wave-uniform)
    if (FILL && off0[pi + 1] + off1[pi + 1] == off0[pi] + off1[pi]) return;
    const ScProbe &P = probes[pi];
    const double rp = A.rp, rp2 = rp * rp;
    const DV pijk = dp3(P.p), uijk = dp3(P.alt);
    const double hijk = P.height;
    const uint32_t mol = A.mol[P.a[0]];
    const double density = __ddiv_rn(A.density + A.density + A.density, 3.0);
    DV vp[3], vec[3];
    for (int k = 0; k < 3; k++) vp[k] = vnorm(vsub(catom(A, P.a[k]), pijk));
    vec[0] = vnorm(vcross(vp[0], vp[1]));
    vec[1] = vnorm(vcross(vp[1], vp[2]));
    vec[2] = vnorm(vcross(vp[2], vp[0]));
    double dm = -1.0;
    int mm = 0;
    for (int k = 0; k < 3; k++) { const double dt = vdot(uijk, vp[k]); if (dt > dm) { dm = dt; mm = k; } }
    const DV south = vmul(uijk, -1.0);
    const DV axis = vnorm(vcross(vp[mm], south));
    // burial is decided by the probe centre (pcen = pijk): one decision for all of this probe's dots
    const bool buried = FILL && sc_buried(A, bur_off, bur_idx, P.i, pijk);
    ScDot *out = FILL ? (mol == 0u ? out0 + off0[pi] : out1 + off1[pi]) : nullptr;
    const uint32_t fr = ENS ? P.i / E.n_per : 0u;
    if (FILL && ENS) out += E.adj[mol][fr];
    uint32_t nd = 0, nl;
    double cs;
    if (sc_arc(v3(0.0, 0.0, 0.0), rp, axis, density, vp[mm], south, nl, cs, [](uint32_t, DV) {}))  // (the latitudes' count and cs first)
        nd = sc_wave_lats<FILL>(rp, axis, density, vp[mm], south, nl, out, [&](DV lat, ScDot *dst, uint32_t &n) {
            const double dt = vdot(lat, south);
            const DV cen = vmul(south, dt);
            double rad = rp2 - dt * dt;
            if (rad <= 0.0) return true;
            rad = __dsqrt_rn(rad);
            uint32_t np;
            double ps;
            if (!sc_circle(cen, rad, south, density, np, ps, [](uint32_t, DV) {})) return false;
            const double area = ps * cs;
            sc_circle(cen, rad, south, density, np, ps, [&](uint32_t, DV p0) {
                if (vdot(p0, vec[0]) >= 0.0 || vdot(p0, vec[1]) >= 0.0 || vdot(p0, vec[2]) >= 0.0) return;
                const DV p = vadd(p0, pijk);
                if (hijk < rp) {  // the nears: other low probes within 2 rp of the centre; a point within rp of one is dropped
                    const bool coll = cells_visit<ENS>(low, p, 1, [&](uint32_t q) {
                        if (q == pi) return false;
                        const DV c = dp3(probes[q].p);
                        return vd2(pijk, c) <= 4.0 * rp2 && vd2(p, c) < rp2;
                    }, fr);
                    if (coll) return;
                }
                int mc = 0;
                double dmin = 2.0 * rp;
                for (int kk = 0; kk < 3; kk++) {
                    const double4 c = A.c[P.a[kk]];
                    const double d = __dsqrt_rn(vd2(p, v3(c.x, c.y, c.z))) - c.w;
                    if (d < dmin) { dmin = d; mc = kk; }
                }
                if (dst) sc_put(dst + n, p, vdiv(vsub(pijk, p), rp), area, P.a[mc], kScDotConcave | (buried ? kScDotBuried : 0u));
                n++;
            });
            return true;
        });
    if (!FILL && lane == 0u) { cnt0[pi] = mol == 0u ? nd : 0u; cnt1[pi] = mol == 1u ? nd : 0u; }
}

// ---- (e) trim: a buried dot with no open (non-buried) dot of its surface within d^2 <= band^2 is trimmed (cells: the open dots, edge >= band)
template <bool ENS = false>
__global__ __launch_bounds__(256) void k_sc_trim(ScDot *dots, uint32_t n, ScCells open, double band2, ScEns E) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    ScDot &d = dots[k];
    if (!(d.flags & kScDotBuried)) return;
    const uint32_t fr = ENS ? d.atom / E.n_per : 0u;
    if (ENS && E.other[fr + 1u] == E.other[fr]) return;  // "No molecular dots generated" for this frame
    const DV p = dp3(d.p);
    const bool hit = cells_visit<ENS>(open, p, 1, [&](uint32_t q) { return vd2(dp3(dots[q].p), p) <= band2; }, fr);
    if (!hit) d.flags |= kScDotTrimmed;
}

// ---- (f) nearest trimmed dot of the other surface: shells of cells around the dot's cell until the next shell's lower bound exceeds the
// best d^2 (exact at any distance); the lower index wins a tie.  Writes nn_dist and score into the trimmed dots of `mine`.
template <bool ENS = false>
__global__ __launch_bounds__(256) void k_sc_nn(ScDot *mine, uint32_t n, const ScDot *theirs, ScCells g, double w, ScEns E) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    ScDot &d = mine[k];
    if (!(d.flags & kScDotTrimmed)) return;
    const DV p = dp3(d.p);
    int cx, cy, cz;
    const uint32_t slab = cell_of<ENS>(g, p, cx, cy, cz, ENS ? d.atom / E.n_per : 0u);
    if (ENS && g.start[slab + (uint32_t)g.nx * (uint32_t)g.ny * (uint32_t)g.nz] == g.start[slab]) return;  // the frame's other surface has no trimmed dot
    const double edge = 1.0 / g.inv;
    const int smax = max(max(g.nx, g.ny), g.nz);
    double best = INFINITY;
    uint32_t bi = ~0u;
    for (int s = 0; s <= smax; s++) {
        if (s >= 1) {  // every cell at Chebyshev distance >= s is at least (s - 1) edges away
            const double lb = (double)(s - 1) * edge * (1.0 - 1e-12);
            if (lb * lb > best) break;
        }
        for (int z = cz - s; z <= cz + s; z++) {
            if (z < 0 || z >= g.nz) continue;
            for (int y = cy - s; y <= cy + s; y++) {
                if (y < 0 || y >= g.ny) continue;
                const bool face = z == cz - s || z == cz + s || y == cy - s || y == cy + s;
                for (int x = cx - s; x <= cx + s; x += (face || s == 0) ? 1 : 2 * s) {
                    if (x < 0 || x >= g.nx) continue;
                    const uint32_t c = slab + ((uint32_t)z * (uint32_t)g.ny + (uint32_t)y) * (uint32_t)g.nx + (uint32_t)x;
                    for (uint32_t e = g.start[c]; e < g.start[c + 1]; e++) {
                        const uint32_t q = g.item[e];
                        const ScDot &o = theirs[q];
                        const double dx = o.p[0] - d.p[0], dy = o.p[1] - d.p[1], dz = o.p[2] - d.p[2];
                        const double d2 = dx * dx + dy * dy + dz * dz;
                        if (d2 < best || (d2 == best && q < bi)) { best = d2; bi = q; }
                    }
                }
            }
        }
    }
    if (bi == ~0u) return;
    const ScDot &o = theirs[bi];
    double r = d.n[0] * o.n[0] + d.n[1] * o.n[1] + d.n[2] * o.n[2];
    r *= exp(-best * w);
    r = r < -0.999 ? -0.999 : (r > 0.999 ? 0.999 : r);
    d.nn_dist = __dsqrt_rn(best);
    d.score = -r;
}

// ---- host driver (runs in this translation unit: it launches the kernels above)
void set_error(const char *fmt, ...);  // (host_common.h)
#define SC_TRY(expr)                                                                                                  \
    do {                                                                                                              \
        const hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) { set_error("HIP error %d (%s) in SC: %s", (int)e_, hipGetErrorString(e_), #expr); return e_ == hipErrorOutOfMemory ? ARP_ERR_OOM : ARP_ERR_HIP; } \
    } while (0)
namespace {
struct ScArena {  // device blocks of one call, freed at its end
    std::vector<void *> blocks;
    hipStream_t st;
    bool failed = false;
    template <class T>
    T *get(size_t n, bool zero = false) {
        void *p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)) != hipSuccess) { failed = true; return nullptr; }
        blocks.push_back(p);
        if (zero && hipMemsetAsync(p, 0, std::max<size_t>(n, 1) * sizeof(T), st) != hipSuccess) failed = true;
        return (T *)p;
    }
    ~ScArena() { (void)hipStreamSynchronize(st); for (void *p : blocks) (void)hipFree(p); }
};
arp_status sc_fail(arp_status st) {  // a failed device allocation or copy of the arena (its HIP status is not kept)
    set_error(st == ARP_ERR_OOM ? "SC: a device allocation failed (out of device memory)" : "SC: a device copy or synchronisation failed");
    return st;
}
inline uint32_t sc_blocks(size_t n) { return (uint32_t)((n + 255u) / 256u); }
// exclusive scan of in[0, n) into out[0, n); with in[n - 1] = 0 the last entry is the total
void sc_scan(ScArena &A, uint32_t *in, uint32_t *out, uint32_t n) {
    const uint32_t nb = (n + kScScanBlock - 1u) / kScScanBlock;
    uint32_t *bsum = A.get<uint32_t>(nb);
    if (A.failed) return;
    hipLaunchKernelGGL(k_sc_scan_block, dim3(nb), dim3(256), 0, A.st, (const uint32_t *)in, out, bsum, n);
    if (nb > 1) {
        uint32_t *boff = A.get<uint32_t>(nb);
        if (A.failed) return;
        sc_scan(A, bsum, boff, nb);
        hipLaunchKernelGGL(k_sc_scan_add, dim3(sc_blocks(n)), dim3(256), 0, A.st, out, (const uint32_t *)boff, n);
    }
}
uint32_t sc_read(ScArena &A, const uint32_t *p) {
    uint32_t v = 0;
    if (hipMemcpyAsync(&v, p, 4, hipMemcpyDeviceToHost, A.st) != hipSuccess || hipStreamSynchronize(A.st) != hipSuccess) A.failed = true;
    return v;
}
struct ScBox { double lo[3], hi[3]; };
// cell list over the points of `base` (stride in doubles) that `mode` includes; edge >= edge_req and >= the longest axis / 128, so at most
// 129 cells per axis ((int)(ext / edge) + 1 with ext / edge up to 128; cell_of clamps to n - 1)
ScCells sc_cells(ScArena &A, const ScBox &box, const double *base, uint32_t stride, uint32_t n, uint32_t mode, double rp, double edge_req,
                 Profiler *prof, const char *name) {
    double ext = 0.0;
    for (int a = 0; a < 3; a++) ext = std::max(ext, box.hi[a] - box.lo[a]);
    const double edge = std::max(edge_req, ext / 128.0);
    ScCells g{};
    g.ox = box.lo[0]; g.oy = box.lo[1]; g.oz = box.lo[2]; g.inv = 1.0 / edge;
    g.nx = (int)((box.hi[0] - box.lo[0]) * g.inv) + 1; g.ny = (int)((box.hi[1] - box.lo[1]) * g.inv) + 1; g.nz = (int)((box.hi[2] - box.lo[2]) * g.inv) + 1;
    const uint32_t nc = (uint32_t)g.nx * (uint32_t)g.ny * (uint32_t)g.nz;
    uint32_t *count = A.get<uint32_t>(nc + 1, true), *start = A.get<uint32_t>(nc + 1), *rank = A.get<uint32_t>(n), *item = A.get<uint32_t>(n);
    if (A.failed) return g;
    if (prof) prof->begin(name, A.st);
    if (n) hipLaunchKernelGGL(k_sc_cell_count, dim3(sc_blocks(n)), dim3(256), 0, A.st, base, stride, n, mode, rp, g, count, rank);
    sc_scan(A, count, start, nc + 1);
    g.start = start; g.item = item;
    if (n) hipLaunchKernelGGL(k_sc_cell_fill, dim3(sc_blocks(n)), dim3(256), 0, A.st, base, stride, n, rp, g, (const uint32_t *)rank, item);
    if (prof) prof->end(A.st);
    return g;
}
}  // namespace

arp_status launch_sc(const ScJob &J, hipStream_t st, Profiler *prof, ScRunOut *out) {
    ScArena A;
    A.st = st;
    const uint32_t n = J.n;
    // host staging: {x, y, z, r}, molecule, serial; the box of every position a stage can produce (dots within r, probes within r + rp)
    std::vector<double> c4(4ull * n);
    std::vector<long long> ser(J.serial, J.serial + n);
    double r_max = 0.0;
    ScBox box{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
    for (uint32_t i = 0; i < n; i++) {
        const double p[3] = {J.x[i], J.y[i], J.z[i]};
        for (int a = 0; a < 3; a++) { c4[4ull * i + a] = p[a]; box.lo[a] = std::min(box.lo[a], p[a]); box.hi[a] = std::max(box.hi[a], p[a]); }
        c4[4ull * i + 3] = J.r[i];
        r_max = std::max(r_max, J.r[i]);
    }
    const double pad = r_max + 2.0 * J.rp + 1.0;
    for (int a = 0; a < 3; a++) { box.lo[a] -= pad; box.hi[a] += pad; }
    double4 *d_c = A.get<double4>(n);
    uint32_t *d_mol = A.get<uint32_t>(n);
    long long *d_ser = A.get<long long>(n);
    if (A.failed) return sc_fail(ARP_ERR_OOM);
    SC_TRY(hipMemcpyAsync(d_c, c4.data(), 32ull * n, hipMemcpyHostToDevice, st));
    SC_TRY(hipMemcpyAsync(d_mol, J.mol, 4ull * n, hipMemcpyHostToDevice, st));
    SC_TRY(hipMemcpyAsync(d_ser, ser.data(), 8ull * n, hipMemcpyHostToDevice, st));
    ScAtoms SA{n, d_c, d_mol, d_ser, J.rp, J.density, J.sep, r_max};

    // (a) atoms.  The cell edge covers the 8 A map and every burial candidate (r_i + r_b + 2 rp + margin)
    const double edge_a = std::max(J.sep, 2.0 * (r_max + J.rp) + kScBurMargin) * (1.0 + 1e-9);
    const ScCells ga = sc_cells(A, box, (const double *)d_c, 4, n, kScPtAll, J.rp, edge_a, prof, "sc_cells_atoms");
    uint32_t *nb_cnt = A.get<uint32_t>(n + 1, true), *bur_cnt = A.get<uint32_t>(n + 1, true), *att = A.get<uint32_t>(n), *acc = A.get<uint32_t>(n);
    uint32_t *nb_off = A.get<uint32_t>(n + 1), *bur_off = A.get<uint32_t>(n + 1);
    unsigned long long *err = A.get<unsigned long long>(2);
    if (A.failed) return sc_fail(ARP_ERR_OOM);
    SC_TRY(hipMemsetAsync(err, 0xFF, 8, st));
    SC_TRY(hipMemsetAsync(err + 1, 0, 8, st));
    if (prof) prof->begin("sc_atoms_count", st);
    hipLaunchKernelGGL(k_sc_atoms<false>, dim3(sc_blocks(n)), dim3(256), 0, st, SA, ga, nb_cnt, bur_cnt, att, acc, err, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, ScEns{});
    if (prof) prof->end(st);
    sc_scan(A, nb_cnt, nb_off, n + 1);
    sc_scan(A, bur_cnt, bur_off, n + 1);
    unsigned long long herr[2];
    SC_TRY(hipMemcpyAsync(herr, err, 16, hipMemcpyDeviceToHost, st));
    const uint32_t n_nb = sc_read(A, nb_off + n), n_bur = sc_read(A, bur_off + n);
    if (A.failed) return sc_fail(ARP_ERR_HIP);
    if (herr[0] != ~0ull) { out->err = kScErrCoincident; out->err_i = (uint32_t)(herr[0] >> 32); out->err_j = (uint32_t)herr[0]; return ARP_OK; }
    uint32_t *nb_idx = A.get<uint32_t>(n_nb), *nb_own = A.get<uint32_t>(n_nb), *bur_idx = A.get<uint32_t>(n_bur);
    double *nb_d2 = A.get<double>(n_nb);
    if (A.failed) return sc_fail(ARP_ERR_OOM);
    if (prof) prof->begin("sc_atoms_fill", st);
    hipLaunchKernelGGL(k_sc_atoms<true>, dim3(sc_blocks(n)), dim3(256), 0, st, SA, ga, nullptr, nullptr, nullptr, nullptr, nullptr, (const uint32_t *)nb_off,
                       nb_idx, nb_d2, nb_own, (const uint32_t *)bur_off, bur_idx, ScEns{});
    if (prof) prof->end(st);

    // (b) pairs: probes, toroidal dots, accessible flags
    ScPairOut po{};
    po.p_cnt = A.get<uint32_t>(n_nb + 1, true); po.t_cnt[0] = A.get<uint32_t>(n_nb + 1, true); po.t_cnt[1] = A.get<uint32_t>(n_nb + 1, true);
    uint32_t *p_off = A.get<uint32_t>(n_nb + 1), *t_off0 = A.get<uint32_t>(n_nb + 1), *t_off1 = A.get<uint32_t>(n_nb + 1);
    po.acc = acc; po.err = err + 1;
    if (A.failed) return sc_fail(ARP_ERR_OOM);
    if (prof) prof->begin("sc_pairs_count", st);
    if (n_nb) hipLaunchKernelGGL(k_sc_pairs<false>, dim3(sc_blocks(n_nb)), dim3(256), 0, st, SA, n_nb, (const uint32_t *)nb_off, (const uint32_t *)nb_idx,
                                 (const double *)nb_d2, (const uint32_t *)nb_own, (const uint32_t *)att, (const uint32_t *)bur_off, (const uint32_t *)bur_idx, po, ScEns{});
    if (prof) prof->end(st);
    sc_scan(A, po.p_cnt, p_off, n_nb + 1);
    sc_scan(A, po.t_cnt[0], t_off0, n_nb + 1);
    sc_scan(A, po.t_cnt[1], t_off1, n_nb + 1);
    SC_TRY(hipMemcpyAsync(herr, err, 16, hipMemcpyDeviceToHost, st));
    const uint32_t n_probe = sc_read(A, p_off + n_nb), n_t0 = sc_read(A, t_off0 + n_nb), n_t1 = sc_read(A, t_off1 + n_nb);
    if (A.failed) return sc_fail(ARP_ERR_HIP);
    if (herr[1] & kScErrSubdiv) { out->err = kScErrSubdiv; return ARP_OK; }
    ScProbe *probes = A.get<ScProbe>(n_probe);
    ScDot *tor0 = A.get<ScDot>(n_t0), *tor1 = A.get<ScDot>(n_t1);
    if (A.failed) return sc_fail(ARP_ERR_OOM);
    po.p_off = p_off; po.t_off[0] = t_off0; po.t_off[1] = t_off1; po.probes = probes; po.tor[0] = tor0; po.tor[1] = tor1;
    if (prof) prof->begin("sc_pairs_fill", st);
    if (n_nb) hipLaunchKernelGGL(k_sc_pairs<true>, dim3(sc_blocks(n_nb)), dim3(256), 0, st, SA, n_nb, (const uint32_t *)nb_off, (const uint32_t *)nb_idx,
                                 (const double *)nb_d2, (const uint32_t *)nb_own, (const uint32_t *)att, (const uint32_t *)bur_off, (const uint32_t *)bur_idx, po, ScEns{});
    if (prof) prof->end(st);

    // (c) contact and (d) concave: counts first, so that each surface is laid out [toroidal | contact | concave]
    uint32_t *cc[2] = {A.get<uint32_t>(n + 1, true), A.get<uint32_t>(n + 1, true)}, *co[2] = {A.get<uint32_t>(n + 1), A.get<uint32_t>(n + 1)};
    uint32_t *kc[2] = {A.get<uint32_t>(n_probe + 1, true), A.get<uint32_t>(n_probe + 1, true)};
    uint32_t *ko[2] = {A.get<uint32_t>(n_probe + 1), A.get<uint32_t>(n_probe + 1)};
    if (A.failed) return sc_fail(ARP_ERR_OOM);
    if (prof) prof->begin("sc_contact_count", st);
    hipLaunchKernelGGL(k_sc_contact<false>, dim3((n + kScWaves - 1) / kScWaves), dim3(kScWaves * 64), 0, st, SA, (const uint32_t *)nb_off, (const uint32_t *)nb_idx, (const uint32_t *)att,
                       (const uint32_t *)acc, (const uint32_t *)bur_off, (const uint32_t *)bur_idx, cc[0], cc[1], nullptr, nullptr, nullptr, nullptr, ScEns{});
    if (prof) prof->end(st);
    const ScCells gl = sc_cells(A, box, (const double *)probes, sizeof(ScProbe) / 8, n_probe, kScPtLowProbe, J.rp, 2.0 * J.rp, prof, "sc_cells_low_probes");
    if (A.failed) return sc_fail(ARP_ERR_OOM);
    if (prof) prof->begin("sc_concave_count", st);
    if (n_probe) hipLaunchKernelGGL(k_sc_concave<false>, dim3((n_probe + kScWaves - 1) / kScWaves), dim3(kScWaves * 64), 0, st, SA, (const ScProbe *)probes, n_probe, gl,
                                    (const uint32_t *)bur_off, (const uint32_t *)bur_idx, kc[0], kc[1], nullptr, nullptr, nullptr, nullptr, ScEns{});
    if (prof) prof->end(st);
    uint32_t nT[2] = {n_t0, n_t1}, nC[2], nK[2];
    for (int m = 0; m < 2; m++) { sc_scan(A, cc[m], co[m], n + 1); sc_scan(A, kc[m], ko[m], n_probe + 1); }
    for (int m = 0; m < 2; m++) { nC[m] = sc_read(A, co[m] + n); nK[m] = sc_read(A, ko[m] + n_probe); }
    if (A.failed) return sc_fail(ARP_ERR_HIP);
    ScDot *surf[2];
    for (int m = 0; m < 2; m++) surf[m] = A.get<ScDot>((size_t)nT[m] + nC[m] + nK[m]);
    if (A.failed) return sc_fail(ARP_ERR_OOM);
    SC_TRY(hipMemcpyAsync(surf[0], tor0, sizeof(ScDot) * nT[0], hipMemcpyDeviceToDevice, st));
    SC_TRY(hipMemcpyAsync(surf[1], tor1, sizeof(ScDot) * nT[1], hipMemcpyDeviceToDevice, st));
    if (prof) prof->begin("sc_contact_fill", st);
    hipLaunchKernelGGL(k_sc_contact<true>, dim3((n + kScWaves - 1) / kScWaves), dim3(kScWaves * 64), 0, st, SA, (const uint32_t *)nb_off, (const uint32_t *)nb_idx, (const uint32_t *)att,
                       (const uint32_t *)acc, (const uint32_t *)bur_off, (const uint32_t *)bur_idx, nullptr, nullptr, (const uint32_t *)co[0],
                       (const uint32_t *)co[1], surf[0] + nT[0], surf[1] + nT[1], ScEns{});
    if (prof) prof->end(st);
    if (prof) prof->begin("sc_concave_fill", st);
    if (n_probe) hipLaunchKernelGGL(k_sc_concave<true>, dim3((n_probe + kScWaves - 1) / kScWaves), dim3(kScWaves * 64), 0, st, SA, (const ScProbe *)probes, n_probe, gl,
                                    (const uint32_t *)bur_off, (const uint32_t *)bur_idx, nullptr, nullptr, (const uint32_t *)ko[0], (const uint32_t *)ko[1],
                                    surf[0] + nT[0] + nC[0], surf[1] + nT[1] + nC[1], ScEns{});
    if (prof) prof->end(st);
    uint32_t nS[2];
    for (int m = 0; m < 2; m++) nS[m] = nT[m] + nC[m] + nK[m];

    // (e) trim and (f) nearest neighbour, only when both surfaces have dots ("No molecular dots generated" otherwise)
    if (nS[0] && nS[1]) {
        uint32_t n_trim[2];
        ScCells gt[2];
        for (int m = 0; m < 2; m++) {
            const ScCells go = sc_cells(A, box, (const double *)surf[m], sizeof(ScDot) / 8, nS[m], kScPtDotOpen, J.rp, J.band * (1.0 + 1e-9) + 1e-9, prof,
                                        "sc_cells_open_dots");
            if (A.failed) return sc_fail(ARP_ERR_OOM);
            if (prof) prof->begin("sc_trim", st);
            hipLaunchKernelGGL(k_sc_trim<false>, dim3(sc_blocks(nS[m])), dim3(256), 0, st, surf[m], nS[m], go, J.band * J.band, ScEns{});
            if (prof) prof->end(st);
            gt[m] = sc_cells(A, box, (const double *)surf[m], sizeof(ScDot) / 8, nS[m], kScPtDotTrimmed, J.rp, 1.5, prof, "sc_cells_trimmed_dots");
            if (A.failed) return sc_fail(ARP_ERR_OOM);
            n_trim[m] = sc_read(A, gt[m].start + (size_t)gt[m].nx * gt[m].ny * gt[m].nz);
        }
        if (A.failed) return sc_fail(ARP_ERR_HIP);
        if (n_trim[0] && n_trim[1])
            for (int m = 0; m < 2; m++) {
                if (prof) prof->begin("sc_nn", st);
                hipLaunchKernelGGL(k_sc_nn<false>, dim3(sc_blocks(nS[m])), dim3(256), 0, st, surf[m], nS[m], (const ScDot *)surf[1 - m], gt[1 - m], J.w, ScEns{});
                if (prof) prof->end(st);
            }
    }
    for (int m = 0; m < 2; m++) {
        out->dots[m].resize(nS[m]);
        SC_TRY(hipMemcpyAsync(out->dots[m].data(), surf[m], sizeof(ScDot) * nS[m], hipMemcpyDeviceToHost, st));
    }
    out->att.resize(n);
    SC_TRY(hipMemcpyAsync(out->att.data(), att, 4ull * n, hipMemcpyDeviceToHost, st));
    SC_TRY(hipGetLastError());
    SC_TRY(hipStreamSynchronize(st));
    out->n_toroidal = (uint64_t)nT[0] + nT[1]; out->n_convex = (uint64_t)nC[0] + nC[1]; out->n_concave = (uint64_t)nK[0] + nK[1]; out->n_probes = n_probe;
    return ARP_OK;
}
#undef SC_TRY
