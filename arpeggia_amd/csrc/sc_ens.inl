// Shape complementarity across the frames of an ensemble.  Included by kernels.hip after sc.inl, inside namespace arp.
//
// A pass takes B whole frames of one topology (n atoms each) through the stages of launch_sc once.  Items are indexed frame-major: atom
// f n + i, then neighbour entries, probes and dots in that order, so the count -> scan -> fill scheme of sc.inl leaves every frame's outputs
// contiguous and in the reference's sequential order.  The kernels are the ENS instantiations of sc.inl's (same per-item code, so every dot
// keeps its bits); what differs is only
//   cells      one slab of nx ny nz cells per frame around that frame's own origin (ScCells::org): no relation crosses a frame, and a frame
//              that drifts away does not coarsen the cells.  The frame of a point is its owner atom / n.
//   state      the coincident-pair word and the subdivision flag are one per frame (ScEns::coinc, ::subdiv).  A frame that fails has its
//              counts zeroed behind the count pass that found it (k_sce_after_atoms, k_sce_after_pairs) and its atoms marked Far, so it
//              produces nothing further and every other frame of the pass is untouched.
//   layout     a surface of a frame is [toroidal | contact | concave], as in launch_sc: k_sce_layout turns the scanned offsets at the frame
//              boundaries into per-frame segment starts and into the shift (ScEns::adj) each kind's fill adds to its offset.
// Then, on the device: k_sc_dot_stats (the statistics of every (frame, surface) segment) and k_sce_member_* (per-atom interface membership).
// Only the per-frame records, the statistics and the per-atom accumulators are copied back.
//
// k_sc_dot_stats, the summation order (arp_sc_dot_stats_host restates it): the terms of a segment of `len` dots are taken by position.
// Lane t of 256 starts from +0.0 and adds the terms of the trimmed dots at positions t, t + 256, t + 512, ... in increasing position (a dot
// that is not trimmed adds nothing); the 256 partial sums p[] are then folded p[t] += p[t + h] for h = 128, 64, ..., 1 and p[0] is the sum.
// The order depends on the segment alone, not on how many segments the call has or where the segment lies.  The terms are area, nn_dist and
// -score; d_mean = sum / k, s_mean = -(sum / k) as sc.cpp sc_stats forms them.  The medians are exact: element k / 2 (ascending) of the
// trimmed dots' values under the total order of the key below, found by an MSB-first radix select, 8 bits a round, on an LDS histogram.

// ---- cell lists with one slab per frame
__device__ inline uint32_t sce_pt_frame(uint32_t mode, const double *q, uint32_t k, uint32_t n_per) {
    if (mode == kScPtAll) return k / n_per;
    if (mode == kScPtLowProbe) return ((const ScProbe *)q)->i / n_per;
    return ((const ScDot *)q)->atom / n_per;
}
__global__ __launch_bounds__(256) void k_sce_cell_count(const double *base, uint32_t stride, uint32_t n, uint32_t mode, double rp, ScCells g, uint32_t n_per,
                                                        uint32_t *count, uint32_t *rank) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    DV p;
    if (!sc_pt(mode, base, stride, k, rp, p)) { rank[k] = ~0u; return; }
    int cx, cy, cz;
    const uint32_t slab = cell_of<true>(g, p, cx, cy, cz, sce_pt_frame(mode, base + (size_t)k * stride, k, n_per));
    const uint32_t c = slab + ((uint32_t)cz * (uint32_t)g.ny + (uint32_t)cy) * (uint32_t)g.nx + (uint32_t)cx;
    rank[k] = atomicAdd(&count[c], 1u);
}
__global__ __launch_bounds__(256) void k_sce_cell_fill(const double *base, uint32_t stride, uint32_t n, uint32_t mode, ScCells g, uint32_t n_per,
                                                       const uint32_t *rank, uint32_t *item) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n || rank[k] == ~0u) return;
    const double *q = base + (size_t)k * stride;
    int cx, cy, cz;
    const uint32_t slab = cell_of<true>(g, dp3(q), cx, cy, cz, sce_pt_frame(mode, q, k, n_per));
    const uint32_t c = slab + ((uint32_t)cz * (uint32_t)g.ny + (uint32_t)cy) * (uint32_t)g.nx + (uint32_t)cx;
    item[g.start[c] + rank[k]] = k;
}

// ---- per-frame state
// behind the atom count pass: the Buried atoms of every frame; a frame with a coincident pair loses its lists and its attention
__global__ __launch_bounds__(256) void k_sce_after_atoms(uint32_t n_all, uint32_t n_per, const uint32_t *mol, const unsigned long long *coinc, uint32_t *nb_cnt,
                                                         uint32_t *bur_cnt, uint32_t *att, ScEnsFrame *fr) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_all) return;
    const uint32_t f = g / n_per;
    if (coinc[f] != ~0ull) { nb_cnt[g] = 0u; bur_cnt[g] = 0u; att[g] = 0u; return; }
    if (att[g]) atomicAdd(&fr[f].att[mol[g]], 1u);
}
// behind the pair count pass: a frame whose sampling failed loses its probes and toroidal dots, and its atoms their attention
__global__ __launch_bounds__(256) void k_sce_after_pairs(uint32_t n_all, uint32_t n_per, uint32_t n_items, const uint32_t *nb_own, const uint32_t *subdiv,
                                                         uint32_t *p_cnt, uint32_t *t_cnt0, uint32_t *t_cnt1, uint32_t *att) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k < n_items && subdiv[nb_own[k] / n_per]) { p_cnt[k] = 0u; t_cnt0[k] = 0u; t_cnt1[k] = 0u; }
    if (k < n_all && subdiv[k / n_per]) att[k] = 0u;
}
// the frame boundaries of every scanned array -> segment starts, fill shifts, per-frame counts.  Thread f of B + 1 (the last closes the segments).
struct ScEnsLayout {
    const uint32_t *nb_off, *p_off, *t_off[2], *c_off[2], *k_off[2];
    const unsigned long long *coinc;
    const uint32_t *subdiv;
    uint32_t *seg[2];                        // [B + 1] segment starts of each surface
    uint32_t *adj_t[2], *adj_c[2], *adj_k[2];  // [B]
    unsigned long long *stat_start;          // [2 B + 1] segment s = m B + f of the two surfaces laid end to end (k_sc_dot_stats)
    uint32_t *stat_other;                    // [2 B]
    ScEnsFrame *fr;
};
__global__ __launch_bounds__(256) void k_sce_layout(uint32_t B, uint32_t n_per, ScEnsLayout L) {
    const uint32_t f = blockIdx.x * 256u + threadIdx.x;
    if (f > B) return;
    const uint32_t a0 = f * n_per, e0 = L.nb_off[a0], p0 = L.p_off[e0];
    const uint32_t tot0 = L.t_off[0][L.nb_off[B * n_per]] + L.c_off[0][B * n_per] + L.k_off[0][L.p_off[L.nb_off[B * n_per]]];
    uint32_t nS[2] = {0u, 0u};
    for (int m = 0; m < 2; m++) {
        const uint32_t T0 = L.t_off[m][e0], C0 = L.c_off[m][a0], K0 = L.k_off[m][p0], seg = T0 + C0 + K0;
        L.seg[m][f] = seg;
        L.stat_start[(uint32_t)m * B + f] = (unsigned long long)(m ? tot0 : 0u) + seg;  // (m = 0, f = B and m = 1, f = 0 write the same value)
        if (f == B) continue;
        const uint32_t a1 = a0 + n_per, e1 = L.nb_off[a1], p1 = L.p_off[e1];
        const uint32_t nT = L.t_off[m][e1] - T0, nC = L.c_off[m][a1] - C0, nK = L.k_off[m][p1] - K0;
        L.adj_t[m][f] = seg - T0; L.adj_c[m][f] = seg + nT - C0; L.adj_k[m][f] = seg + nT + nC - K0;  // (never negative: C0 + K0, T1 + K0, T1 + C1)
        L.stat_other[(uint32_t)m * B + f] = (uint32_t)(1 - m) * B + f;
        ScEnsFrame &R = L.fr[f];
        R.nT[m] = nT; R.nC[m] = nC; R.nK[m] = nK;
        nS[m] = nT + nC + nK;
        if (m == 0) R.n_probes = p1 - p0;
    }
    if (f == B) return;
    ScEnsFrame &R = L.fr[f];
    const unsigned long long w = L.coinc[f];
    R.ci = (uint32_t)(w >> 32); R.cj = (uint32_t)w; R.subdiv = L.subdiv[f];
    R.ok = (w == ~0ull && !L.subdiv[f] && nS[0] && nS[1]) ? 1u : 0u;
}
// the toroidal dots of every frame into their segments
__global__ __launch_bounds__(256) void k_sce_tor_move(const ScDot *tor, uint32_t n, uint32_t n_per, const uint32_t *adj, ScDot *surf) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= n) return;
    const ScDot d = tor[t];
    surf[t + adj[d.atom / n_per]] = d;
}

// ---- statistics of dot segments.  Strided arrays: the dots of sc.inl (80 B records) or the caller's columns (arp_sc_dot_stats).
struct ScStatIn {
    const char *flags, *area, *nn, *score;
    uint32_t stride_f, stride_d;  // bytes between dots: of flags, of the three doubles
};
__host__ __device__ inline unsigned long long sc_key(double v) {  // order-preserving: a < b as doubles (with -0 < +0) iff key(a) < key(b)
    unsigned long long u;
    __builtin_memcpy(&u, &v, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ inline double sc_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
    double v;
    __builtin_memcpy(&v, &u, 8);
    return v;
}
// grid (n_seg, 2), 256 threads.  Block (s, 0): counts, area, d_mean, d_median; block (s, 1): s_mean, s_median.
__global__ __launch_bounds__(256) void k_sc_dot_stats(ScStatIn in, const unsigned long long *start, const uint32_t *other, arp_sc_surface *out) {
    __shared__ double part[3][256];
    __shared__ uint32_t hist[256], cnt[256], sh_bin, sh_rank;
    const uint32_t s = blockIdx.x, q = blockIdx.y, t = threadIdx.x;
    const unsigned long long b0 = start[s], len = start[s + 1] - b0;
    auto flags_at = [&](unsigned long long k) { return *(const uint32_t *)(in.flags + k * in.stride_f); };
    auto val_at = [&](const char *base, unsigned long long k) { return *(const double *)(base + k * in.stride_d); };
    double a = 0.0, d = 0.0, sc = 0.0;
    uint32_t c = 0;
    for (unsigned long long k = t; k < len; k += 256u) {
        if (!(flags_at(b0 + k) & kScDotTrimmed)) continue;
        c++;
        if (q == 0u) { a += val_at(in.area, b0 + k); d += val_at(in.nn, b0 + k); }
        else sc += -val_at(in.score, b0 + k);
    }
    part[0][t] = a; part[1][t] = d; part[2][t] = sc; cnt[t] = c;
    __syncthreads();
    for (uint32_t h = 128; h >= 1u; h >>= 1) {
        if (t < h) { part[0][t] += part[0][t + h]; part[1][t] += part[1][t + h]; part[2][t] += part[2][t + h]; cnt[t] += cnt[t + h]; }
        __syncthreads();
    }
    const uint32_t k_trim = cnt[0];
    // the other segment: any trimmed dot?
    const unsigned long long o0 = start[other[s]], olen = start[other[s] + 1] - o0;
    int seen = 0;
    for (unsigned long long k = t; k < olen && !seen; k += 256u) seen = (flags_at(o0 + k) & kScDotTrimmed) != 0u;
    const bool live = __syncthreads_or(seen) != 0 && k_trim != 0u;
    arp_sc_surface &S = out[s];
    if (q == 0u && t == 0u) {
        S.n_atoms = 0; S.n_buried_atoms = 0; S.n_far_atoms = 0;
        S.n_all_dots = len; S.n_trimmed_dots = k_trim; S.trimmed_area = part[0][0];
        S.d_mean = live ? __ddiv_rn(part[1][0], (double)k_trim) : 0.0;
        if (!live) S.d_median = 0.0;
    }
    if (q == 1u && t == 0u) {
        S.s_mean = live ? -__ddiv_rn(part[2][0], (double)k_trim) : 0.0;
        if (!live) S.s_median = 0.0;
    }
    if (!live) return;  // (block-uniform)
    // radix select of rank k / 2 among the trimmed dots' keys
    const char *col = q == 0u ? in.nn : in.score;
    unsigned long long prefix = 0;
    if (t == 0u) sh_rank = k_trim / 2u;
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[t] = 0u;
        __syncthreads();
        for (unsigned long long k = t; k < len; k += 256u) {
            if (!(flags_at(b0 + k) & kScDotTrimmed)) continue;
            const unsigned long long key = sc_key(val_at(col, b0 + k));
            if (shift == 56 || (key >> (shift + 8)) == prefix) atomicAdd(&hist[(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (t == 0u) {
            uint32_t r = sh_rank, b = 0;
            while (b < 255u && r >= hist[b]) { r -= hist[b]; b++; }
            sh_bin = b; sh_rank = r;
        }
        __syncthreads();
        prefix = (prefix << 8) | sh_bin;
    }
    if (t == 0u) { if (q == 0u) S.d_median = sc_unkey(prefix); else S.s_median = sc_unkey(prefix); }
}
// the host restatement (arp_sc_dot_stats_host): the same order of every sum, the same key order for the medians
void sc_dot_stats_host(uint64_t n_seg, const uint64_t *start, const uint32_t *flags, const double *area, const double *nn, const double *score,
                       const uint32_t *other, arp_sc_surface *out) {
    std::vector<unsigned long long> keys;
    for (uint64_t s = 0; s < n_seg; s++) {
        const uint64_t b0 = start[s], len = start[s + 1] - b0;
        double part[3][256];
        uint64_t k_trim = 0;
        for (uint32_t t = 0; t < 256u; t++) {
            double a = 0.0, d = 0.0, sc = 0.0;
            for (uint64_t k = t; k < len; k += 256u) {
                if (!(flags[b0 + k] & kScDotTrimmed)) continue;
                k_trim++;
                a += area[b0 + k]; d += nn[b0 + k]; sc += -score[b0 + k];
            }
            part[0][t] = a; part[1][t] = d; part[2][t] = sc;
        }
        for (uint32_t h = 128; h >= 1u; h >>= 1)
            for (uint32_t t = 0; t < h; t++) for (int c = 0; c < 3; c++) part[c][t] += part[c][t + h];
        bool live = false;
        for (uint64_t k = start[other[s]]; k < start[other[s] + 1] && !live; k++) live = (flags[k] & kScDotTrimmed) != 0u;
        live = live && k_trim != 0;
        arp_sc_surface S{};
        S.n_all_dots = len; S.n_trimmed_dots = k_trim; S.trimmed_area = part[0][0];
        if (live) {
            S.d_mean = part[1][0] / (double)k_trim; S.s_mean = -(part[2][0] / (double)k_trim);
            for (int c = 0; c < 2; c++) {
                keys.clear();
                for (uint64_t k = b0; k < b0 + len; k++) if (flags[k] & kScDotTrimmed) keys.push_back(sc_key(c ? score[k] : nn[k]));
                std::nth_element(keys.begin(), keys.begin() + (ptrdiff_t)(k_trim / 2), keys.end());
                (c ? S.s_median : S.d_median) = sc_unkey(keys[k_trim / 2]);
            }
        }
        out[s] = S;
    }
}

// ---- per-atom interface membership: trimmed dots per (frame, atom) of the frames that succeeded, then folded over the frames (integer atomics)
__global__ __launch_bounds__(256) void k_sce_member_count(const ScDot *dots, uint32_t n, uint32_t n_per, const ScEnsFrame *fr, uint32_t *cnt) {
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= n) return;
    const ScDot &d = dots[k];
    if ((d.flags & kScDotTrimmed) && fr[d.atom / n_per].ok) atomicAdd(&cnt[d.atom], 1u);
}
__global__ __launch_bounds__(256) void k_sce_member_fold(const uint32_t *cnt, uint32_t n_all, uint32_t n_per, uint32_t *frames_in, unsigned long long *trimmed) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= n_all || cnt[g] == 0u) return;
    atomicAdd(&frames_in[g % n_per], 1u);
    atomicAdd(&trimmed[g % n_per], (unsigned long long)cnt[g]);
}

// ---- host driver
#define SC_TRY(expr)                                                                                                  \
    do {                                                                                                              \
        const hipError_t e_ = (expr);                                                                                 \
        if (e_ != hipSuccess) { set_error("HIP error %d (%s) in the SC ensemble: %s", (int)e_, hipGetErrorString(e_), #expr); return e_ == hipErrorOutOfMemory ? ARP_ERR_OOM : ARP_ERR_HIP; } \
    } while (0)
namespace {
// One device block per pass, handed out front to back (256-byte steps).  A request past the end sets `over`: the pass is abandoned before it
// writes anything that outlives it, and runs again with fewer frames or a larger block.
struct ScEnsArena {
    char *base = nullptr;
    size_t cap = 0, used = 0;
    hipStream_t st;
    bool over = false, failed = false;
    template <class T>
    T *get(size_t n, bool zero = false) {
        const size_t bytes = (std::max<size_t>(n, 1) * sizeof(T) + 255u) & ~(size_t)255u;
        if (over || used + bytes > cap) { over = true; return nullptr; }
        T *p = (T *)(base + used);
        used += bytes;
        if (zero && hipMemsetAsync(p, 0, bytes, st) != hipSuccess) failed = true;
        return p;
    }
    bool resize(size_t bytes) {
        (void)hipStreamSynchronize(st);
        if (base) (void)hipFree(base);
        base = nullptr; cap = 0;
        if (hipMalloc((void **)&base, bytes) != hipSuccess) { (void)hipGetLastError(); base = nullptr; return false; }
        cap = bytes;
        return true;
    }
    ~ScEnsArena() { (void)hipStreamSynchronize(st); if (base) (void)hipFree(base); }
};
void sce_scan(ScEnsArena &A, uint32_t *in, uint32_t *out, uint32_t n) {
    const uint32_t nb = (n + kScScanBlock - 1u) / kScScanBlock;
    uint32_t *bsum = A.get<uint32_t>(nb);
    if (A.over) return;
    hipLaunchKernelGGL(k_sc_scan_block, dim3(nb), dim3(256), 0, A.st, (const uint32_t *)in, out, bsum, n);
    if (nb > 1) {
        uint32_t *boff = A.get<uint32_t>(nb);
        if (A.over) return;
        sce_scan(A, bsum, boff, nb);
        hipLaunchKernelGGL(k_sc_scan_add, dim3(sc_blocks(n)), dim3(256), 0, A.st, out, (const uint32_t *)boff, n);
    }
}
// the cell list of sc_cells with one slab per frame; dims: the largest frame's box (every frame's points lie inside its own box)
ScCells sce_cells(ScEnsArena &A, const double ext[3], const double *org, uint32_t B, uint32_t n_per, const double *base, uint32_t stride, uint32_t n,
                  uint32_t mode, double rp, double edge_req, Profiler *prof, const char *name) {
    const double edge = std::max(edge_req, std::max(ext[0], std::max(ext[1], ext[2])) / 128.0);
    ScCells g{};
    g.inv = 1.0 / edge; g.org = org;
    g.nx = (int)(ext[0] * g.inv) + 1; g.ny = (int)(ext[1] * g.inv) + 1; g.nz = (int)(ext[2] * g.inv) + 1;
    const size_t nc = (size_t)g.nx * g.ny * g.nz * B;
    if (nc >= 0x7FFFFFFFull) { A.over = true; return g; }
    uint32_t *count = A.get<uint32_t>(nc + 1, true), *start = A.get<uint32_t>(nc + 1), *rank = A.get<uint32_t>(n), *item = A.get<uint32_t>(n);
    if (A.over) return g;
    if (prof) prof->begin(name, A.st);
    if (n) hipLaunchKernelGGL(k_sce_cell_count, dim3(sc_blocks(n)), dim3(256), 0, A.st, base, stride, n, mode, rp, g, n_per, count, rank);
    sce_scan(A, count, start, (uint32_t)nc + 1u);
    g.start = start; g.item = item;
    if (n && !A.over) hipLaunchKernelGGL(k_sce_cell_fill, dim3(sc_blocks(n)), dim3(256), 0, A.st, base, stride, n, mode, g, n_per, (const uint32_t *)rank, item);
    if (prof) prof->end(A.st);
    return g;
}
}  // namespace

// One pass: frames [f0, f0 + B).  *over: the arena was too small (nothing that outlives the pass was written).
static arp_status sce_pass(const ScEnsJob &J, ScEnsArena &A, uint64_t f0, uint32_t B, uint32_t *d_frames_in, unsigned long long *d_trimmed, Profiler *prof,
                           ScEnsOut *out, bool *over) {
    hipStream_t st = A.st;
    A.used = 0; A.over = false;
    *over = true;
    const uint32_t n = J.n, N = B * n;
    // host staging: {x, y, z, r} of every frame, each frame's box (padded as launch_sc pads it) and the common extent of the slabs
    std::vector<double> c4(4ull * N), org(3ull * B);
    std::vector<uint32_t> mol(N);
    std::vector<long long> ser(N);
    struct Drain { hipStream_t st; ~Drain() { (void)hipStreamSynchronize(st); } } drain{st};  // no copy reads the vectors above after any return
    double r_max = 0.0, ext[3] = {0.0, 0.0, 0.0};
    for (uint32_t i = 0; i < n; i++) r_max = std::max(r_max, J.r[i]);
    const double pad = r_max + 2.0 * J.rp + 1.0;
    for (uint32_t f = 0; f < B; f++) {
        double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        const double *x = J.xyz + 3ull * (f0 + f) * n;
        for (uint32_t i = 0; i < n; i++) {
            const size_t g = (size_t)f * n + i;
            for (int a = 0; a < 3; a++) { const double v = x[3ull * i + a]; c4[4 * g + a] = v; lo[a] = std::min(lo[a], v); hi[a] = std::max(hi[a], v); }
            c4[4 * g + 3] = J.r[i]; mol[g] = J.mol[i]; ser[g] = J.serial[i];
        }
        for (int a = 0; a < 3; a++) { org[3ull * f + a] = lo[a] - pad; ext[a] = std::max(ext[a], hi[a] - lo[a] + 2.0 * pad); }
    }
    double4 *d_c = A.get<double4>(N);
    uint32_t *d_mol = A.get<uint32_t>(N);
    long long *d_ser = A.get<long long>(N);
    double *d_org = A.get<double>(3ull * B);
    ScEnsFrame *d_fr = A.get<ScEnsFrame>(B, true);
    unsigned long long *coinc = A.get<unsigned long long>(B);
    uint32_t *subdiv = A.get<uint32_t>(B, true);
    if (A.over) return ARP_OK;
    SC_TRY(hipMemcpyAsync(d_c, c4.data(), 32ull * N, hipMemcpyHostToDevice, st));
    SC_TRY(hipMemcpyAsync(d_mol, mol.data(), 4ull * N, hipMemcpyHostToDevice, st));
    SC_TRY(hipMemcpyAsync(d_ser, ser.data(), 8ull * N, hipMemcpyHostToDevice, st));
    SC_TRY(hipMemcpyAsync(d_org, org.data(), 24ull * B, hipMemcpyHostToDevice, st));
    SC_TRY(hipMemsetAsync(coinc, 0xFF, 8ull * B, st));
    ScAtoms SA{N, d_c, d_mol, d_ser, J.rp, J.density, J.sep, r_max};
    ScEns E{};
    E.n_per = n; E.coinc = coinc; E.subdiv = subdiv;
    uint32_t tot[8];
    auto read = [&](int k, const uint32_t *p) { return hipMemcpyAsync(&tot[k], p, 4, hipMemcpyDeviceToHost, st); };

    // (a) atoms
    const double edge_a = std::max(J.sep, 2.0 * (r_max + J.rp) + kScBurMargin) * (1.0 + 1e-9);
    const ScCells ga = sce_cells(A, ext, d_org, B, n, (const double *)d_c, 4, N, kScPtAll, J.rp, edge_a, prof, "sc_ens_cells_atoms");
    uint32_t *nb_cnt = A.get<uint32_t>(N + 1, true), *bur_cnt = A.get<uint32_t>(N + 1, true), *att = A.get<uint32_t>(N), *acc = A.get<uint32_t>(N);
    uint32_t *nb_off = A.get<uint32_t>(N + 1), *bur_off = A.get<uint32_t>(N + 1);
    if (A.over) return ARP_OK;
    if (prof) prof->begin("sc_ens_atoms_count", st);
    hipLaunchKernelGGL((k_sc_atoms<false, true>), dim3(sc_blocks(N)), dim3(256), 0, st, SA, ga, nb_cnt, bur_cnt, att, acc, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, E);
    hipLaunchKernelGGL(k_sce_after_atoms, dim3(sc_blocks(N)), dim3(256), 0, st, N, n, (const uint32_t *)d_mol, (const unsigned long long *)coinc, nb_cnt, bur_cnt,
                       att, d_fr);
    if (prof) prof->end(st);
    sce_scan(A, nb_cnt, nb_off, N + 1);
    sce_scan(A, bur_cnt, bur_off, N + 1);
    if (A.over) return ARP_OK;
    SC_TRY(read(0, nb_off + N));
    SC_TRY(read(1, bur_off + N));
    SC_TRY(hipStreamSynchronize(st));
    const uint32_t n_nb = tot[0], n_bur = tot[1];
    uint32_t *nb_idx = A.get<uint32_t>(n_nb), *nb_own = A.get<uint32_t>(n_nb), *bur_idx = A.get<uint32_t>(n_bur);
    double *nb_d2 = A.get<double>(n_nb);
    if (A.over) return ARP_OK;
    if (prof) prof->begin("sc_ens_atoms_fill", st);
    hipLaunchKernelGGL((k_sc_atoms<true, true>), dim3(sc_blocks(N)), dim3(256), 0, st, SA, ga, nullptr, nullptr, nullptr, nullptr, nullptr, (const uint32_t *)nb_off,
                       nb_idx, nb_d2, nb_own, (const uint32_t *)bur_off, bur_idx, E);
    if (prof) prof->end(st);

    // (b) pairs
    ScPairOut po{};
    po.p_cnt = A.get<uint32_t>(n_nb + 1, true); po.t_cnt[0] = A.get<uint32_t>(n_nb + 1, true); po.t_cnt[1] = A.get<uint32_t>(n_nb + 1, true);
    uint32_t *p_off = A.get<uint32_t>(n_nb + 1), *t_off0 = A.get<uint32_t>(n_nb + 1), *t_off1 = A.get<uint32_t>(n_nb + 1);
    po.acc = acc; po.err = nullptr;
    if (A.over) return ARP_OK;
    if (prof) prof->begin("sc_ens_pairs_count", st);
    if (n_nb) hipLaunchKernelGGL((k_sc_pairs<false, true>), dim3(sc_blocks(n_nb)), dim3(256), 0, st, SA, n_nb, (const uint32_t *)nb_off, (const uint32_t *)nb_idx,
                                 (const double *)nb_d2, (const uint32_t *)nb_own, (const uint32_t *)att, (const uint32_t *)bur_off, (const uint32_t *)bur_idx, po, E);
    hipLaunchKernelGGL(k_sce_after_pairs, dim3(sc_blocks(std::max(N, n_nb))), dim3(256), 0, st, N, n, n_nb, (const uint32_t *)nb_own, (const uint32_t *)subdiv,
                       po.p_cnt, po.t_cnt[0], po.t_cnt[1], att);
    if (prof) prof->end(st);
    sce_scan(A, po.p_cnt, p_off, n_nb + 1);
    sce_scan(A, po.t_cnt[0], t_off0, n_nb + 1);
    sce_scan(A, po.t_cnt[1], t_off1, n_nb + 1);
    if (A.over) return ARP_OK;
    SC_TRY(read(0, p_off + n_nb));
    SC_TRY(read(1, t_off0 + n_nb));
    SC_TRY(read(2, t_off1 + n_nb));
    SC_TRY(hipStreamSynchronize(st));
    const uint32_t n_probe = tot[0], nT[2] = {tot[1], tot[2]};
    ScProbe *probes = A.get<ScProbe>(n_probe);
    ScDot *tor[2] = {A.get<ScDot>(nT[0]), A.get<ScDot>(nT[1])};
    if (A.over) return ARP_OK;
    po.p_off = p_off; po.t_off[0] = t_off0; po.t_off[1] = t_off1; po.probes = probes; po.tor[0] = tor[0]; po.tor[1] = tor[1];
    if (prof) prof->begin("sc_ens_pairs_fill", st);
    if (n_nb) hipLaunchKernelGGL((k_sc_pairs<true, true>), dim3(sc_blocks(n_nb)), dim3(256), 0, st, SA, n_nb, (const uint32_t *)nb_off, (const uint32_t *)nb_idx,
                                 (const double *)nb_d2, (const uint32_t *)nb_own, (const uint32_t *)att, (const uint32_t *)bur_off, (const uint32_t *)bur_idx, po, E);
    if (prof) prof->end(st);

    // (c) contact and (d) concave counts
    uint32_t *cc[2] = {A.get<uint32_t>(N + 1, true), A.get<uint32_t>(N + 1, true)}, *co[2] = {A.get<uint32_t>(N + 1), A.get<uint32_t>(N + 1)};
    uint32_t *kc[2] = {A.get<uint32_t>(n_probe + 1, true), A.get<uint32_t>(n_probe + 1, true)};
    uint32_t *ko[2] = {A.get<uint32_t>(n_probe + 1), A.get<uint32_t>(n_probe + 1)};
    if (A.over) return ARP_OK;
    const uint32_t wave_blocks = (N + kScWaves - 1) / kScWaves, probe_blocks = (n_probe + kScWaves - 1) / kScWaves;
    if (prof) prof->begin("sc_ens_contact_count", st);
    hipLaunchKernelGGL((k_sc_contact<false, true>), dim3(wave_blocks), dim3(kScWaves * 64), 0, st, SA, (const uint32_t *)nb_off, (const uint32_t *)nb_idx,
                       (const uint32_t *)att, (const uint32_t *)acc, (const uint32_t *)bur_off, (const uint32_t *)bur_idx, cc[0], cc[1], nullptr, nullptr, nullptr,
                       nullptr, E);
    if (prof) prof->end(st);
    const ScCells gl = sce_cells(A, ext, d_org, B, n, (const double *)probes, sizeof(ScProbe) / 8, n_probe, kScPtLowProbe, J.rp, 2.0 * J.rp, prof,
                                 "sc_ens_cells_low_probes");
    if (A.over) return ARP_OK;
    if (prof) prof->begin("sc_ens_concave_count", st);
    if (n_probe) hipLaunchKernelGGL((k_sc_concave<false, true>), dim3(probe_blocks), dim3(kScWaves * 64), 0, st, SA, (const ScProbe *)probes, n_probe, gl,
                                    (const uint32_t *)bur_off, (const uint32_t *)bur_idx, kc[0], kc[1], nullptr, nullptr, nullptr, nullptr, E);
    if (prof) prof->end(st);
    for (int m = 0; m < 2; m++) { sce_scan(A, cc[m], co[m], N + 1); sce_scan(A, kc[m], ko[m], n_probe + 1); }
    // the layout of the two surfaces
    ScEnsLayout L{};
    L.nb_off = nb_off; L.p_off = p_off; L.t_off[0] = t_off0; L.t_off[1] = t_off1; L.coinc = coinc; L.subdiv = subdiv; L.fr = d_fr;
    for (int m = 0; m < 2; m++) {
        L.c_off[m] = co[m]; L.k_off[m] = ko[m];
        L.seg[m] = A.get<uint32_t>(B + 1); L.adj_t[m] = A.get<uint32_t>(B); L.adj_c[m] = A.get<uint32_t>(B); L.adj_k[m] = A.get<uint32_t>(B);
    }
    L.stat_start = A.get<unsigned long long>(2ull * B + 1); L.stat_other = A.get<uint32_t>(2ull * B);
    if (A.over) return ARP_OK;
    hipLaunchKernelGGL(k_sce_layout, dim3(sc_blocks(B + 1)), dim3(256), 0, st, B, n, L);
    for (int m = 0; m < 2; m++) { SC_TRY(read(2 * m, co[m] + N)); SC_TRY(read(2 * m + 1, ko[m] + n_probe)); }
    SC_TRY(hipStreamSynchronize(st));
    size_t nS[2];
    for (int m = 0; m < 2; m++) nS[m] = (size_t)nT[m] + tot[2 * m] + tot[2 * m + 1];
    if (nS[0] + nS[1] >= 0xFFFFFFFFull) return ARP_OK;  // (over: fewer frames)
    ScDot *all = A.get<ScDot>(nS[0] + nS[1]);
    if (A.over) return ARP_OK;
    ScDot *surf[2] = {all, all + nS[0]};
    for (int m = 0; m < 2; m++)
        if (nT[m]) hipLaunchKernelGGL(k_sce_tor_move, dim3(sc_blocks(nT[m])), dim3(256), 0, st, (const ScDot *)tor[m], nT[m], n, (const uint32_t *)L.adj_t[m], surf[m]);
    ScEns Ec = E, Ek = E;
    for (int m = 0; m < 2; m++) { Ec.adj[m] = L.adj_c[m]; Ek.adj[m] = L.adj_k[m]; }
    if (prof) prof->begin("sc_ens_contact_fill", st);
    hipLaunchKernelGGL((k_sc_contact<true, true>), dim3(wave_blocks), dim3(kScWaves * 64), 0, st, SA, (const uint32_t *)nb_off, (const uint32_t *)nb_idx,
                       (const uint32_t *)att, (const uint32_t *)acc, (const uint32_t *)bur_off, (const uint32_t *)bur_idx, nullptr, nullptr, (const uint32_t *)co[0],
                       (const uint32_t *)co[1], surf[0], surf[1], Ec);
    if (prof) prof->end(st);
    if (prof) prof->begin("sc_ens_concave_fill", st);
    if (n_probe) hipLaunchKernelGGL((k_sc_concave<true, true>), dim3(probe_blocks), dim3(kScWaves * 64), 0, st, SA, (const ScProbe *)probes, n_probe, gl,
                                    (const uint32_t *)bur_off, (const uint32_t *)bur_idx, nullptr, nullptr, (const uint32_t *)ko[0], (const uint32_t *)ko[1], surf[0],
                                    surf[1], Ek);
    if (prof) prof->end(st);

    // (e) trim and (f) nearest neighbour; a frame without dots on one surface takes no part (ScEns::other, the empty slab in k_sc_nn)
    ScCells gt[2];
    for (int m = 0; m < 2; m++) {
        const ScCells go = sce_cells(A, ext, d_org, B, n, (const double *)surf[m], sizeof(ScDot) / 8, (uint32_t)nS[m], kScPtDotOpen, J.rp,
                                     J.band * (1.0 + 1e-9) + 1e-9, prof, "sc_ens_cells_open_dots");
        if (A.over) return ARP_OK;
        ScEns Et = E;
        Et.other = L.seg[1 - m];
        if (prof) prof->begin("sc_ens_trim", st);
        if (nS[m]) hipLaunchKernelGGL(k_sc_trim<true>, dim3(sc_blocks(nS[m])), dim3(256), 0, st, surf[m], (uint32_t)nS[m], go, J.band * J.band, Et);
        if (prof) prof->end(st);
        gt[m] = sce_cells(A, ext, d_org, B, n, (const double *)surf[m], sizeof(ScDot) / 8, (uint32_t)nS[m], kScPtDotTrimmed, J.rp, 1.5, prof,
                          "sc_ens_cells_trimmed_dots");
        if (A.over) return ARP_OK;
    }
    for (int m = 0; m < 2; m++) {
        if (prof) prof->begin("sc_ens_nn", st);
        if (nS[m]) hipLaunchKernelGGL(k_sc_nn<true>, dim3(sc_blocks(nS[m])), dim3(256), 0, st, surf[m], (uint32_t)nS[m], (const ScDot *)surf[1 - m], gt[1 - m], J.w, E);
        if (prof) prof->end(st);
    }
    // statistics of the 2 B segments, per-atom membership
    arp_sc_surface *d_stat = A.get<arp_sc_surface>(2ull * B);
    uint32_t *member = A.get<uint32_t>(N, true);
    if (A.over) return ARP_OK;
    ScStatIn in{(const char *)&all->flags, (const char *)&all->area, (const char *)&all->nn_dist, (const char *)&all->score, sizeof(ScDot), sizeof(ScDot)};
    if (prof) prof->begin("sc_ens_stats", st);
    hipLaunchKernelGGL(k_sc_dot_stats, dim3(2u * B, 2), dim3(256), 0, st, in, (const unsigned long long *)L.stat_start, (const uint32_t *)L.stat_other, d_stat);
    if (prof) prof->end(st);
    if (prof) prof->begin("sc_ens_members", st);
    if (nS[0] + nS[1]) hipLaunchKernelGGL(k_sce_member_count, dim3(sc_blocks(nS[0] + nS[1])), dim3(256), 0, st, (const ScDot *)all, (uint32_t)(nS[0] + nS[1]), n,
                                          (const ScEnsFrame *)d_fr, member);
    hipLaunchKernelGGL(k_sce_member_fold, dim3(sc_blocks(N)), dim3(256), 0, st, (const uint32_t *)member, N, n, d_frames_in, d_trimmed);
    if (prof) prof->end(st);
    std::vector<arp_sc_surface> stat(2ull * B);
    SC_TRY(hipMemcpyAsync(stat.data(), d_stat, sizeof(arp_sc_surface) * 2ull * B, hipMemcpyDeviceToHost, st));
    SC_TRY(hipMemcpyAsync(out->frames + f0, d_fr, sizeof(ScEnsFrame) * (size_t)B, hipMemcpyDeviceToHost, st));
    SC_TRY(hipGetLastError());
    SC_TRY(hipStreamSynchronize(st));
    for (uint32_t f = 0; f < B; f++) for (int m = 0; m < 2; m++) out->surf[2 * (f0 + f) + m] = stat[(size_t)m * B + f];
    *over = false;
    return ARP_OK;
}

arp_status launch_sc_ens(const ScEnsJob &J, hipStream_t st, Profiler *prof, ScEnsOut *out) {
    const uint32_t n = J.n;
    ScEnsArena A, acc;  // acc: the per-atom accumulators, which live through every pass
    A.st = st; acc.st = st;
    if (!acc.resize(12ull * n + 512)) { set_error("SC ensemble: a device allocation failed (out of device memory)"); return ARP_ERR_OOM; }
    uint32_t *d_frames_in = acc.get<uint32_t>(n, true);
    unsigned long long *d_trimmed = acc.get<unsigned long long>(n, true);
    if (acc.failed) { set_error("SC ensemble: a device memset failed"); return ARP_ERR_HIP; }
    // the budget of a pass: half of the free device memory, 2 GiB at most (every index of a pass then stays far below 2^32: a dot takes 80 bytes)
    size_t free_b = 0, total_b = 0;
    SC_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t budget = std::min<size_t>(free_b / 2, 2ull << 30);
    const uint32_t b_max = (uint32_t)std::min<uint64_t>(0x7FFFFFFFull / std::max<uint32_t>(n, 1), 1u << 20);
    const bool fixed = J.frames_per_pass > 0;
    uint32_t B = fixed ? std::min<uint32_t>(J.frames_per_pass, b_max) : 1u;
    size_t per_frame = 0;
    uint32_t prof_b = 0;  // the profiler keeps the laps of the first pass with the most frames
    // the first block is a guess (a few hundred dots an atom at the default density never happens: about 30 do); a pass that does not fit says so
    if (!A.resize(std::min<size_t>(std::max<size_t>(budget, 1u << 20), ((size_t)n * 32768u + (1u << 20)) * B))) { set_error("SC ensemble: a device allocation failed (out of device memory)"); return ARP_ERR_OOM; }
    for (uint64_t f0 = 0; f0 < J.n_frames;) {
        const uint32_t b = (uint32_t)std::min<uint64_t>(B, J.n_frames - f0);
        bool over = false;
        Profiler *lap = prof && b > prof_b ? prof : nullptr;
        if (lap) lap->n = 0;
        const arp_status s = sce_pass(J, A, f0, b, d_frames_in, d_trimmed, lap, out, &over);
        if (s != ARP_OK) return s;
        if (A.failed) { set_error("SC ensemble: a device memset failed"); return ARP_ERR_HIP; }
        if (over) {
            if (A.cap < budget) {  // a larger block first
                if (!A.resize(std::min(budget, A.cap * 2))) { set_error("SC ensemble: a device allocation failed (out of device memory)"); return ARP_ERR_OOM; }
            } else if (b > 1 && !fixed) B = b / 2;
            else { set_error("SC ensemble: %u frame(s) of %u atoms do not fit the pass budget of %llu bytes", b, n, (unsigned long long)budget); return ARP_ERR_OOM; }
            continue;
        }
        per_frame = std::max(per_frame, A.used / b + 1);
        if (lap) prof_b = b;
        f0 += b;
        if (!fixed && f0 < J.n_frames) {  // size the next passes from what this one took, with a quarter to spare for frames that swell
            const size_t want = per_frame + per_frame / 4;
            B = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(budget / want, 1), std::min<uint64_t>(b_max, J.n_frames - f0));
            const size_t need = std::min(budget, want * B + (1u << 20));
            if (need > A.cap && !A.resize(need)) { set_error("SC ensemble: a device allocation failed (out of device memory)"); return ARP_ERR_OOM; }
        }
    }
    SC_TRY(hipMemcpyAsync(out->frames_in_interface, d_frames_in, 4ull * n, hipMemcpyDeviceToHost, st));
    SC_TRY(hipMemcpyAsync(out->trimmed_dots, d_trimmed, 8ull * n, hipMemcpyDeviceToHost, st));
    SC_TRY(hipStreamSynchronize(st));
    return ARP_OK;
}

// arp_sc_dot_stats: the statistics kernel on the caller's columns
arp_status launch_sc_dot_stats(uint64_t n_seg, const uint64_t *start, const uint32_t *flags, const double *area, const double *nn, const double *score,
                               const uint32_t *other, arp_sc_surface *out, hipStream_t st) {
    if (n_seg == 0) return ARP_OK;
    const uint64_t n = start[n_seg];
    ScEnsArena A;
    A.st = st;
    if (!A.resize(28ull * n + 8ull * (n_seg + 1) + 4ull * n_seg + sizeof(arp_sc_surface) * n_seg + 8 * 256)) { set_error("arp_sc_dot_stats: a device allocation failed (out of device memory)"); return ARP_ERR_OOM; }
    uint32_t *d_flags = A.get<uint32_t>(n), *d_other = A.get<uint32_t>(n_seg);
    double *d_area = A.get<double>(n), *d_nn = A.get<double>(n), *d_score = A.get<double>(n);
    unsigned long long *d_start = A.get<unsigned long long>(n_seg + 1);
    arp_sc_surface *d_out = A.get<arp_sc_surface>(n_seg);
    if (A.over) { set_error("arp_sc_dot_stats: internal sizing error"); return ARP_ERR_HIP; }
    SC_TRY(hipMemcpyAsync(d_flags, flags, 4ull * n, hipMemcpyHostToDevice, st));
    SC_TRY(hipMemcpyAsync(d_area, area, 8ull * n, hipMemcpyHostToDevice, st));
    SC_TRY(hipMemcpyAsync(d_nn, nn, 8ull * n, hipMemcpyHostToDevice, st));
    SC_TRY(hipMemcpyAsync(d_score, score, 8ull * n, hipMemcpyHostToDevice, st));
    SC_TRY(hipMemcpyAsync(d_other, other, 4ull * n_seg, hipMemcpyHostToDevice, st));
    SC_TRY(hipMemcpyAsync(d_start, start, 8ull * (n_seg + 1), hipMemcpyHostToDevice, st));
    ScStatIn in{(const char *)d_flags, (const char *)d_area, (const char *)d_nn, (const char *)d_score, 4, 8};
    hipLaunchKernelGGL(k_sc_dot_stats, dim3((uint32_t)n_seg, 2), dim3(256), 0, st, in, (const unsigned long long *)d_start, (const uint32_t *)d_other, d_out);
    SC_TRY(hipGetLastError());
    SC_TRY(hipMemcpyAsync(out, d_out, sizeof(arp_sc_surface) * n_seg, hipMemcpyDeviceToHost, st));
    SC_TRY(hipStreamSynchronize(st));
    return ARP_OK;
}
#undef SC_TRY
