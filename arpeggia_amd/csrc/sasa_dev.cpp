// Atom SASA and the SAP chain on the device (sasa.inl, sap.inl, ens.inl run them; reference src/sasa.rs:174-247, src/sap.rs:137-250): the
// launch chain SASA -> SAP weight -> neighbour sum, and its callers -- arp_sap_neighbor_sum, sasa_run / bsa_run (one structure: arp_atom_sasa,
// arp_atom_sasa_groups and the structure-level entry points of sasa.cpp; they share GridIn) and ens_run / bsa_ens_run (the frames of an
// ensemble: arp_sasa_ensemble, arp_dsasa_ensemble; they share EnsPasses).
#include <cctype>
#include <cmath>
#include <cstring>
#include <algorithm>

#include "engine.h"
#include "table_dev.h"

using namespace arp;

// ---- SAP residue table (reference src/sap.rs:41-101) --------------------------------------------------------------------------
namespace arp {
struct SapResidue { const char *n; float h, a; };
#define ARP_SAP_ROW(n, h, a) {n, h, a},
static const SapResidue kSapResidues[20] = {ARP_SAP_RESIDUES(ARP_SAP_ROW)};
#undef ARP_SAP_ROW
uint32_t sap_residue_code(const char *resn) {
    if (!resn) return 20u;
    char up[8] = {0};
    for (int k = 0; k < 7 && resn[k]; k++) up[k] = (char)toupper((unsigned char)resn[k]);
    for (uint32_t r = 0; r < 20u; r++)
        if (strcmp(kSapResidues[r].n, up) == 0) return r;
    return 20u;
}
}  // namespace arp

extern "C" float arp_sap_weight(const char *resn, float sasa) {
    // hydrophobicity (Black & Mould minus glycine, sap.rs:41-64) x clamp(sasa / max side-chain SASA (sap.rs:77-101), 0, 1); 0 for residues
    // without a hydrophobicity value (sap.rs:198-209).  The table is ARP_SAP_RESIDUES (arp_internal.h), shared with the device weight kernel.
    const uint32_t r = sap_residue_code(resn);
    if (r >= 20u) return 0.0f;
    const SapResidue &t = kSapResidues[r];
    return t.h * std::min(1.0f, std::max(0.0f, sasa / t.a));
}

// ---- the launch chain ------------------------------------------------------------------------------------------------------------
namespace {
// search radius of the SASA grid: a burier j of a point of i is closer than R_i |s_k| + R_j <= 2 R_max (1 + 2^-23); 1e-5 covers that and the f32 gather test
double sasa_cutoff(float r_max) { return 2.0 * (double)r_max * (1.0 + 1e-5) + 1e-6; }
// attribute word of the SAP grid (the contact search's, over the side-chain atoms only): the rest is kept out by the bit that keeps hydrogens out of the contact grid
uint32_t sap_attr(uint8_t sidechain) { return sidechain ? (ARP_ATTR_LIGAND | ARP_ATTR_RECEPTOR) : ARP_ATTR_H; }

// Each stage uploads the parameters of its search radius and builds its grid in the context's workspace, whose cell list is then no pair pass's any more.
// buried != nullptr: the split walk -- sasa / count are three planes of d.n entries (launch_sasa)
arp_status sasa_stage(arp_context *ctx, const DevAtoms &d, float r_max, const float *R, const float *sphere, uint32_t n_points, float *sasa, int32_t *count,
                      int32_t *buried = nullptr) {
    arp_params prm;
    arp_default_params(&prm);
    prm.dist_cutoff = sasa_cutoff(r_max);
    const arp_status s = upload_params(ctx, &prm);
    if (s != ARP_OK) return s;
    mark_grid_foreign(ctx);
    launch_sasa(d, ctx->ws, prm.dist_cutoff, R, sphere, n_points, r_max, sasa, count, buried, ctx->stream, context_profiler(ctx));
    HIP_TRY(hipGetLastError());
    return ARP_OK;
}
// attribute word of the split walk's grid: the group mask as the two set bits of the contact search (the grid build copies them into Fat::pw)
uint32_t bsa_attr(uint8_t group) { return group ? ((group & 1u) ? ARP_ATTR_LIGAND : 0u) | ((group & 2u) ? ARP_ATTR_RECEPTOR : 0u) : ARP_ATTR_H; }
// out[i] = the f32 sum of w[j] over the grid atoms j within sap_radius of grid atom i; code != nullptr: w is first derived from the SASA values
arp_status sap_stage(arp_context *ctx, const DevAtoms &e, float sap_radius, const uint32_t *code, const int32_t *src, const float *sasa, float *w, float *out) {
    arp_params prm;
    arp_default_params(&prm);
    prm.dist_cutoff = (double)sap_radius;
    const arp_status s = upload_params(ctx, &prm);
    if (s != ARP_OK) return s;
    mark_grid_foreign(ctx);
    if (code) launch_sap_weight(e.n, code, src, sasa, w, ctx->stream);
    const double r2 = (double)(sap_radius * sap_radius);  // sap.rs:183-184: the product is formed in f32
    launch_neighbor_sum(e, ctx->ws, (double)sap_radius, r2, w, out, ctx->stream, context_profiler(ctx));
    HIP_TRY(hipGetLastError());
    return ARP_OK;
}
}  // namespace

// ---- SAP neighbour sum (reference src/sap.rs:155-204) ---------------------------------------------------
extern "C" arp_status arp_sap_neighbor_sum(arp_context *ctx, uint64_t n, const double *x, const double *y, const double *z, const uint8_t *sidechain,
                                           const float *weight, float sap_radius, float *out) try {
    arp_status s = check_device(ctx);
    if (s != ARP_OK) return s;
    if (n && (!x || !y || !z || !sidechain || !weight || !out)) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    if (n >= 0x5000000ull) { set_error("too many atoms for one SAP neighbour sum (the kernel addresses the sorted records with 32-bit byte offsets: < 83886080 atoms)"); return ARP_ERR_BAD_INPUT; }
    if (!(sap_radius >= 0.0f)) { set_error("bad sap_radius"); return ARP_ERR_BAD_INPUT; }
    if (n == 0) return ARP_OK;
    std::vector<uint32_t> attr(n), zero32(n, 0);
    for (uint64_t i = 0; i < n; i++) attr[i] = sap_attr(sidechain[i]);
    arp_atoms a{};
    a.n = n; a.x = x; a.y = y; a.z = z; a.attr = attr.data(); a.res_ord = zero32.data(); a.chain_rank = zero32.data(); a.model = zero32.data();
    a.n_res = 0; a.location = ARP_MEM_HOST;
    if ((s = ensure_workspace(ctx, n)) != ARP_OK) return s;
    DevAtoms d{};
    if ((s = stage_inputs(ctx, &a, &d)) != ARP_OK) return s;
    const uint64_t seg = seg_align(n * 4);  // {weights, sums} on the device; {weights, sums} pinned
    char *dev = nullptr, *pin = nullptr;
    if ((s = context_scratch(ctx, 0, 2 * seg, 2 * seg, &dev, &pin)) != ARP_OK) return s;
    float *d_w = (float *)dev, *d_out = (float *)(dev + seg), *h_out = (float *)(pin + seg);
    memcpy(pin, weight, n * 4);
    HIP_TRY(hipMemcpyAsync(d_w, pin, n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemsetAsync(d_out, 0, n * 4, ctx->stream));  // atoms outside the side-chain set keep 0
    if ((s = sap_stage(ctx, d, sap_radius, nullptr, nullptr, nullptr, d_w, d_out)) != ARP_OK) return s;
    HIP_TRY(hipMemcpyAsync(h_out, d_out, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    // non-finite coordinates are reported by the grid build through the pair pass's status word only; check here
    for (uint64_t i = 0; i < n; i++)
        if (sidechain[i] && !(std::isfinite(x[i]) && std::isfinite(y[i]) && std::isfinite(z[i]))) { set_error("non-finite atom coordinate"); return ARP_ERR_BAD_INPUT; }
    memcpy(out, h_out, n * 4);
    return ARP_OK;
} ARP_ABI_CATCH

// ---- segment sums (seg.inl) --------------------------------------------------------------------------------------
namespace arp {
arp_status seg_check(uint64_t m, uint64_t n_seg, const uint32_t *start, const uint32_t *item) {
    if (n_seg >= (1ull << 31) || m >= (1ull << 32)) { set_error("segment sum: too many segments or items per row (< 2^31 segments, < 2^32 items per row)"); return ARP_ERR_BAD_INPUT; }
    if (start[0] != 0u) { set_error("segment sum: seg_start[0] must be 0"); return ARP_ERR_BAD_INPUT; }
    for (uint64_t s = 0; s < n_seg; s++)
        if (start[s + 1] < start[s]) { set_error("segment sum: seg_start is not monotone at segment %llu", (unsigned long long)s); return ARP_ERR_BAD_INPUT; }
    if (start[n_seg] > 0x7FFFFFFFu - 64u) { set_error("segment sum: too many listed items (< 2^31 - 64)"); return ARP_ERR_BAD_INPUT; }
    for (uint32_t q = 0; q < start[n_seg]; q++)
        if (item[q] >= m) { set_error("segment sum: seg_item[%u] = %u is not below m = %llu", q, item[q], (unsigned long long)m); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}
}  // namespace arp
namespace {
// Where one CSR sits in a block (offsets: device and pinned alike) and the segments the wave kernel takes (seg.inl kSegLaneItems)
struct SegLayout {
    uint64_t o_start = 0, o_item = 0, o_long = 0, o_out = 0;
    std::vector<uint32_t> long_ids;
    void take_csr(Carver &lay, const SegJob &g) {
        for (uint32_t s = 0; s < g.n_seg; s++) if (g.start[s + 1] - g.start[s] > 64u) long_ids.push_back(s);
        o_start = lay.take(4ull * (g.n_seg + 1)); o_item = lay.take(4ull * g.start[g.n_seg]); o_long = lay.take(4ull * long_ids.size());
    }
    void fill(char *pin, const SegJob &g) const {
        memcpy(pin + o_start, g.start, 4ull * (g.n_seg + 1)); memcpy(pin + o_item, g.item, 4ull * g.start[g.n_seg]);
        memcpy(pin + o_long, long_ids.data(), 4ull * long_ids.size());
    }
    SegCsr csr(const char *dev, const SegJob &g) const {
        return SegCsr{g.n_seg, (uint32_t)long_ids.size(), (const uint32_t *)(dev + o_start), (const uint32_t *)(dev + o_item), (const uint32_t *)(dev + o_long)};
    }
};

// The grid input of a single-structure run (sasa_run, bsa_run), in SegLayout's style: where {f32-rounded x y z (f64), attr, zeros, model, R,
// sphere} sit in the block, what fills them, the walk over them and the way back.  attr(i): the attribute word of atom i -- an atom is in the
// grid unless the word is ARP_ATTR_H, and only then are its coordinates checked and its radius read.
struct GridIn {
    const SasaAtoms &j;
    uint64_t o_x = 0, o_y = 0, o_z = 0, o_attr = 0, o_zero = 0, o_model = 0, o_R = 0, o_sph = 0;
    float r_max = 0.0f;
    template <class Attr>
    arp_status begin(arp_context *ctx, Attr attr, Carver &lay) {  // the checks of a run, r_max, and the head of the block
        const arp_status s = check_device(ctx);
        if (s != ARP_OK) return s;
        if (ctx->pending) { set_error("a call enqueued on this context has not been collected (arp_contacts_atomic_result)"); return ARP_ERR_BAD_INPUT; }
        if (j.n >= 0x5000000ull) { set_error("too many atoms for one SASA call (< 83886080)"); return ARP_ERR_BAD_INPUT; }
        for (uint64_t i = 0; i < j.n; i++) {
            if (attr(i) == ARP_ATTR_H) continue;
            if (!(std::isfinite(j.x[i]) && std::isfinite(j.y[i]) && std::isfinite(j.z[i]))) { set_error("non-finite atom coordinate"); return ARP_ERR_BAD_INPUT; }
            r_max = std::max(r_max, j.R[i]);
        }
        o_x = lay.take(8 * j.n); o_y = lay.take(8 * j.n); o_z = lay.take(8 * j.n); o_attr = lay.take(4 * j.n); o_zero = lay.take(4 * j.n);
        o_model = lay.take(4 * j.n); o_R = lay.take(4 * j.n); o_sph = lay.take(12ull * j.n_points);
        return ARP_OK;
    }
    template <class Attr>
    void fill(char *pin, Attr attr) const {
        double *hx = (double *)(pin + o_x), *hy = (double *)(pin + o_y), *hz = (double *)(pin + o_z);
        uint32_t *hattr = (uint32_t *)(pin + o_attr), *hmodel = (uint32_t *)(pin + o_model);
        float *hR = (float *)(pin + o_R);
        for (uint64_t i = 0; i < j.n; i++) {
            hx[i] = (double)(float)j.x[i]; hy[i] = (double)(float)j.y[i]; hz[i] = (double)(float)j.z[i];  // sasa.rs:196-198
            hattr[i] = attr(i);
            hmodel[i] = j.model ? j.model[i] : 0u;
            hR[i] = hattr[i] == ARP_ATTR_H ? 0.0f : j.R[i];
        }
        memset(pin + o_zero, 0, 4 * j.n);
        memcpy(pin + o_sph, j.sphere, 12ull * j.n_points);
    }
    // Inputs [0, in_bytes) of the block go up, outputs [in_bytes, end) are zeroed (atoms outside the grid keep 0 everywhere), then the walk over
    // *d (buried != nullptr: the split one) and the copy of its tests word, which back() reads.
    arp_status walk(arp_context *ctx, char *dev, const char *pin, uint64_t in_bytes, uint64_t end, bool per_model, float *sasa, int32_t *count, int32_t *buried,
                    DevAtoms *d) const {
        arp_status s = ensure_workspace(ctx, j.n);
        if (s != ARP_OK) return s;
        HIP_TRY(hipMemcpyAsync(dev, pin, in_bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemsetAsync(dev + in_bytes, 0, end - in_bytes, ctx->stream));
        *d = DevAtoms{};
        d->n = (uint32_t)j.n; d->per_model = per_model ? 1u : 0u;
        d->x = (const double *)(dev + o_x); d->y = (const double *)(dev + o_y); d->z = (const double *)(dev + o_z);
        d->attr = (const uint32_t *)(dev + o_attr); d->res_ord = d->chain_rank = (const uint32_t *)(dev + o_zero); d->model = (const uint32_t *)(dev + o_model);
        if ((s = sasa_stage(ctx, *d, r_max, (const float *)(dev + o_R), (const float *)(dev + o_sph), j.n_points, sasa, count, buried)) != ARP_OK) return s;
        HIP_TRY(hipMemcpyAsync(ctx->h_result + kHostSasaTestsSlot, ctx->ws.result + kSasaTestsWord, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
        return ARP_OK;
    }
    // [back0, end) of the block comes back (the per-atom values stay on the device when nobody asked for them); the call's one synchronisation
    arp_status back(arp_context *ctx, const char *dev, char *pin, uint64_t back0, uint64_t end) const {
        if (end > back0) HIP_TRY(hipMemcpyAsync(pin + back0, dev + back0, end - back0, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->sasa_tests = ctx->h_result[kHostSasaTestsSlot];
        return ARP_OK;
    }
};

// The passes of an ensemble run (ens_run, bsa_ens_run).  Frames go through the device in passes of whole frames; a pass is
// one packed input of frames x m atoms, model = frame, every model with its own origin (DevAtoms::per_model).  Per pass only the coordinates are
// uploaded (pinned staging, refilled while the device works on the previous pass); the accumulators stay on the device until the last pass.
// Block: {topology | accumulators + totals | one pass}; the pinned block repeats the first two at the same offsets (one copy each way) and adds
// the coordinate staging and what the caller wants back per pass.  The caller lays out, fills and reads what is its own between the calls.
constexpr uint64_t kEnsAutoAtoms = 1u << 21;  // packed atoms per pass when the knob ens_chunk_atoms is 0 (1ubq x 3400 frames, 6bft x 230)
struct EnsPasses {
    const EnsAtoms *j = nullptr;
    uint64_t per = 0, pn = 0;  // frames and packed atoms of a full pass; per == 0: nothing to do
    float r_max = 0.0f;
    uint64_t o_sel = 0, o_R = 0, o_sph = 0, topo_bytes = 0, shared_bytes = 0, o_xyz = 0, o_x = 0, o_y = 0, o_z = 0, o_zero = 0, o_model = 0, o_Rp = 0, h_xyz = 0;
    EnsTopo tp{};  // (the caller adds the SAP members)
    EnsPack pk{};
    // checks, frames per pass, and the head of the topology: {sel, R, sphere}
    arp_status begin(arp_context *ctx, const EnsAtoms &job, const char *what, Carver &lay) {
        j = &job;
        const arp_status s = check_device(ctx);
        if (s != ARP_OK) return s;
        if (ctx->pending) { set_error("a call enqueued on this context has not been collected (arp_contacts_atomic_result)"); return ARP_ERR_BAD_INPUT; }
        const uint64_t m = job.m, F = job.n_frames;
        if (m == 0 || F == 0) return ARP_OK;
        // frames per pass: the atom budget; a model ordinal per frame (grid.inl kPackModels); one pass below the SASA / SAP kernels' atom limit
        constexpr uint64_t kMaxPassAtoms = 0x5000000ull - 1u;
        if (m > kMaxPassAtoms) { set_error("%s: too many selected atoms for one frame (< 83886080)", what); return ARP_ERR_BAD_INPUT; }
        const uint64_t budget = job.chunk_atoms ? job.chunk_atoms : kEnsAutoAtoms;
        per = std::min<uint64_t>({std::max<uint64_t>(1, budget / m), F, 65535u, kMaxPassAtoms / m});
        pn = per * m;
        for (uint64_t k = 0; k < m; k++) r_max = std::max(r_max, job.R[k]);
        o_sel = lay.take(4 * m); o_R = lay.take(4 * m); o_sph = lay.take(12ull * job.n_points);
        return ARP_OK;
    }
    void end_topology(Carver &lay) { topo_bytes = lay.off; }
    // after the accumulators: the head of a pass on the device {xyz as uploaded, x y z, zeros, model, R}
    void take_pass(Carver &lay) {
        shared_bytes = lay.off;
        o_xyz = lay.take(24 * per * j->n_top); o_x = lay.take(8 * pn); o_y = lay.take(8 * pn); o_z = lay.take(8 * pn); o_zero = lay.take(4 * pn);
        o_model = lay.take(4 * pn); o_Rp = lay.take(4 * pn);
    }
    // after the pass: the device block ends (returned), the pinned tail starts with the coordinate staging
    uint64_t take_staging(Carver &lay) {
        const uint64_t dev_bytes = lay.off;
        lay.off = shared_bytes;
        h_xyz = lay.take(24 * per * j->n_top);
        return dev_bytes;
    }
    arp_status open(arp_context *ctx, uint64_t dev_bytes, uint64_t pin_bytes, char **dev, char **pin) {
        arp_status s = ensure_workspace(ctx, pn);
        if (s != ARP_OK) return s;
        if ((s = context_scratch(ctx, 0, dev_bytes, pin_bytes, dev, pin)) != ARP_OK) return s;
        memcpy(*pin + o_sel, j->sel, 4 * j->m); memcpy(*pin + o_R, j->R, 4 * j->m); memcpy(*pin + o_sph, j->sphere, 12ull * j->n_points);
        char *d = *dev;
        tp = EnsTopo{(uint32_t)j->n_top, (uint32_t)j->m, (const uint32_t *)(d + o_sel), (const float *)(d + o_R), nullptr, nullptr};
        pk.x = (double *)(d + o_x); pk.y = (double *)(d + o_y); pk.z = (double *)(d + o_z); pk.model = (uint32_t *)(d + o_model); pk.R = (float *)(d + o_Rp);
        return ARP_OK;
    }
    arp_status upload(arp_context *ctx, char *dev, const char *pin) const {
        HIP_TRY(hipMemcpyAsync(dev, pin, topo_bytes, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipMemsetAsync(dev + o_zero, 0, 4 * pn, ctx->stream));  // residue ordinal, chain rank (and the attribute word where every packed atom is in the grid)
        return ARP_OK;
    }
    // The loop.  pass(f0, fc, d): the caller's stage, reduces and optional copies back for frames [f0, f0 + fc) packed as d (attr: the packed
    // attribute words, nullptr: the zeros); then the accumulators come back into the pinned block, and the call's last synchronisation.
    template <class Pass>
    arp_status run(arp_context *ctx, char *dev, char *pin, const uint32_t *attr, Pass pass) const {
        hipStream_t st = ctx->stream;
        const uint64_t m = j->m, N = j->n_top, F = j->n_frames;
        struct Event { hipEvent_t e = nullptr; ~Event() { if (e) (void)hipEventDestroy(e); } } staged;  // behind the upload of the staging buffer: the host refills it only after that copy has run
        HIP_TRY(hipEventCreateWithFlags(&staged.e, hipEventDisableTiming));
        for (uint64_t f0 = 0; f0 < F; f0 += per) {
            const uint64_t fc = std::min<uint64_t>(per, F - f0);
            if (f0) HIP_TRY(hipEventSynchronize(staged.e));
            memcpy(pin + h_xyz, j->xyz + f0 * N * 3, 24 * fc * N);
            HIP_TRY(hipMemcpyAsync(dev + o_xyz, pin + h_xyz, 24 * fc * N, hipMemcpyHostToDevice, st));
            HIP_TRY(hipEventRecord(staged.e, st));
            launch_ens_tile((uint32_t)fc, (const double *)(dev + o_xyz), tp, pk, st);
            DevAtoms d{};
            d.n = (uint32_t)(fc * m); d.per_model = 1u;
            d.x = pk.x; d.y = pk.y; d.z = pk.z;
            d.res_ord = d.chain_rank = (const uint32_t *)(dev + o_zero); d.attr = attr ? attr : d.res_ord; d.model = pk.model;
            const arp_status s = pass(f0, fc, d);
            if (s != ARP_OK) return s;
        }
        HIP_TRY(hipMemcpyAsync(pin + topo_bytes, dev + topo_bytes, shared_bytes - topo_bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return ARP_OK;
    }
};
}  // namespace

extern "C" arp_status arp_segment_sum(arp_context *ctx, uint64_t rows, uint64_t m, const float *values, uint64_t n_seg, const uint32_t *seg_start,
                                      const uint32_t *seg_item, float *out) try {
    if (rows == 0 || n_seg == 0 || m == 0) return ARP_OK;
    if (!values || !seg_start || !out || (seg_start[n_seg] && !seg_item)) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    arp_status s = seg_check(m, n_seg, seg_start, seg_item);
    if (s != ARP_OK) return s;
    if (rows > (1ull << 40) / m || rows > (1ull << 40) / n_seg) { set_error("segment sum: rows x m and rows x n_seg must stay below 2^40"); return ARP_ERR_BAD_INPUT; }
    if (!ctx) return ARP_OK;  // the checks alone
    if ((s = check_device(ctx)) != ARP_OK) return s;
    if (ctx->pending) { set_error("a call enqueued on this context has not been collected (arp_contacts_atomic_result)"); return ARP_ERR_BAD_INPUT; }
    SegJob g;
    g.n_seg = (uint32_t)n_seg; g.start = seg_start; g.item = seg_item;
    Carver lay;
    SegLayout sl;
    sl.take_csr(lay, g);
    const uint64_t o_val = lay.take(4 * rows * m), in_bytes = lay.off;
    sl.o_out = lay.take(4 * rows * n_seg);
    char *dev = nullptr, *pin = nullptr;
    if ((s = context_scratch(ctx, 0, lay.off, lay.off, &dev, &pin)) != ARP_OK) return s;
    sl.fill(pin, g);
    memcpy(pin + o_val, values, 4 * rows * m);
    HIP_TRY(hipMemcpyAsync(dev, pin, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    launch_segment_sum(rows, (uint32_t)m, (const float *)(dev + o_val), sl.csr(dev, g), (float *)(dev + sl.o_out), ctx->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(pin + sl.o_out, dev + sl.o_out, 4 * rows * n_seg, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(out, pin + sl.o_out, 4 * rows * n_seg);
    return ARP_OK;
} ARP_ABI_CATCH

// ---- atom SASA (sasa.inl; reference src/sasa.rs:174-247) and the SAP chain (src/sap.rs:137-250) --------------------------------------
namespace arp {
void sasa_sphere_points(uint32_t n, float *xyz) {
    // golden spiral: t = k / n, theta = acos(1 - 2 t), phi = (2 pi golden) k; (sin theta cos phi, sin theta sin phi, cos theta) in f64, rounded to f32
    const double golden = (1.0 + std::sqrt(5.0)) / 2.0, step = 2.0 * 3.141592653589793 * golden;
    for (uint32_t k = 0; k < n; k++) {
        const double t = (double)k / (double)n, theta = std::acos(1.0 - 2.0 * t), phi = step * (double)k;
        xyz[3 * k] = (float)(std::sin(theta) * std::cos(phi));
        xyz[3 * k + 1] = (float)(std::sin(theta) * std::sin(phi));
        xyz[3 * k + 2] = (float)std::cos(theta);
    }
}

arp_status sasa_run(arp_context *ctx, const SasaJob &j, float *sasa, int32_t *count, float *sap) {
    const auto attr = [&](uint64_t i) { return j.include[i] ? 0u : (uint32_t)ARP_ATTR_H; };  // (the attribute bit that keeps an atom out of the grid)
    // one pinned block out, one back: inputs {the grid input, [x y z, SAP attr, code, src], [CSRs]}, outputs {sasa, count, [w, sap], [sums]}
    Carver lay;
    GridIn in{j};
    arp_status s = in.begin(ctx, attr, lay);
    const uint64_t n = j.n;
    if (s != ARP_OK || n == 0) return s;
    const bool with_sap = j.sidechain != nullptr;
    for (uint64_t i = 0; with_sap && i < n; i++)
        if (j.sidechain[i] && !(std::isfinite(j.x[i]) && std::isfinite(j.y[i]) && std::isfinite(j.z[i]))) { set_error("non-finite atom coordinate"); return ARP_ERR_BAD_INPUT; }
    uint64_t o_px = 0, o_py = 0, o_pz = 0, o_pattr = 0, o_code = 0, o_src = 0;
    if (with_sap) { o_px = lay.take(8 * n); o_py = lay.take(8 * n); o_pz = lay.take(8 * n); o_pattr = lay.take(4 * n); o_code = lay.take(4 * n); o_src = lay.take(4 * n); }
    std::vector<SegLayout> seg(j.n_segs);
    for (uint32_t g = 0; g < j.n_segs; g++) seg[g].take_csr(lay, j.segs[g]);
    const uint64_t in_bytes = lay.off;
    const uint64_t o_sasa = lay.take(4 * n), o_count = lay.take(4 * n), o_w = with_sap ? lay.take(4 * n) : 0, o_sap = with_sap ? lay.take(4 * n) : 0;
    const uint64_t seg_out0 = lay.off;
    for (uint32_t g = 0; g < j.n_segs; g++) seg[g].o_out = lay.take(4ull * j.segs[g].n_seg);
    char *dev = nullptr, *pin = nullptr;
    if ((s = context_scratch(ctx, 0, lay.off, lay.off, &dev, &pin)) != ARP_OK) return s;
    in.fill(pin, attr);
    if (with_sap) {
        memcpy(pin + o_px, j.x, 8 * n); memcpy(pin + o_py, j.y, 8 * n); memcpy(pin + o_pz, j.z, 8 * n);
        uint32_t *pa = (uint32_t *)(pin + o_pattr);
        for (uint64_t i = 0; i < n; i++) pa[i] = sap_attr(j.sidechain[i]);
        memcpy(pin + o_code, j.res_code, 4 * n); memcpy(pin + o_src, j.src, 4 * n);
    }
    for (uint32_t g = 0; g < j.n_segs; g++) seg[g].fill(pin, j.segs[g]);
    DevAtoms d;
    float *d_sasa = (float *)(dev + o_sasa);
    if ((s = in.walk(ctx, dev, pin, in_bytes, lay.off, false, d_sasa, (int32_t *)(dev + o_count), nullptr, &d)) != ARP_OK) return s;
    if (with_sap) {
        DevAtoms e = d;
        e.x = (const double *)(dev + o_px); e.y = (const double *)(dev + o_py); e.z = (const double *)(dev + o_pz);
        e.attr = (const uint32_t *)(dev + o_pattr); e.model = e.res_ord;  // (zeros)
        if ((s = sap_stage(ctx, e, j.sap_radius, (const uint32_t *)(dev + o_code), (const int32_t *)(dev + o_src), d_sasa, (float *)(dev + o_w), (float *)(dev + o_sap))) != ARP_OK) return s;
    }
    for (uint32_t g = 0; g < j.n_segs; g++) launch_segment_sum(1, (uint32_t)n, d_sasa, seg[g].csr(dev, j.segs[g]), (float *)(dev + seg[g].o_out), ctx->stream);
    if (j.n_segs) HIP_TRY(hipGetLastError());
    if ((s = in.back(ctx, dev, pin, (sasa || count || sap) ? in_bytes : seg_out0, lay.off)) != ARP_OK) return s;
    for (uint32_t g = 0; g < j.n_segs; g++) memcpy(j.segs[g].out, pin + seg[g].o_out, 4ull * j.segs[g].n_seg);
    if (sasa) memcpy(sasa, pin + o_sasa, 4 * n);
    if (count) memcpy(count, pin + o_count, 4 * n);
    if (sap && with_sap) memcpy(sap, pin + o_sap, 4 * n);
    return ARP_OK;
}

// Buried surface per atom: sasa_run's staging with the group mask as the attribute word and the split walk; the three
// planes of areas are three rows of n values for the segment sum.
arp_status bsa_run(arp_context *ctx, const BsaJob &j, float *sasa3, int32_t *count3, int32_t *buried) {
    const auto attr = [&](uint64_t i) { return bsa_attr(j.group[i]); };
    // inputs {the grid input, [CSR]}, outputs {sasa x 3, count x 3, buried, [sums x 3]}
    Carver lay;
    GridIn in{j};
    arp_status s = in.begin(ctx, attr, lay);
    const uint64_t n = j.n;
    if (s != ARP_OK || n == 0) return s;
    SegLayout seg;
    if (j.seg) seg.take_csr(lay, *j.seg);
    const uint64_t in_bytes = lay.off;
    const uint64_t o_sasa = lay.take(12 * n), o_count = lay.take(12 * n), o_buried = lay.take(4 * n);
    const uint64_t seg_out0 = lay.off;
    if (j.seg) seg.o_out = lay.take(12ull * j.seg->n_seg);
    char *dev = nullptr, *pin = nullptr;
    if ((s = context_scratch(ctx, 0, lay.off, lay.off, &dev, &pin)) != ARP_OK) return s;
    in.fill(pin, attr);
    if (j.seg) seg.fill(pin, *j.seg);
    DevAtoms d;
    float *d_sasa = (float *)(dev + o_sasa);
    if ((s = in.walk(ctx, dev, pin, in_bytes, lay.off, j.per_model, d_sasa, (int32_t *)(dev + o_count), (int32_t *)(dev + o_buried), &d)) != ARP_OK) return s;
    if (j.seg) {
        launch_segment_sum(3, (uint32_t)n, d_sasa, seg.csr(dev, *j.seg), (float *)(dev + seg.o_out), ctx->stream);
        HIP_TRY(hipGetLastError());
    }
    if ((s = in.back(ctx, dev, pin, (sasa3 || count3 || buried) ? in_bytes : seg_out0, lay.off)) != ARP_OK) return s;
    if (j.seg) memcpy(j.seg->out, pin + seg.o_out, 12ull * j.seg->n_seg);
    if (sasa3) memcpy(sasa3, pin + o_sasa, 12 * n);
    if (count3) memcpy(count3, pin + o_count, 12 * n);
    if (buried) memcpy(buried, pin + o_buried, 4 * n);
    return ARP_OK;
}

// SASA / SAP statistics over the frames of an ensemble (arp_sasa_ensemble): on every pass of EnsPasses the SASA and SAP
// kernels of sasa_run run as they are, then the folds into the per-atom (and per-residue) accumulators.
arp_status ens_run(arp_context *ctx, const EnsJob &j, const EnsOut &o) {
    EnsPasses ep;
    Carver lay;
    arp_status s = ep.begin(ctx, j, "sasa ensemble", lay);
    if (s != ARP_OK || !ep.per) return s;
    const uint64_t m = j.m, F = j.n_frames, per = ep.per, pn = ep.pn;
    const uint64_t o_code = lay.take(4 * m), o_pattr = lay.take(4 * m);
    const bool with_res = j.res != nullptr;  // (then j.chain is given as well)
    const uint64_t n_res = with_res ? j.res->n_seg : 0, n_chain = with_res ? j.chain->n_seg : 0;
    SegLayout seg_res, seg_chain;
    if (with_res) { seg_res.take_csr(lay, *j.res); seg_chain.take_csr(lay, *j.chain); }
    ep.end_topology(lay);
    const uint64_t o_rt1 = lay.take(8 * n_res), o_rt2 = lay.take(8 * n_res), o_rmin = lay.take(4 * n_res), o_rmax = lay.take(4 * n_res), o_chain = lay.take(4 * F * n_chain);
    const uint64_t o_s1 = lay.take(8 * m), o_s2 = lay.take(8 * m), o_t1 = lay.take(8 * m), o_t2 = lay.take(8 * m), o_cmin = lay.take(4 * m), o_cmax = lay.take(4 * m), o_pmin = lay.take(4 * m),
                   o_pmax = lay.take(4 * m), o_total = lay.take(4 * F);
    ep.take_pass(lay);
    const uint64_t o_sasa = lay.take(4 * pn), o_count = lay.take(4 * pn);
    uint64_t o_px = 0, o_py = 0, o_pz = 0, o_pa = 0, o_pc = 0, o_src = 0, o_w = 0, o_sap = 0;
    if (j.with_sap) { o_px = lay.take(8 * pn); o_py = lay.take(8 * pn); o_pz = lay.take(8 * pn); o_pa = lay.take(4 * pn); o_pc = lay.take(4 * pn); o_src = lay.take(4 * pn); o_w = lay.take(4 * pn); o_sap = lay.take(4 * pn); }
    const uint64_t o_rs = lay.take(4 * per * n_res);
    const uint64_t dev_bytes = ep.take_staging(lay);
    const uint64_t h_count = o.count ? lay.take(4 * pn) : 0, h_sap = o.sap ? lay.take(4 * pn) : 0, h_rs = o.residue_sasa ? lay.take(4 * per * n_res) : 0;
    char *dev = nullptr, *pin = nullptr;
    if ((s = ep.open(ctx, dev_bytes, lay.off, &dev, &pin)) != ARP_OK) return s;
    if (j.with_sap) {
        memcpy(pin + o_code, j.res_code, 4 * m);
        uint32_t *pa = (uint32_t *)(pin + o_pattr);
        for (uint64_t k = 0; k < m; k++) pa[k] = sap_attr(j.sidechain[k]);
    }
    if (with_res) { seg_res.fill(pin, *j.res); seg_chain.fill(pin, *j.chain); }
    const SegCsr csr_res = with_res ? seg_res.csr(dev, *j.res) : SegCsr{}, csr_chain = with_res ? seg_chain.csr(dev, *j.chain) : SegCsr{};
    const SegAcc racc{(double *)(dev + o_rt1), (double *)(dev + o_rt2), (float *)(dev + o_rmin), (float *)(dev + o_rmax)};
    hipStream_t st = ctx->stream;
    if ((s = ep.upload(ctx, dev, pin)) != ARP_OK) return s;
    if (j.with_sap) HIP_TRY(hipMemsetAsync(dev + o_sap, 0, 4 * pn, st));  // backbone atoms are outside the SAP grid in every frame: they keep 0
    ep.tp.code = (const uint32_t *)(dev + o_code); ep.tp.pattr = (const uint32_t *)(dev + o_pattr);
    EnsPack &pk = ep.pk;
    if (j.with_sap) {
        pk.px = (double *)(dev + o_px); pk.py = (double *)(dev + o_py); pk.pz = (double *)(dev + o_pz);
        pk.pattr = (uint32_t *)(dev + o_pa); pk.code = (uint32_t *)(dev + o_pc); pk.src = (int32_t *)(dev + o_src);
    }
    EnsAcc acc{(unsigned long long *)(dev + o_s1), (unsigned long long *)(dev + o_s2), (int32_t *)(dev + o_cmin), (int32_t *)(dev + o_cmax),
               (double *)(dev + o_t1), (double *)(dev + o_t2), (float *)(dev + o_pmin), (float *)(dev + o_pmax)};
    float *d_sasa = (float *)(dev + o_sasa), *d_sap = j.with_sap ? (float *)(dev + o_sap) : nullptr;
    int32_t *d_count = (int32_t *)(dev + o_count);
    s = ep.run(ctx, dev, pin, nullptr, [&](uint64_t f0, uint64_t fc, const DevAtoms &d) -> arp_status {
        const uint64_t cn = fc * m;
        arp_status s = sasa_stage(ctx, d, ep.r_max, pk.R, (const float *)(dev + ep.o_sph), j.n_points, d_sasa, d_count);
        if (s != ARP_OK) return s;
        if (j.with_sap) {
            DevAtoms e = d;
            e.x = pk.px; e.y = pk.py; e.z = pk.pz; e.attr = pk.pattr;
            if ((s = sap_stage(ctx, e, j.sap_radius, pk.code, pk.src, d_sasa, (float *)(dev + o_w), d_sap)) != ARP_OK) return s;
        }
        launch_ens_reduce((uint32_t)fc, (uint32_t)m, d_count, d_sasa, d_sap, acc, f0 == 0, (float *)(dev + o_total) + f0, st);
        if (with_res) {  // the pass's [frame][residue] and [frame][chain] sums of the SASA values, then the residues' fold over its frames
            launch_segment_sum(fc, (uint32_t)m, d_sasa, csr_res, (float *)(dev + o_rs), st);
            launch_segment_sum(fc, (uint32_t)m, d_sasa, csr_chain, (float *)(dev + o_chain) + f0 * n_chain, st);
            launch_ens_res_reduce((uint32_t)fc, (uint32_t)n_res, (const float *)(dev + o_rs), racc, f0 == 0, st);
        }
        HIP_TRY(hipGetLastError());
        if (o.count || o.sap || o.residue_sasa) {  // the pass's own values, only when the caller wants them
            if (o.count) HIP_TRY(hipMemcpyAsync(pin + h_count, d_count, 4 * cn, hipMemcpyDeviceToHost, st));
            if (o.sap) HIP_TRY(hipMemcpyAsync(pin + h_sap, d_sap, 4 * cn, hipMemcpyDeviceToHost, st));
            if (o.residue_sasa) HIP_TRY(hipMemcpyAsync(pin + h_rs, dev + o_rs, 4 * fc * n_res, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (o.count) memcpy(o.count + f0 * m, pin + h_count, 4 * cn);
            if (o.sap) memcpy(o.sap + f0 * m, pin + h_sap, 4 * cn);
            if (o.residue_sasa) memcpy(o.residue_sasa + f0 * n_res, pin + h_rs, 4 * fc * n_res);
        }
        return ARP_OK;
    });
    if (s != ARP_OK) return s;
    memcpy(o.s1, pin + o_s1, 8 * m); memcpy(o.s2, pin + o_s2, 8 * m); memcpy(o.cmin, pin + o_cmin, 4 * m); memcpy(o.cmax, pin + o_cmax, 4 * m);
    memcpy(o.total, pin + o_total, 4 * F);
    if (j.with_sap) { memcpy(o.t1, pin + o_t1, 8 * m); memcpy(o.t2, pin + o_t2, 8 * m); memcpy(o.pmin, pin + o_pmin, 4 * m); memcpy(o.pmax, pin + o_pmax, 4 * m); }
    if (with_res) {
        memcpy(o.rt1, pin + o_rt1, 8 * n_res); memcpy(o.rt2, pin + o_rt2, 8 * n_res); memcpy(o.rmin, pin + o_rmin, 4 * n_res); memcpy(o.rmax, pin + o_rmax, 4 * n_res);
        memcpy(o.chain_sasa, pin + o_chain, 4 * F * n_chain);
    }
    return ARP_OK;
}

// dSASA over the frames (arp_dsasa_ensemble): the passes of EnsPasses with the split walk on the pack -- k_bsa_tile_attr
// repeats the masks, k_ens_reduce and k_ens_totals run as they are on what k_sasa_split writes.
arp_status bsa_ens_run(arp_context *ctx, const BsaEnsJob &j, const BsaEnsOut &o) {
    EnsPasses ep;
    Carver lay;
    arp_status s = ep.begin(ctx, j, "dsasa ensemble", lay);
    if (s != ARP_OK || !ep.per) return s;
    const uint64_t m = j.m, F = j.n_frames, pn = ep.pn;
    const uint64_t o_gattr = lay.take(4 * m);
    ep.end_topology(lay);
    const uint64_t o_s1 = lay.take(8 * m), o_s2 = lay.take(8 * m), o_bmin = lay.take(4 * m), o_bmax = lay.take(4 * m), o_fb = lay.take(4 * m), o_total = lay.take(12 * F);
    ep.take_pass(lay);
    const uint64_t o_attr = lay.take(4 * pn), o_sasa = lay.take(12 * pn), o_count = lay.take(12 * pn), o_buried = lay.take(4 * pn);
    const uint64_t dev_bytes = ep.take_staging(lay);
    const uint64_t h_buried = o.buried ? lay.take(4 * pn) : 0;
    char *dev = nullptr, *pin = nullptr;
    if ((s = ep.open(ctx, dev_bytes, lay.off, &dev, &pin)) != ARP_OK) return s;
    uint32_t *ga = (uint32_t *)(pin + o_gattr);
    for (uint64_t k = 0; k < m; k++) ga[k] = bsa_attr(j.group[k]);
    hipStream_t st = ctx->stream;
    if ((s = ep.upload(ctx, dev, pin)) != ARP_OK) return s;
    EnsAcc acc{(unsigned long long *)(dev + o_s1), (unsigned long long *)(dev + o_s2), (int32_t *)(dev + o_bmin), (int32_t *)(dev + o_bmax), nullptr, nullptr, nullptr, nullptr};
    float *d_sasa = (float *)(dev + o_sasa);
    int32_t *d_buried = (int32_t *)(dev + o_buried);
    s = ep.run(ctx, dev, pin, (const uint32_t *)(dev + o_attr), [&](uint64_t f0, uint64_t fc, const DevAtoms &d) -> arp_status {
        launch_bsa_tile_attr((uint32_t)fc, (uint32_t)m, (const uint32_t *)(dev + o_gattr), (uint32_t *)(dev + o_attr), st);
        const arp_status s = sasa_stage(ctx, d, ep.r_max, ep.pk.R, (const float *)(dev + ep.o_sph), j.n_points, d_sasa, (int32_t *)(dev + o_count), d_buried);
        if (s != ARP_OK) return s;
        float *const tot[3] = {(float *)(dev + o_total) + f0, (float *)(dev + o_total) + F + f0, (float *)(dev + o_total) + 2 * F + f0};
        launch_bsa_ens_reduce((uint32_t)fc, (uint32_t)m, d_buried, d_sasa, acc, (uint32_t *)(dev + o_fb), f0 == 0, tot, st);
        HIP_TRY(hipGetLastError());
        if (o.buried) {  // the pass's own values, only when the caller wants them
            HIP_TRY(hipMemcpyAsync(pin + h_buried, d_buried, 4 * fc * m, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            memcpy(o.buried + f0 * m, pin + h_buried, 4 * fc * m);
        }
        return ARP_OK;
    });
    if (s != ARP_OK) return s;
    memcpy(o.s1, pin + o_s1, 8 * m); memcpy(o.s2, pin + o_s2, 8 * m); memcpy(o.bmin, pin + o_bmin, 4 * m); memcpy(o.bmax, pin + o_bmax, 4 * m);
    memcpy(o.frames_buried, pin + o_fb, 4 * m);
    for (int g = 0; g < 3; g++) memcpy(o.total[g], pin + o_total + 4 * F * g, 4 * F);
    return ARP_OK;
}
}  // namespace arp

extern "C" arp_status arp_sasa_sphere_points(uint32_t n, float *xyz) try {
    if (n < 1 || n > ARP_SASA_MAX_POINTS || !xyz) { set_error("arp_sasa_sphere_points: n must be 1..%d and xyz non-null", ARP_SASA_MAX_POINTS); return ARP_ERR_BAD_INPUT; }
    sasa_sphere_points(n, xyz);
    return ARP_OK;
} ARP_ABI_CATCH

namespace arp {
arp_status sasa_check_params(float probe, int32_t n_points) {
    if (n_points < 1 || n_points > ARP_SASA_MAX_POINTS) { set_error("n_points must be 1..%d (got %d)", ARP_SASA_MAX_POINTS, (int)n_points); return ARP_ERR_BAD_INPUT; }
    if (!(std::isfinite(probe) && probe >= 0.0f)) { set_error("probe radius must be finite and >= 0"); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}
}  // namespace arp

extern "C" arp_status arp_atom_sasa(arp_context *ctx, uint64_t n, const double *x, const double *y, const double *z, const float *radius,
                                    const uint8_t *include, float probe, int32_t n_points, float *out_sasa, int32_t *out_count) try {
    arp_status s = check_device(ctx);
    if (s != ARP_OK) return s;
    if ((s = sasa_check_params(probe, n_points)) != ARP_OK) return s;
    if (n && (!x || !y || !z || !radius || !out_sasa)) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    std::vector<uint8_t> all;
    if (!include) { all.assign(n, 1); include = all.data(); }
    std::vector<float> R(n, 0.0f);
    for (uint64_t i = 0; i < n; i++) {
        if (!include[i]) continue;
        if (!(std::isfinite(radius[i]) && radius[i] >= 0.0f)) { set_error("atom %llu: radius must be finite and >= 0", (unsigned long long)i); return ARP_ERR_BAD_INPUT; }
        R[i] = radius[i] + probe;  // sasa.rs:200-206 + rust-sasa: r + probe in f32
    }
    std::vector<float> sphere(3ull * (uint32_t)n_points);
    sasa_sphere_points((uint32_t)n_points, sphere.data());
    SasaJob j;
    j.n = n; j.x = x; j.y = y; j.z = z; j.R = R.data(); j.include = include; j.n_points = (uint32_t)n_points; j.sphere = sphere.data();
    std::vector<int32_t> cnt(out_count ? 0 : n);
    return sasa_run(ctx, j, out_sasa, out_count ? out_count : cnt.data(), nullptr);
} ARP_ABI_CATCH

extern "C" arp_status arp_atom_sasa_groups(arp_context *ctx, uint64_t n, const double *x, const double *y, const double *z, const float *radius,
                                           const uint8_t *group, float probe, int32_t n_points, int32_t *out_count, float *out_sasa, int32_t *out_buried) try {
    // (the argument checks come first: they need no device)
    arp_status s = sasa_check_params(probe, n_points);
    if (s != ARP_OK) return s;
    if (n && (!x || !y || !z || !radius || !group || !out_count || !out_sasa || !out_buried)) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    std::vector<float> R(n, 0.0f);
    for (uint64_t i = 0; i < n; i++) {
        if (group[i] > 3u) { set_error("atom %llu: group mask %u is not one of 0 (out), 1, 2, 3 (both)", (unsigned long long)i, (unsigned)group[i]); return ARP_ERR_BAD_INPUT; }
        if (!group[i]) continue;
        if (!(std::isfinite(radius[i]) && radius[i] >= 0.0f)) { set_error("atom %llu: radius must be finite and >= 0", (unsigned long long)i); return ARP_ERR_BAD_INPUT; }
        R[i] = radius[i] + probe;  // as arp_atom_sasa
    }
    if ((s = check_device(ctx)) != ARP_OK) return s;
    std::vector<float> sphere(3ull * (uint32_t)n_points);
    sasa_sphere_points((uint32_t)n_points, sphere.data());
    BsaJob j;
    j.n = n; j.x = x; j.y = y; j.z = z; j.R = R.data(); j.group = group; j.n_points = (uint32_t)n_points; j.sphere = sphere.data();
    return bsa_run(ctx, j, out_sasa, out_count, out_buried);
} ARP_ABI_CATCH

extern "C" uint64_t arp_sasa_tests(const arp_context *ctx) { return ctx ? ctx->sasa_tests : 0u; }
