// Host engine: context / workspace management, the pair-pass protocol and the C-ABI entry points of the atomic-contact hot path
// (include/arpeggia_amd.h); batch.cpp holds the pack pipeline, sasa_dev.cpp the SASA / SAP chain, engine.h what the three share.  Compiled with hipcc for
// the HIP runtime API; all device code lives in kernels.hip.  There is NO CPU compute path: without a gfx950 device every compute call returns ARP_ERR_NO_DEVICE.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <algorithm>
#include <sys/mman.h>

#include "engine.h"
#include "table_dev.h"
#include "table_plan.h"

namespace arp {

thread_local char g_err[512] = "";
void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
}

// ---- exact squared-distance decision bounds (see DevParams) ------------------------------------------------
// min{ s >= 0 : sqrt(s) >= T }  so that  (sqrt(s) < T)  <=>  (s < bound_lt(T)).  Host sqrt is correctly rounded.
double bound_lt(double T) {
    if (!(T > 0.0)) return 0.0;  // T <= 0 or NaN: d < T never holds for d >= 0
    if (std::isinf(T)) return INFINITY;
    double s = T * T;
    if (!std::isfinite(s)) s = DBL_MAX;
    while (s > 0.0 && std::sqrt(s) >= T) s = std::nextafter(s, 0.0);
    while (std::sqrt(s) < T) s = std::nextafter(s, INFINITY);
    return s;
}
// min{ s >= 0 : sqrt(s) > T }  so that  (sqrt(s) <= T)  <=>  (s < bound_le(T)).
double bound_le(double T) {
    if (!(T >= 0.0)) return 0.0;
    if (std::isinf(T)) return INFINITY;
    double s = T * T;
    if (!std::isfinite(s)) s = DBL_MAX;
    while (s > 0.0 && std::sqrt(s) > T) s = std::nextafter(s, 0.0);
    while (std::sqrt(s) <= T) s = std::nextafter(s, INFINITY);
    return s;
}

void make_dev_params(const arp_params &p, DevParams *d) {
    memset(d, 0, sizeof *d);
    const double c = p.vdw_comp;
    d->r2 = d->r2_call = p.dist_cutoff * p.dist_cutoff;  // complex.rs:191 (r2 itself is rewritten by every call's grid sizing)
    d->s_ion = bound_le(4.0);
    d->s_polar = bound_le(3.5);
    d->s_hphob = bound_le(4.5);
    for (int a = 0; a < 16; a++) {
        for (int b = 0; b < 16; b++) {
            double sum_cov = p.cov_radius[a] + p.cov_radius[b];  // vdw.rs:27
            double sum_vdw = p.vdw_radius[a] + p.vdw_radius[b];  // vdw.rs:28
            d->s_clash[a * 16 + b] = bound_lt(sum_cov - c);
            d->s_cov[a * 16 + b] = bound_lt(sum_cov + c);
            d->s_vdw[a * 16 + b] = bound_lt(sum_vdw + c);
            // vdw.rs:32-43 is a first-match chain (clash, covalent, vdW); k_emit counts how many of the three bounds a distance is below,
            // which is the same thing only for NESTED bounds.  A negative vdw_comp (cov - c > cov + c) or caller radii with vdw < cov break the
            // nesting; raising each bound to its predecessor restores it without changing any first-match outcome: below the clash bound
            // the pair is a clash whatever the others say, and a distance at or above it is below max(cov, clash) exactly when it is below cov.
            d->s_cov[a * 16 + b] = std::max(d->s_cov[a * 16 + b], d->s_clash[a * 16 + b]);
            d->s_vdw[a * 16 + b] = std::max(d->s_vdw[a * 16 + b], d->s_cov[a * 16 + b]);
        }
        d->s_hacc[a] = bound_le(p.h_vdw_radius + p.vdw_radius[a] + c);  // hbond.rs:54
    }
    d->s_cov_max = 0.0;
    for (int k = 0; k < 256; k++) d->s_cov_max = std::max(d->s_cov_max, d->s_cov[k]);  // (s_cov >= s_clash after the clamp above)
    d->r2f = (float)d->r2;
    d->strip_force = g_debug.strip_rows > 0 ? (uint32_t)g_debug.strip_rows : 0u;
    d->flags = p.flags;
}

}  // namespace arp

using namespace arp;

// ---- context -------------------------------------------------------------------------------------------------
arp_status arp::check_device(arp_context *ctx) {
    if (!ctx) { set_error("null context"); return ARP_ERR_BAD_INPUT; }
    HIP_TRY(hipSetDevice(ctx->device));
    return ARP_OK;
}

template <typename T>
static arp_status dev_alloc(arp_context *ctx, T **p, size_t count) {
    void *q = nullptr;
    HIP_TRY(hipMalloc(&q, std::max<size_t>(count, 1) * sizeof(T)));
    ctx->ws_allocs.push_back(q);
    *p = (T *)q;
    return ARP_OK;
}

static void free_workspace(arp_context *ctx) {
    ctx->grid_x = nullptr; ctx->grid_n = 0; ctx->params_on_device = nullptr;
    for (void *p : ctx->ws_allocs) (void)hipFree(p);
    ctx->ws_allocs.clear();
    ctx->ws = Workspace{};
}

arp_status arp::ensure_workspace(arp_context *ctx, uint64_t n) {
    Workspace &w = ctx->ws;
    if (w.n_cap >= n && w.grid) return ARP_OK;
    if (n >= 0xFFFFFFF0ull) { set_error("too many atoms for 32-bit indices"); return ARP_ERR_BAD_INPUT; }
    (void)hipStreamSynchronize(ctx->stream);
    free_workspace(ctx);
    uint64_t cap = std::max<uint64_t>(n + n / 8, 1024);
    uint64_t ccap = std::min<uint64_t>(8 * cap + 65536, 0xFFFFFFF0ull);  // (a multiple of four either way: k_scan_single reads cell_count in whole 16-byte words, scan.inl scan_tile_load)
    arp_status s = ARP_OK;
    auto A = [&](auto &ptr, size_t cnt) { if (s == ARP_OK) s = dev_alloc(ctx, &ptr, cnt); };  // (after a failure the rest is skipped)
    A(w.partials, 1024 * 8); A(w.tickets, 4); A(w.grid, 1); A(w.params, 1);
    A(w.cell_of_atom, cap); A(w.rank_of_atom, cap); A(w.cell_count, ccap + 1); A(w.cell_start, ccap + 1);
    A(w.perm, cap); A(w.slot_cell, cap);
    A(w.sorted.rec, cap + 64); A(w.sorted.fat, cap + 64); A(w.sorted.rkey, cap + 64);
    A(w.task_count, cap / 64 + 2); A(w.task_base, cap / 64 + 2);
    A(w.scan_tmp, 1024 + 1); A(w.scan_tmp64, 1024 + 1); A(w.result, 32 + 1024);  // scan_tmp*: >= kScanBlocks + 1; result: 32 words (kRes*, kSasaTestsWord) + the kScanBlocks chunk totals of k_scan_single
    A(w.hole_list, 2048); A(w.task_ctr, kTaskCtrWords); w.scratch_cap = emit_scratch_records(); A(w.scratch, w.scratch_cap);
    A(w.model_box, 65536u * 6u); A(w.model_org, 65536u * 6u);
    w.defer_cap = (uint64_t)ctx->defer_scale * std::max<uint64_t>(16 * cap, 1u << 20) + (1u << 20);  // + one partly used 512-entry chunk per block
    if (g_debug.defer_entries > 0) w.defer_cap = (uint64_t)ctx->defer_scale * (uint64_t)g_debug.defer_entries;  // tests: a tiny list, so that the grow-and-repeat path runs
    A(w.defer_list, w.defer_cap);
    if (s != ARP_OK) { free_workspace(ctx); return s; }
    w.n_cap = (uint32_t)cap;
    w.ncells_cap = (uint32_t)ccap;
    {   // Every pointer a kernel may dereference must exist before the first launch.  (Round 1 recorded one GPU fault "on address
        // (nil)": an intermediate build launched k_bounds with the then-new `partials` member not yet allocated here.  A member
        // added to Workspace without its allocation now fails this check on the host instead of faulting on the device.)
        const void *members[] = {w.partials, w.tickets, w.grid, w.params, w.cell_of_atom, w.rank_of_atom, w.cell_count, w.cell_start, w.perm, w.slot_cell,
                                 w.sorted.rec, w.sorted.fat, w.sorted.rkey, w.task_count, w.task_base, w.scan_tmp, w.scan_tmp64, w.result, w.hole_list, w.scratch,
                                 w.task_ctr, w.defer_list, w.model_box, w.model_org};
        for (const void *m : members)
            if (!m) { free_workspace(ctx); set_error("internal error: a workspace member was not allocated"); return ARP_ERR_HIP; }
    }
    // self-cleaning state: the kernels leave these zeroed for the next call
    HIP_TRY(hipMemsetAsync(w.cell_count, 0, (ccap + 1) * sizeof(uint32_t), ctx->stream));
    HIP_TRY(hipMemsetAsync(w.tickets, 0, 4 * sizeof(uint32_t), ctx->stream));
    return ARP_OK;
}

extern "C" arp_status arp_context_create(int32_t device, arp_context **out) try {
    if (!out) { set_error("null out"); return ARP_ERR_BAD_INPUT; }
    *out = nullptr;
    int cnt = arp_device_count();
    if (cnt <= 0) { set_error("no gfx950 (MI355X) device visible; this engine has no CPU fallback"); return ARP_ERR_NO_DEVICE; }
    if (device < 0 || device >= cnt) { set_error("device %d out of range (0..%d)", device, cnt - 1); return ARP_ERR_NO_DEVICE; }
    arp_context *ctx = new arp_context();
    ctx->device = device;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipHostMalloc((void **)&ctx->h_params, sizeof(DevParams), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc((void **)&ctx->h_result, kHostResultWords * sizeof(unsigned long long), hipHostMallocDefault);
    if (e != hipSuccess) {
        set_error("HIP error %d (%s) creating the context", (int)e, hipGetErrorString(e));
        arp_context_destroy(ctx);
        return ARP_ERR_HIP;
    }
    ctx->stream = ctx->own_stream;
    *out = ctx;
    return ARP_OK;
} ARP_ABI_CATCH

static void free_staged(arp_context *ctx) {
    auto &s = ctx->st;
    if (ctx->nodefer_x == (const double *)s.dev) { ctx->nodefer_x = nullptr; ctx->nodefer_n = 0; }  // (a memo must not outlive the buffer it names)
    if (s.dev) (void)hipFree(s.dev);
    if (s.pinned) (void)hipHostFree(s.pinned);
    s = arp_context::Staged{};
}

// The context's buffers only ever grow: the stream is drained, the old block freed, the new one allocated (the capacity stays 0 if that fails).
arp_status arp::regrow(arp_context *ctx, void **p, uint64_t *cap, uint64_t want, uint64_t bytes, bool pinned) {
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (*p) (void)(pinned ? hipHostFree(*p) : hipFree(*p));
    *p = nullptr; *cap = 0;
    HIP_TRY(pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes));
    *cap = want;
    return ARP_OK;
}
arp_status arp::regrow_staged(arp_context *ctx, uint64_t cap) {  // the staging pair of the inputs: a device block and its pinned twin
    (void)hipStreamSynchronize(ctx->stream);
    free_staged(ctx);
    HIP_TRY(hipMalloc((void **)&ctx->st.dev, cap));
    HIP_TRY(hipHostMalloc((void **)&ctx->st.pinned, cap, hipHostMallocDefault));
    ctx->st.bytes = cap;
    return ARP_OK;
}

extern "C" void arp_context_destroy(arp_context *ctx) {
    if (!ctx) return;
    if (ctx->peer) { arp_context_destroy(ctx->peer); ctx->peer = nullptr; }
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    free_workspace(ctx);
    free_staged(ctx);
    if (ctx->out_buf) (void)hipFree(ctx->out_buf);
    for (int k = 0; k < 2; k++) { if (ctx->scr_dev[k]) (void)hipFree(ctx->scr_dev[k]); if (ctx->scr_pin[k]) (void)hipHostFree(ctx->scr_pin[k]); }
    if (ctx->grp_buf) (void)hipFree(ctx->grp_buf);
    if (ctx->h_offsets) (void)hipHostFree(ctx->h_offsets);
    for (int k = 0; k < 2; k++) { if (ctx->bounce[k]) (void)hipHostFree(ctx->bounce[k]); if (ctx->bounce_ev[k]) (void)hipEventDestroy(ctx->bounce_ev[k]); }
    if (ctx->params_ev) (void)hipEventDestroy(ctx->params_ev);
    if (ctx->h_params) (void)hipHostFree(ctx->h_params);
    if (ctx->h_result) (void)hipHostFree(ctx->h_result);
    if (ctx->prof.created) for (int k = 0; k < Profiler::kMax; k++) { (void)hipEventDestroy(ctx->prof.ev0[k]); (void)hipEventDestroy(ctx->prof.ev1[k]); }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

extern "C" arp_status arp_context_set_stream(arp_context *ctx, void *hip_stream) {
    arp_status s = check_device(ctx);
    if (s != ARP_OK) return s;
    (void)hipStreamSynchronize(ctx->stream);
    ctx->stream = (hipStream_t)hip_stream;
    return ARP_OK;
}

extern "C" arp_status arp_context_synchronize(arp_context *ctx) {
    arp_status s = check_device(ctx);
    if (s != ARP_OK) return s;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return ARP_OK;
}

// ---- input handling -------------------------------------------------------------------------------------------
static arp_status validate(const arp_atoms *a, const arp_params *p) {
    if (!a || !p) { set_error("null atoms/params"); return ARP_ERR_BAD_INPUT; }
    if (a->n >= 0xFFFFFFF0ull) { set_error("too many atoms"); return ARP_ERR_BAD_INPUT; }
    if (a->n && (!a->x || !a->y || !a->z || !a->attr || !a->res_ord || !a->chain_rank || !a->model)) { set_error("null atom array"); return ARP_ERR_BAD_INPUT; }
    if (a->n_res && (!a->res_id || !a->res_h_ptr || !a->res_cb || !a->res_sg)) { set_error("null residue table"); return ARP_ERR_BAD_INPUT; }
    if (a->n_res >= 0xFFFFFFF0ull) { set_error("too many residues"); return ARP_ERR_BAD_INPUT; }
    if (a->location != ARP_MEM_HOST && a->location != ARP_MEM_DEVICE) { set_error("bad location"); return ARP_ERR_BAD_INPUT; }
    if (std::isnan(p->dist_cutoff) || std::isnan(p->vdw_comp)) { set_error("NaN parameter"); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}

arp_status arp::stage_inputs(arp_context *ctx, const arp_atoms *a, DevAtoms *d) {
    d->n = (uint32_t)a->n;
    d->n_res = (uint32_t)a->n_res;
    if (a->location == ARP_MEM_DEVICE) {
        d->x = a->x; d->y = a->y; d->z = a->z; d->attr = a->attr; d->res_ord = a->res_ord; d->chain_rank = a->chain_rank; d->model = a->model;
        d->res_id = a->res_id; d->res_h_ptr = a->res_h_ptr; d->res_h_idx = a->res_h_idx; d->res_cb = a->res_cb; d->res_sg = a->res_sg;
        return ARP_OK;
    }
    auto &s = ctx->st;
    uint64_t nh = 0;
    if (a->n_res) nh = a->res_h_ptr[a->n_res];
    if (nh && !a->res_h_idx) { set_error("null res_h_idx"); return ARP_ERR_BAD_INPUT; }
    // layout of the block: 256-byte aligned segments
    struct Seg { const void *src; uint64_t bytes, off; };
    const uint64_t n = a->n, nr = a->n_res;
    Seg seg[12] = {{a->x, n * 8, 0}, {a->y, n * 8, 0}, {a->z, n * 8, 0}, {a->attr, n * 4, 0}, {a->res_ord, n * 4, 0}, {a->chain_rank, n * 4, 0},
                   {a->model, n * 4, 0}, {nr ? a->res_id : nullptr, nr ? n * 4 : 0, 0}, {nr ? a->res_h_ptr : nullptr, nr ? (nr + 1) * 4 : 0, 0},
                   {nr ? a->res_cb : nullptr, nr * 4, 0}, {nr ? a->res_sg : nullptr, nr * 4, 0}, {nh ? a->res_h_idx : nullptr, nh * 4, 0}};
    Carver lay;
    for (Seg &g : seg) g.off = lay.take(g.bytes);
    const uint64_t total = std::max<uint64_t>(lay.off, 256);
    arp_status rs;
    if (s.bytes < total && (rs = regrow_staged(ctx, total + total / 8)) != ARP_OK) return rs;
    for (const Seg &g : seg) if (g.bytes) memcpy(s.pinned + g.off, g.src, g.bytes);
    HIP_TRY(hipMemcpyAsync(s.dev, s.pinned, total, hipMemcpyHostToDevice, ctx->stream));
    // The deferred-pass memo identifies an input by (x pointer, n): for host inputs that pointer is THIS staging buffer, whatever structure it
    // carries -- every host call of the same size would hit, and a stale hit costs a whole second pass.  Host inputs never use the memo.
    ctx->nodefer_x = nullptr; ctx->nodefer_n = 0;
    auto at = [&](int k) -> const void * { return s.dev + seg[k].off; };
    d->x = (const double *)at(0); d->y = (const double *)at(1); d->z = (const double *)at(2);
    d->attr = (const uint32_t *)at(3); d->res_ord = (const uint32_t *)at(4);
    d->chain_rank = (const uint32_t *)at(5); d->model = (const uint32_t *)at(6);
    d->res_id = (const uint32_t *)at(7); d->res_h_ptr = (const uint32_t *)at(8); d->res_cb = (const uint32_t *)at(9); d->res_sg = (const uint32_t *)at(10);
    d->res_h_idx = (const uint32_t *)at(11);
    return ARP_OK;
}

arp_status arp::upload_params(arp_context *ctx, const arp_params *p) {
    // The device copy is uploaded when the parameters (or the workspace it lives in) change, not per call: the three fields a call derives
    // from its input (DevParams::r2, r2f, s_cov_max) are rewritten by every call's grid sizing from fields that nothing on the device writes.
    if (!ctx->have_params || memcmp(&ctx->last_params, p, sizeof *p) != 0) {
        // the pinned block may still be in flight from the previous upload: wait for THAT copy (an event behind it), not for the stream -- a batch
        // whose flags differ from the previous call's used to drain the 52 MB input copy it had just queued (~1 ms per pack, profiles/r05_experiments.txt)
        if (ctx->params_ev_armed) HIP_TRY(hipEventSynchronize(ctx->params_ev));
        make_dev_params(*p, ctx->h_params);
        ctx->last_params = *p;
        ctx->have_params = true;
        ctx->params_on_device = nullptr;
    }
    if (ctx->params_on_device != ctx->ws.params || ctx->params_stream != ctx->stream) {
        HIP_TRY(hipMemcpyAsync(ctx->ws.params, ctx->h_params, sizeof(DevParams), hipMemcpyHostToDevice, ctx->stream));
        if (!ctx->params_ev) HIP_TRY(hipEventCreateWithFlags(&ctx->params_ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(ctx->params_ev, ctx->stream));
        ctx->params_ev_armed = true;
        ctx->params_on_device = ctx->ws.params; ctx->params_stream = ctx->stream;
    }
    return ARP_OK;
}

// ---- device -> host of a large pair list ------------------------------------------------------------------------------
// hipMemcpy into freshly malloc'd pageable memory runs at ~2 GB/s (page faults + the runtime's staging); a 460 MB list took
// 230 ms.  Here the pages are populated by helper threads (MADV_POPULATE_WRITE, huge pages where the kernel grants them)
// while the list streams through two pinned 16 MB bounce buffers.
static arp_pair *download_pairs(arp_context *ctx, const arp_pair *dev, unsigned long long total, arp_status *status) {
    const size_t bytes = (size_t)total * sizeof(arp_pair);
    *status = ARP_OK;
    constexpr size_t kBounce = 16u << 20;
    if (bytes < 4 * kBounce) {
        arp_pair *host = (arp_pair *)malloc(bytes);
        if (!host) { set_error("out of host memory"); *status = ARP_ERR_OOM; return nullptr; }
        hipError_t e = hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { free(host); set_error("HIP error %d copying pairs to the host", (int)e); *status = ARP_ERR_HIP; return nullptr; }
        return host;
    }
    const size_t kHuge = 2u << 20;
    char *host = (char *)aligned_alloc(kHuge, (bytes + kHuge - 1) / kHuge * kHuge);
    if (!host) { set_error("out of host memory"); *status = ARP_ERR_OOM; return nullptr; }
#ifdef MADV_HUGEPAGE
    (void)madvise(host, bytes, MADV_HUGEPAGE);
#endif
    const int n_pop = 4;
    std::vector<std::thread> pop;
    for (int t = 0; t < n_pop; t++) try {
        pop.emplace_back([=]() {
            const size_t lo = bytes / n_pop * t / 4096 * 4096, hi = (t + 1 == n_pop) ? bytes : bytes / n_pop * (t + 1) / 4096 * 4096;
#ifdef MADV_POPULATE_WRITE
            if (madvise(host + lo, hi - lo, MADV_POPULATE_WRITE) == 0) return;
#endif
            (void)lo; (void)hi;  // older kernels: the copy below faults the pages in
        });
    } catch (const std::system_error &) { break; }  // no helper thread: the copy faults the pages in itself
    bool have_bounce = ctx->bounce[0] && ctx->bounce[1] && ctx->bounce_ev[0] && ctx->bounce_ev[1];
    if (!have_bounce) {  // all four handles or none: a half-built set would hand null buffers to later calls
        have_bounce = true;
        for (int k = 0; k < 2 && have_bounce; k++)
            have_bounce = hipHostMalloc((void **)&ctx->bounce[k], kBounce, hipHostMallocDefault) == hipSuccess &&
                          hipEventCreateWithFlags(&ctx->bounce_ev[k], hipEventDisableTiming) == hipSuccess;
        if (!have_bounce) {
            (void)hipGetLastError();
            for (int k = 0; k < 2; k++) {
                if (ctx->bounce[k]) (void)hipHostFree(ctx->bounce[k]);
                if (ctx->bounce_ev[k]) (void)hipEventDestroy(ctx->bounce_ev[k]);
                ctx->bounce[k] = nullptr; ctx->bounce_ev[k] = nullptr;
            }
        }
    }
    if (!have_bounce) {  // no pinned staging: the plain copy still works, only slower
        const hipError_t e = hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost);
        for (auto &t : pop) t.join();
        if (e != hipSuccess) { free(host); set_error("HIP error %d copying pairs to the host", (int)e); *status = ARP_ERR_HIP; return nullptr; }
        return (arp_pair *)host;
    }
    hipError_t e = hipSuccess;
    const size_t n_chunks = (bytes + kBounce - 1) / kBounce;
    for (size_t c = 0; c <= n_chunks && e == hipSuccess; c++) {
        if (c < n_chunks) {
            const size_t off = c * kBounce, len = std::min(kBounce, bytes - off);
            e = hipMemcpyAsync(ctx->bounce[c & 1], (const char *)dev + off, len, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipEventRecord(ctx->bounce_ev[c & 1], ctx->stream);
        }
        if (c > 0 && e == hipSuccess) {  // drain the previous chunk while this one is in flight
            const size_t off = (c - 1) * kBounce, len = std::min(kBounce, bytes - off);
            e = hipEventSynchronize(ctx->bounce_ev[(c - 1) & 1]);
            if (e == hipSuccess) memcpy(host + off, ctx->bounce[(c - 1) & 1], len);
        }
    }
    for (auto &t : pop) t.join();
    if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); free(host); set_error("HIP error %d copying pairs to the host", (int)e); *status = ARP_ERR_HIP; return nullptr; }
    return (arp_pair *)host;
}

// The deferred-probe list (candidates whose rules need a hydrogen / disulfide probe) is sized for 16 candidates per atom; a
// denser input overflows it (status bit 8).  Like the pair buffer, it is then grown and the pass repeated.
static arp_status grow_defer_list(arp_context *ctx, uint64_t n) {
    if (ctx->defer_scale >= 64) { set_error("deferred-probe list overflow after growing it 64-fold"); return ARP_ERR_CAPACITY; }
    ctx->defer_scale *= 4;
    (void)hipStreamSynchronize(ctx->stream);
    free_workspace(ctx);
    return ensure_workspace(ctx, n);
}

// ---- the pair pass ---------------------------------------------------------------------------------------------
// One protocol for every caller (PairPass, engine.h): the callers differ in what they put into the PairPass and in how they grow their pair buffer.
void arp::mark_grid_owner(arp_context *ctx, const double *x, uint64_t n, bool rkey_valid, uint32_t narrow_ib) {
    ctx->grid_x = x; ctx->grid_n = n; ctx->rkey_valid = rkey_valid; ctx->narrow_ib = narrow_ib;
}
void arp::mark_grid_foreign(arp_context *ctx) {
    mark_grid_owner(ctx, nullptr, 0, false);  // the workspace's cell list holds another input (context_grid must not hand it out)
    ctx->nodefer_x = nullptr; ctx->nodefer_n = 0;
}

// The emit plan of a pass (emit_plan.h), made here and nowhere else.  THE INVARIANT: the cell list holds what the plan's kernels read -- residue words
// (Sorted::rkey) if plan.res, the narrow exact record (Xrec) with plan.narrow_ib index bits if that is not 0, else the wide one (Fat).
// A pass that builds its list (p.grid) plans freely and pass_issue has k_place write exactly that: narrow_ok when the single-pass emitter is the list's
// one reader (an Emit pass nobody walks the records after) -- k_place then scatters three 16-byte parts per atom instead of four, k_emit gathers two per
// survivor instead of three.  A pass on a list that stands plans under the format the context recorded for it (mark_grid_owner): it may use the residue
// words only if they are there (plan.res implies res_wanted), and a route that reads another exact record than the list's is refused.
static arp_status plan_pass(arp_context *ctx, const PairPass &p, bool ordered, EmitPlan *plan) {
    const uint32_t flags = p.params->flags;
    EmitQuery q;
    q.n = p.d.n; q.per_model = p.d.per_model != 0u; q.ordered = ordered; q.contacts_only = (flags & ARP_FLAG_CONTACTS_ONLY) != 0; q.skip_deferred = p.skip;
    q.scratch_cap = ctx->ws.scratch_cap; q.knob_emit_kernel = g_debug.emit_kernel;
    if (p.grid) {
        q.res_wanted = (flags & ARP_FLAG_RESIDUE_RUNS) ? true : ((flags & ARP_FLAG_NO_RESIDUE_RUNS) ? false : ctx->res_hint);
        q.narrow_ok = p.mode == PairPass::Emit && !p.wide_record; q.knob_index_bits = g_debug.index_bits;
    } else { q.res_wanted = ctx->rkey_valid; q.narrow_ok = ctx->narrow_ib != 0u; q.knob_index_bits = (int)ctx->narrow_ib; }
    *plan = plan_emit(q);
    if (!p.grid && plan->narrow_ib != ctx->narrow_ib) { set_error("internal error: the emit plan reads another exact record than the cell list holds"); return ARP_ERR_HIP; }
    return ARP_OK;
}

arp_status arp::pass_issue(arp_context *ctx, PairPass &p) {
    const bool ordered = (p.params->flags & ARP_FLAG_DETERMINISTIC) != 0, only = (p.params->flags & ARP_FLAG_CONTACTS_ONLY) != 0;
    Profiler *prof = p.profile ? context_profiler(ctx) : nullptr;
    p.skip = p.direct = p.collected = false;
    const bool emit = p.mode == PairPass::Emit;
    if (emit) p.skip = p.speculate && p.d.x != nullptr && ctx->nodefer_x == p.d.x && ctx->nodefer_n == p.d.n;  // the memo names this input
    arp_status s;
    EmitPlan plan{};
    if ((p.grid || emit) && (s = plan_pass(ctx, p, ordered, &plan)) != ARP_OK) return s;
    if (p.grid) {  // builds the cell list as the plan reads it and records whose it is (a pack's grid, per-model origins, is nobody's)
        launch_grid(p.d, ctx->ws, ctx->stream, prof, p.params->dist_cutoff, ordered, plan.res, plan.narrow_ib);
        mark_grid_owner(ctx, p.d.per_model ? nullptr : p.d.x, p.d.per_model ? 0 : p.d.n, plan.res, plan.narrow_ib);
    }
    if (p.mode == PairPass::Count) {
        // (with ARP_FLAG_CONTACTS_ONLY the count that sizes the single-pass emitter's buffer is the cheap candidate count; the ordered fill needs the exact one)
        launch_count(p.d, ctx->ws, ctx->stream, prof, p.capacity, p.have_out, p.have_out ? only : only && ordered);
    } else if (p.mode == PairPass::OrderedFill) {
        if (p.grid) launch_count(p.d, ctx->ws, ctx->stream, prof, p.capacity, true, only);
        launch_fill_ordered(p.d, ctx->ws, p.out, p.capacity, ctx->stream, prof, only);
    } else {
        if ((s = launch_emit(p.d, ctx->ws, p.out, p.capacity, ctx->stream, prof, plan)) != ARP_OK) return s;
        p.direct = plan.route == EmitRoute::Direct || plan.route == EmitRoute::Stage;  // hole-free: the host derives the count (finish_result)
    }
    if (p.between && (s = p.between(ctx, p, p.between_arg)) != ARP_OK) return s;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctx->h_result, ctx->ws.result, kResultWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    return ARP_OK;
}

// After the result words of a pass have arrived.  The hole-free sequences (the plan's route was Direct or Stage) have no fix-up kernel to
// publish the pair count and the flags that depend on it: the records lie back to back from position 0 and kResEmitHead counts them; its
// probes run inline, so kResDeferred (the chunks of a deferred list) stays 0 (the input-error flags were set by the grid sizing).
static void finish_result(arp_context *ctx, bool direct, bool skipped, unsigned long long capacity) {
    unsigned long long *r = ctx->h_result;
    if (!direct) return;
    r[kResPairs] = r[kResEmitHead];
    if (r[kResPairs] > capacity) r[kResFlags] |= kStatCapacity;                  // the list did not fit (k_fixup: P > capacity)
    if (skipped && r[kResDeferred] != 0ull) r[kResFlags] |= kStatStaleSkip;      // the probe pass was skipped on a memo that no longer holds
}
constexpr unsigned long long kResRunsMin = 64;  // of the 255 atoms k_place samples
static void note_residue_runs(arp_context *ctx) { ctx->res_hint = ctx->h_result[kResResRuns] >= kResRunsMin; }
// the deferred-pass memo after a single-pass (emit) call
static void note_deferred(arp_context *ctx, const DevAtoms &d, bool skipped) {
    if (ctx->st.dev && d.x == (const double *)ctx->st.dev) return;  // host input staged by the context: no memo (stage_inputs)
    const unsigned long long *r = ctx->h_result;
    if (skipped) { if (r[kResFlags] & kStatStaleSkip) { ctx->nodefer_x = nullptr; ctx->nodefer_n = 0; } return; }
    if (r[kResDeferred] == 0ull && !(r[kResFlags] & ~kStatCapacity)) { ctx->nodefer_x = d.x; ctx->nodefer_n = d.n; }
    else if (ctx->nodefer_x == d.x) { ctx->nodefer_x = nullptr; ctx->nodefer_n = 0; }
}
constexpr arp_status kRetryDeferPass = -2;  // internal: the deferred pass was skipped on a memo that no longer holds
static arp_status flags_to_status(unsigned long long flags) {
    if (flags & kStatStaleSkip) return kRetryDeferPass;
    if (flags & kStatNonFinite) { set_error("non-finite atom coordinate"); return ARP_ERR_BAD_INPUT; }
    if (flags & kStatSparseModels) { set_error("model ordinals must be dense: the largest model id exceeds what the workspace of this input holds (model ids count 0, 1, 2, ...)"); return ARP_ERR_BAD_INPUT; }
    if (flags & kStatHolePlan) { set_error("internal error: inconsistent hole plan in k_fixup"); return ARP_ERR_HIP; }
    if (flags & kStatCysNoCb) { set_error("CYS SG..SG covalent pair whose residue has no CB (the reference panics in is_disulfide, vdw.rs:58)"); return ARP_ERR_BAD_INPUT; }
    if (flags & kStatDeferOverflow) return kRetryDefer;  // the deferred-probe list overflowed: pass_finish grows it and repeats the pass
    return ARP_OK;
}
static arp_status pass_collect(arp_context *ctx, PairPass &p) {
    finish_result(ctx, p.direct, p.skip, p.capacity);
    note_residue_runs(ctx);
    if (p.memo) note_deferred(ctx, p.d, p.skip);
    p.collected = true;
    return flags_to_status(ctx->h_result[kResFlags]);
}

arp_status arp::pass_finish(arp_context *ctx, PairPass &p, arp_status (*reissue)(arp_context *, PairPass &)) {
    for (;;) {
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        arp_status s = pass_collect(ctx, p);
        if (s == kRetryDefer && (p.max_reissues < 0 || p.reissues < p.max_reissues)) {
            p.collected = false;  // like a pair buffer: grow the list, repeat the pass.  The workspace is a new one: parameters and cell list go there again
            if ((s = grow_defer_list(ctx, p.d.n)) != ARP_OK || (s = upload_params(ctx, p.params)) != ARP_OK) return s;
            p.grid = true;
        } else if (s != kRetryDeferPass) return s;  // (kRetryDeferPass: the memo was stale, note_deferred has dropped it -- once more, with the probe pass)
        p.reissues++;
        if ((s = reissue(ctx, p)) != ARP_OK) return s;
    }
}

// ---- the hot path ----------------------------------------------------------------------------------------------
extern "C" arp_status arp_contacts_atomic_enqueue(arp_context *ctx, const arp_atoms *atoms, const arp_params *params, arp_pair *out,
                                                  uint64_t capacity) try {
    arp_status s = check_device(ctx);
    if (s != ARP_OK) return s;
    if ((s = validate(atoms, params)) != ARP_OK) return s;
    if (atoms->location != ARP_MEM_DEVICE) { set_error("arp_contacts_atomic_enqueue needs device-resident inputs"); return ARP_ERR_BAD_INPUT; }
    if (!out && capacity) { set_error("null output buffer"); return ARP_ERR_BAD_INPUT; }
    if ((s = ensure_workspace(ctx, atoms->n)) != ARP_OK) return s;
    DevAtoms d{};
    if ((s = stage_inputs(ctx, atoms, &d)) != ARP_OK) return s;
    if ((s = upload_params(ctx, params)) != ARP_OK) return s;
    // remembered with the context's copy of the parameters and the caller's device pointers (kept alive until arp_contacts_atomic_result): it may run again
    PairPass &p = ctx->enqueued;
    p = PairPass{d, &ctx->last_params, out, capacity, PairPass::Emit};
    if (!out || capacity == 0) p.mode = PairPass::Count;  // size query: reports ARP_ERR_CAPACITY + the count
    else if (params->flags & ARP_FLAG_DETERMINISTIC) p.mode = PairPass::OrderedFill;
    else { p.memo = true; p.speculate = !(params->flags & ARP_FLAG_NO_SPECULATION); }  // (only this entry point honours ARP_FLAG_NO_SPECULATION)
    if ((s = pass_issue(ctx, p)) != ARP_OK) return s;
    ctx->pending = true;
    return ARP_OK;
} ARP_ABI_CATCH

extern "C" arp_status arp_contacts_atomic_result(arp_context *ctx, uint64_t *n_pairs) try {
    arp_status s = check_device(ctx);
    if (s != ARP_OK) return s;
    if (!ctx->pending) { set_error("no enqueued call"); return ARP_ERR_BAD_INPUT; }
    ctx->pending = false;
    const PairPass &p = ctx->enqueued;
    s = pass_finish(ctx, ctx->enqueued);
    if (n_pairs && p.collected) *n_pairs = ctx->h_result[kResPairs];
    if (s != ARP_OK) return s;
    if (ctx->h_result[kResPairs] > p.capacity) { set_error("pair buffer too small: %llu pairs needed, capacity %llu", ctx->h_result[kResPairs], p.capacity); return ARP_ERR_CAPACITY; }
    return ARP_OK;
} ARP_ABI_CATCH

// Single-pass emitter into the context's reusable device buffer: ONE pass -- no count pass, no hipMalloc/hipFree per call (together
// ~half of the latency of a PDB-sized structure).  A buffer that turns out too small only makes the pass report the size (k_fixup);
// it is then grown and the pass repeated.  Leaves the list in ctx->out_buf[0 .. *total).
static arp_status single_pass_into_context_buffer(arp_context *ctx, const DevAtoms &d, const arp_params *params, unsigned long long *total_out, bool wide_record = false) {
    arp_status s;
    // first guess: 64 records per atom (twice the all-pairs density of a protein), at most 2 GiB; a larger result costs one more pass
    uint64_t want = std::max<uint64_t>(ctx->out_cap, std::min<uint64_t>(std::max<uint64_t>(64 * (uint64_t)d.n, 1u << 16), 1u << 27));
    for (int attempt = 0;; attempt++) {
        if (ctx->out_cap < want && (s = regrow(ctx, (void **)&ctx->out_buf, &ctx->out_cap, want, want * sizeof(arp_pair), false)) != ARP_OK) return s;
        PairPass p{d, params, ctx->out_buf, ctx->out_cap, PairPass::Emit};
        p.memo = p.speculate = true;  // (the synchronous paths use the memo whatever ARP_FLAG_NO_SPECULATION says)
        p.wide_record = wide_record;
        if ((s = pass_run(ctx, p)) != ARP_OK) return s;
        const unsigned long long total = *total_out = ctx->h_result[kResPairs];
        if (total <= ctx->out_cap) return ARP_OK;
        if (attempt) { set_error("internal error: pair count changed between passes"); return ARP_ERR_HIP; }
        want = total + total / 8;
    }
}

// The table path's pair pass (table_cache.cpp get_contacts_device): device-resident inputs, the list stays in the context's buffer --
// *data is a VIEW, valid until the next call on this context.
arp_status arp::contacts_atomic_view(arp_context *ctx, const arp_atoms *atoms, const arp_params *params, const arp_pair **data, uint64_t *n) {
    *data = nullptr; *n = 0;
    if (!atoms || atoms->location != ARP_MEM_DEVICE || !params || (params->flags & ARP_FLAG_DETERMINISTIC)) { set_error("contacts_atomic_view: bad arguments"); return ARP_ERR_BAD_INPUT; }
    arp_status s = check_device(ctx);
    if (s != ARP_OK) return s;
    if ((s = validate(atoms, params)) != ARP_OK) return s;
    if ((s = ensure_workspace(ctx, atoms->n)) != ARP_OK) return s;
    DevAtoms d{};
    if ((s = stage_inputs(ctx, atoms, &d)) != ARP_OK) return s;
    if ((s = upload_params(ctx, params)) != ARP_OK) return s;
    unsigned long long total = 0;
    const auto t0 = std::chrono::steady_clock::now();
    s = single_pass_into_context_buffer(ctx, d, params, &total, /* wide_record: the table path's ring walk reads Fat by slot (context_grid) */ true);
    if (g_debug.timing) fprintf(stderr, "    pair pass (launches + sync)      %8.3f ms\n", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    if (s != ARP_OK) return s;
    *data = ctx->out_buf; *n = total;
    return ARP_OK;
}

extern "C" arp_status arp_contacts_atomic(arp_context *ctx, const arp_atoms *atoms, const arp_params *params, int32_t out_location,
                                          arp_pairs *out) try {
    if (!out) { set_error("null out"); return ARP_ERR_BAD_INPUT; }
    out->n = 0; out->data = nullptr; out->location = out_location;
    arp_status s = check_device(ctx);
    if (s != ARP_OK) return s;
    if ((s = validate(atoms, params)) != ARP_OK) return s;
    if (out_location != ARP_MEM_HOST && out_location != ARP_MEM_DEVICE) { set_error("bad out_location"); return ARP_ERR_BAD_INPUT; }
    if ((s = ensure_workspace(ctx, atoms->n)) != ARP_OK) return s;
    DevAtoms d{};
    if ((s = stage_inputs(ctx, atoms, &d)) != ARP_OK) return s;
    if ((s = upload_params(ctx, params)) != ARP_OK) return s;
    const bool ordered = (params->flags & ARP_FLAG_DETERMINISTIC) != 0;
    unsigned long long total = 0;
    arp_pair *dev = ctx->out_buf, *own = nullptr;  // own: the list's own device buffer (device output, or the ordered fill), sized by a count pass
    if (out_location == ARP_MEM_HOST && !ordered) {
        if ((s = single_pass_into_context_buffer(ctx, d, params, &total)) != ARP_OK) return s;
        dev = ctx->out_buf;
    } else {
        // count pass -> output size -> ordered fill or single-pass emit on the count pass's cell list.  Neither consults nor updates the memo.
        PairPass p{d, params, nullptr, 0, PairPass::Count};
        p.have_out = false;
        if ((s = pass_run(ctx, p)) != ARP_OK) return s;
        if ((total = ctx->h_result[kResPairs]) == 0) return ARP_OK;
        HIP_TRY(hipMalloc((void **)&own, total * sizeof(arp_pair)));
        p.mode = ordered ? PairPass::OrderedFill : PairPass::Emit;
        p.out = dev = own; p.capacity = total; p.grid = false;
        if ((s = pass_run(ctx, p)) != ARP_OK) { (void)hipFree(own); return s; }
        total = std::min<unsigned long long>(total, ctx->h_result[kResPairs]);  // fewer than the candidates with ARP_FLAG_CONTACTS_ONLY
    }
    if (total == 0) { if (own) (void)hipFree(own); return ARP_OK; }
    if (out_location == ARP_MEM_DEVICE) {
        out->data = own; out->n = total;
        return ARP_OK;
    }
    arp_pair *host = download_pairs(ctx, dev, total, &s);
    if (own) (void)hipFree(own);
    if (!host) return s;
    out->data = host; out->n = total;
    return ARP_OK;
} ARP_ABI_CATCH

// ---- accessors for the table path (table_dev.hip) ---------------------------------------------------------------------------
namespace arp {
void *context_stream(arp_context *ctx) { return (void *)ctx->stream; }
int context_device(arp_context *ctx) { return ctx->device; }
bool context_grid(arp_context *ctx, const double *x, uint64_t n, const GridParams **grid, const uint32_t **cell_start, const Fat **fat) {
    if (!ctx || ctx->pending || !ctx->ws.grid || !x || ctx->grid_x != x || ctx->grid_n != n || ctx->narrow_ib != 0u) return false;
    *grid = ctx->ws.grid; *cell_start = ctx->ws.cell_start; *fat = ctx->ws.sorted.fat;
    return true;
}
arp_status context_sc(arp_context *ctx, bool call, hipStream_t *st, Profiler **prof, std::vector<ScDot> **dots) {
    arp_status s = check_device(ctx);
    if (s != ARP_OK) return s;
    if (ctx->pending) { set_error("a call enqueued on this context has not been collected (arp_contacts_atomic_result)"); return ARP_ERR_BAD_INPUT; }
    *st = ctx->stream;
    *prof = ctx->prof.enabled ? &ctx->prof : nullptr;
    if (*prof && call) ctx->prof.n = 0;  // the timings of this call only
    *dots = ctx->sc_dots;
    return ARP_OK;
}
arp_status context_scratch(arp_context *ctx, int slot, uint64_t dev_bytes, uint64_t pinned_bytes, char **dev, char **pinned) {
    arp_status s = check_device(ctx);
    if (s != ARP_OK) return s;
    if (slot < 0 || slot > 1) { set_error("bad scratch slot"); return ARP_ERR_BAD_INPUT; }
    const uint64_t dev_cap = dev_bytes + dev_bytes / 4 + 4096, pin_cap = pinned_bytes + pinned_bytes / 4 + 4096;
    if (ctx->scr_dev_cap[slot] < dev_bytes && (s = regrow(ctx, (void **)&ctx->scr_dev[slot], &ctx->scr_dev_cap[slot], dev_cap, dev_cap, false)) != ARP_OK) return s;
    if (ctx->scr_pin_cap[slot] < pinned_bytes && (s = regrow(ctx, (void **)&ctx->scr_pin[slot], &ctx->scr_pin_cap[slot], pin_cap, pin_cap, true)) != ARP_OK) return s;
    *dev = ctx->scr_dev[slot]; *pinned = ctx->scr_pin[slot];
    return ARP_OK;
}
}  // namespace arp

// ---- profiling ---------------------------------------------------------------------------------------------------
extern "C" arp_status arp_profile_enable(arp_context *ctx, int32_t on) {
    arp_status s = check_device(ctx);
    if (s != ARP_OK) return s;
    ctx->prof.enabled = on != 0;
    ctx->prof.n = 0;
    return ARP_OK;
}
extern "C" int32_t arp_profile_read(arp_context *ctx, const char **names, float *ms, int32_t cap) {
    if (check_device(ctx) != ARP_OK) return 0;
    (void)hipStreamSynchronize(ctx->stream);
    int n = std::min<int>(ctx->prof.n, cap);
    for (int k = 0; k < n; k++) {
        names[k] = ctx->prof.names[k];
        float t = 0.f;
        (void)hipEventElapsedTime(&t, ctx->prof.ev0[k], ctx->prof.ev1[k]);
        ms[k] = t;
    }
    return n;
}

// ---- library-level -----------------------------------------------------------------------------------------------
namespace arp { DebugKnobs g_debug{}; }
extern "C" uint64_t arp_pair_rare_batches(const arp_context *ctx) { return (ctx && ctx->h_result) ? ctx->h_result[kResRare] : 0u; }

extern "C" arp_status arp_debug_set(const char *key, int64_t value) {
    if (!key) { set_error("null key"); return ARP_ERR_BAD_INPUT; }
    const std::string k(key);
    if (k == "timing") g_debug.timing = value != 0;
    else if (k == "emit_kernel") g_debug.emit_kernel = (int)value;
    else if (k == "defer_entries") g_debug.defer_entries = (long)value;
    else if (k == "table_host") g_debug.table_host = value != 0;
    else if (k == "freq_chunk_atoms") {
        if (value < 0) { set_error("arp_debug_set: freq_chunk_atoms takes 0 (automatic) or a positive atom count"); return ARP_ERR_BAD_INPUT; }
        g_debug.freq_chunk_atoms = (long)value;
    }
    else if (k == "freq_cap_items") {
        if (value < 0) { set_error("arp_debug_set: freq_cap_items takes 0 (automatic) or a positive item count"); return ARP_ERR_BAD_INPUT; }
        g_debug.freq_cap_items = (long)value;
    }
    else if (k == "freq_frame_bits") {
        if (value < 0 || value > 17) { set_error("arp_debug_set: freq_frame_bits takes 0 (automatic) or 1 .. 17"); return ARP_ERR_BAD_INPUT; }
        g_debug.freq_frame_bits = (long)value;
    }
    else if (k == "ens_chunk_atoms") {
        if (value < 0) { set_error("arp_debug_set: ens_chunk_atoms takes 0 (automatic) or a positive atom count"); return ARP_ERR_BAD_INPUT; }
        g_debug.ens_chunk_atoms = (long)value;
    }
    else if (k == "sc_ens_frames") {
        if (value < 0 || value > (1 << 20)) { set_error("arp_debug_set: sc_ens_frames takes 0 (automatic) or a frame count up to 2^20"); return ARP_ERR_BAD_INPUT; }
        g_debug.sc_ens_frames = (long)value;
    }
    else if (k == "timeline_cap_bytes") {
        if (value < 0) { set_error("arp_debug_set: timeline_cap_bytes takes 0 (2^31 bytes) or a positive byte count"); return ARP_ERR_BAD_INPUT; }
        g_debug.timeline_cap_bytes = (long long)value;
    }
    else if (k == "similarity_cap_bytes") {
        if (value < 0) { set_error("arp_debug_set: similarity_cap_bytes takes 0 (2^31 bytes) or a positive byte count"); return ARP_ERR_BAD_INPUT; }
        g_debug.similarity_cap_bytes = (long long)value;
    }
    else if (k == "autocorr_cap_bytes") {
        if (value < 0) { set_error("arp_debug_set: autocorr_cap_bytes takes 0 (2^31 bytes) or a positive byte count"); return ARP_ERR_BAD_INPUT; }
        g_debug.autocorr_cap_bytes = (long long)value;
    }
    else if (k == "cluster_cap_bytes") {
        if (value < 0) { set_error("arp_debug_set: cluster_cap_bytes takes 0 (2^31 bytes) or a positive byte count"); return ARP_ERR_BAD_INPUT; }
        g_debug.cluster_cap_bytes = (long long)value;
    }
    else if (k == "rmsd_chunk_atoms") {
        if (value < 0) { set_error("arp_debug_set: rmsd_chunk_atoms takes 0 (automatic) or a positive atom count"); return ARP_ERR_BAD_INPUT; }
        g_debug.rmsd_chunk_atoms = (long)value;
    }
    else if (k == "rmsd_cap_bytes") {
        if (value < 0) { set_error("arp_debug_set: rmsd_cap_bytes takes 0 (2^31 bytes) or a positive byte count"); return ARP_ERR_BAD_INPUT; }
        g_debug.rmsd_cap_bytes = (long long)value;
    }
    else if (k == "index_bits") {
        if (value > (int64_t)kNarrowMaxBits) { set_error("arp_debug_set: index_bits takes 0 (automatic), 1 .. 20 (the index width of the narrow exact record) or a negative value (the wide record always)"); return ARP_ERR_BAD_INPUT; }
        g_debug.index_bits = (int)value;
    }
    else if (k == "table_key_bits") {
        if (!table_key_bits_valid(value)) { set_error("arp_debug_set: table_key_bits takes 0 (64) or %d .. %d (no pass of the table sort is narrower than %d bits)", kTableMinKeyBits, kTableMaxKeyBits, kTableMinKeyBits); return ARP_ERR_BAD_INPUT; }
        g_debug.table_key_bits = (int)value;
    }
    else if (k == "strip_rows") {
        if (value < 0 || value > 1024 || (value & (value - 1)) != 0) { set_error("arp_debug_set: strip_rows takes 0 or a power of two up to 1024"); return ARP_ERR_BAD_INPUT; }
        g_debug.strip_rows = (int)value;
    }
    else if (k == "scan_kernel") {
        if (value < 0 || value > 2) { set_error("arp_debug_set: scan_kernel takes 0 (automatic), 1 (the look-back cell scan on 256 blocks) or 2 (on 1024 blocks)"); return ARP_ERR_BAD_INPUT; }
        g_debug.scan_kernel = (int)value;
    }
    else if (k == "torsion_hist2_route") {
        if (value < 0 || value > 3) { set_error("arp_debug_set: torsion_hist2_route takes 0 (automatic), 1 (LDS tables), 2 (wave-matched global adds) or 3 (one global add per sample)"); return ARP_ERR_BAD_INPUT; }
        g_debug.torsion_hist2_route = (int)value;
    }
    else { set_error("arp_debug_set: unknown key '%s' (timing, emit_kernel, defer_entries, strip_rows, index_bits, scan_kernel, table_host, freq_chunk_atoms, freq_cap_items, freq_frame_bits, ens_chunk_atoms, sc_ens_frames, timeline_cap_bytes, similarity_cap_bytes, autocorr_cap_bytes, cluster_cap_bytes, rmsd_chunk_atoms, rmsd_cap_bytes, table_key_bits, torsion_hist2_route)", key); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}
extern "C" arp_status arp_debug_get(const char *key, int64_t *value) {
    if (!key || !value) { set_error("arp_debug_get: null argument"); return ARP_ERR_BAD_INPUT; }
    const std::string k(key);
    const TableRoute r = table_route_last();
    if (k == "table_small") *value = r.small;
    else if (k == "table_pairs") *value = r.pairs;
    else if (k == "table_atom_rows") *value = r.atom_rows;
    else if (k == "table_ring_rows") *value = r.ring_rows;
    else if (k == "table_plan") *value = r.plan;
    else if (k == "table_long_way") *value = r.long_way;
    else if (k == "table_ring_cap") *value = r.ring_cap;
    else { set_error("arp_debug_get: unknown key '%s' (table_small, table_pairs, table_atom_rows, table_ring_rows, table_plan, table_long_way, table_ring_cap)", key); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}
extern "C" int32_t arp_api_version(void) { return ARP_API_VERSION; }
extern "C" arp_status arp_check_api_version(int32_t header_version) {
    if (header_version == ARP_API_VERSION) return ARP_OK;
    set_error("API version mismatch: the caller was compiled against version %d of arpeggia_amd.h, the library implements version %d "
              "(v2: arp_atoms.chain_rank and arp_atoms.model are uint32_t)", (int)header_version, (int)ARP_API_VERSION);
    return ARP_ERR_BAD_INPUT;
}
extern "C" const char *arp_last_error(void) { return g_err; }
extern "C" const char *arp_strerror(arp_status s) {
    switch (s) {
        case ARP_OK: return "ok";
        case ARP_ERR_BAD_GROUPS: return "Invalid chain groups format! Use '/' for all-to-all comparisons.";
        case ARP_ERR_EMPTY_GROUPS: return "Empty chain groups!";
        case ARP_ERR_NO_RINGS: return "Error building ring positions";
        case ARP_ERR_BAD_INPUT: return "bad input";
        case ARP_ERR_HIP: return "HIP runtime error";
        case ARP_ERR_OOM: return "out of memory";
        case ARP_ERR_NO_DEVICE: return "no gfx950 device (no CPU fallback)";
        case ARP_ERR_IO: return "I/O error";
        case ARP_ERR_CAPACITY: return "pair buffer too small";
        default: return "unknown status";
    }
}
extern "C" int32_t arp_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int ok = 0;
    for (int d = 0; d < n; d++) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, d) != hipSuccess) continue;
        if (strncmp(p.gcnArchName, "gfx950", 6) == 0) ok++;
        else return ok;  // devices are addressed by ordinal: stop at the first foreign one
    }
    return ok;
}
static const char *k_interactions[ARP_N_INTERACTIONS] = {
    "StericClash", "CovalentBond", "Disulfide", "VanDerWaalsContact", "IonicBond", "HydrogenBond", "WeakHydrogenBond",
    "PolarContact", "WeakPolarContact", "IonicRepulsion", "SaltBridge", "PiDisplacedStacking", "PiTStacking",
    "PiSandwichStacking", "PiParallelInPlaneStacking", "PiTiltedStacking", "PiLStacking", "CationPi", "HydrophobicContact"};
extern "C" const char *arp_interaction_name(int32_t code) {
    if (code == ARP_WaterBridge) return "WaterBridge";  // (a row code of the ensemble tables, not a bit of arp_pair.kind: outside the enum)
    return (code >= 0 && code < ARP_N_INTERACTIONS) ? k_interactions[code] : "?";
}
