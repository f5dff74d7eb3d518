// The batch path of the hot path (arp_contacts_atomic_batch): structures packed into shared launches, two packs in flight per device, and the
// pooled pinned blocks their pair lists land in (also handed to the table path: pinned_block).  The pair pass itself is engine.cpp's.
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <memory>
#include <numeric>
#include <unordered_map>

#include "engine.h"
#include "table_dev.h"

using namespace arp;

// ---- pair lists that share one pinned block (the batch path) --------------------------------------------------------------------
// A pack's pair list crosses PCIe once, into ONE pinned block, and every member's arp_pairs is a view into it: no per-member malloc, no
// second copy (~70 k records = 1.1 MB per 5k-atom structure with full candidate lists: crossing PCIe once is the floor of that path,
// ~20 us per structure).  The block is reference-counted through a registry keyed by the members' data pointers -- arp_pairs_free
// finds it there -- and an idle block goes back to a pool instead of to the driver: pinning memory costs far more than the copy it saves.
namespace {
struct SharedBlock { char *pinned = nullptr; size_t cap = 0; long refs = 0; };
std::mutex g_shared_mu;
std::unordered_map<const void *, SharedBlock *> g_shared_views;
std::vector<SharedBlock *> g_shared_pool;
size_t g_shared_pool_bytes = 0;
// idle pinned memory kept for the next batch / table: 4 GiB unless ARPEGGIA_AMD_HOST_POOL_MB says otherwise (0 = keep nothing).  (2 GiB was
// measured in round 4: a batch of 2048 five-thousand-atom structures with full candidate lists returns 2.3 GB of lists, the blocks beyond the
// limit were unpinned and pinned again on every call -- 24 -> 41 us per structure.)
const size_t kSharedPoolLimit = [] {
    const char *e = getenv("ARPEGGIA_AMD_HOST_POOL_MB");
    const long long mb = e ? atoll(e) : 4096;
    return (size_t)(mb < 0 ? 0 : mb) << 20;
}();

SharedBlock *shared_acquire(size_t bytes) {
    {
        std::lock_guard<std::mutex> lk(g_shared_mu);
        size_t best = g_shared_pool.size();
        for (size_t k = 0; k < g_shared_pool.size(); k++)
            // (the smallest pooled block that fits -- but not one more than twice the request + 1 MiB: a 1 KB table must not pin a multi-GB block
            // for as long as one of its views lives)
            if (g_shared_pool[k]->cap >= bytes && g_shared_pool[k]->cap <= 2 * bytes + (1u << 20) &&
                (best == g_shared_pool.size() || g_shared_pool[k]->cap < g_shared_pool[best]->cap)) best = k;
        if (best != g_shared_pool.size()) {
            SharedBlock *b = g_shared_pool[best];
            g_shared_pool.erase(g_shared_pool.begin() + (long)best);
            g_shared_pool_bytes -= b->cap;
            return b;
        }
    }
    SharedBlock *b = new (std::nothrow) SharedBlock();
    if (!b) return nullptr;
    const size_t cap = bytes + bytes / 8 + 4096;
    if (hipHostMalloc((void **)&b->pinned, cap, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); delete b; return nullptr; }
    b->cap = cap;
    return b;
}
void shared_release(SharedBlock *b) {  // (g_shared_mu held)
    if (g_shared_pool_bytes + b->cap <= kSharedPoolLimit) { g_shared_pool.push_back(b); g_shared_pool_bytes += b->cap; return; }
    (void)hipHostFree(b->pinned);
    delete b;
}
}  // namespace

std::shared_ptr<char> arp::pinned_block(size_t bytes) {
    SharedBlock *b = shared_acquire(bytes);
    if (!b) return nullptr;
    return std::shared_ptr<char>(b->pinned, [b](char *) { std::lock_guard<std::mutex> lk(g_shared_mu); shared_release(b); });
}

extern "C" uint64_t arp_release_host_pool(void) {
    std::vector<SharedBlock *> idle;
    {
        std::lock_guard<std::mutex> lk(g_shared_mu);
        idle.swap(g_shared_pool);
        g_shared_pool_bytes = 0;
    }
    uint64_t bytes = 0;
    for (SharedBlock *b : idle) { bytes += b->cap; (void)hipHostFree(b->pinned); delete b; }
    return bytes;
}

extern "C" void arp_pairs_free(arp_pairs *pairs) {
    if (!pairs || !pairs->data) return;
    if (pairs->location == ARP_MEM_DEVICE) (void)hipFree(pairs->data);
    else {
        bool shared = false;
        {
            std::lock_guard<std::mutex> lk(g_shared_mu);
            auto it = g_shared_views.find(pairs->data);
            if (it != g_shared_views.end()) {
                shared = true;
                SharedBlock *b = it->second;
                g_shared_views.erase(it);
                if (--b->refs == 0) shared_release(b);
            }
        }
        if (!shared) free(pairs->data);
    }
    pairs->data = nullptr; pairs->n = 0;
}

namespace {
constexpr uint64_t kPackAtoms = 1u << 20;    // atoms per pack: ~200 structures of 5k atoms; ~50 packs keep the pipeline full on a 10^4 batch
constexpr uint32_t kPackMembers = 32768;     // members per pack (the device also checks that the models fit 16 bits)

struct PackPlan {
    std::vector<int32_t> members;
    uint64_t n = 0, n_res = 0, n_h = 0;
    bool single = false;                     // not packable: goes through arp_contacts_atomic on its own
};

bool packable(const arp_atoms *a) {
    if (!a || a->location != ARP_MEM_HOST || a->n == 0 || a->n_res == 0 || a->n >= kPackAtoms) return false;
    if (!a->x || !a->y || !a->z || !a->attr || !a->res_ord || !a->chain_rank || !a->model || !a->res_id || !a->res_h_ptr || !a->res_cb || !a->res_sg) return false;
    if (a->res_h_ptr[a->n_res] && !a->res_h_idx) return false;
    return true;
}

// segments of a pack's block, 256-byte aligned: the twelve input arrays, the descriptor table, then device-only scratch
struct PackLayout {
    enum { X, Y, Z, ATTR, RES_ORD, CHAIN, MODEL, RES_ID, RES_H_PTR, RES_CB, RES_SG, RES_H_IDX, DESC, N_MODELS, STATUS, COUNT, OFFSET, CURSOR, N_SEG };
    uint64_t off[N_SEG], upload = 0, total = 0;
    PackLayout(uint64_t n, uint64_t nr, uint64_t nh, uint64_t K) {
        const uint64_t bytes[N_SEG] = {n * 8, n * 8, n * 8, n * 4, n * 4, n * 4, n * 4, n * 4, (nr + 1) * 4, nr * 4, nr * 4, nh * 4, (K + 1) * 16,
                                       K * 4, 256, K * 8, (K + 1) * 8, K * 8};
        Carver lay;
        for (int k = 0; k < N_SEG; k++) { off[k] = lay.take(bytes[k]); if (k == DESC) upload = lay.off; }
        total = std::max<uint64_t>(lay.off, 256);
    }
};

template <class F>
void run_helpers(int helpers, size_t n, F &&fn) {  // fn(item) over [0, n) on up to `helpers` threads (dynamic: items differ in size)
    if (helpers <= 1 || n <= 1) { for (size_t k = 0; k < n; k++) fn(k); return; }
    std::atomic<size_t> next{0};
    std::exception_ptr first_error;  // (as parallel_for, host_common.h: no exception leaves a helper thread, none unwinds past a joinable one)
    std::mutex error_mu;
    auto work = [&]() noexcept {
        try { for (size_t k; (k = next.fetch_add(1, std::memory_order_relaxed)) < n;) fn(k); }
        catch (...) { next.store(n, std::memory_order_relaxed); std::lock_guard<std::mutex> lk(error_mu); if (!first_error) first_error = std::current_exception(); }
    };
    std::vector<std::thread> th;
    th.reserve((size_t)helpers);
    {
        struct JoinAll { std::vector<std::thread> &t; ~JoinAll() { for (auto &x : t) if (x.joinable()) x.join(); } } join_all{th};
        for (int t = 1; t < helpers; t++) try { th.emplace_back(work); } catch (const std::system_error &) { break; }
        work();
    }
    if (first_error) std::rethrow_exception(first_error);
}

struct BatchLap : LapTimer {  // arp_debug_set("timing", 1): where a pack's host time goes (stderr)
    BatchLap() : LapTimer("    batch %-28s %8.3f ms\n") {}
};

struct BatchSlot {
    arp_context *ctx = nullptr;
    PackPlan plan;
    bool in_flight = false;
    PackArrays pa{};
    PairPass pass{};                         // the pack's pair pass (pass.d: the packed arrays)
};

arp_status ensure_pack_buffers(arp_context *ctx, uint64_t in_bytes, uint64_t out_records, uint64_t K) {
    arp_status s;
    if (ctx->st.bytes < in_bytes && (s = regrow_staged(ctx, in_bytes + in_bytes / 4)) != ARP_OK) return s;
    if (ctx->out_cap < out_records || ctx->grp_cap < out_records) {
        const uint64_t bytes = out_records * sizeof(arp_pair);
        if ((s = regrow(ctx, (void **)&ctx->out_buf, &ctx->out_cap, out_records, bytes, false)) != ARP_OK) return s;
        if ((s = regrow(ctx, (void **)&ctx->grp_buf, &ctx->grp_cap, out_records, bytes, false)) != ARP_OK) return s;
    }
    const uint64_t off_cap = K + 4 + K / 4;
    if (ctx->h_offsets_cap < K + 4) return regrow(ctx, (void **)&ctx->h_offsets, &ctx->h_offsets_cap, off_cap, off_cap * sizeof(unsigned long long), true);
    return ARP_OK;
}

// between the pack's pair kernels and the copy of their result words: the split of the list by member
arp_status pack_split_step(arp_context *ctx, const PairPass &p, void *slot) {
    const BatchSlot &sl = *static_cast<const BatchSlot *>(slot);
    // (a pack never takes the hole-free sequence of small inputs -- DevAtoms::per_model rules it out in the emit plan, emit_plan.h --: that sequence leaves
    // the pair count and the capacity flag for the HOST to derive (engine.cpp finish_result), and the split kernels read the count on the device)
    if (p.direct) { set_error("internal error: a pack ran the hole-free emit sequence, whose pair count only exists on the host"); return ARP_ERR_HIP; }
    launch_pack_split(sl.pa, ctx->ws.result, ctx->out_buf, std::min(ctx->out_cap, ctx->grp_cap), ctx->grp_buf, p.mode == PairPass::OrderedFill, ctx->stream);
    return ARP_OK;
}

// steps 4-6 of a pack: grid + pair kernels + split + the small D2H of counts (everything asynchronous on the slot's stream)
arp_status enqueue_pack_kernels(arp_context *ctx, PairPass &p) {
    const PackArrays &pa = static_cast<const BatchSlot *>(p.between_arg)->pa;
    p.out = ctx->out_buf; p.capacity = ctx->out_cap;  // (the buffer as it is now: finalize_pack grows it)
    const arp_status s = pass_issue(ctx, p);
    if (s != ARP_OK) return s;
    HIP_TRY(hipMemcpyAsync(ctx->h_offsets, pa.offset, (pa.K + 1) * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(ctx->h_offsets + pa.K + 1, pa.status, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    return ARP_OK;
}

arp_status launch_pack(BatchSlot &sl, const arp_atoms *const *atoms, const arp_params *params, int helpers) {
    arp_context *ctx = sl.ctx;
    const PackPlan &pk = sl.plan;
    const uint64_t K = pk.members.size();
    arp_status s = check_device(ctx);
    if (s != ARP_OK) return s;
    if ((s = ensure_workspace(ctx, pk.n)) != ARP_OK) return s;
    const PackLayout lay(pk.n, pk.n_res, pk.n_h, K);
    // output guess: contacts-only lists hold ~1 record per atom, full candidate lists ~15-30; a pack that needs more is re-run (finalize)
    const bool only = (params->flags & ARP_FLAG_CONTACTS_ONLY) != 0;
    const uint64_t guess = std::max<uint64_t>((only ? 4u : 32u) * pk.n, 1u << 16);
    BatchLap lap;
    if ((s = ensure_pack_buffers(ctx, lay.total, std::max(guess, ctx->out_cap), K)) != ARP_OK) return s;
    lap("launch: buffers");
    char *pin = ctx->st.pinned, *dev = ctx->st.dev;
    // member offsets (serial: three running sums), then the copies -- the only per-atom host work of the batch path
    PackDesc *desc = reinterpret_cast<PackDesc *>(pin + lay.off[PackLayout::DESC]);
    {
        uint64_t o = 0, ro = 0, ho = 0;
        for (uint64_t m = 0; m < K; m++) {
            const arp_atoms &a = *atoms[pk.members[m]];
            desc[m] = PackDesc{(uint32_t)o, (uint32_t)ro, (uint32_t)ho, 0u};
            o += a.n; ro += a.n_res; ho += a.res_h_ptr[a.n_res];
        }
        desc[K] = PackDesc{(uint32_t)o, (uint32_t)ro, (uint32_t)ho, 0u};
    }
    auto seg = [&](int k) { return pin + lay.off[k]; };
    run_helpers(helpers, (size_t)K, [&](size_t m) {
        const arp_atoms &a = *atoms[pk.members[m]];
        const PackDesc d = desc[m];
        const uint64_t nh = a.res_h_ptr[a.n_res];
        memcpy(seg(PackLayout::X) + 8ull * d.first_atom, a.x, a.n * 8); memcpy(seg(PackLayout::Y) + 8ull * d.first_atom, a.y, a.n * 8);
        memcpy(seg(PackLayout::Z) + 8ull * d.first_atom, a.z, a.n * 8);
        memcpy(seg(PackLayout::ATTR) + 4ull * d.first_atom, a.attr, a.n * 4); memcpy(seg(PackLayout::RES_ORD) + 4ull * d.first_atom, a.res_ord, a.n * 4);
        memcpy(seg(PackLayout::CHAIN) + 4ull * d.first_atom, a.chain_rank, a.n * 4); memcpy(seg(PackLayout::MODEL) + 4ull * d.first_atom, a.model, a.n * 4);
        memcpy(seg(PackLayout::RES_ID) + 4ull * d.first_atom, a.res_id, a.n * 4);
        memcpy(seg(PackLayout::RES_H_PTR) + 4ull * d.first_res, a.res_h_ptr, a.n_res * 4);
        memcpy(seg(PackLayout::RES_CB) + 4ull * d.first_res, a.res_cb, a.n_res * 4); memcpy(seg(PackLayout::RES_SG) + 4ull * d.first_res, a.res_sg, a.n_res * 4);
        if (nh) memcpy(seg(PackLayout::RES_H_IDX) + 4ull * d.first_h, a.res_h_idx, nh * 4);
    });
    lap("launch: assemble (host)");
    HIP_TRY(hipMemcpyAsync(dev, pin, lay.upload, hipMemcpyHostToDevice, ctx->stream));
    lap("launch:   H2D call");
    auto at = [&](int k) { return dev + lay.off[k]; };
    PackArrays &pa = sl.pa;
    pa.n = (uint32_t)pk.n; pa.n_res = (uint32_t)pk.n_res; pa.n_h = (uint32_t)pk.n_h; pa.K = (uint32_t)K;
    pa.desc = (PackDesc *)at(PackLayout::DESC); pa.model = (uint32_t *)at(PackLayout::MODEL); pa.res_id = (uint32_t *)at(PackLayout::RES_ID);
    pa.res_h_ptr = (uint32_t *)at(PackLayout::RES_H_PTR); pa.res_cb = (uint32_t *)at(PackLayout::RES_CB); pa.res_sg = (uint32_t *)at(PackLayout::RES_SG);
    pa.res_h_idx = (uint32_t *)at(PackLayout::RES_H_IDX); pa.n_models = (uint32_t *)at(PackLayout::N_MODELS); pa.status = (uint32_t *)at(PackLayout::STATUS);
    pa.count = (unsigned long long *)at(PackLayout::COUNT); pa.offset = (unsigned long long *)at(PackLayout::OFFSET); pa.cursor = (unsigned long long *)at(PackLayout::CURSOR);
    launch_pack_fix(pa, ctx->stream);
    lap("launch:   pack_fix calls");
    sl.pass = PairPass{};
    DevAtoms &d = sl.pass.d;
    d.n = pa.n; d.n_res = pa.n_res; d.per_model = 1u;
    d.x = (const double *)at(PackLayout::X); d.y = (const double *)at(PackLayout::Y); d.z = (const double *)at(PackLayout::Z);
    d.attr = (const uint32_t *)at(PackLayout::ATTR); d.res_ord = (const uint32_t *)at(PackLayout::RES_ORD);
    d.chain_rank = (const uint32_t *)at(PackLayout::CHAIN); d.model = pa.model;
    d.res_id = pa.res_id; d.res_h_ptr = pa.res_h_ptr; d.res_h_idx = pa.res_h_idx; d.res_cb = pa.res_cb; d.res_sg = pa.res_sg;
    // (ordered calls are never packed, see the plan.)  A pack never skips the probe pass and keeps no memo; it is not profiled; a deferred-probe
    // list that is still too small after 4 repeats sends the pack's members through arp_contacts_atomic one by one (finalize_pack)
    sl.pass.params = params; sl.pass.mode = PairPass::Emit; sl.pass.profile = false; sl.pass.max_reissues = 4;
    sl.pass.between = pack_split_step; sl.pass.between_arg = &sl;
    if ((s = upload_params(ctx, params)) != ARP_OK) return s;
    lap("launch:   params");
    if ((s = enqueue_pack_kernels(ctx, sl.pass)) != ARP_OK) return s;
    lap("launch: enqueue (kernels)");
    sl.in_flight = true;
    return ARP_OK;
}

// wait for a pack, fetch the grouped list, hand the members their lists.  An input error inside the pack (or more models than 16
// bits hold) is re-run member by member so that the failing structure reports it.
arp_status finalize_pack(BatchSlot &sl, const arp_atoms *const *atoms, const arp_params *params, arp_pairs *outs) {
    if (!sl.in_flight) return ARP_OK;
    sl.in_flight = false;
    arp_context *ctx = sl.ctx;
    const PackPlan &pk = sl.plan;
    const uint64_t K = pk.members.size();
    arp_status s = check_device(ctx);
    if (s != ARP_OK) return s;
    unsigned long long total = 0;
    BatchLap lap;
    PairPass &p = sl.pass;
    for (;;) {
        s = pass_finish(ctx, p, enqueue_pack_kernels);
        lap("finalize: wait for kernels");
        if (s != ARP_OK && !p.collected) return s;
        const uint32_t pack_status = *reinterpret_cast<const uint32_t *>(ctx->h_offsets + K + 1);
        if (s != ARP_OK || pack_status != 0u) {  // (s: also a deferred-probe list that overflowed once too often)
            for (int32_t k : pk.members)
                if ((s = arp_contacts_atomic(ctx, atoms[k], params, ARP_MEM_HOST, &outs[k])) != ARP_OK) return s;
            return ARP_OK;
        }
        total = ctx->h_result[kResPairs];
        if (total <= ctx->out_cap) break;
        if (p.reissues >= p.max_reissues) { set_error("internal error: pair count changed between passes"); return ARP_ERR_HIP; }
        const PackLayout lay(pk.n, pk.n_res, pk.n_h, K);
        if ((s = ensure_pack_buffers(ctx, lay.total, total + total / 8, K)) != ARP_OK) return s;  // (the staged inputs stay where they are)
        p.reissues++;
        if ((s = upload_params(ctx, params)) != ARP_OK || (s = enqueue_pack_kernels(ctx, p)) != ARP_OK) return s;
    }
    SharedBlock *blk = nullptr;
    if (total) {
        if (!(blk = shared_acquire(total * sizeof(arp_pair)))) { set_error("out of pinned host memory for the batch's pair lists"); return ARP_ERR_OOM; }
        lap("finalize: pinned block");
        hipError_t e = hipMemcpyAsync(blk->pinned, ctx->grp_buf, total * sizeof(arp_pair), hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            std::lock_guard<std::mutex> lk(g_shared_mu);
            shared_release(blk);
            set_error("HIP error %d (%s) copying the batch's pair lists to the host", (int)e, hipGetErrorString(e));
            return ARP_ERR_HIP;
        }
    }
    lap("finalize: D2H of the lists");
    const unsigned long long *off = ctx->h_offsets;
    std::lock_guard<std::mutex> lk(g_shared_mu);
    for (uint64_t m = 0; m < K; m++) {  // every member's list is a view into the pack's block (arp_pairs_free drops the reference)
        arp_pairs &out = outs[pk.members[m]];
        const unsigned long long cnt = off[m + 1] - off[m];
        out.n = cnt; out.location = ARP_MEM_HOST; out.data = nullptr;
        if (!cnt) continue;
        out.data = reinterpret_cast<arp_pair *>(blk->pinned) + off[m];
        g_shared_views.emplace(out.data, blk);
        blk->refs++;
    }
    if (blk && blk->refs == 0) shared_release(blk);
    return ARP_OK;
}
}  // namespace

extern "C" arp_status arp_contacts_atomic_batch(arp_context *const *ctxs, int32_t n_ctx, const arp_atoms *const *atoms, int32_t n_structures,
                                                const arp_params *params, arp_pairs *outs) try {
    if (!ctxs || n_ctx <= 0 || !atoms || n_structures < 0 || !outs || !params) { set_error("bad batch arguments"); return ARP_ERR_BAD_INPUT; }
    for (int32_t k = 0; k < n_structures; k++) outs[k] = arp_pairs{0, nullptr, ARP_MEM_HOST, 0};
    for (int32_t k = 0; k < n_structures; k++)
        if (!atoms[k]) { set_error("null structure %d in the batch", k); return ARP_ERR_BAD_INPUT; }
    for (int d = 0; d < n_ctx; d++)
        if (!ctxs[d]) { set_error("null context %d in the batch", d); return ARP_ERR_BAD_INPUT; }
    // longest-processing-time-first deal over the devices (the same rule as arpeggia_amd/sharding.py)
    std::vector<int32_t> order(n_structures);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return atoms[a]->n > atoms[b]->n; });
    std::vector<std::vector<int32_t>> queue(n_ctx);
    std::vector<uint64_t> load(n_ctx, 0);
    for (int32_t k : order) {
        int best = (int)(std::min_element(load.begin(), load.end()) - load.begin());
        queue[best].push_back(k);
        load[best] += atoms[k]->n + 1;
    }
    const int hw = (int)std::max(1u, std::thread::hardware_concurrency());
    const int helpers = std::max(1, std::min(8, hw / std::max(1, n_ctx)));
    std::vector<arp_status> st(n_ctx, ARP_OK);
    std::vector<std::string> msg(n_ctx);
    auto device_worker_body = [&](int d) {
        auto fail = [&](arp_status s) { st[d] = s; msg[d] = arp_last_error(); };
        // plan: consecutive members of the device's share form packs; what cannot be packed runs alone
        std::vector<PackPlan> plans;
        {
            PackPlan cur;
            auto close = [&]() { if (!cur.members.empty()) plans.push_back(std::move(cur)); cur = PackPlan{}; };
            for (int32_t k : queue[d]) {
                const arp_atoms *a = atoms[k];
                // The ordered emitter's promise (output byte-identical run to run) cannot be kept through a pack: its records are laid
                // out task by task, and the task that straddles two members interleaves their records.  Ordered calls go one by one.
                if (!packable(a) || (params->flags & ARP_FLAG_DETERMINISTIC)) {
                    close();
                    PackPlan one; one.members.push_back(k); one.single = true; plans.push_back(std::move(one));
                    continue;
                }
                if (!cur.members.empty() && (cur.n + a->n > kPackAtoms || cur.members.size() >= kPackMembers)) close();
                cur.members.push_back(k);
                cur.n += a->n; cur.n_res += a->n_res; cur.n_h += a->res_h_ptr[a->n_res];
            }
            close();
            for (PackPlan &p : plans) if (!p.single && p.members.size() == 1) p.single = true;  // nothing to share a launch with
        }
        BatchSlot slot[2];
        slot[0].ctx = ctxs[d];
        arp_status s = ARP_OK;
        const size_t np = plans.size();
        for (size_t i = 0; i <= np && s == ARP_OK; i++) {
            if (i < np) {
                if (plans[i].single) {  // synchronous: drain the pipeline first (it uses both contexts)
                    for (int q = 0; q < 2 && s == ARP_OK; q++) s = finalize_pack(slot[(i + q) & 1], atoms, params, outs);
                    if (s == ARP_OK) s = arp_contacts_atomic(ctxs[d], atoms[plans[i].members[0]], params, ARP_MEM_HOST, &outs[plans[i].members[0]]);
                    continue;
                }
                BatchSlot &sl = slot[i & 1];
                if (!sl.ctx) {  // the second context of the device: same device, its own stream and workspace; lives with the first
                    if (!ctxs[d]->peer && (s = arp_context_create(ctxs[d]->device, &ctxs[d]->peer)) != ARP_OK) break;
                    sl.ctx = ctxs[d]->peer;
                }
                sl.plan = std::move(plans[i]);
                if ((s = launch_pack(sl, atoms, params, helpers)) != ARP_OK) break;
            }
            if (i >= 1 && !(i - 1 < np && plans[i - 1].single)) s = finalize_pack(slot[(i - 1) & 1], atoms, params, outs);
        }
        if (s != ARP_OK) {
            fail(s);
            for (int q = 0; q < 2; q++) if (slot[q].ctx) (void)hipStreamSynchronize(slot[q].ctx->stream);
        }
    };
    // ARP_ABI_CATCH only guards the calling thread: an exception that left a std::thread's function would terminate the host process.  Every
    // worker therefore turns its own exceptions into a status (msg[d] is a short constant: no allocation on the way out of bad_alloc).
    auto device_worker = [&](int d) noexcept {
        try { device_worker_body(d); }
        catch (const std::bad_alloc &) { st[d] = ARP_ERR_OOM; try { msg[d] = "out of host memory in a batch worker"; } catch (...) {} }
        catch (const std::exception &e) { st[d] = ARP_ERR_HIP; try { msg[d] = e.what(); } catch (...) {} }
        catch (...) { st[d] = ARP_ERR_HIP; }
        if (st[d] != ARP_OK) {  // whatever was launched on this device's streams must not outlive the buffers the caller is about to get back
            (void)hipStreamSynchronize(ctxs[d]->stream);
            if (ctxs[d]->peer) (void)hipStreamSynchronize(ctxs[d]->peer->stream);
        }
    };
    std::vector<std::thread> th;
    th.reserve((size_t)n_ctx);  // (no reallocation while joinable threads sit in the vector)
    struct JoinAll { std::vector<std::thread> &t; ~JoinAll() { for (auto &x : t) if (x.joinable()) x.join(); } } join_all{th};
    for (int d = 1; d < n_ctx; d++)
        try { th.emplace_back(device_worker, d); } catch (const std::system_error &) { device_worker(d); }  // no thread: this device's share runs here
    device_worker(0);
    for (auto &t : th) t.join();
    for (int d = 0; d < n_ctx; d++)
        if (st[d] != ARP_OK) {
            for (int32_t k = 0; k < n_structures; k++) arp_pairs_free(&outs[k]);
            set_error("%s", msg[d].c_str());
            return st[d];
        }
    return ARP_OK;
} ARP_ABI_CATCH
