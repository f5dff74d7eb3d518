// Host-only internals of the engine: the context and the helpers that engine.cpp (context, workspace, pair pass), batch.cpp (pack pipeline)
// and sasa_dev.cpp (SASA / SAP chain) share.  Nothing here crosses the C ABI.
#pragma once
#include "arp_internal.h"
#include "host_common.h"

namespace arp {
// One pass of the pair kernels over one input.  pass_issue queues it (cell list, kernels, the copy of the result words), pass_collect reads
// what came back once the stream has been synchronised, pass_finish / pass_run drive the two to completion.
struct PairPass {
    enum Mode { Count, OrderedFill, Emit };  // candidate count only / count + ordered fill (ARP_FLAG_DETERMINISTIC) / single-pass emit
    DevAtoms d{};
    const arp_params *params = nullptr;  // (must outlive the pass: a repeat uploads them again)
    arp_pair *out = nullptr;
    unsigned long long capacity = 0;
    Mode mode = Emit;
    bool have_out = true;    // Count: the caller holds `capacity` records (0: a size query), a longer list is reported; false: the count that sizes a buffer
    bool grid = true;        // build the cell list first; false: the fill of a count / fill sequence, on the list (and the counts) of its count pass
    bool memo = false, speculate = false;  // Emit: keep the deferred-pass memo up to date / and skip the probe pass when it names this input
    bool profile = true;     // time the kernels when the context's profiler is on
    int reissues = 0, max_reissues = -1;  // how often the pass was queued again; a list overflow past max_reissues (>= 0) is the caller's (kRetryDefer)
    // launches that belong between the pass's kernels and the copy of its result words (the pack's split)
    arp_status (*between)(arp_context *ctx, const PairPass &p, void *arg) = nullptr; void *between_arg = nullptr;
    // set by pass_issue: the probe pass was skipped / the hole-free sequence ran; by pass_finish: its status is what the pass reported, not a runtime failure
    bool skip = false, direct = false, collected = false;
    bool wide_record = false;  // Emit: the cell list must carry the wide exact record (Fat) -- somebody reads it after the pass (the ring walk of the table path)
};
constexpr arp_status kRetryDefer = -1;  // internal, never crosses the C ABI: the deferred-probe list overflowed (pass_finish with max_reissues)
}  // namespace arp

struct arp_context {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    arp::Workspace ws{};
    std::vector<void *> ws_allocs;
    // device staging of host inputs
    // host inputs travel as ONE block: the twelve arrays are packed into a pinned buffer and cross PCIe in a single copy
    // (twelve small pageable copies cost ~100 us of launch overhead on a PDB-sized structure)
    struct Staged { char *dev = nullptr, *pinned = nullptr; uint64_t bytes = 0; } st;
    arp_pair *out_buf = nullptr;            // reusable device output of the host-output path (grow-only)
    char *bounce[2] = {nullptr, nullptr};   // pinned staging of large device -> host copies
    hipEvent_t bounce_ev[2] = {nullptr, nullptr};
    uint64_t out_cap = 0;
    arp_pair *grp_buf = nullptr;            // batch path: the pack's pair list grouped by member (device); it lands in a SharedBlock on the host
    uint64_t grp_cap = 0;
    unsigned long long *h_offsets = nullptr;  // pinned: per-member offsets into the grouped list (+ the pack status word)
    uint64_t h_offsets_cap = 0;
    arp::DevParams *h_params = nullptr;    // pinned
    unsigned long long *h_result = nullptr;  // pinned [kHostResultWords]: the kRes* words of the last pair pass; [kHostSasaTestsSlot]: sasa_run
    // Residue-rule memo: the last input's residues were runs of atoms (k_place's sample, kResResRuns) -- the next call's launcher then picks the
    // kernels that apply the reference's residue rule before the gathers (k_emit<.., RES>).  Same result either way; ARP_FLAG_RESIDUE_RUNS /
    // ARP_FLAG_NO_RESIDUE_RUNS overrule the memo.
    bool res_hint = false;
    std::vector<arp::ScDot> sc_dots[2];     // the dots of the last successful SC call (arp_sc_dots)
    // Cell-list memo (mark_grid_owner / mark_grid_foreign): the arrays the workspace's cell list was last built from (context_grid), and whether
    // its residue words (Sorted::rkey) were written with it
    const double *grid_x = nullptr; uint64_t grid_n = 0;
    bool rkey_valid = false;
    uint32_t narrow_ib = 0;                // ... and, when != 0, that its exact records are the narrow ones (Xrec) with that many index bits
    // Deferred-pass memo: the arrays (address + length) of the last single-pass call that deferred NOTHING to the probe pass (no hydrogens,
    // no CYS SG pair in the covalent band -- every X-ray structure without hydrogens).  The next call on the same arrays does not launch
    // k_pairs_deferred; should it defer after all (the caller rewrote the arrays), k_fixup raises kStatStaleSkip and the call is repeated
    // with the pass.  A guess that is checked on the device, never a correctness assumption.
    const double *nodefer_x = nullptr; uint64_t nodefer_n = 0;
    arp_params last_params{};
    bool have_params = false;
    arp::DevParams *params_on_device = nullptr;  // the workspace block that holds the current parameters (upload_params); reset with the workspace
    hipStream_t params_stream = nullptr;    // ... uploaded on this stream (a caller who swaps streams gets a fresh upload, ordered on the new one)
    hipEvent_t params_ev = nullptr;         // recorded behind the last upload of h_params: the block is rewritten only after that copy has run
    bool params_ev_armed = false;
    arp::PairPass enqueued{};              // the enqueued call, kept so that arp_contacts_atomic_result can collect it (and queue it again)
    bool pending = false;
    char *scr_dev[2] = {nullptr, nullptr}, *scr_pin[2] = {nullptr, nullptr};  // table path: two grow-only scratch blocks (device / pinned)
    uint64_t scr_dev_cap[2] = {0, 0}, scr_pin_cap[2] = {0, 0};
    arp_context *peer = nullptr;           // batch path: the second context of this device (own stream + workspace), kept across calls
    uint32_t defer_scale = 1;              // the deferred-probe list is sized defer_scale x the default; grown on overflow
    uint64_t sasa_tests = 0;               // f32 distance tests of the last SASA call (arp_sasa_tests)
    arp::Profiler prof;
};

namespace arp {
void make_dev_params(const arp_params &p, DevParams *d);
arp_status check_device(arp_context *ctx);
arp_status ensure_workspace(arp_context *ctx, uint64_t n);
arp_status stage_inputs(arp_context *ctx, const arp_atoms *a, DevAtoms *d);  // device inputs: as they are; host inputs: one pinned block, one copy
arp_status upload_params(arp_context *ctx, const arp_params *p);
// grow-only buffers of the context: *p gets `bytes` (device or pinned host), *cap becomes `want`; the staging pair of the inputs gets `cap` bytes each
arp_status regrow(arp_context *ctx, void **p, uint64_t *cap, uint64_t want, uint64_t bytes, bool pinned);
arp_status regrow_staged(arp_context *ctx, uint64_t cap);
inline Profiler *context_profiler(arp_context *ctx) { return ctx->prof.enabled ? &ctx->prof : nullptr; }
// The workspace's cell list now belongs to the arrays (x, n) (x == nullptr: to an input nothing can name, a pack) / to a caller outside the
// pair pass, which also drops the deferred-pass memo.  Every path that builds a grid in the context's workspace says which.
void mark_grid_owner(arp_context *ctx, const double *x, uint64_t n, bool rkey_valid, uint32_t narrow_ib = 0);
void mark_grid_foreign(arp_context *ctx);
arp_status pass_issue(arp_context *ctx, PairPass &p);   // asynchronous on the context's stream
// An issued pass: synchronise, collect; on a stale memo or after growing an overflowed deferred-probe list queue it again (reissue: the caller's way) and start over.
arp_status pass_finish(arp_context *ctx, PairPass &p, arp_status (*reissue)(arp_context *, PairPass &) = pass_issue);
inline arp_status pass_run(arp_context *ctx, PairPass &p) { const arp_status s = pass_issue(ctx, p); return s != ARP_OK ? s : pass_finish(ctx, p); }
}  // namespace arp
