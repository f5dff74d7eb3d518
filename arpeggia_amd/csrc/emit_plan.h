// The emit plan: which launch sequence of the single-pass emitter a call runs and which record format its cell list carries, decided ONCE, on the
// host, by one pure function of the call's size, flags and knobs.  The engine plans before it builds the cell list (k_place writes the residue words
// and the exact record the planned kernel reads) and hands the same plan to the launch (pairs_emit.inl launch_emit).
// No HIP in here: a host compiler builds this header on its own (tests/emit_plan/plan_dump.cpp).
#pragma once
#include <cstdint>
#include <initializer_list>

namespace arp {

constexpr uint32_t kESlotBits = 24;        // k_emit (pairs_emit.inl): neighbour slot bits of a queue entry (v_mul_u32_u24 turns the entry into the record offset); larger inputs go to k_pairs
// Record p of the cell-sorted array through a 32-bit byte offset from the (scalar) base (pairs.inl fat_at): valid below 2^32 / 48 slots; larger
// inputs take the count + ordered fill with inline probes, which address in 64 bits.
constexpr uint32_t kBigSlots = 0x5000000u;
constexpr uint32_t kNarrowMaxBits = 20;  // index bits of Xrec::ot at most (2^20 atoms): the tag keeps 12 bits or more.  Fewer tag bits alias too often: a resident input of
                                         // 1250 five-thousand-atom models (6.25 x 10^6 atoms, 23 + 9 bits) ran k_emit 48 us longer than on the wide record, k_place 35 us shorter
constexpr int kWavesPerBlock = 8;          // k_pairs and the probe passes
constexpr int kEmitWavesPerSimd = 6;       // register budget of k_pairs<kEmit>: 80 VGPRs at 6, 64 at 8
constexpr uint32_t kEmitBlocks = (1024u * kEmitWavesPerSimd) / kWavesPerBlock;  // k_pairs<kEmit>: blocks of 8 waves, 6 waves per SIMD
constexpr int kEWaves = 12;                   // k_emit, waves per block: two blocks per CU share the CU's LDS, 6 waves per SIMD
constexpr uint32_t kEBlocks = 256u * 2u;
constexpr uint32_t kDeferBlocks = 384;       // the probe passes: fills the chip at k_pairs_deferred's 3 waves per SIMD when the list is long
// records per global allocation (one device atomic each).  The wave whose allocation crosses the end of the block's chunk fetches the
// next one while the block's other waves sleep: 2048 -> 4096 halves those stalls (emit 221 -> 208 us); 8192 gains 2 us more and costs
// the fix-up 8 us (holes grow with the chunk).
constexpr uint32_t kChunkRecords = 4096, kSmallChunkRecords = 2048;  // records per allocation chunk (powers of two; the smaller one: k_emit's four-way task split; its 4-wave kernels stage and flush instead)
constexpr uint32_t kWaveStageRecords = 1024;  // a wave's region of the scratch block in the scratch-staged sequence (pairs_emit.inl stage_copy_g)
// Fewer tasks than the chip has wave slots (kSharedTasks): every task is shared out over four waves by window kind (eight below kEightTasks, two
// per kind set: 6bft's 128 tasks run 3 us faster that way, an S2 cloud of the same size 1.3 us slower), and below kDirectTasks the blocks shrink
// to four waves so that the few tasks reach more CUs.  Thresholds from size sweeps of the kernel (tests/microbench/ab_r3ae.sh .. ab_r3ag.sh,
// profiles/r03_small_inputs.txt): a task is a chain of dependent round trips, and an input that does not fill the chip has nothing else to hide it behind.
// The 4-wave kernels are the hole-free ones (Direct) and have no residue-rule variant (a call of that size is launches and round trips, not
// batches); a pack that small keeps the 12-wave sequence with its fix-up, which is what publishes the count its members' lists are split by on the device.
constexpr uint32_t kDirectTasks = 320, kEightTasks = 160, kSharedTasks = 4608, kDirectBlocks = 1536;
// Stage: the hole-free sequence of the task-split 12-wave kernels (k_emit<.., STAGE>: records staged per wave in the scratch block, no fix-up launch) -- for
// inputs the engine's memo says defer nothing (skip_deferred: the kernel raises status bit 128 if they do after all and the host repeats the call with the
// chunked sequence), whose waves' regions fit the scratch block.  Up to kStageTasks tasks = 131 k atoms: every record crosses the L2 twice more on this
// route, which costs the kernel ~1 us per 3 x 10^5 records -- S2 per step, staged against chunks + fix-up: 3 x 10^4 atoms 53 against 64 us, 6 x 10^4 64 / 71,
// 10^5 76 / 82 (S1 65 / 80), 1.9 x 10^5 106 / 102, 2.9 x 10^5 146 / 129.
constexpr uint32_t kStageTasks = 2048;

// Ordered: count + ordered fill (beyond kBigSlots); Gather: k_pairs<kEmit> (beyond k_emit's 2^24 slots, or
// arp_debug_set("emit_kernel", 1)); the rest are k_emit's: Direct = 4-wave hole-free, Stage = 12-wave scratch-staged hole-free, Chunked = 12-wave + probe pass + fix-up.
enum class EmitRoute { Ordered, Gather, Direct, Stage, Chunked };
struct EmitQuery {
    uint32_t n = 0;
    bool per_model = false, contacts_only = false, skip_deferred = false;
    bool ordered = false;     // ARP_FLAG_DETERMINISTIC: the cell list is the ordered fill's (k_gather: the wide record, no residue words)
    bool res_wanted = false;  // the input's residues are runs of atoms (the caller's flag, or the engine's hint); on a cell list that stands: its residue words are valid
    bool narrow_ok = false;   // an Emit pass nobody walks the records after; on a cell list that stands: it holds narrow records, knob_index_bits wide
    unsigned long long scratch_cap = 0;
    int knob_emit_kernel = 0, knob_index_bits = 0;  // arp_debug_set
};
struct EmitPlan {
    EmitRoute route;
    uint32_t waves, split, blocks, chunk_records;  // of the emit kernel's launch (chunk_records 0: no allocation chunks)
    bool only;               // ARP_FLAG_CONTACTS_ONLY
    bool res;                // the residue-rule kernels (k_emit<.., RES>); k_place writes Sorted::rkey (Gather: written as the size asks, not read)
    uint32_t narrow_ib;      // index bits of the narrow exact record (Xrec) k_place writes and the kernels read; 0: the wide record (Fat)
    bool probes, patch;      // a probe pass follows the emit kernel / it is k_patch_deferred (kinds in place), not k_pairs_deferred (emits, adds holes)
    uint32_t fixup_holes;    // hole-list entries k_fixup is told; 0: the list has no holes and nothing follows the emit kernel
};

// The k_emit instantiations there are, in the order the code object carries them; launch_emit (pairs_emit.inl) looks a plan up here and nowhere else.
struct EmitVariant { int waves, split; bool only, direct, res, stage, narrow; };
constexpr int kEmitVariantCount = 24;
struct EmitVariants { EmitVariant v[kEmitVariantCount]; };
constexpr EmitVariants make_emit_variants() {
    EmitVariants t{};
    int k = 0;
    for (bool only : {true, false})
        for (bool res : {true, false}) t.v[k++] = {kEWaves, 4, only, false, res, true, false};  // Stage
    for (bool only : {true, false}) {
        for (int split : {8, 4}) t.v[k++] = {4, split, only, true, false, false, false};      // Direct
        for (int split : {4, 1})
            for (bool res : {true, false})
                for (bool narrow : {true, false}) t.v[k++] = {kEWaves, split, only, false, res, false, narrow};  // Chunked
    }
    return t;
}
constexpr EmitVariants kEmitVariants = make_emit_variants();
inline int emit_variant_index(const EmitPlan &p) {  // -1: none (and for the routes that are not k_emit's)
    const bool direct = p.route == EmitRoute::Direct, stage = p.route == EmitRoute::Stage;
    if (!direct && !stage && p.route != EmitRoute::Chunked) return -1;
    for (int k = 0; k < kEmitVariantCount; k++) {
        const EmitVariant &v = kEmitVariants.v[k];
        if ((uint32_t)v.waves == p.waves && (uint32_t)v.split == p.split && v.only == p.only && v.direct == direct && v.res == p.res && v.stage == stage &&
            v.narrow == (p.narrow_ib != 0u)) return k;
    }
    return -1;
}

inline EmitPlan plan_emit(const EmitQuery &q) {
    EmitPlan p{};
    p.only = q.contacts_only;
    const uint32_t tasks = (q.n + 63u) / 64u;
    auto blocks_of = [&](uint32_t per, uint32_t cap) { const uint32_t want = (p.split * tasks + per - 1u) / per; return want < 1u ? 1u : (want > cap ? cap : want); };
    if (q.n >= kBigSlots) { p.route = EmitRoute::Ordered; return p; }
    const bool e_slots = q.n < (1u << kESlotBits) - 64u, direct = tasks < kDirectTasks && !q.per_model;
    p.res = !q.ordered && e_slots && !direct && q.res_wanted;
    if (q.knob_emit_kernel == 1 || !e_slots) {
        p.route = EmitRoute::Gather; p.waves = kWavesPerBlock; p.split = 1u; p.blocks = blocks_of(kWavesPerBlock, kEmitBlocks); p.chunk_records = kChunkRecords;
        p.probes = !q.skip_deferred; p.fixup_holes = p.blocks + (p.probes ? kDeferBlocks : 0u);
        return p;
    }
    if (direct) {
        p.route = EmitRoute::Direct; p.waves = 4u; p.split = tasks < kEightTasks ? 8u : 4u; p.blocks = blocks_of(4u, kDirectBlocks);
        return p;
    }
    p.waves = kEWaves; p.split = tasks < kSharedTasks ? 4u : 1u; p.blocks = blocks_of(kEWaves, kEBlocks);
    const bool stage = tasks <= kStageTasks && !q.per_model && q.skip_deferred && (unsigned long long)p.blocks * kEWaves * kWaveStageRecords <= q.scratch_cap;
    if (stage) { p.route = EmitRoute::Stage; return p; }
    p.route = EmitRoute::Chunked; p.chunk_records = p.split == 4u ? kSmallChunkRecords : kChunkRecords;
    p.probes = !q.skip_deferred; p.patch = !p.only; p.fixup_holes = p.blocks + (p.probes && !p.patch ? kDeferBlocks : 0u);
    // The narrow exact record (arp_internal.h Xrec) is read by the chunked 12-wave kernels of single inputs alone.  The 4-wave kernels keep the wide
    // record: they have no residue-rule variant, so on a protein every batch would hold pairs of one residue, which the tags cannot decide, and take
    // the rare branch.  The scratch-staged kernels keep it as well -- at 10^5 atoms the narrow record measured -1.1 us on S2 and +0.3 us on S1 per
    // step (profiles/r20_narrow_record.md): not worth four more kernels.  Packs keep it too: measured on 1250 five-thousand-atom members, k_place ran
    // 40 us shorter and k_emit 54 us longer, the step 7 us longer (ibid.).  Index bits: as few as hold the largest index, so the tag gets the rest --
    // 20 + 12 at 10^6 atoms, 17 + 15 at 10^5; beyond kNarrowMaxBits the record stays wide.  arp_debug_set("index_bits", v): v in 1 .. 20 fixes the
    // width (an input whose last index does not fit it keeps the wide record), v < 0 keeps the wide record always.
    if (q.narrow_ok && !q.ordered && !q.per_model && q.knob_index_bits >= 0) {
        uint32_t need = 1u;
        while (need < 32u && ((q.n - 1u) >> need) != 0u) need++;
        const uint32_t ib = q.knob_index_bits > 0 ? (uint32_t)q.knob_index_bits : need;
        if (ib >= need && ib <= kNarrowMaxBits) p.narrow_ib = ib;
    }
    return p;
}

}  // namespace arp
