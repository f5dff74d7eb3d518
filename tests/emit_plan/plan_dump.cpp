// The emit plan on the command line (tests/test_emit_plan_host.py): host-only, nothing but emit_plan.h.
//   plan_dump            reads queries from stdin, one per line: n per_model ordered contacts_only skip_deferred res_wanted narrow_ok scratch_cap
//                        knob_emit_kernel knob_index_bits; prints one plan per line: route waves split blocks chunk_records only res narrow_ib probes
//                        patch fixup_holes variant (the plan's index in kEmitVariants, -1: none)
//   plan_dump constants  the named thresholds, one "name value" per line
//   plan_dump variants   the keys of kEmitVariants, one per line: waves split only direct res stage narrow
#include <cstdio>
#include <cstring>

#include "../../arpeggia_amd/csrc/emit_plan.h"

using namespace arp;

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "constants")) {
#define C(name) printf(#name " %llu\n", (unsigned long long)name)
        C(kESlotBits); C(kBigSlots); C(kNarrowMaxBits); C(kEWaves); C(kEBlocks); C(kDeferBlocks); C(kEmitBlocks); C(kChunkRecords); C(kSmallChunkRecords);
        C(kWaveStageRecords); C(kDirectTasks); C(kEightTasks); C(kSharedTasks); C(kStageTasks); C(kDirectBlocks);
#undef C
        return 0;
    }
    if (argc > 1 && !strcmp(argv[1], "variants")) {
        for (const EmitVariant &v : kEmitVariants.v) printf("%d %d %d %d %d %d %d\n", v.waves, v.split, v.only, v.direct, v.res, v.stage, v.narrow);
        return 0;
    }
    static const char *const kRoutes[] = {"Ordered", "Gather", "Direct", "Stage", "Chunked"};
    unsigned n;
    int pm, ord, only, skip, res, narrow, k_emit, k_bits;
    unsigned long long scratch;
    while (scanf("%u %d %d %d %d %d %d %llu %d %d", &n, &pm, &ord, &only, &skip, &res, &narrow, &scratch, &k_emit, &k_bits) == 10) {
        EmitQuery q;
        q.n = n; q.per_model = pm; q.ordered = ord; q.contacts_only = only; q.skip_deferred = skip; q.res_wanted = res; q.narrow_ok = narrow;
        q.scratch_cap = scratch; q.knob_emit_kernel = k_emit; q.knob_index_bits = k_bits;
        const EmitPlan p = plan_emit(q);
        printf("%s %u %u %u %u %d %d %u %d %d %u %d\n", kRoutes[(int)p.route], p.waves, p.split, p.blocks, p.chunk_records, p.only, p.res, p.narrow_ib, p.probes,
               p.patch, p.fixup_holes, emit_variant_index(p));
    }
    return 0;
}
