// The table plan on the command line (tests/test_table_plan_host.py): host-only, nothing but table_plan.h.
//   plan_dump            reads queries from stdin, one per line: n_pairs n_models n_chains max_ent_rank any_icode knob_key_bits; prints one plan per line:
//                        small_try few_pairs keys_fit_small model_bits chain_bits rank_bits limit digits, then "P" and pass end_bit of every pass of the
//                        general path, then "L" and the same of the long way
//   plan_dump constants  the named constants, one "name value" per line
//   plan_dump valid      reads knob values from stdin, prints 1 (arp_debug_set takes it) or 0 per line
#include <cstdio>
#include <cstring>

#include "../../arpeggia_amd/csrc/table_plan.h"

using namespace arp;

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "constants")) {
#define C(name) printf(#name " %llu\n", (unsigned long long)name)
        C(kSmallRows); C(kSmallThreads); C(kSmallIdxBits); C(kSmallPairs); C(kTableMinKeyBits); C(kTableMaxKeyBits);
#undef C
        return 0;
    }
    if (argc > 1 && !strcmp(argv[1], "valid")) {
        long long v;
        while (scanf("%lld", &v) == 1) printf("%d\n", table_key_bits_valid(v) ? 1 : 0);
        return 0;
    }
    unsigned long long n_pairs, n_models, n_chains;
    unsigned max_rank;
    int icode, knob;
    while (scanf("%llu %llu %llu %u %d %d", &n_pairs, &n_models, &n_chains, &max_rank, &icode, &knob) == 6) {
        TableQuery q;
        q.n_pairs = n_pairs; q.n_models = n_models; q.n_chains = n_chains; q.max_ent_rank = max_rank; q.any_icode = icode != 0; q.knob_key_bits = knob;
        const TablePlan p = plan_table(q);
        printf("%d %d %d %u %u %u %u %d P", p.small_try, p.few_pairs, p.keys_fit_small, p.model_bits, p.chain_bits, p.rank_bits, p.limit, p.digits);
        for (int k = 0; k < p.n_pass; k++) printf(" %d %d", p.pass[k], p.end_bit[k]);
        printf(" L");
        for (int k = 0; k < p.n_long; k++) printf(" %d %d", p.long_pass[k], p.long_end_bit[k]);
        printf("\n");
    }
    return 0;
}
