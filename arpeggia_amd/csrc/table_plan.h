// The table plan: which route a call of device_table (table_dev.hip) takes and which radix passes its general path runs, decided by one pure
// function of the call's pair count, the structure's key widths and one knob.  device_table asks here and decides nothing itself; the route it then
// went is kept in a TableRoute record (arp_debug_get, include/arpeggia_amd.h).
// No HIP in here: a host compiler builds this header on its own (tests/table_plan/plan_dump.cpp).
#pragma once
#include <cstdint>

namespace arp {

// The one-launch path (k_table_small): one workgroup of kSmallThreads threads sorts up to kSmallRows words of {ten keys, kSmallIdxBits of row index};
// the launcher tries it up to kSmallPairs pairs.
constexpr uint32_t kSmallRows = 4096, kSmallThreads = 1024, kSmallIdxBits = 12, kSmallPairs = 2048;
// arp_debug_set("table_key_bits", v): v stands for the 64 of the three width tests below, so that small inputs reach the plans of wide keys.  The knob
// moves the plan only: every pass sorts on the real width of its key, so a value below a structure's widest pass is harmless.  The knob is process-wide
// and set before any structure is known, so the bound it is checked against is not that structure's widest pass but the narrowest pass any structure can
// have: kTableMinKeyBits = pass 2 with one rank bit + five interaction bits.  Nothing below it can stand for a key word at all; nothing above 64 fits one.
constexpr int kTableMinKeyBits = 6, kTableMaxKeyBits = 64;
inline bool table_key_bits_valid(long long v) { return v == 0 || (v >= kTableMinKeyBits && v <= kTableMaxKeyBits); }

inline uint32_t table_width(uint64_t v) { uint32_t b = 1; while (b < 32 && (1ull << b) < v) b++; return b; }  // bits that hold 0 .. v-1

struct TableQuery {
    uint64_t n_pairs = 0, n_models = 0, n_chains = 0;
    uint32_t max_ent_rank = 0;  // the largest rank of an entity inside its chain
    bool any_icode = false;     // an atom carries an insertion code (else the long way skips that pass)
    int knob_key_bits = 0;      // arp_debug_set("table_key_bits"): 0 = 64
};
// Passes are k_row_key's: 0 distance, 1 insertion codes, 2 {to rank, interaction}, 3 from rank, 4 {model, from chain, to chain}, 5 = 4 + 3, 6 = 5 + 2.
struct TablePlan {
    uint32_t model_bits, chain_bits, rank_bits, limit;
    bool few_pairs, keys_fit_small, small_try;  // small_try = few_pairs && keys_fit_small: k_table_small is launched
    int n_pass, pass[3], end_bit[3];            // the general path, least significant key first (k_tie_fix puts tied rows in order afterwards)
    int n_long, long_pass[5], long_end_bit[5];  // "the long way": the tie-breaking keys as passes of their own in front of the same passes
    int digits;                                 // the passes as decimal digits: 6, 25 or 234
};

inline bool table_few_pairs(uint64_t n_pairs) { return n_pairs <= kSmallPairs; }  // (known before the structure's ranks are: device_table's first branch)

inline TablePlan plan_table(const TableQuery &q) {
    TablePlan p{};
    p.model_bits = table_width(q.n_models > 1 ? q.n_models : 1);
    p.chain_bits = table_width(q.n_chains > 1 ? q.n_chains : 1);
    p.rank_bits = table_width((uint64_t)q.max_ent_rank + 1);
    p.limit = q.knob_key_bits > 0 ? (uint32_t)q.knob_key_bits : 64u;
    const uint32_t top = p.model_bits + 2 * p.chain_bits, all = top + 2 * p.rank_bits + 5;
    p.few_pairs = table_few_pairs(q.n_pairs);
    p.keys_fit_small = all + kSmallIdxBits <= p.limit;  // the ten keys + a row index in one sort word
    p.small_try = p.few_pairs && p.keys_fit_small;
    auto add = [&](int pass, uint32_t end) { p.pass[p.n_pass] = pass; p.end_bit[p.n_pass++] = (int)end; };
    if (all <= p.limit) add(6, all);
    else {
        add(2, p.rank_bits + 5);
        if (top + p.rank_bits <= p.limit) add(5, top + p.rank_bits);
        else { add(3, p.rank_bits); add(4, top); }
    }
    p.long_pass[p.n_long] = 0; p.long_end_bit[p.n_long++] = 32;
    if (q.any_icode) { p.long_pass[p.n_long] = 1; p.long_end_bit[p.n_long++] = 64; }
    for (int k = 0; k < p.n_pass; k++) { p.long_pass[p.n_long] = p.pass[k]; p.long_end_bit[p.n_long++] = p.end_bit[k]; p.digits = 10 * p.digits + p.pass[k]; }
    return p;
}

// What the last table call of the process did (arp_debug_get "table_*").
struct TableRoute {
    long long small = -1;   // -1: k_table_small not tried; 0: it finished the table; 1 / 2 / 3: its status (rows, tie run, ring rows); 4: refused by key width
    long long pairs = 0, atom_rows = 0, ring_rows = 0;
    long long plan = 0;     // the general path's passes as decimal digits; 0: it did not sort
    long long long_way = 0; // 1: a tie run beyond k_tie_fix, sorted again the long way
    long long ring_cap = 0; // ring rows reserved when the call ended
};

}  // namespace arp
