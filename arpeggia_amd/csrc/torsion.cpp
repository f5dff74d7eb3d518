// Torsion angles (phi, psi, omega, chi), their rotamer states and Ramachandran maps across the frames of an ensemble: the checks and
// the host half of arp_torsions (device pipeline: torsion.inl), and the definition in plain sequential C++, arp_torsions_host, its yardstick.  One torsion is
// torsion_eval / torsion_bin of table_dev.h on both sides.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "debug_knobs.h"
#include "table.h"

using namespace arp;

namespace {
// the checks that need no topology: bins, histograms, pairs
arp_status shape_check(uint64_t n_tors, uint32_t n_bins, const uint32_t *pairs, uint64_t n_pairs, uint32_t n_groups, bool hist, bool hist2) {
    if (n_tors == 0) { set_error("torsions: no torsions (n_tors == 0)"); return ARP_ERR_BAD_INPUT; }
    if (n_tors >= (1ull << 31)) { set_error("torsions: %llu torsions, at most 2^31 - 1 are supported", (unsigned long long)n_tors); return ARP_ERR_BAD_INPUT; }
    if (n_bins > kTorsionMaxBins) { set_error("torsions: n_bins = %u, at most %u are supported", n_bins, kTorsionMaxBins); return ARP_ERR_BAD_INPUT; }
    if ((hist || hist2) && n_bins == 0) { set_error("torsions: a histogram is asked for with n_bins == 0"); return ARP_ERR_BAD_INPUT; }
    if (hist2 && (n_groups == 0 || n_pairs == 0)) { set_error("torsions: hist2 is asked for with n_groups == %u and n_pairs == %llu", n_groups, (unsigned long long)n_pairs); return ARP_ERR_BAD_INPUT; }
    if (n_pairs >= (1ull << 31)) { set_error("torsions: %llu pairs, at most 2^31 - 1 are supported", (unsigned long long)n_pairs); return ARP_ERR_BAD_INPUT; }
    if (n_pairs && !pairs) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    for (uint64_t p = 0; p < n_pairs; p++) {
        for (int k = 0; k < 2; k++)
            if (pairs[3 * p + k] >= n_tors) {
                set_error("torsions: pairs[%llu][%d] = %u is not a torsion (%llu torsions)", (unsigned long long)p, k, pairs[3 * p + k], (unsigned long long)n_tors);
                return ARP_ERR_BAD_INPUT;
            }
        if (pairs[3 * p + 2] >= n_groups) {
            set_error("torsions: pairs[%llu][2] = %u is not a group (%u groups)", (unsigned long long)p, pairs[3 * p + 2], n_groups);
            return ARP_ERR_BAD_INPUT;
        }
    }
    return ARP_OK;
}
}  // namespace

extern "C" arp_status arp_torsions_host(uint64_t n_frames, uint64_t n_tors, const double *quad_xyz, uint32_t n_bins, const uint32_t *pairs, uint64_t n_pairs, uint32_t n_groups,
                                        float *angles, double *cossin, uint8_t *states, double *sums, uint32_t *n_defined, uint32_t *state_counts, uint32_t *n_transitions,
                                        uint32_t *hist, uint32_t *hist2) try {
    const uint64_t F = n_frames, D = n_tors, B = n_bins;
    if (F == 0) { set_error("torsions: at least one frame is needed"); return ARP_ERR_BAD_INPUT; }
    const arp_status st = shape_check(D, n_bins, pairs, n_pairs, n_groups, hist != nullptr, hist2 != nullptr);
    if (st != ARP_OK) return st;
    if (!quad_xyz || !sums || !n_defined || !state_counts || !n_transitions) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    for (uint64_t v = 0; v < F * D * 12; v++)
        if (!std::isfinite(quad_xyz[v])) {
            set_error("torsions: non-finite coordinate in frame %llu, torsion %llu", (unsigned long long)(v / (12 * D)), (unsigned long long)(v / 12 % D));
            return ARP_ERR_BAD_INPUT;
        }
    std::fill(sums, sums + D * 2, 0.0);
    std::fill(n_defined, n_defined + D, 0u);
    std::fill(state_counts, state_counts + D * 4, 0u);
    std::fill(n_transitions, n_transitions + D, 0u);
    if (hist) std::fill(hist, hist + D * B, 0u);
    if (hist2) std::fill(hist2, hist2 + (uint64_t)n_groups * B * B, 0u);
    std::vector<uint8_t> prev(D, 0), now(D, 0);
    std::vector<uint32_t> bin(D, 0);
    for (uint64_t f = 0; f < F; f++) {
        for (uint64_t d = 0; d < D; d++) {
            const double *q = quad_xyz + (f * D + d) * 12;
            const Torsion t = torsion_eval(q, q + 3, q + 6, q + 9);
            now[d] = t.state;
            const uint64_t e = f * D + d;
            if (angles) {
                const float a = (float)t.a;
                if (t.state) std::memcpy(angles + e, &a, 4);
                else std::memcpy(angles + e, &kTorsionNanBits, 4);
            }
            if (cossin) { cossin[2 * e] = t.c; cossin[2 * e + 1] = t.s; }
            if (states) states[e] = t.state;
            state_counts[4 * d + t.state]++;
            if (f && prev[d] && now[d] && prev[d] != now[d]) n_transitions[d]++;
            if (!t.state) continue;
            n_defined[d]++;
            sums[2 * d] += t.c; sums[2 * d + 1] += t.s;
            if (B) {
                bin[d] = torsion_bin(t.a, n_bins);
                if (hist) hist[d * B + bin[d]]++;
            }
        }
        if (hist2)
            for (uint64_t p = 0; p < n_pairs; p++) {
                const uint32_t a = pairs[3 * p], b = pairs[3 * p + 1], g = pairs[3 * p + 2];
                if (now[a] && now[b]) hist2[((uint64_t)g * B + bin[a]) * B + bin[b]]++;
            }
        prev.swap(now);
    }
    return ARP_OK;
} ARP_ABI_CATCH

extern "C" arp_status arp_torsions(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const uint32_t *quads, uint64_t n_tors, uint32_t n_bins,
                                   const uint32_t *pairs, uint64_t n_pairs, uint32_t n_groups, float *angles, double *cossin, uint8_t *states, double *sums, uint32_t *n_defined,
                                   uint32_t *state_counts, uint32_t *n_transitions, uint32_t *hist, uint32_t *hist2) try {
    std::vector<double> model_xyz;
    const double *frames = nullptr;
    uint64_t n0 = 0, F = 0;
    arp_status st = rmsd_frames_check(s, n_frames, xyz, &model_xyz, &frames, &n0, &F);
    if (st != ARP_OK) return st;
    if (F >= (1ull << 32)) { set_error("torsions: 2^32 or more frames"); return ARP_ERR_BAD_INPUT; }
    if ((st = shape_check(n_tors, n_bins, pairs, n_pairs, n_groups, hist != nullptr, hist2 != nullptr)) != ARP_OK) return st;
    if (!quads) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    for (uint64_t e = 0; e < n_tors * 4; e++)
        if (quads[e] >= n0) {
            set_error("torsions: quads[%llu][%llu] = %u is not an atom of the topology (%llu atoms)", (unsigned long long)(e / 4), (unsigned long long)(e % 4), quads[e],
                      (unsigned long long)n0);
            return ARP_ERR_BAD_INPUT;
        }
    const uint64_t need = torsion_resident_bytes(F, n_tors, n_bins, n_groups, hist != nullptr, hist2 != nullptr);
    if (need > rmsd_cap()) {
        set_error("torsions: the states of %llu frames (F) x %llu torsions (D) and the histograms of %u groups x %u bins need %llu bytes, the limit is %llu (rmsd_cap_bytes)",
                  (unsigned long long)F, (unsigned long long)n_tors, n_groups, n_bins, (unsigned long long)need, (unsigned long long)rmsd_cap());
        return ARP_ERR_CAPACITY;
    }
    if (!ctx) return ARP_OK;  // validation only
    if (!sums || !n_defined || !state_counts || !n_transitions) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    TorsionJob job;
    job.n_atoms = n0; job.n_frames = F; job.n_tors = n_tors; job.n_pairs = hist2 ? n_pairs : 0u; job.n_bins = n_bins; job.n_groups = n_groups;
    job.xyz = frames; job.quads = quads; job.pairs = pairs;
    job.chunk_atoms = g_debug.rmsd_chunk_atoms > 0 ? (uint64_t)g_debug.rmsd_chunk_atoms : 0u;
    job.hist2_route = g_debug.torsion_hist2_route;
    TorsionOut out;
    out.angles = angles; out.cossin = cossin; out.states = states; out.sums = sums; out.n_defined = n_defined; out.state_counts = state_counts; out.n_transitions = n_transitions;
    out.hist = hist; out.hist2 = hist2;
    return device_torsions(ctx, job, &out);
} ARP_ABI_CATCH
