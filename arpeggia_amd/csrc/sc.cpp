// Shape complementarity, host side (reference src/sc/mod.rs:51-80, sc_calculator.rs:29-347): the selection, the Lawrence & Colman radii,
// input checks, the statistics of the per-dot arrays (sums in dot order, medians by nth_element) and the C ABI.  The device stages are in
// sc.inl (launch_sc); the contract is DESIGN.md section 3.6.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

#include "arp_internal.h"
#include "host_common.h"

namespace arp {
// engine.cpp: the stream, the profiler (restarted when `call`) and the kept dots of the context
arp_status context_sc(arp_context *ctx, bool call, hipStream_t *st, Profiler **prof, std::vector<ScDot> **dots);

// Lawrence & Colman (1993) atomic radii, the reference's embedded table (atomic_radii.rs:9-410) in its order: residue pattern, atom
// pattern, radius.  Generated from tests/golden/sc_radii.csv by tools/sc_radii_table.py.
struct ScRadius { const char *res, *atom; double r; };
static const ScRadius kScRadii[] = {
    {"ALA", "CB", 1.95}, {"ARG", "NH*", 1.70}, {"ARG", "CZ", 1.80}, {"ARG", "NE", 1.65}, {"ARG", "CD", 1.90}, {"ARG", "CG", 1.90},
    {"ASN", "ND2", 1.70}, {"ASN", "OD1", 1.60}, {"ASN", "CG", 1.80}, {"ASP", "OD*", 1.60}, {"ASP", "CG", 1.80}, {"GLN", "NE2", 1.70},
    {"GLN", "OE1", 1.60}, {"GLN", "CD", 1.80}, {"GLN", "CG", 1.90}, {"GLU", "OE*", 1.60}, {"GLU", "CD", 1.80}, {"GLU", "CG", 1.90},
    {"GLY", "CA", 1.90}, {"HIS", "CD2", 1.90}, {"HIS", "NE2", 1.65}, {"HIS", "CE1", 1.90}, {"HIS", "ND1", 1.65}, {"HIS", "CG", 1.80},
    {"HOH", "O**", 1.70}, {"ILE", "CD1", 1.95}, {"ILE", "CG1", 1.90}, {"ILE", "CB", 1.85}, {"ILE", "CG2", 1.95}, {"LEU", "CD*", 1.95},
    {"LEU", "CG", 1.85}, {"LYS", "NZ", 1.75}, {"LYS", "CE", 1.90}, {"LYS", "CD", 1.90}, {"LYS", "CG", 1.90}, {"MET", "CE", 1.95},
    {"MET", "CG", 1.90}, {"PHE", "CD*", 1.90}, {"PHE", "CE*", 1.90}, {"PHE", "CZ", 1.90}, {"PHE", "CG", 1.80}, {"PRO", "CD", 1.90},
    {"PRO", "CG", 1.90}, {"SER", "OG", 1.70}, {"SUL", "S", 1.90}, {"SUL", "O***", 1.65}, {"THR", "CG2", 1.95}, {"THR", "OG1", 1.70},
    {"THR", "CB", 1.85}, {"TRP", "CE2", 1.80}, {"TRP", "CE3", 1.90}, {"TRP", "CD1", 1.90}, {"TRP", "CD2", 1.80}, {"TRP", "CZ*", 1.90},
    {"TRP", "CH2", 1.90}, {"TRP", "NE1", 1.65}, {"TRP", "CG", 1.80}, {"TYR", "OH", 1.70}, {"TYR", "CD*", 1.90}, {"TYR", "CE*", 1.90},
    {"TYR", "CZ", 1.80}, {"TYR", "CG", 1.80}, {"VAL", "CG*", 1.95}, {"VAL", "CB", 1.85}, {"WAT", "O", 1.70}, {"WAT", "O*", 1.70},
    {"***", "H", 0.50}, {"***", "H*", 0.50}, {"***", "H**", 0.50}, {"***", "H***", 0.50}, {"***", "CA", 1.85}, {"***", "C", 1.80},
    {"***", "O", 1.60}, {"***", "N", 1.65}, {"***", "CB", 1.90}, {"***", "OT*", 1.60}, {"***", "OXT", 1.60}, {"***", "S*", 1.90},
    {"***", "P", 1.80},
};

// atomic_radii.rs:413-440: trailing spaces trimmed from both; a pattern starting with '*' matches anything; '*' at position p matches
// when the first p characters are equal; otherwise exact
static bool wildcard_match(const char *query, const char *pattern) {
    size_t q = strlen(query), p = strlen(pattern);
    while (q && query[q - 1] == ' ') q--;
    while (p && pattern[p - 1] == ' ') p--;
    if (p && pattern[0] == '*') return true;
    const char *star = (const char *)memchr(pattern, '*', p);
    if (star) {
        const size_t k = (size_t)(star - pattern);
        return q >= k && memcmp(query, pattern, k) == 0;
    }
    return q == p && memcmp(query, pattern, q) == 0;
}

static double sc_radius(const char *resn, const char *atomn, const char *element) {
    for (const ScRadius &e : kScRadii)  // sc_calculator.rs:57-70 via surface_generator.rs:95-109: first match
        if (wildcard_match(resn, e.res) && wildcard_match(atomn, e.atom)) return e.r;
    const int32_t c = element ? arp_element_class(element) : -1;  // fallback: pdbtbx's van der Waals radius
    if (c < 0) return 0.0;
    arp_params p;
    arp_default_params(&p);
    const double v = p.vdw_radius[c];
    return v > 0.0 ? v : 0.0;
}

static bool settings_ok(const arp_sc_settings &s) {
    return std::isfinite(s.probe_radius) && s.probe_radius > 0.0 && std::isfinite(s.dot_density) && s.dot_density > 0.0 && std::isfinite(s.peripheral_band) &&
           s.peripheral_band >= 0.0 && std::isfinite(s.separation_cutoff) && s.separation_cutoff > 0.0 && std::isfinite(s.gaussian_w);
}

// mod.rs:51-80: parse_groups, prepare_pdb_for_sasa(remove H, solvent and ions, chains of both groups), filter_pdb_by_model -- steps 1-4 of
// arp_structure_sasa_select (sasa.cpp select_atoms), no step 5 -- and the molecule of each atom (group 1 first)
static arp_status sc_select(const arp_structure *s, const char *groups, int32_t model_num, std::vector<uint32_t> *atoms, std::vector<uint8_t> *mol) {
    std::vector<std::string> g1, g2;
    arp_status st = parse_groups(s->chain_ids, groups, &g1, &g2);
    if (st != ARP_OK) return st;
    std::unordered_set<std::string> k1(g1.begin(), g1.end()), both = k1;
    both.insert(g2.begin(), g2.end());
    *atoms = select_atoms(s, both, true, true, false, model_num);
    mol->resize(atoms->size());
    for (size_t k = 0; k < atoms->size(); k++) (*mol)[k] = k1.count(std::string(s->chain.at((*atoms)[k]))) ? 0 : 1;
    return ARP_OK;
}

// the combined surface and the three headline numbers from the two surfaces (sc_calculator.rs:316-347)
static void sc_combine(arp_sc_results *o);
// sc_calculator.rs:143-347 on the device's per-dot arrays
static void sc_stats(const std::vector<ScDot> *dots, arp_sc_results *o) {
    for (int m = 0; m < 2; m++) {
        arp_sc_surface &S = o->surface[m];
        S.n_all_dots = dots[m].size();
        std::vector<double> d, sv;
        double area = 0.0, dsum = 0.0, ssum = 0.0;
        for (const ScDot &p : dots[m]) {
            if (!(p.flags & ARP_SC_DOT_TRIMMED)) continue;
            area += p.area;
            d.push_back(p.nn_dist); sv.push_back(p.score);
            dsum += p.nn_dist; ssum += -p.score;
        }
        S.n_trimmed_dots = d.size();
        S.trimmed_area = area;
        bool other = false;
        for (const ScDot &p : dots[1 - m]) if (p.flags & ARP_SC_DOT_TRIMMED) { other = true; break; }
        if (d.empty() || !other) continue;  // (calc_neighbor_distance returns early: zeros)
        const size_t k = d.size() / 2;
        std::nth_element(d.begin(), d.begin() + k, d.end());
        std::nth_element(sv.begin(), sv.begin() + k, sv.end());
        S.d_mean = dsum / (double)d.size(); S.d_median = d[k];
        S.s_mean = -(ssum / (double)sv.size()); S.s_median = sv[k];
    }
    sc_combine(o);
}
static void sc_combine(arp_sc_results *o) {
    arp_sc_surface &C = o->combined;
    const arp_sc_surface &a = o->surface[0], &b = o->surface[1];
    C.n_atoms = a.n_atoms + b.n_atoms; C.n_buried_atoms = a.n_buried_atoms + b.n_buried_atoms; C.n_far_atoms = a.n_far_atoms + b.n_far_atoms;
    C.n_all_dots = a.n_all_dots + b.n_all_dots; C.n_trimmed_dots = a.n_trimmed_dots + b.n_trimmed_dots; C.trimmed_area = a.trimmed_area + b.trimmed_area;
    C.d_mean = (a.d_mean + b.d_mean) / 2.0; C.d_median = (a.d_median + b.d_median) / 2.0;
    C.s_mean = (a.s_mean + b.s_mean) / 2.0; C.s_median = (a.s_median + b.s_median) / 2.0;
    o->sc = C.s_median; o->distance = C.d_median; o->area = C.trimmed_area;
}

// names(i) describes atom i for the Coincident message ("serial:resn:atomn" at the structure level)
template <class Names>
static arp_status sc_run(arp_context *ctx, uint64_t n, const double *x, const double *y, const double *z, const double *r, const uint8_t *molecule,
                         const int64_t *serial, const arp_sc_settings &set, arp_sc_results *out, Names &&names) {
    memset(out, 0, sizeof *out);
    if (!settings_ok(set)) { set_error("bad SC settings (probe radius and dot density must be > 0, the band >= 0, the cutoff > 0, all finite)"); return ARP_ERR_BAD_INPUT; }
    if (n >= 0x40000000ull) { set_error("too many atoms for one SC call"); return ARP_ERR_BAD_INPUT; }
    std::vector<uint32_t> mol(n);
    std::vector<long long> ser(n);
    for (uint64_t i = 0; i < n; i++) {
        if (!(std::isfinite(x[i]) && std::isfinite(y[i]) && std::isfinite(z[i]))) { set_error("non-finite atom coordinate"); return ARP_ERR_BAD_INPUT; }
        if (!(std::isfinite(r[i]) && r[i] > 0.0)) { set_error("atom %llu: the radius must be finite and > 0", (unsigned long long)i); return ARP_ERR_BAD_INPUT; }
        if (molecule[i] > 1) { set_error("molecule must be 0 or 1"); return ARP_ERR_BAD_INPUT; }
        mol[i] = molecule[i];
        ser[i] = serial ? (long long)serial[i] : (long long)i;
        out->surface[mol[i]].n_atoms++;
    }
    {
        std::vector<long long> s = ser;
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end()) { set_error("duplicate atom serial numbers: the reference keys its maps by serial"); return ARP_ERR_BAD_INPUT; }
    }
    if (n == 0) { set_error("No atoms defined"); return ARP_ERR_BAD_INPUT; }
    if (out->surface[0].n_atoms == 0) { set_error("Failed to read radii: No atoms for chain group 1"); return ARP_ERR_BAD_INPUT; }  // (group 1 only, :148-155)
    hipStream_t st;
    Profiler *prof;
    std::vector<ScDot> *keep;
    arp_status s = context_sc(ctx, true, &st, &prof, &keep);
    if (s != ARP_OK) return s;
    ScJob j{(uint32_t)n, x, y, z, r, mol.data(), ser.data(), set.probe_radius, set.dot_density, set.peripheral_band, set.separation_cutoff, set.gaussian_w};
    ScRunOut R;
    if ((s = launch_sc(j, st, prof, &R)) != ARP_OK) return s;
    if (R.err == kScErrCoincident) {
        set_error("Overlapping atoms detected: %s == %s", names(R.err_i).c_str(), names(R.err_j).c_str());
        return ARP_ERR_BAD_INPUT;
    }
    if (R.err == kScErrSubdiv) { set_error("Sampling limit exceeded"); return ARP_ERR_BAD_INPUT; }
    for (uint64_t i = 0; i < n; i++) (R.att[i] ? out->surface[mol[i]].n_buried_atoms : out->surface[mol[i]].n_far_atoms)++;
    out->n_convex = R.n_convex; out->n_toroidal = R.n_toroidal; out->n_concave = R.n_concave; out->n_probes = R.n_probes;
    if (R.dots[0].empty() || R.dots[1].empty()) {
        out->surface[0].n_all_dots = R.dots[0].size(); out->surface[1].n_all_dots = R.dots[1].size();
        set_error("Failed to read radii: No molecular dots generated");
        return ARP_ERR_BAD_INPUT;
    }
    sc_stats(R.dots, out);
    keep[0].swap(R.dots[0]); keep[1].swap(R.dots[1]);
    return ARP_OK;
}

// ---- the frames of an ensemble (device side: sc_ens.inl) ----
// The checks of sc_run that do not depend on the coordinates, in its order; fills mol, ser and the atom counts per molecule.
static arp_status sc_ens_check(uint64_t n, uint64_t n_frames, const double *r, const uint8_t *molecule, const int64_t *serial, const arp_sc_settings &set,
                               std::vector<uint32_t> *mol, std::vector<long long> *ser, uint64_t n_atoms[2]) {
    if (!settings_ok(set)) { set_error("bad SC settings (probe radius and dot density must be > 0, the band >= 0, the cutoff > 0, all finite)"); return ARP_ERR_BAD_INPUT; }
    if (n_frames == 0) { set_error("sc ensemble: at least one frame is needed"); return ARP_ERR_BAD_INPUT; }
    if (n >= 0x40000000ull) { set_error("too many atoms for one SC call"); return ARP_ERR_BAD_INPUT; }
    if (n_frames > (1ull << 40) / std::max<uint64_t>(n, 1)) { set_error("sc ensemble: too many frames"); return ARP_ERR_BAD_INPUT; }
    mol->resize(n); ser->resize(n);
    n_atoms[0] = n_atoms[1] = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (!(std::isfinite(r[i]) && r[i] > 0.0)) { set_error("atom %llu: the radius must be finite and > 0", (unsigned long long)i); return ARP_ERR_BAD_INPUT; }
        if (molecule[i] > 1) { set_error("molecule must be 0 or 1"); return ARP_ERR_BAD_INPUT; }
        (*mol)[i] = molecule[i];
        (*ser)[i] = serial ? (long long)serial[i] : (long long)i;
        n_atoms[molecule[i]]++;
    }
    std::vector<long long> sorted = *ser;
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) { set_error("duplicate atom serial numbers: the reference keys its maps by serial"); return ARP_ERR_BAD_INPUT; }
    if (n == 0) { set_error("No atoms defined"); return ARP_ERR_BAD_INPUT; }
    if (n_atoms[0] == 0) { set_error("Failed to read radii: No atoms for chain group 1"); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}
// xyz: [F][n][3], checked finite by the caller.  results[f] of a failed frame holds what arp_sc leaves in *out on the same error.
static arp_status sc_ens_run(arp_context *ctx, uint64_t n, uint64_t F, const double *xyz, const double *r, const std::vector<uint32_t> &mol,
                             const std::vector<long long> &ser, const uint64_t n_atoms[2], const arp_sc_settings &set, arp_sc_results *results, uint32_t *status,
                             uint32_t *err_atoms, uint32_t *frames_in_interface, uint64_t *trimmed_dots) {
    hipStream_t st;
    Profiler *prof;
    std::vector<ScDot> *keep;  // (left as the last single-frame call made them)
    arp_status s = context_sc(ctx, true, &st, &prof, &keep);
    if (s != ARP_OK) return s;
    ScEnsJob j{(uint32_t)n, F, xyz, r, mol.data(), ser.data(), set.probe_radius, set.dot_density, set.peripheral_band, set.separation_cutoff, set.gaussian_w,
               g_debug.sc_ens_frames > 0 ? (uint32_t)g_debug.sc_ens_frames : 0u};
    std::vector<arp_sc_surface> surf(2 * F);
    std::vector<ScEnsFrame> fr(F);
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "accumulator width");
    ScEnsOut o{surf.data(), fr.data(), frames_in_interface, (unsigned long long *)trimmed_dots};
    if ((s = launch_sc_ens(j, st, prof, &o)) != ARP_OK) return s;
    for (uint64_t f = 0; f < F; f++) {
        arp_sc_results &R = results[f];
        memset(&R, 0, sizeof R);
        const ScEnsFrame &q = fr[f];
        for (int m = 0; m < 2; m++) R.surface[m].n_atoms = n_atoms[m];
        if (err_atoms) { err_atoms[2 * f] = ~0u; err_atoms[2 * f + 1] = ~0u; }
        if (q.ci != ~0u || q.cj != ~0u) {
            status[f] = ARP_SC_FRAME_COINCIDENT;
            if (err_atoms) { err_atoms[2 * f] = q.ci; err_atoms[2 * f + 1] = q.cj; }
            continue;
        }
        if (q.subdiv) { status[f] = ARP_SC_FRAME_SUBDIV; continue; }
        uint64_t nS[2];
        for (int m = 0; m < 2; m++) {
            R.surface[m].n_buried_atoms = q.att[m]; R.surface[m].n_far_atoms = n_atoms[m] - q.att[m];
            nS[m] = (uint64_t)q.nT[m] + q.nC[m] + q.nK[m];
        }
        R.n_convex = (uint64_t)q.nC[0] + q.nC[1]; R.n_toroidal = (uint64_t)q.nT[0] + q.nT[1]; R.n_concave = (uint64_t)q.nK[0] + q.nK[1]; R.n_probes = q.n_probes;
        if (nS[0] == 0 || nS[1] == 0) {
            status[f] = ARP_SC_FRAME_NO_DOTS;
            R.surface[0].n_all_dots = nS[0]; R.surface[1].n_all_dots = nS[1];
            continue;
        }
        status[f] = ARP_SC_FRAME_OK;
        for (int m = 0; m < 2; m++) {
            const arp_sc_surface &D = surf[2 * f + m];
            arp_sc_surface &S = R.surface[m];
            S.n_all_dots = D.n_all_dots; S.n_trimmed_dots = D.n_trimmed_dots; S.trimmed_area = D.trimmed_area;
            S.d_mean = D.d_mean; S.d_median = D.d_median; S.s_mean = D.s_mean; S.s_median = D.s_median;
        }
        sc_combine(&R);
    }
    return ARP_OK;
}
// the first frame with a non-finite coordinate among the listed atoms (all when sel is null) is an input error
static arp_status sc_ens_finite(uint64_t F, uint64_t n0, const double *xyz, const std::vector<uint32_t> *sel, uint64_t n) {
    for (uint64_t f = 0; f < F; f++)
        for (uint64_t k = 0; k < n; k++) {
            const uint64_t i = sel ? (*sel)[k] : k;
            const double *c = xyz + 3 * (f * n0 + i);
            if (!(std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2]))) {
                set_error("sc ensemble: non-finite coordinate in frame %llu, atom %llu", (unsigned long long)f, (unsigned long long)i);
                return ARP_ERR_BAD_INPUT;
            }
        }
    return ARP_OK;
}
}  // namespace arp

using namespace arp;

extern "C" void arp_sc_default_settings(arp_sc_settings *o) {
    if (o) *o = arp_sc_settings{1.7, 15.0, 1.5, 8.0, 0.5};  // settings.rs
}

extern "C" double arp_sc_radius(const char *resn, const char *atomn, const char *element) {
    return sc_radius(resn ? resn : "", atomn ? atomn : "", element);
}

extern "C" arp_status arp_sc(arp_context *ctx, uint64_t n, const double *x, const double *y, const double *z, const double *radius, const uint8_t *molecule,
                             const int64_t *serial, const arp_sc_settings *settings, arp_sc_results *out) try {
    if (!ctx || !out || (n && (!x || !y || !z || !radius || !molecule))) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    arp_sc_settings set;
    arp_sc_default_settings(&set);
    if (settings) set = *settings;
    return sc_run(ctx, n, x, y, z, radius, molecule, serial, set, out, [&](uint32_t i) { return std::to_string(serial ? (long long)serial[i] : (long long)i); });
} ARP_ABI_CATCH

extern "C" arp_status arp_structure_sc_select(const arp_structure *s, const char *groups, int32_t model_num, uint64_t *n_out, uint32_t *out_atoms,
                                              uint8_t *out_molecule) try {
    if (!s || !groups || !n_out) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    std::vector<uint32_t> atoms;
    std::vector<uint8_t> mol;
    arp_status st = sc_select(s, groups, model_num, &atoms, &mol);
    if (st != ARP_OK) return st;
    *n_out = atoms.size();
    if (out_atoms) std::copy(atoms.begin(), atoms.end(), out_atoms);
    if (out_molecule) std::copy(mol.begin(), mol.end(), out_molecule);
    return ARP_OK;
} ARP_ABI_CATCH

extern "C" arp_status arp_structure_sc(arp_context *ctx, const arp_structure *s, const char *groups, int32_t model_num, arp_sc_results *out) try {
    if (!ctx || !s || !groups || !out) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    std::vector<uint32_t> atoms;
    std::vector<uint8_t> mol;
    arp_status st = sc_select(s, groups, model_num, &atoms, &mol);
    if (st != ARP_OK) return st;
    const uint64_t m = atoms.size();
    std::vector<double> x(m), y(m), z(m), r(m);
    std::vector<int64_t> ser(m);
    for (uint64_t k = 0; k < m; k++) {
        const uint32_t i = atoms[k];
        x[k] = s->x[i]; y[k] = s->y[i]; z[k] = s->z[i]; ser[k] = s->serial[i];
        r[k] = sc_radius(s->res_resn.at(i), s->name.at(i), s->elem.at(i));
        if (!(r[k] > 0.0)) {
            // the fallback knows the van der Waals radii of this project's element classes only (arp_params.vdw_radius); pdbtbx has more
            // (e.g. Fe, Cu, Mn), for which the reference computes a value -- DESIGN.md section 3.6
            set_error("atom %d (%s:%s, element '%s'): no Lawrence & Colman radius and no van der Waals radius for this element class", s->serial[i],
                      s->res_resn.at(i), s->name.at(i), s->elem.at(i));
            return ARP_ERR_BAD_INPUT;
        }
    }
    return sc_run(ctx, m, x.data(), y.data(), z.data(), r.data(), mol.data(), ser.data(), arp_sc_settings{1.7, 15.0, 1.5, 8.0, 0.5}, out, [&](uint32_t k) {
        const uint32_t i = atoms[k];
        return std::to_string(s->serial[i]) + ":" + s->res_resn.at(i) + ":" + s->name.at(i);
    });
} ARP_ABI_CATCH

extern "C" arp_status arp_sc_dots(arp_context *ctx, int32_t surface, uint64_t cap, uint64_t *n, double *xyz, double *normal, double *area, uint32_t *flags,
                                  double *nn_dist, double *score) try {
    if (!ctx || !n || surface < 0 || surface > 1) { set_error("bad argument"); return ARP_ERR_BAD_INPUT; }
    hipStream_t st;
    Profiler *prof;
    std::vector<ScDot> *keep;
    arp_status s = context_sc(ctx, false, &st, &prof, &keep);
    if (s != ARP_OK) return s;
    const std::vector<ScDot> &D = keep[surface];
    *n = D.size();
    if (cap < D.size()) return ARP_OK;
    for (size_t k = 0; k < D.size(); k++) {
        for (int c = 0; c < 3; c++) { if (xyz) xyz[3 * k + c] = D[k].p[c]; if (normal) normal[3 * k + c] = D[k].n[c]; }
        if (area) area[k] = D[k].area;
        if (flags) flags[k] = D[k].flags;
        if (nn_dist) nn_dist[k] = D[k].nn_dist;
        if (score) score[k] = D[k].score;
    }
    return ARP_OK;
} ARP_ABI_CATCH

extern "C" arp_status arp_sc_ensemble(arp_context *ctx, uint64_t n, uint64_t n_frames, const double *xyz, const double *radius, const uint8_t *molecule,
                                      const int64_t *serial, const arp_sc_settings *settings, arp_sc_results *results, uint32_t *status, uint32_t *err_atoms,
                                      uint32_t *frames_in_interface, uint64_t *trimmed_dots) try {
    if (n && (!xyz || !radius || !molecule)) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    if (ctx && (!results || !status || !frames_in_interface || !trimmed_dots)) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    arp_sc_settings set;
    arp_sc_default_settings(&set);
    if (settings) set = *settings;
    std::vector<uint32_t> mol;
    std::vector<long long> ser;
    uint64_t n_atoms[2];
    arp_status st = sc_ens_check(n, n_frames, radius, molecule, serial, set, &mol, &ser, n_atoms);
    if (st != ARP_OK) return st;
    if ((st = sc_ens_finite(n_frames, n, xyz, nullptr, n)) != ARP_OK) return st;
    if (!ctx) return ARP_OK;  // the checks only
    return sc_ens_run(ctx, n, n_frames, xyz, radius, mol, ser, n_atoms, set, results, status, err_atoms, frames_in_interface, trimmed_dots);
} ARP_ABI_CATCH

extern "C" arp_status arp_structure_sc_ensemble(arp_context *ctx, const arp_structure *s, uint64_t n_frames, const double *xyz, const char *groups,
                                                uint64_t *n_rows, uint64_t *frames_used, uint32_t *out_atoms, uint8_t *out_molecule, arp_sc_results *results,
                                                uint32_t *status, uint32_t *err_atoms, uint32_t *frames_in_interface, uint64_t *trimmed_dots) try {
    if (!s || !groups || !n_rows || !frames_used) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    *n_rows = 0; *frames_used = 0;
    // validation: nothing here touches the device
    uint64_t n0 = 0, r0 = 0, nm = 1;
    arp_status st = freq_topology(s, xyz == nullptr, &n0, &r0, &nm);
    if (st != ARP_OK) return st;
    const uint64_t F = xyz ? n_frames : nm;
    std::vector<uint32_t> atoms;
    std::vector<uint8_t> molecule;
    if ((st = sc_select(s, groups, 0, &atoms, &molecule)) != ARP_OK) return st;
    while (!atoms.empty() && atoms.back() >= n0) { atoms.pop_back(); molecule.pop_back(); }
    const uint64_t m = atoms.size();
    std::vector<double> r(m);
    std::vector<int64_t> serial(m);
    for (uint64_t k = 0; k < m; k++) {
        const uint32_t i = atoms[k];
        serial[k] = s->serial[i];
        r[k] = sc_radius(s->res_resn.at(i), s->name.at(i), s->elem.at(i));
        if (!(r[k] > 0.0)) {  // (as arp_structure_sc refuses it)
            set_error("atom %d (%s:%s, element '%s'): no Lawrence & Colman radius and no van der Waals radius for this element class", s->serial[i],
                      s->res_resn.at(i), s->name.at(i), s->elem.at(i));
            return ARP_ERR_BAD_INPUT;
        }
    }
    const arp_sc_settings set{1.7, 15.0, 1.5, 8.0, 0.5};
    std::vector<uint32_t> mol;
    std::vector<long long> ser;
    uint64_t n_atoms[2];
    if ((st = sc_ens_check(m, F, r.data(), molecule.data(), serial.data(), set, &mol, &ser, n_atoms)) != ARP_OK) return st;
    std::vector<double> model_xyz;
    if (!xyz) {
        model_xyz.resize(F * n0 * 3);
        for (uint64_t a = 0; a < F * n0; a++) { model_xyz[3 * a] = s->x[a]; model_xyz[3 * a + 1] = s->y[a]; model_xyz[3 * a + 2] = s->z[a]; }
        xyz = model_xyz.data();
    }
    if ((st = sc_ens_finite(F, n0, xyz, &atoms, m)) != ARP_OK) return st;
    *frames_used = F;
    if (out_atoms) std::copy(atoms.begin(), atoms.end(), out_atoms);
    if (out_molecule) std::copy(molecule.begin(), molecule.end(), out_molecule);
    if (!ctx) { *n_rows = m; return ARP_OK; }  // validation only: the selection and the frame count
    if (!out_atoms || !out_molecule || !results || !status || !frames_in_interface || !trimmed_dots) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    std::vector<double> packed(F * m * 3);
    for (uint64_t f = 0; f < F; f++)
        for (uint64_t k = 0; k < m; k++) for (int c = 0; c < 3; c++) packed[3 * (f * m + k) + c] = xyz[3 * (f * n0 + atoms[k]) + c];
    if ((st = sc_ens_run(ctx, m, F, packed.data(), r.data(), mol, ser, n_atoms, set, results, status, err_atoms, frames_in_interface, trimmed_dots)) != ARP_OK) return st;
    *n_rows = m;
    return ARP_OK;
} ARP_ABI_CATCH

static arp_status sc_dot_stats_check(uint64_t n_seg, const uint64_t *seg_start, const uint32_t *flags, const double *area, const double *nn_dist,
                                     const double *score, const uint32_t *other, arp_sc_surface *out) {
    if (!seg_start || !other || !out) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    if (n_seg >= 0x7FFFFFFFull) { set_error("arp_sc_dot_stats: too many segments"); return ARP_ERR_BAD_INPUT; }
    for (uint64_t k = 0; k < n_seg; k++) {
        if (seg_start[k + 1] < seg_start[k]) { set_error("arp_sc_dot_stats: seg_start must not decrease"); return ARP_ERR_BAD_INPUT; }
        if (other[k] >= n_seg) { set_error("arp_sc_dot_stats: other[%llu] names no segment", (unsigned long long)k); return ARP_ERR_BAD_INPUT; }
    }
    if (seg_start[0] != 0) { set_error("arp_sc_dot_stats: seg_start[0] must be 0"); return ARP_ERR_BAD_INPUT; }
    if (seg_start[n_seg] && (!flags || !area || !nn_dist || !score)) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}

extern "C" arp_status arp_sc_dot_stats_host(uint64_t n_seg, const uint64_t *seg_start, const uint32_t *flags, const double *area, const double *nn_dist,
                                            const double *score, const uint32_t *other, arp_sc_surface *out) try {
    const arp_status st = sc_dot_stats_check(n_seg, seg_start, flags, area, nn_dist, score, other, out);
    if (st != ARP_OK) return st;
    sc_dot_stats_host(n_seg, seg_start, flags, area, nn_dist, score, other, out);
    return ARP_OK;
} ARP_ABI_CATCH

extern "C" arp_status arp_sc_dot_stats(arp_context *ctx, uint64_t n_seg, const uint64_t *seg_start, const uint32_t *flags, const double *area,
                                       const double *nn_dist, const double *score, const uint32_t *other, arp_sc_surface *out) try {
    if (!ctx) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    arp_status st = sc_dot_stats_check(n_seg, seg_start, flags, area, nn_dist, score, other, out);
    if (st != ARP_OK) return st;
    hipStream_t stream;
    Profiler *prof;
    std::vector<ScDot> *keep;
    if ((st = context_sc(ctx, false, &stream, &prof, &keep)) != ARP_OK) return st;
    return launch_sc_dot_stats(n_seg, seg_start, flags, area, nn_dist, score, other, out, stream);
} ARP_ABI_CATCH

extern "C" arp_status arp_sc_dot_atoms(arp_context *ctx, int32_t surface, uint64_t cap, uint64_t *n, uint32_t *atom) try {
    if (!ctx || !n || surface < 0 || surface > 1) { set_error("bad argument"); return ARP_ERR_BAD_INPUT; }
    hipStream_t st;
    Profiler *prof;
    std::vector<ScDot> *keep;
    const arp_status s = context_sc(ctx, false, &st, &prof, &keep);
    if (s != ARP_OK) return s;
    const std::vector<ScDot> &D = keep[surface];
    *n = D.size();
    if (cap < D.size() || !atom) return ARP_OK;
    for (size_t k = 0; k < D.size(); k++) atom[k] = D[k].atom;
    return ARP_OK;
} ARP_ABI_CATCH
