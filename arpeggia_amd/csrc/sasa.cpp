// Structure-level SASA (atom, residue, chain, relative), SAP score and dSASA (reference src/sasa.rs:27-561, src/sap.rs:137-259): the atom
// selection of prepare_pdb_for_sasa + filter_pdb_by_model on the parsed structure, then one device run (sasa_dev.cpp sasa_run, kernels in
// sasa.inl and seg.inl).  The reference computes the residue and chain levels through rust-sasa's SASAOptions with a radius table of its own;
// here the table is named by the caller (ARP_RADII_PROTOR: the table that reproduces the reference's chain-level pin).
// dSASA, chain-level in the reference, is built from atom-level SASA (arpeggia_amd.h arp_structure_dsasa).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "arp_internal.h"
#include "host_common.h"

namespace arp {

// sasa.rs:44-51 SOLVENT_RESIDUES + ION_RESIDUES (exact, case-sensitive names, as `contains` compares them)
static bool solvent_or_ion(const char *resn) {
    static const char *k[] = {"HOH", "H2O", "D2O", "WAT", "TIP", "TIP3", "TIP4", "SPC", "NA", "CL", "K", "CA", "MG", "ZN", "FE", "MN",
                              "CU", "CO", "NI", "CD", "SO4", "PO4", "NO3", "ACE", "NH2"};
    for (const char *r : k) if (strcmp(r, resn) == 0) return true;
    return false;
}

// sasa.rs:71-81 parse_chain_string: split on ',', trim, drop empty entries
static std::unordered_set<std::string> chain_set(const char *chains) {
    std::unordered_set<std::string> out;
    std::string cur;
    auto push = [&]() {
        size_t b = 0, e = cur.size();
        while (b < e && isspace((unsigned char)cur[b])) b++;
        while (e > b && isspace((unsigned char)cur[e - 1])) e--;
        if (e > b) out.insert(cur.substr(b, e - b));
        cur.clear();
    };
    if (chains) {
        for (const char *p = chains; *p; p++) { if (*p == ',') push(); else cur.push_back(*p); }
        push();
    }
    return out;
}

// Steps 1-5 of arpeggia_amd.h arp_structure_sasa_select.  keep: chain ids to keep (empty = all); model_filter: step 4; serial_filter: step 5.
// (Also the selection of shape complementarity, sc.cpp: steps 1-4.)
std::vector<uint32_t> select_atoms(const arp_structure *s, const std::unordered_set<std::string> &keep, bool remove_h, bool model_filter,
                                          bool serial_filter, int32_t model_num) {
    const uint64_t n = s->n;
    uint32_t n_models = 0;
    for (uint64_t i = 0; i < n; i++) n_models = std::max(n_models, s->model[i] + 1u);
    uint32_t model_idx = ARP_NONE;  // step 4 (filter_pdb_by_model): only when there is more than one model
    if (model_filter && n_models > 1) {
        model_idx = 0;
        if (model_num != 0) {
            std::vector<int32_t> serial_of(n_models, 0);
            std::vector<uint8_t> seen(n_models, 0);
            for (uint64_t i = 0; i < n; i++) if (!seen[s->model[i]]) { seen[s->model[i]] = 1; serial_of[s->model[i]] = s->model_serial[i]; }
            for (uint32_t m = 0; m < n_models; m++) if (seen[m] && serial_of[m] == model_num) { model_idx = m; break; }
        }
    }
    std::vector<uint32_t> out;
    out.reserve(n);
    for (uint64_t i = 0; i < n; i++) {
        if (!keep.empty() && !keep.count(std::string(s->chain.at(i)))) continue;  // step 1
        if (remove_h && (s->base_attr[i] & ARP_ATTR_H)) continue;               // step 2 (element H)
        if (solvent_or_ion(s->res_resn.at(i))) continue;                           // step 3 (Residue::name)
        if (model_idx != ARP_NONE && s->model[i] != model_idx) continue;           // step 4
        if (serial_filter && s->model_serial[i] != model_num) continue;            // step 5 (sasa.rs:193)
        out.push_back((uint32_t)i);
    }
    return out;
}

static bool is_backbone(const char *name) {  // pdbtbx Atom::is_backbone (not in the reference's tree): the set the SAP test uses
    return !strcmp(name, "N") || !strcmp(name, "CA") || !strcmp(name, "C") || !strcmp(name, "O") || !strcmp(name, "OXT");
}

// ---- radius tables -------------------------------------------------------------------------------------------
// ARP_RADII_PROTOR: the ProtOr radii of Tsai, Taylor, Chothia & Gerstein 1999 by (residue, atom name), as FreeSASA lists them -- the table
// rust-sasa is believed to embed: with it the chain-level total of 1ubq is the reference's own pin (sasa.rs test_sasa_regression_ubiquitin).
namespace {
constexpr float C3H0 = 1.61f, C3H1 = 1.76f, C4H1 = 1.88f, C4H2 = 1.88f, C4H3 = 1.88f, N3H0 = 1.64f, N3H1 = 1.64f, N3H2 = 1.64f, N4H3 = 1.64f,
                O1H0 = 1.42f, O2H1 = 1.46f, S2H0 = 1.77f, S2H1 = 1.77f;
struct ProtorRow { const char *resn, *atom; float r; };
const ProtorRow ARP_PROTOR[] = {
    {"ANY", "N", N3H1}, {"ANY", "CA", C4H1}, {"ANY", "C", C3H0}, {"ANY", "O", O1H0}, {"ANY", "CB", C4H2}, {"ANY", "OXT", O2H1},
    {"ALA", "CB", C4H3},
    {"ARG", "CG", C4H2}, {"ARG", "CD", C4H2}, {"ARG", "NE", N3H1}, {"ARG", "CZ", C3H0}, {"ARG", "NH1", N3H2}, {"ARG", "NH2", N3H2},
    {"ASN", "CG", C3H0}, {"ASN", "OD1", O1H0}, {"ASN", "ND2", N3H2},
    {"ASP", "CG", C3H0}, {"ASP", "OD1", O1H0}, {"ASP", "OD2", O1H0},
    {"CYS", "SG", S2H1},
    {"GLN", "CG", C4H2}, {"GLN", "CD", C3H0}, {"GLN", "OE1", O1H0}, {"GLN", "NE2", N3H2},
    {"GLU", "CG", C4H2}, {"GLU", "CD", C3H0}, {"GLU", "OE1", O1H0}, {"GLU", "OE2", O1H0},
    {"GLY", "CA", C4H2},
    {"HIS", "CG", C3H0}, {"HIS", "ND1", N3H1}, {"HIS", "CD2", C3H1}, {"HIS", "NE2", N3H1}, {"HIS", "CE1", C3H1},
    {"ILE", "CB", C4H1}, {"ILE", "CG1", C4H2}, {"ILE", "CG2", C4H3}, {"ILE", "CD1", C4H3},
    {"LEU", "CG", C4H1}, {"LEU", "CD1", C4H3}, {"LEU", "CD2", C4H3},
    {"LYS", "CG", C4H2}, {"LYS", "CD", C4H2}, {"LYS", "CE", C4H2}, {"LYS", "NZ", N4H3},
    {"MET", "CG", C4H2}, {"MET", "SD", S2H0}, {"MET", "CE", C4H3},
    {"PHE", "CG", C3H0}, {"PHE", "CD1", C3H1}, {"PHE", "CD2", C3H1}, {"PHE", "CE1", C3H1}, {"PHE", "CE2", C3H1}, {"PHE", "CZ", C3H1},
    {"PRO", "N", N3H0}, {"PRO", "CG", C4H2}, {"PRO", "CD", C4H2},
    {"SER", "OG", O2H1},
    {"THR", "CB", C4H1}, {"THR", "OG1", O2H1}, {"THR", "CG2", C4H3},
    {"TRP", "CG", C3H0}, {"TRP", "CD2", C3H0}, {"TRP", "CE2", C3H0}, {"TRP", "CD1", C3H1}, {"TRP", "CE3", C3H1}, {"TRP", "CZ2", C3H1},
    {"TRP", "CZ3", C3H1}, {"TRP", "CH2", C3H1}, {"TRP", "NE1", N3H1},
    {"TYR", "CG", C3H0}, {"TYR", "CZ", C3H0}, {"TYR", "CD1", C3H1}, {"TYR", "CD2", C3H1}, {"TYR", "CE1", C3H1}, {"TYR", "CE2", C3H1}, {"TYR", "OH", O2H1},
    {"VAL", "CB", C4H1}, {"VAL", "CG1", C4H3}, {"VAL", "CG2", C4H3},
};
// Tien et al. 2013 (theoretical MaxASA of Gly-X-Gly), the values of the reference's get_max_asa (sasa.rs:460-483)
struct MaxAsaRow { const char *resn; float v; };
const MaxAsaRow kMaxAsa[] = {{"ALA", 129.0f}, {"ARG", 274.0f}, {"ASN", 195.0f}, {"ASP", 193.0f}, {"CYS", 167.0f}, {"GLU", 223.0f}, {"GLN", 225.0f},
                             {"GLY", 104.0f}, {"HIS", 224.0f}, {"MET", 224.0f}, {"ILE", 197.0f}, {"LEU", 201.0f}, {"LYS", 236.0f}, {"PHE", 240.0f},
                             {"PRO", 159.0f}, {"SER", 155.0f}, {"THR", 172.0f}, {"TRP", 285.0f}, {"TYR", 263.0f}, {"VAL", 174.0f}};
// ASSUMPTION: rust-sasa's own list of polar residues is not part of the reference's tree, and the reference only tests that the column
// exists.  These are the residues with a charged or hydrogen-bonding side chain.
const char *const kPolar[] = {"ARG", "ASN", "ASP", "GLN", "GLU", "HIS", "LYS", "SER", "THR", "TYR"};

void upper(const char *in, char (&up)[8]) {
    memset(up, 0, sizeof up);
    for (int k = 0; k < 7 && in && in[k]; k++) up[k] = (char)toupper((unsigned char)in[k]);
}
const ProtorRow *protor_find(const char *resn, const char *atomn) {
    for (const ProtorRow &r : ARP_PROTOR) if (!strcmp(r.resn, resn) && !strcmp(r.atom, atomn)) return &r;
    return nullptr;
}
}  // namespace

// The radius of one atom in f32.  vdw: the element's van der Waals radius (arp_params.vdw_radius), what every SASA entry point used before the
// tables had names.  protor: (residue, atom name), then (ANY, atom name), then -- ASSUMPTION: with_allow_vdw_fallback(true) falls back to an
// element table of rust-sasa's that is not on disk -- the same van der Waals radius.  fell_back (nullable) says that the fallback was taken.
static arp_status sasa_radius(const char *resn, const char *atomn, int32_t elem_class, int32_t table, float *out, bool *fell_back = nullptr) {
    if (table != ARP_RADII_VDW && table != ARP_RADII_PROTOR) { set_error("unknown radius table %d (ARP_RADII_VDW = 0, ARP_RADII_PROTOR = 1)", (int)table); return ARP_ERR_BAD_INPUT; }
    if (fell_back) *fell_back = false;
    if (table == ARP_RADII_PROTOR) {
        char up[8];
        upper(resn, up);
        const ProtorRow *r = protor_find(up, atomn ? atomn : "");
        if (!r) r = protor_find("ANY", atomn ? atomn : "");
        if (r) { *out = r->r; return ARP_OK; }
        if (fell_back) *fell_back = true;
    }
    arp_params p;
    arp_default_params(&p);
    const double vdw = elem_class >= 0 && elem_class < 16 ? p.vdw_radius[elem_class] : 0.0;
    if (!(vdw > 0.0)) { set_error("the element has no van der Waals radius"); return ARP_ERR_BAD_INPUT; }
    *out = (float)vdw;
    return ARP_OK;
}

// Radius + probe of every structure atom (f32: sasa.rs:200-206 casts van_der_waals to f32, rust-sasa adds the probe in f32)
static arp_status radii(const arp_structure *s, const std::vector<uint32_t> &atoms, float probe, std::vector<float> *R, int32_t table = ARP_RADII_VDW) {
    R->assign(s->n, 0.0f);
    for (uint32_t i : atoms) {
        float r = 0.0f;
        if (sasa_radius(s->res_resn.at(i), s->name.at(i), (int32_t)(s->base_attr[i] & ARP_ATTR_ELEM_MASK), table, &r) != ARP_OK) {
            if (table != ARP_RADII_VDW && table != ARP_RADII_PROTOR) return ARP_ERR_BAD_INPUT;
            set_error("atom %d: element '%s' has no van der Waals radius (the reference unwraps None, sasa.rs:201-206)", s->serial[i], s->elem.at(i)); return ARP_ERR_BAD_INPUT;
        }
        (*R)[i] = r + probe;
    }
    return ARP_OK;
}

static void sort_rows(const arp_structure *s, std::vector<uint32_t> &rows) {  // sasa.rs:247: by atomi (stable: structure order among equal serials)
    std::stable_sort(rows.begin(), rows.end(), [&](uint32_t a, uint32_t b) { return s->serial[a] < s->serial[b]; });
}

}  // namespace arp

using namespace arp;

extern "C" arp_status arp_structure_sasa_select(const arp_structure *s, const char *chains, int32_t model_num, int32_t remove_hydrogens,
                                                uint64_t *n_out, uint32_t *out_atoms) try {
    if (!s || !n_out) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    const std::vector<uint32_t> sel = select_atoms(s, chain_set(chains), remove_hydrogens != 0, true, true, model_num);
    *n_out = sel.size();
    if (out_atoms) std::copy(sel.begin(), sel.end(), out_atoms);
    return ARP_OK;
} ARP_ABI_CATCH

static arp_status check_table(int32_t table) {
    if (table == ARP_RADII_VDW || table == ARP_RADII_PROTOR) return ARP_OK;
    set_error("unknown radius table %d (ARP_RADII_VDW = 0, ARP_RADII_PROTOR = 1)", (int)table);
    return ARP_ERR_BAD_INPUT;
}

static arp_status atom_sasa_impl(arp_context *ctx, const arp_structure *s, const char *chains, int32_t model_num, int32_t remove_hydrogens, float probe,
                                 int32_t n_points, int32_t table, uint64_t *n_rows, uint32_t *out_atoms, float *out_sasa, int32_t *out_count) {
    if (!ctx || !s || !n_rows || !out_atoms || !out_sasa) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    arp_status st = sasa_check_params(probe, n_points);
    if (st != ARP_OK) return st;
    if ((st = check_table(table)) != ARP_OK) return st;
    *n_rows = 0;
    std::vector<uint32_t> sel = select_atoms(s, chain_set(chains), remove_hydrogens != 0, true, true, model_num);
    std::vector<float> R;
    if ((st = radii(s, sel, probe, &R, table)) != ARP_OK) return st;
    // the job runs over the selected atoms only (compact arrays)
    const uint64_t m = sel.size();
    std::vector<double> x(m), y(m), z(m);
    std::vector<float> Rm(m), sasa(m), sphere(3ull * (uint32_t)n_points);
    std::vector<int32_t> count(m);
    std::vector<uint8_t> inc(m, 1);
    for (uint64_t k = 0; k < m; k++) { const uint32_t i = sel[k]; x[k] = s->x[i]; y[k] = s->y[i]; z[k] = s->z[i]; Rm[k] = R[i]; }
    sasa_sphere_points((uint32_t)n_points, sphere.data());
    SasaJob j;
    j.n = m; j.x = x.data(); j.y = y.data(); j.z = z.data(); j.R = Rm.data(); j.include = inc.data(); j.n_points = (uint32_t)n_points; j.sphere = sphere.data();
    if ((st = sasa_run(ctx, j, sasa.data(), count.data(), nullptr)) != ARP_OK) return st;
    std::vector<uint32_t> order(m);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return s->serial[sel[a]] < s->serial[sel[b]]; });
    for (uint64_t r = 0; r < m; r++) {
        out_atoms[r] = sel[order[r]]; out_sasa[r] = sasa[order[r]];
        if (out_count) out_count[r] = count[order[r]];
    }
    *n_rows = m;
    return ARP_OK;
}

extern "C" arp_status arp_structure_atom_sasa(arp_context *ctx, const arp_structure *s, const char *chains, int32_t model_num, int32_t remove_hydrogens,
                                              float probe, int32_t n_points, uint64_t *n_rows, uint32_t *out_atoms, float *out_sasa, int32_t *out_count) try {
    return atom_sasa_impl(ctx, s, chains, model_num, remove_hydrogens, probe, n_points, ARP_RADII_VDW, n_rows, out_atoms, out_sasa, out_count);
} ARP_ABI_CATCH

extern "C" arp_status arp_structure_atom_sasa_radii(arp_context *ctx, const arp_structure *s, const char *chains, int32_t model_num, int32_t remove_hydrogens,
                                                    float probe, int32_t n_points, int32_t table, uint64_t *n_rows, uint32_t *out_atoms, float *out_sasa,
                                                    int32_t *out_count) try {
    return atom_sasa_impl(ctx, s, chains, model_num, remove_hydrogens, probe, n_points, table, n_rows, out_atoms, out_sasa, out_count);
} ARP_ABI_CATCH

extern "C" arp_status arp_structure_sap_score(arp_context *ctx, const arp_structure *s, const char *chains, int32_t model_num, float probe,
                                              int32_t n_points, float sap_radius, uint64_t *n_rows, uint32_t *out_atoms, float *out_sasa, float *out_sap) try {
    if (!ctx || !s || !n_rows || !out_atoms || !out_sasa || !out_sap) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    arp_status st = sasa_check_params(probe, n_points);
    if (st != ARP_OK) return st;
    if (!(sap_radius >= 0.0f)) { set_error("bad sap_radius"); return ARP_ERR_BAD_INPUT; }
    *n_rows = 0;
    const std::unordered_set<std::string> keep = chain_set(chains);
    // the neighbour set: steps 1-3 without the model filter (sap.rs:182); the SASA rows: steps 1-5 (sap.rs:147) -- a subset of it
    const std::vector<uint32_t> nb = select_atoms(s, keep, true, false, false, model_num);
    const std::vector<uint32_t> sel = select_atoms(s, keep, true, true, true, model_num);
    std::vector<float> R;
    if ((st = radii(s, sel, probe, &R)) != ARP_OK) return st;
    const uint64_t m = nb.size();
    std::vector<uint32_t> pos(s->n, ARP_NONE);
    for (uint64_t k = 0; k < m; k++) pos[nb[k]] = (uint32_t)k;
    std::vector<uint8_t> inc(m, 0), side(m, 0);
    for (uint32_t i : sel) inc[pos[i]] = 1;
    // the SASA map of sap.rs:164-168 (serial -> row; rows in atomi order, a later row of the same serial wins) and the residue names that
    // have a row (sap.rs:172-179)
    std::vector<uint32_t> rows = sel;
    sort_rows(s, rows);
    std::unordered_map<int32_t, int32_t> row_of_serial;
    std::unordered_set<std::string> resn_with_row;
    for (uint32_t i : rows) { row_of_serial[s->serial[i]] = (int32_t)pos[i]; resn_with_row.insert(s->res_resn.at(i)); }
    std::vector<double> x(m), y(m), z(m);
    std::vector<float> Rm(m), sasa(m), sap(m), sphere(3ull * (uint32_t)n_points);
    std::vector<uint32_t> code(m);
    std::vector<int32_t> src(m), count(m);
    for (uint64_t k = 0; k < m; k++) {
        const uint32_t i = nb[k];
        x[k] = s->x[i]; y[k] = s->y[i]; z[k] = s->z[i]; Rm[k] = R[i];
        side[k] = !is_backbone(s->name.at(i));  // AtomConformerResidueChainModel::is_sidechain
        code[k] = resn_with_row.count(s->res_resn.at(i)) ? sap_residue_code(s->res_resn.at(i)) : 20u;
        auto it = row_of_serial.find(s->serial[i]);
        src[k] = it == row_of_serial.end() ? -1 : it->second;
    }
    sasa_sphere_points((uint32_t)n_points, sphere.data());
    SasaJob j;
    j.n = m; j.x = x.data(); j.y = y.data(); j.z = z.data(); j.R = Rm.data(); j.include = inc.data(); j.n_points = (uint32_t)n_points; j.sphere = sphere.data();
    j.sidechain = side.data(); j.res_code = code.data(); j.src = src.data(); j.sap_radius = sap_radius;
    if ((st = sasa_run(ctx, j, sasa.data(), count.data(), sap.data())) != ARP_OK) return st;
    // sap.rs:187-215: score by serial over the side-chain atoms of the neighbour set (a later atom of the same serial wins);
    // sap.rs:218-238: the rows whose serial is a non-backbone serial of the WHOLE structure, with the score of that serial (0 if none)
    std::unordered_map<int32_t, float> score_of_serial;
    for (uint64_t k = 0; k < m; k++) if (side[k]) score_of_serial[s->serial[nb[k]]] = sap[k];
    std::unordered_set<int32_t> non_backbone;
    for (uint64_t i = 0; i < s->n; i++) if (!is_backbone(s->name.at(i))) non_backbone.insert(s->serial[i]);
    uint64_t r = 0;
    for (uint32_t i : rows) {
        if (!non_backbone.count(s->serial[i])) continue;
        auto it = score_of_serial.find(s->serial[i]);
        out_atoms[r] = i; out_sasa[r] = sasa[pos[i]]; out_sap[r] = it == score_of_serial.end() ? 0.0f : it->second;
        r++;
    }
    *n_rows = r;
    return ARP_OK;
} ARP_ABI_CATCH

static arp_status dsasa_impl(arp_context *ctx, const arp_structure *s, const char *groups, float probe, int32_t n_points, int32_t model_num, int32_t table,
                             float *out) {
    if (!ctx || !s || !groups || !out) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    arp_status st = sasa_check_params(probe, n_points);
    if (st != ARP_OK) return st;
    if ((st = check_table(table)) != ARP_OK) return st;
    std::vector<std::string> g1, g2;
    if ((st = parse_groups(s->chain_ids, groups, &g1, &g2)) != ARP_OK) return st;  // utils.rs:71-115 (sasa.rs:411)
    std::unordered_set<std::string> k1(g1.begin(), g1.end()), k2(g2.begin(), g2.end()), kc = k1;
    kc.insert(g2.begin(), g2.end());
    // complex, group 1, group 2 = models 0, 1, 2 of one grid: remove_chains_by (exact ids) then get_chain_sasa's selection (steps 2-4)
    const std::vector<uint32_t> sets[3] = {select_atoms(s, kc, true, true, false, model_num), select_atoms(s, k1, true, true, false, model_num),
                                           select_atoms(s, k2, true, true, false, model_num)};
    std::vector<double> x, y, z;
    std::vector<float> R;
    std::vector<uint32_t> model;
    for (int g = 0; g < 3; g++) {
        std::vector<float> Rg;
        if ((st = radii(s, sets[g], probe, &Rg, table)) != ARP_OK) return st;
        for (uint32_t i : sets[g]) { x.push_back(s->x[i]); y.push_back(s->y[i]); z.push_back(s->z[i]); R.push_back(Rg[i]); model.push_back((uint32_t)g); }
    }
    const uint64_t m = x.size();
    std::vector<uint8_t> inc(m, 1);
    std::vector<float> sasa(m), sphere(3ull * (uint32_t)n_points);
    std::vector<int32_t> count(m);
    sasa_sphere_points((uint32_t)n_points, sphere.data());
    SasaJob j;
    j.n = m; j.x = x.data(); j.y = y.data(); j.z = z.data(); j.R = R.data(); j.include = inc.data(); j.model = model.data();
    j.n_points = (uint32_t)n_points; j.sphere = sphere.data();
    if ((st = sasa_run(ctx, j, sasa.data(), count.data(), nullptr)) != ARP_OK) return st;
    double tot[3] = {0.0, 0.0, 0.0};
    for (uint64_t k = 0; k < m; k++) tot[model[k]] += (double)sasa[k];
    const float complex_total = (float)tot[0], g1_total = (float)tot[1], g2_total = (float)tot[2];
    *out = g1_total + g2_total - complex_total;  // sasa.rs:450 (f32)
    if (*out < 0.0f) { set_error("Negative dSASA calculated. Please check the input file and chain groups."); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}

extern "C" arp_status arp_structure_dsasa(arp_context *ctx, const arp_structure *s, const char *groups, float probe, int32_t n_points, int32_t model_num,
                                          float *out) try {
    return dsasa_impl(ctx, s, groups, probe, n_points, model_num, ARP_RADII_VDW, out);
} ARP_ABI_CATCH

extern "C" arp_status arp_structure_dsasa_radii(arp_context *ctx, const arp_structure *s, const char *groups, float probe, int32_t n_points, int32_t model_num,
                                                int32_t table, float *out) try {
    return dsasa_impl(ctx, s, groups, probe, n_points, model_num, table, out);
} ARP_ABI_CATCH

// ---- radius and residue tables over the C ABI ---------------------------------------------------------------------------------------------
extern "C" arp_status arp_sasa_radius(const char *resn, const char *atomn, const char *element, int32_t table, float *out) try {
    if (!out) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    return sasa_radius(resn ? resn : "", atomn ? atomn : "", element ? arp_element_class(element) : -1, table, out);
} ARP_ABI_CATCH

extern "C" float arp_max_asa(const char *resn) {
    char up[8];
    upper(resn, up);
    for (const MaxAsaRow &r : kMaxAsa) if (!strcmp(r.resn, up)) return r.v;
    return 0.0f;
}

extern "C" int32_t arp_residue_is_polar(const char *resn) {
    char up[8];
    upper(resn, up);
    for (const char *r : kPolar) if (!strcmp(r, up)) return 1;
    return 0;
}

// ---- residue- and chain-level SASA (sasa.rs:284-382, 520-561) ----------------------------------------------------------
namespace {
// The segments of a selection, in row order: per residue (the ingest's residue id: chain, resi, insertion), rows sorted stably by (chain as a
// byte string, resi, insertion); or per chain id, sorted.  Items are positions in `sel`, in selection order.  first[r]: the structure atom the
// row takes its identity from (the first selected atom of the segment).
struct Segments { std::vector<uint32_t> start, item, first; };
Segments build_segments(const arp_structure *s, const std::vector<uint32_t> &sel, bool by_chain) {
    std::vector<std::vector<uint32_t>> groups;
    if (by_chain) {
        std::unordered_map<std::string, uint32_t> at;
        for (uint32_t k = 0; k < sel.size(); k++) {
            auto it = at.emplace(s->chain.str(sel[k]), (uint32_t)groups.size());
            if (it.second) groups.emplace_back();
            groups[it.first->second].push_back(k);
        }
    } else {
        std::unordered_map<uint32_t, uint32_t> at;
        for (uint32_t k = 0; k < sel.size(); k++) {
            auto it = at.emplace(s->res_id[sel[k]], (uint32_t)groups.size());
            if (it.second) groups.emplace_back();
            groups[it.first->second].push_back(k);
        }
    }
    std::vector<uint32_t> order(groups.size());
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        const uint32_t i = sel[groups[a][0]], j = sel[groups[b][0]];
        const int c = s->chain.str(i).compare(s->chain.str(j));
        if (c || by_chain) return c < 0;
        if (s->resi[i] != s->resi[j]) return s->resi[i] < s->resi[j];
        return s->icode.str(i).compare(s->icode.str(j)) < 0;
    });
    Segments g;
    g.start.push_back(0u);
    for (uint32_t r : order) {
        g.first.push_back(sel[groups[r][0]]);
        g.item.insert(g.item.end(), groups[r].begin(), groups[r].end());
        g.start.push_back((uint32_t)g.item.size());
    }
    return g;
}

// One device run over the selection (steps 1-4, hydrogens out) with the table's radii; the per-atom values are summed on the device and only
// the sums come back.  Writes the rows of one level.
arp_status level_sasa(arp_context *ctx, const arp_structure *s, const char *chains, int32_t model_num, float probe, int32_t n_points, int32_t table,
                      bool by_chain, uint64_t *n_rows, uint32_t *out_atoms, float *out_sasa) {
    if (!ctx || !s || !n_rows || !out_atoms || !out_sasa) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    arp_status st = sasa_check_params(probe, n_points);
    if (st != ARP_OK) return st;
    if ((st = check_table(table)) != ARP_OK) return st;
    *n_rows = 0;
    const std::vector<uint32_t> sel = select_atoms(s, chain_set(chains), true, true, false, model_num);  // no serial filter: sasa.rs:294-295
    std::vector<float> R;
    if ((st = radii(s, sel, probe, &R, table)) != ARP_OK) return st;
    const uint64_t m = sel.size();
    if (m == 0) return ARP_OK;
    const Segments g = build_segments(s, sel, by_chain);
    std::vector<double> x(m), y(m), z(m);
    std::vector<float> Rm(m), sphere(3ull * (uint32_t)n_points);
    std::vector<uint8_t> inc(m, 1);
    for (uint64_t k = 0; k < m; k++) { const uint32_t i = sel[k]; x[k] = s->x[i]; y[k] = s->y[i]; z[k] = s->z[i]; Rm[k] = R[i]; }
    sasa_sphere_points((uint32_t)n_points, sphere.data());
    SegJob sj;
    sj.n_seg = (uint32_t)g.first.size(); sj.start = g.start.data(); sj.item = g.item.data(); sj.out = out_sasa;
    SasaJob j;
    j.n = m; j.x = x.data(); j.y = y.data(); j.z = z.data(); j.R = Rm.data(); j.include = inc.data(); j.n_points = (uint32_t)n_points; j.sphere = sphere.data();
    j.segs = &sj; j.n_segs = 1;
    if ((st = sasa_run(ctx, j, nullptr, nullptr, nullptr)) != ARP_OK) return st;
    std::copy(g.first.begin(), g.first.end(), out_atoms);
    *n_rows = g.first.size();
    return ARP_OK;
}
void residue_columns(const arp_structure *s, uint64_t n, const uint32_t *atoms, const float *sasa, uint8_t *is_polar, float *relative, uint8_t *valid) {
    for (uint64_t r = 0; r < n; r++) {
        const char *resn = s->res_resn.at(atoms[r]);
        if (is_polar) is_polar[r] = (uint8_t)arp_residue_is_polar(resn);
        if (relative) {
            const float mx = arp_max_asa(resn);
            valid[r] = mx > 0.0f;
            relative[r] = mx > 0.0f ? sasa[r] / mx : NAN;  // sasa.rs:547
        }
    }
}
}  // namespace

extern "C" arp_status arp_structure_residue_sasa(arp_context *ctx, const arp_structure *s, const char *chains, int32_t model_num, float probe, int32_t n_points,
                                                 int32_t table, uint64_t *n_rows, uint32_t *out_atoms, float *out_sasa, uint8_t *out_is_polar) try {
    const arp_status st = level_sasa(ctx, s, chains, model_num, probe, n_points, table, false, n_rows, out_atoms, out_sasa);
    if (st == ARP_OK) residue_columns(s, *n_rows, out_atoms, out_sasa, out_is_polar, nullptr, nullptr);
    return st;
} ARP_ABI_CATCH

extern "C" arp_status arp_structure_chain_sasa(arp_context *ctx, const arp_structure *s, const char *chains, int32_t model_num, float probe, int32_t n_points,
                                               int32_t table, uint64_t *n_rows, uint32_t *out_atoms, float *out_sasa) try {
    return level_sasa(ctx, s, chains, model_num, probe, n_points, table, true, n_rows, out_atoms, out_sasa);
} ARP_ABI_CATCH

extern "C" arp_status arp_structure_relative_sasa(arp_context *ctx, const arp_structure *s, const char *chains, int32_t model_num, float probe, int32_t n_points,
                                                  int32_t table, uint64_t *n_rows, uint32_t *out_atoms, float *out_sasa, uint8_t *out_is_polar,
                                                  float *out_relative, uint8_t *out_valid) try {
    if (!out_relative || !out_valid) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    const arp_status st = level_sasa(ctx, s, chains, model_num, probe, n_points, table, false, n_rows, out_atoms, out_sasa);
    if (st == ARP_OK) residue_columns(s, *n_rows, out_atoms, out_sasa, out_is_polar, out_relative, out_valid);
    return st;
} ARP_ABI_CATCH

// ---- SASA / SAP statistics over the frames of an ensemble (device path: sasa_dev.cpp ens_run, ens.inl) ----------------
extern "C" arp_status arp_sasa_ensemble_stats(uint64_t n_frames, uint64_t m, const float *R, int32_t n_points, const uint64_t *s1, const uint64_t *s2,
                                              const int32_t *cmin, const int32_t *cmax, const double *t1, const double *t2, float *mean_sasa,
                                              float *std_sasa, float *min_sasa, float *max_sasa, float *mean_sap, float *std_sap) try {
    if (n_frames == 0 || n_points < 1) { set_error("sasa ensemble statistics: n_frames and n_points must be positive"); return ARP_ERR_BAD_INPUT; }
    if (m && (!R || !s1 || !s2 || !cmin || !cmax || !mean_sasa || !std_sasa || !min_sasa || !max_sasa)) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    if (m && (t1 || t2 || mean_sap || std_sap) && !(t1 && t2 && mean_sap && std_sap)) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    const double F = (double)n_frames, n = (double)n_points;
    for (uint64_t k = 0; k < m; k++) {
        // b = (4 pi R) R as k_sasa forms it (sasa.inl); every value below is one f64 chain, left to right, rounded to f32 once
        const double ri = (double)R[k], b = (4.0 * 3.141592653589793 * ri) * ri;
        const unsigned __int128 d = (unsigned __int128)n_frames * s2[k] - (unsigned __int128)s1[k] * s1[k];  // F S2 - S1^2 >= 0 (Cauchy-Schwarz), exact
        mean_sasa[k] = (float)(b * (double)s1[k] / n / F);
        std_sasa[k] = (float)(b * std::sqrt((double)d) / n / F);
        min_sasa[k] = (float)(b * (double)cmin[k] / n);  // (the value k_sasa gives the frame with that count)
        max_sasa[k] = (float)(b * (double)cmax[k] / n);
        if (t1) {
            const double mu = t1[k] / F, var = t2[k] / F - mu * mu;
            mean_sap[k] = (float)mu;
            std_sap[k] = (float)std::sqrt(var > 0.0 ? var : 0.0);
        }
    }
    return ARP_OK;
} ARP_ABI_CATCH

namespace {
struct ResidueEnsOut {  // arp_sasa_ensemble_residues: its outputs, filled instead of the per-atom ones
    uint64_t *n_chains;
    uint32_t *res_atoms, *chain_atoms;
    uint8_t *is_polar, *relative_valid;
    float *mean, *sd, *vmin, *vmax, *mean_relative, *chain_sasa, *residue_sasa;
};
}  // namespace

// The residue level of the ensemble path once the inputs have been checked: sel (m atoms of the topology, ascending), their R, F frames.
static arp_status residue_ensemble(arp_context *ctx, const arp_structure *s, const std::vector<uint32_t> &sel, const std::vector<float> &R, uint64_t F, uint64_t n0,
                                   const double *frames, float probe, int32_t n_points, const ResidueEnsOut &ro, uint64_t *n_rows) {
    (void)probe;
    const uint64_t m = sel.size();
    const Segments res = build_segments(s, sel, false), chn = build_segments(s, sel, true);
    const uint64_t nr = res.first.size(), nc = chn.first.size();
    if (ro.res_atoms) std::copy(res.first.begin(), res.first.end(), ro.res_atoms);
    if (ro.chain_atoms) std::copy(chn.first.begin(), chn.first.end(), ro.chain_atoms);
    *ro.n_chains = nc;
    if (!ctx) { *n_rows = nr; return ARP_OK; }  // validation only: the rows, the chains and the frame count
    if (!ro.res_atoms || !ro.chain_atoms || !ro.is_polar || !ro.relative_valid || !ro.mean || !ro.sd || !ro.vmin || !ro.vmax || !ro.mean_relative || !ro.chain_sasa) {
        set_error("null argument");
        return ARP_ERR_BAD_INPUT;
    }
    if (m == 0) return ARP_OK;  // an empty selection: no rows, no chains
    std::vector<float> Rm(m), sphere(3ull * (uint32_t)n_points), total(F);
    for (uint64_t k = 0; k < m; k++) Rm[k] = R[sel[k]];
    sasa_sphere_points((uint32_t)n_points, sphere.data());
    SegJob rj, cj;
    rj.n_seg = (uint32_t)nr; rj.start = res.start.data(); rj.item = res.item.data();
    cj.n_seg = (uint32_t)nc; cj.start = chn.start.data(); cj.item = chn.item.data();
    EnsJob j;
    j.n_top = n0; j.m = m; j.n_frames = F; j.xyz = frames; j.sel = sel.data(); j.R = Rm.data(); j.n_points = (uint32_t)n_points; j.sphere = sphere.data();
    j.chunk_atoms = g_debug.ens_chunk_atoms > 0 ? (uint64_t)g_debug.ens_chunk_atoms : 0u;
    j.res = &rj; j.chain = &cj;
    std::vector<unsigned long long> s1(m), s2(m);
    std::vector<int32_t> cmin(m), cmax(m);
    std::vector<double> t1(nr), t2(nr);
    EnsOut o;
    o.s1 = s1.data(); o.s2 = s2.data(); o.cmin = cmin.data(); o.cmax = cmax.data(); o.total = total.data();
    o.rt1 = t1.data(); o.rt2 = t2.data(); o.rmin = ro.vmin; o.rmax = ro.vmax; o.chain_sasa = ro.chain_sasa; o.residue_sasa = ro.residue_sasa;
    const arp_status st = ens_run(ctx, j, o);
    if (st != ARP_OK) return st;
    const double Fd = (double)F;
    for (uint64_t r = 0; r < nr; r++) {  // as arp_sasa_ensemble_stats finishes SAP
        const double mu = t1[r] / Fd, var = t2[r] / Fd - mu * mu;
        ro.mean[r] = (float)mu;
        ro.sd[r] = (float)std::sqrt(var > 0.0 ? var : 0.0);
    }
    residue_columns(s, nr, ro.res_atoms, ro.mean, ro.is_polar, ro.mean_relative, ro.relative_valid);
    *n_rows = nr;
    return ARP_OK;
}

namespace {
// What every ensemble entry point checks and selects before anything touches the device: model 0 as the topology, the frame count, the
// parameters and the table, then keep(&chains) -- the entry point's own checks and its chain set (empty = all) --, steps 1-3 of
// arp_structure_sasa_select on model 0's atoms (the prefix [0, n0) of the structure), their radii, the models as frames, finite coordinates.
struct EnsInput {
    uint64_t n0 = 0, F = 0;
    std::vector<uint32_t> sel;       // ascending
    std::vector<float> R;            // per structure atom: radius + probe of the selected ones
    std::vector<double> model_xyz;   // the models' coordinates as F x n0 x 3 when no frames were given
    const double *frames = nullptr;
};
template <class Keep>
arp_status ensemble_input(const arp_structure *s, uint64_t n_frames, const double *xyz, float probe, int32_t n_points, int32_t table, const char *what, Keep keep,
                          EnsInput *in) {
    uint64_t r0 = 0, nm = 1;
    arp_status st = freq_topology(s, xyz == nullptr, &in->n0, &r0, &nm);
    if (st != ARP_OK) return st;
    const uint64_t n0 = in->n0, F = in->F = xyz ? n_frames : nm;
    if (F == 0) { set_error("%s: at least one frame is needed", what); return ARP_ERR_BAD_INPUT; }
    if (n0 >= (1ull << 29)) { set_error("%s: the topology has %llu atoms, at most 2^29 - 1 are supported", what, (unsigned long long)n0); return ARP_ERR_BAD_INPUT; }
    if (F > (1ull << 40) / std::max<uint64_t>(n0, 1)) { set_error("%s: too many frames", what); return ARP_ERR_BAD_INPUT; }
    if ((st = sasa_check_params(probe, n_points)) != ARP_OK) return st;
    if ((st = check_table(table)) != ARP_OK) return st;
    std::unordered_set<std::string> chains;
    if ((st = keep(&chains)) != ARP_OK) return st;
    in->sel = select_atoms(s, chains, true, false, false, 0);
    while (!in->sel.empty() && in->sel.back() >= n0) in->sel.pop_back();
    if ((st = radii(s, in->sel, probe, &in->R, table)) != ARP_OK) return st;
    if (!xyz) {
        in->model_xyz.resize(F * n0 * 3);
        for (uint64_t a = 0; a < F * n0; a++) { in->model_xyz[3 * a] = s->x[a]; in->model_xyz[3 * a + 1] = s->y[a]; in->model_xyz[3 * a + 2] = s->z[a]; }
    }
    in->frames = xyz ? xyz : in->model_xyz.data();
    for (uint64_t f = 0; f < F; f++)
        for (uint32_t i : in->sel) {
            const double *c = in->frames + 3 * (f * n0 + i);
            if (!(std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2]))) {
                set_error("%s: non-finite coordinate in frame %llu, atom %llu", what, (unsigned long long)f, (unsigned long long)i);
                return ARP_ERR_BAD_INPUT;
            }
        }
    return ARP_OK;
}
}  // namespace

static arp_status sasa_ensemble_impl(arp_context *ctx, const arp_structure *s, uint64_t n_frames, const double *xyz, const char *chains, float probe,
                                     int32_t n_points, int32_t with_sap, float sap_radius, int32_t table, const ResidueEnsOut *ro, uint64_t *n_rows,
                                     uint64_t *frames_used, uint32_t *out_atoms, float *mean_sasa, float *std_sasa, float *min_sasa, float *max_sasa,
                                     float *mean_sap, float *std_sap, float *min_sap, float *max_sap, float *total_sasa, int32_t *out_count, float *out_sap) {
    if (!s || !n_rows || !frames_used || (ro && !ro->n_chains)) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    *n_rows = 0; *frames_used = 0;
    if (ro) *ro->n_chains = 0;
    // validation: nothing here touches the device.  (The table is checked before the SAP arguments: no entry point passes both.)
    EnsInput in;
    arp_status st = ensemble_input(s, n_frames, xyz, probe, n_points, table, "sasa ensemble", [&](std::unordered_set<std::string> *keep) {
        if (with_sap && !(sap_radius >= 0.0f)) { set_error("bad sap_radius"); return ARP_ERR_BAD_INPUT; }
        if (!with_sap && out_sap) { set_error("sasa ensemble: out_sap needs with_sap"); return ARP_ERR_BAD_INPUT; }
        *keep = chain_set(chains);
        return ARP_OK;
    }, &in);
    if (st != ARP_OK) return st;
    const auto &[n0, F, sel, R, model_xyz, frames] = in;
    const uint64_t m = sel.size();
    *frames_used = F;
    if (ro) return residue_ensemble(ctx, s, sel, R, F, n0, frames, probe, n_points, *ro, n_rows);
    if (out_atoms) std::copy(sel.begin(), sel.end(), out_atoms);
    if (!ctx) { *n_rows = m; return ARP_OK; }  // validation only: the selection and the frame count
    if (!out_atoms || !mean_sasa || !std_sasa || !min_sasa || !max_sasa || !total_sasa || (with_sap && (!mean_sap || !std_sap || !min_sap || !max_sap))) {
        set_error("null argument");
        return ARP_ERR_BAD_INPUT;
    }
    if (m == 0) { std::fill(total_sasa, total_sasa + F, 0.0f); return ARP_OK; }  // an empty selection: no rows, every frame's total is 0
    std::vector<float> Rm(m), sphere(3ull * (uint32_t)n_points);
    std::vector<uint8_t> side(m, 0);
    std::vector<uint32_t> code(m, 20u);
    for (uint64_t k = 0; k < m; k++) {
        const uint32_t i = sel[k];
        Rm[k] = R[i];
        side[k] = !is_backbone(s->name.at(i));
        code[k] = sap_residue_code(s->res_resn.at(i));
    }
    sasa_sphere_points((uint32_t)n_points, sphere.data());
    EnsJob j;
    j.n_top = n0; j.m = m; j.n_frames = F; j.xyz = frames; j.sel = sel.data(); j.R = Rm.data(); j.n_points = (uint32_t)n_points; j.sphere = sphere.data();
    j.with_sap = with_sap != 0; j.sidechain = side.data(); j.res_code = code.data(); j.sap_radius = sap_radius;
    j.chunk_atoms = g_debug.ens_chunk_atoms > 0 ? (uint64_t)g_debug.ens_chunk_atoms : 0u;
    std::vector<unsigned long long> s1(m), s2(m);
    std::vector<int32_t> cmin(m), cmax(m);
    std::vector<double> t1(with_sap ? m : 0), t2(with_sap ? m : 0);
    EnsOut o;
    o.s1 = s1.data(); o.s2 = s2.data(); o.cmin = cmin.data(); o.cmax = cmax.data(); o.total = total_sasa; o.count = out_count;
    if (with_sap) { o.t1 = t1.data(); o.t2 = t2.data(); o.pmin = min_sap; o.pmax = max_sap; o.sap = out_sap; }
    if ((st = ens_run(ctx, j, o)) != ARP_OK) return st;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "accumulator width");
    if ((st = arp_sasa_ensemble_stats(F, m, Rm.data(), n_points, (const uint64_t *)s1.data(), (const uint64_t *)s2.data(), cmin.data(), cmax.data(),
                                      with_sap ? t1.data() : nullptr, with_sap ? t2.data() : nullptr, mean_sasa, std_sasa, min_sasa, max_sasa,
                                      with_sap ? mean_sap : nullptr, with_sap ? std_sap : nullptr)) != ARP_OK) return st;
    *n_rows = m;
    return ARP_OK;
}

extern "C" arp_status arp_sasa_ensemble(arp_context *ctx, const arp_structure *s, uint64_t n_frames, const double *xyz, const char *chains, float probe,
                                        int32_t n_points, int32_t with_sap, float sap_radius, uint64_t *n_rows, uint64_t *frames_used, uint32_t *out_atoms,
                                        float *mean_sasa, float *std_sasa, float *min_sasa, float *max_sasa, float *mean_sap, float *std_sap, float *min_sap,
                                        float *max_sap, float *total_sasa, int32_t *out_count, float *out_sap) try {
    return sasa_ensemble_impl(ctx, s, n_frames, xyz, chains, probe, n_points, with_sap, sap_radius, ARP_RADII_VDW, nullptr, n_rows, frames_used, out_atoms,
                              mean_sasa, std_sasa, min_sasa, max_sasa, mean_sap, std_sap, min_sap, max_sap, total_sasa, out_count, out_sap);
} ARP_ABI_CATCH

extern "C" arp_status arp_sasa_ensemble_radii(arp_context *ctx, const arp_structure *s, uint64_t n_frames, const double *xyz, const char *chains, float probe,
                                              int32_t n_points, int32_t table, uint64_t *n_rows, uint64_t *frames_used, uint32_t *out_atoms, float *mean_sasa,
                                              float *std_sasa, float *min_sasa, float *max_sasa, float *total_sasa, int32_t *out_count) try {
    return sasa_ensemble_impl(ctx, s, n_frames, xyz, chains, probe, n_points, 0, 0.0f, table, nullptr, n_rows, frames_used, out_atoms, mean_sasa, std_sasa,
                              min_sasa, max_sasa, nullptr, nullptr, nullptr, nullptr, total_sasa, out_count, nullptr);
} ARP_ABI_CATCH

extern "C" arp_status arp_sasa_ensemble_residues(arp_context *ctx, const arp_structure *s, uint64_t n_frames, const double *xyz, const char *chains, float probe,
                                                 int32_t n_points, int32_t table, uint64_t *n_rows, uint64_t *n_chains, uint64_t *frames_used,
                                                 uint32_t *out_res_atoms, uint8_t *out_is_polar, float *mean_sasa, float *std_sasa, float *min_sasa,
                                                 float *max_sasa, float *mean_relative, uint8_t *relative_valid, uint32_t *out_chain_atoms, float *chain_sasa,
                                                 float *residue_sasa) try {
    const ResidueEnsOut ro{n_chains, out_res_atoms, out_chain_atoms, out_is_polar, relative_valid, mean_sasa, std_sasa, min_sasa, max_sasa, mean_relative,
                           chain_sasa, residue_sasa};
    return sasa_ensemble_impl(ctx, s, n_frames, xyz, chains, probe, n_points, 0, 0.0f, table, &ro, n_rows, frames_used, nullptr, nullptr, nullptr, nullptr,
                              nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
} ARP_ABI_CATCH

// ---- buried surface per atom and residue, dSASA over the frames of an ensemble (kernel: sasa.inl k_sasa_split) -------------
namespace {
// groups -> the two chain sets of dsasa_impl (utils.rs:71-115, sasa.rs:411) and their union
struct GroupSets { std::unordered_set<std::string> k1, k2, kc; };
arp_status group_sets(const arp_structure *s, const char *groups, GroupSets *g) {
    std::vector<std::string> g1, g2;
    const arp_status st = parse_groups(s->chain_ids, groups, &g1, &g2);
    if (st != ARP_OK) return st;
    g->k1.insert(g1.begin(), g1.end()); g->k2.insert(g2.begin(), g2.end());
    g->kc = g->k1; g->kc.insert(g2.begin(), g2.end());
    return ARP_OK;
}
// the mask of a selected atom: membership of its chain (an empty set keeps every chain, as select_atoms reads it)
uint8_t group_mask(const arp_structure *s, const GroupSets &g, uint32_t i) {
    const std::string c(s->chain.at(i));
    return (uint8_t)(((g.k1.empty() || g.k1.count(c)) ? 1u : 0u) | ((g.k2.empty() || g.k2.count(c)) ? 2u : 0u));
}
}  // namespace

extern "C" arp_status arp_dsasa_total(float total_complex, float total_g1, float total_g2, float *out) {
    if (!out) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    *out = total_g1 + total_g2 - total_complex;  // sasa.rs:450 (f32)
    if (*out < 0.0f) { set_error("Negative dSASA calculated. Please check the input file and chain groups."); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}

extern "C" arp_status arp_structure_buried_sasa(arp_context *ctx, const arp_structure *s, const char *groups, float probe, int32_t n_points, int32_t model_num,
                                                int32_t table, uint64_t *n_rows, uint32_t *out_atoms, uint8_t *out_group, float *out_sasa, int32_t *out_count,
                                                int32_t *out_buried, uint64_t *n_res_rows, uint32_t *out_res_atoms, float *out_res_sasa,
                                                uint32_t *out_res_buried_atoms, float *out_totals) try {
    if (!s || !groups || !n_rows || !n_res_rows || !out_atoms || !out_group || !out_sasa || !out_count || !out_buried || !out_res_atoms || !out_res_sasa ||
        !out_res_buried_atoms || !out_totals) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    *n_rows = 0; *n_res_rows = 0;
    arp_status st = sasa_check_params(probe, n_points);
    if (st != ARP_OK) return st;
    if ((st = check_table(table)) != ARP_OK) return st;
    GroupSets gs;
    if ((st = group_sets(s, groups, &gs)) != ARP_OK) return st;
    if (!ctx) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    // the rows: the union selection of dsasa_impl (remove_chains_by + get_chain_sasa's steps 2-4)
    const std::vector<uint32_t> sel = select_atoms(s, gs.kc, true, true, false, model_num);
    std::vector<float> R;
    if ((st = radii(s, sel, probe, &R, table)) != ARP_OK) return st;
    const uint64_t m = sel.size();
    for (int g = 0; g < 4; g++) out_totals[g] = 0.0f;
    if (m == 0) return ARP_OK;
    const Segments res = build_segments(s, sel, false);
    const uint64_t nr = res.first.size();
    std::vector<double> x(m), y(m), z(m);
    std::vector<float> Rm(m), sasa(3 * m), sphere(3ull * (uint32_t)n_points), rsum(3 * nr);
    std::vector<int32_t> count(3 * m), buried(m);
    std::vector<uint8_t> grp(m);
    for (uint64_t k = 0; k < m; k++) { const uint32_t i = sel[k]; x[k] = s->x[i]; y[k] = s->y[i]; z[k] = s->z[i]; Rm[k] = R[i]; grp[k] = group_mask(s, gs, i); }
    sasa_sphere_points((uint32_t)n_points, sphere.data());
    SegJob sj;
    sj.n_seg = (uint32_t)nr; sj.start = res.start.data(); sj.item = res.item.data(); sj.out = rsum.data();
    BsaJob j;
    j.n = m; j.x = x.data(); j.y = y.data(); j.z = z.data(); j.R = Rm.data(); j.group = grp.data(); j.n_points = (uint32_t)n_points; j.sphere = sphere.data();
    j.seg = &sj;
    if ((st = bsa_run(ctx, j, sasa.data(), count.data(), buried.data())) != ARP_OK) return st;
    // the totals as dsasa_impl forms them: every sum in f64 in selection order (a non-member adds +0.0), one rounding to f32, then f32 arithmetic
    double tot[3] = {0.0, 0.0, 0.0};
    for (int g = 0; g < 3; g++) for (uint64_t k = 0; k < m; k++) tot[g] += (double)sasa[g * m + k];
    out_totals[0] = (float)tot[0]; out_totals[1] = (float)tot[1]; out_totals[2] = (float)tot[2];
    if ((st = arp_dsasa_total(out_totals[0], out_totals[1], out_totals[2], &out_totals[3])) != ARP_OK) return st;
    std::vector<uint32_t> order(m);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return s->serial[sel[a]] < s->serial[sel[b]]; });  // arp_structure_atom_sasa's order
    for (uint64_t r = 0; r < m; r++) {
        const uint32_t k = order[r];
        out_atoms[r] = sel[k]; out_group[r] = grp[k]; out_buried[r] = buried[k];
        for (int g = 0; g < 3; g++) { out_sasa[g * m + r] = sasa[g * m + k]; out_count[g * m + r] = count[g * m + k]; }
    }
    for (uint64_t r = 0; r < nr; r++) {
        out_res_atoms[r] = res.first[r];
        uint32_t nb = 0;
        for (uint32_t q = res.start[r]; q < res.start[r + 1]; q++) nb += buried[res.item[q]] > 0;
        out_res_buried_atoms[r] = nb;
    }
    std::copy(rsum.begin(), rsum.end(), out_res_sasa);
    *n_rows = m; *n_res_rows = nr;
    return ARP_OK;
} ARP_ABI_CATCH

extern "C" arp_status arp_dsasa_ensemble(arp_context *ctx, const arp_structure *s, uint64_t n_frames, const double *xyz, const char *groups, float probe,
                                         int32_t n_points, int32_t table, uint64_t *n_rows, uint64_t *frames_used, uint32_t *out_atoms, uint8_t *out_group,
                                         float *out_R, uint64_t *sum_buried, uint64_t *sum_buried_sq, int32_t *min_buried, int32_t *max_buried,
                                         uint32_t *frames_buried, float *total_complex, float *total_g1, float *total_g2, float *dsasa, int32_t *out_buried) try {
    if (!s || !groups || !n_rows || !frames_used) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    *n_rows = 0; *frames_used = 0;
    // validation: nothing here touches the device
    GroupSets gs;
    EnsInput in;
    arp_status st = ensemble_input(s, n_frames, xyz, probe, n_points, table, "dsasa ensemble", [&](std::unordered_set<std::string> *keep) {
        const arp_status g = group_sets(s, groups, &gs);
        *keep = gs.kc;
        return g;
    }, &in);
    if (st != ARP_OK) return st;
    const auto &[n0, F, sel, R, model_xyz, frames] = in;
    const uint64_t m = sel.size();
    std::vector<float> Rm(m);
    std::vector<uint8_t> grp(m);
    for (uint64_t k = 0; k < m; k++) { Rm[k] = R[sel[k]]; grp[k] = group_mask(s, gs, sel[k]); }
    *frames_used = F;
    if (out_atoms) std::copy(sel.begin(), sel.end(), out_atoms);
    if (out_group) std::copy(grp.begin(), grp.end(), out_group);
    if (out_R) std::copy(Rm.begin(), Rm.end(), out_R);
    if (!ctx) { *n_rows = m; return ARP_OK; }  // validation only: the selection and the frame count
    if (!out_atoms || !out_group || !out_R || !sum_buried || !sum_buried_sq || !min_buried || !max_buried || !frames_buried || !total_complex || !total_g1 ||
        !total_g2 || !dsasa) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    if (m == 0) { for (float *t : {total_complex, total_g1, total_g2, dsasa}) std::fill(t, t + F, 0.0f); return ARP_OK; }
    std::vector<float> sphere(3ull * (uint32_t)n_points);
    sasa_sphere_points((uint32_t)n_points, sphere.data());
    BsaEnsJob j;
    j.n_top = n0; j.m = m; j.n_frames = F; j.xyz = frames; j.sel = sel.data(); j.R = Rm.data(); j.group = grp.data(); j.n_points = (uint32_t)n_points;
    j.sphere = sphere.data(); j.chunk_atoms = g_debug.ens_chunk_atoms > 0 ? (uint64_t)g_debug.ens_chunk_atoms : 0u;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "accumulator width");
    BsaEnsOut o;
    o.s1 = (unsigned long long *)sum_buried; o.s2 = (unsigned long long *)sum_buried_sq; o.bmin = min_buried; o.bmax = max_buried; o.frames_buried = frames_buried;
    o.total[0] = total_complex; o.total[1] = total_g1; o.total[2] = total_g2; o.buried = out_buried;
    if ((st = bsa_ens_run(ctx, j, o)) != ARP_OK) return st;
    for (uint64_t f = 0; f < F; f++) dsasa[f] = total_g1[f] + total_g2[f] - total_complex[f];  // (f32; a negative frame value is returned as it is)
    *n_rows = m;
    return ARP_OK;
} ARP_ABI_CATCH
