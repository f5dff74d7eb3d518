// The host side of `arpeggia::get_contacts` (src/contacts/mod.rs:61-137): which entities a structure has (ring and side-chain plane
// entities, their keys and names -- kept with the structure), the structure's device-resident copy, and arp_get_contacts itself, which
// runs the pair pass and the device table (table_dev.hip) on them.  The table object it returns lives in table.cpp.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include <hip/hip_runtime.h>

#include "table.h"

namespace arp {

#ifdef ARP_WITH_HOST_TABLE   // host-side plane maths: only the test-only host assembly (tests/hosttable/table_host.inl) fits planes on the CPU
// ---- plane maths (residues.rs:24-75, 270-298) ----------------------------------------------------------------------
// Least-squares plane: centroid + eigenvector of the smallest eigenvalue of the 3x3 scatter matrix (cyclic Jacobi).
// nalgebra's svd.u.column(2) is the same direction up to sign; every use folds the angle into [0, 90] degrees.
bool fit_plane(const std::vector<std::array<double, 3>> &pts, Plane *out) {
    const size_t n = pts.size();
    if (n < 3) return false;  // residues.rs:273
    double c[3] = {0, 0, 0};
    for (auto &p : pts) for (int k = 0; k < 3; k++) c[k] += p[k];
    for (int k = 0; k < 3; k++) c[k] /= (double)n;
    double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (auto &p : pts) {
        double d[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) A[i][j] += d[i] * d[j];
    }
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 64; sweep++) {
        double off = fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]);
        double diag = fabs(A[0][0]) + fabs(A[1][1]) + fabs(A[2][2]);
        if (off <= 1e-300 || off <= 1e-18 * diag) break;
        for (int p = 0; p < 2; p++)
            for (int q = p + 1; q < 3; q++) {
                if (fabs(A[p][q]) <= 1e-300) continue;
                double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < 3; k++) { double akp = A[k][p], akq = A[k][q]; A[k][p] = cs * akp - sn * akq; A[k][q] = sn * akp + cs * akq; }
                for (int k = 0; k < 3; k++) { double apk = A[p][k], aqk = A[q][k]; A[p][k] = cs * apk - sn * aqk; A[q][k] = sn * apk + cs * aqk; }
                for (int k = 0; k < 3; k++) { double vkp = V[k][p], vkq = V[k][q]; V[k][p] = cs * vkp - sn * vkq; V[k][q] = sn * vkp + cs * vkq; }
            }
    }
    int best = 0;
    for (int k = 1; k < 3; k++) if (A[k][k] < A[best][best]) best = k;
    double nn = sqrt(V[0][best] * V[0][best] + V[1][best] * V[1][best] + V[2][best] * V[2][best]);
    for (int k = 0; k < 3; k++) { out->c[k] = c[k]; out->n[k] = V[k][best] / nn; }
    return true;
}
static const double kRad2Deg = 180.0 / 3.14159265358979323846264338327950288;
static double norm3(const double v[3]) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
static double fold_deg(double rad) {  // residues.rs:50-53,70-73
    if (rad > 1.57079632679489661923) rad = 3.14159265358979323846 - rad;
    return rad * kRad2Deg;
}
static double point_dist(const Plane &p, const double q[3]) { double v[3] = {q[0] - p.c[0], q[1] - p.c[1], q[2] - p.c[2]}; return norm3(v); }
static double point_angle(const Plane &p, const double q[3]) {
    double v[3] = {q[0] - p.c[0], q[1] - p.c[1], q[2] - p.c[2]};
    double dot = p.n[0] * v[0] + p.n[1] * v[1] + p.n[2] * v[2];
    return fold_deg(acos(dot / (norm3(p.n) * norm3(v))));
}
static double plane_dihedral(const Plane &a, const Plane &b) {
    double dot = a.n[0] * b.n[0] + a.n[1] * b.n[1] + a.n[2] * b.n[2];
    return fold_deg(acos(dot / (norm3(a.n) * norm3(b.n))));
}

#endif

// ---- plane tables (complex.rs:442-514) ------------------------------------------------------------------------------
static bool in_words(const char *words, const char *w) {
    size_t L = strlen(w);
    for (const char *p = words; *p;) {
        const char *e = strchr(p, ' ');
        size_t len = e ? (size_t)(e - p) : strlen(p);
        if (len == L && strncmp(p, w, L) == 0) return true;
        p += len;
        while (*p == ' ') p++;
    }
    return false;
}
static const char *ring_atoms_of(const std::string &resn) {  // residues.rs:163-186
    if (resn == "HIS") return "CG ND1 CE1 NE2 CD2";
    if (resn == "PHE" || resn == "TYR") return "CG CD1 CD2 CE1 CE2 CZ";
    if (resn == "TRP") return "CG CD1 CD2 NE1 CE2 CE3 CZ2 CZ3 CH2";
    return nullptr;
}
static const char *sc_atoms_of(const std::string &resn) {  // residues.rs:188-268
    static const std::map<std::string, const char *> m = {
        {"ARG", "NE CZ NH1 NH2"}, {"ASN", "CB CG OD1 ND2"}, {"ASP", "CB CG OD1 OD2"}, {"CYS", "CA CB SG"}, {"GLU", "CG CD OE1 OE2"},
        {"GLN", "CG CD OE1 NE2"}, {"ILE", "CB CG1 CG2 CD1"}, {"LEU", "CB CG CD1 CD2"}, {"LYS", "CG CD CE NZ"}, {"MET", "CG SD CE"},
        {"PRO", "N CA CB CG CD"}, {"SER", "CA CB OG"}, {"THR", "CA CB OG1 CG2"}, {"VAL", "CA CB CG1 CG2"}};
    if (const char *r = ring_atoms_of(resn)) return r;
    auto it = m.find(resn);
    return it == m.end() ? nullptr : it->second;
}

static uint64_t pack_name(const char *s, size_t cap) {  // up to `cap` bytes, NUL padded
    uint64_t v = 0;
    size_t n = 0;
    while (n < cap && s[n]) n++;
    memcpy(&v, s, n);
    return v;
}
static PlaneKey plane_key(int32_t model, const char *chain, int32_t resi, const char *icode, const char *altloc, const char *resn) {
    return PlaneKey{model, resi, (uint32_t)pack_name(icode, 4), (uint32_t)pack_name(altloc, 4), pack_name(chain, 8), pack_name(resn, 8)};
}

void build_planes(const arp_structure &s, bool rings, const std::vector<char> &has_plane, const std::vector<Plane> *fitted_in, std::vector<PlaneEntry> *out,
                  PlaneIndex *index, std::vector<int64_t> *first_of_res, size_t n_res_use) {
    const bool model0_only = n_res_use < s.residues.size();
    const size_t n_res = std::min(n_res_use, s.residues.size());
    std::vector<int32_t> serials;
    for (const ChainInfo &c : s.chains) {
        if (model0_only && c.model_idx != 0u) continue;
        if (std::find(serials.begin(), serials.end(), c.model_serial) == serials.end()) serials.push_back(c.model_serial);
    }
    // res2idx: (model serial, chain, resi, icode) -> residue
    // With ONE model serial a plane entry can only resolve to the residue it was fitted from (the hierarchy holds one residue
    // per (chain, resi, icode)); the keyed lookup below is needed for multi-model files only.
    const bool one_model = serials.size() <= 1;
    const bool direct = model0_only || s.chains.empty() || s.chains.back().model_idx == 0;  // a single model in the file
    if (direct) first_of_res->assign(s.residues.size(), -1);
    std::unordered_map<PlaneKey, uint32_t, PlaneKeyHash> res_of;
    if (!one_model) {
        res_of.reserve(s.residues.size() * 2);
        for (uint32_t r = 0; r < s.residues.size(); r++) {
            const ResidueInfo &ri = s.residues[r];
            res_of[plane_key(s.chains[ri.chain].model_serial, s.chains[ri.chain].id.c_str(), ri.resi, ri.icode.c_str(), "", "")] = r;
        }
    }
    if (!direct) index->reserve(s.residues.size() * 2);
    // complex.rs:447-449 / 489-492: for EVERY model serial, ALL chains of ALL models are visited; later inserts overwrite
    // the plane of a residue does not depend on the model serial it is filed under: fit once, file per serial
    static const std::vector<Plane> no_planes;
    const std::vector<Plane> &fitted = fitted_in ? *fitted_in : no_planes;
    for (int32_t m : serials)
        for (uint32_t r = 0; r < n_res; r++) {
            const ResidueInfo &ri = s.residues[r];
            if (!has_plane[r]) continue;
            const Plane pl = fitted_in ? fitted[r] : Plane{};
            if (direct) (*first_of_res)[r] = (int64_t)out->size();
            for (uint32_t k = 0; k < ri.altlocs.size(); k++) {
                const std::string &alt = ri.altlocs[k];
                size_t slot;
                if (direct) { slot = out->size(); out->push_back(PlaneEntry{}); }
                else {
                    const PlaneKey key = plane_key(m, s.chains[ri.chain].id.c_str(), ri.resi, ri.icode.c_str(), alt.c_str(), ri.name.c_str());
                    auto it = index->find(key);
                    if (it == index->end()) { it = index->emplace(key, out->size()).first; out->push_back(PlaneEntry{}); }
                    slot = it->second;
                }
                PlaneEntry &e = (*out)[slot];
                e.model_serial = m; e.chain = s.chains[ri.chain].id; e.resi = ri.resi; e.icode = ri.icode; e.altloc = alt; e.resn = ri.name;
                e.plane = pl; e.res = r; e.alt_k = k;
                if (one_model) { e.has_ord = true; e.ord = ri.ord; }
            }
        }
    if (!one_model) for (PlaneEntry &e : *out) {
        auto it = res_of.find(plane_key(e.model_serial, e.chain.c_str(), e.resi, e.icode.c_str(), "", ""));
        if (it == res_of.end()) continue;
        const ResidueInfo &ri = s.residues[it->second];
        if (ri.name != e.resn || std::find(ri.altlocs.begin(), ri.altlocs.end(), e.altloc) == ri.altlocs.end()) continue;
        e.has_ord = true; e.ord = ri.ord;
    }
}

// plane atoms per residue: bit 1 = ring-plane atom (residues.rs:163-186), bit 2 = sc-plane atom (residues.rs:188-268)
static void plane_atom_bits(const arp_structure &s, std::vector<uint8_t> *bits, std::vector<char> *has_ring, std::vector<char> *has_sc) {
    bits->assign(s.n, 0);
    has_ring->assign(s.residues.size(), 0); has_sc->assign(s.residues.size(), 0);
    parallel_for(s.residues.size(), 512, [&](size_t r0, size_t r1, size_t) {
        for (size_t r = r0; r < r1; r++) {
            const ResidueInfo &ri = s.residues[r];
            const char *rn = ring_atoms_of(ri.name), *sn = sc_atoms_of(ri.name);
            if (!rn && !sn) continue;
            uint32_t nr = 0, ns = 0;
            for (uint32_t a : ri.atoms) {
                uint8_t b = 0;
                if (rn && in_words(rn, s.name.at(a))) { b |= 1u; nr++; }
                if (sn && in_words(sn, s.name.at(a))) { b |= 2u; ns++; }
                (*bits)[a] = b;
            }
            (*has_ring)[r] = nr >= 3; (*has_sc)[r] = ns >= 3;  // residues.rs:273
        }
    });
}
#ifdef ARP_WITH_HOST_TABLE
static void fit_planes_host(const arp_structure &s, const std::vector<uint8_t> &bits, uint8_t want, std::vector<Plane> *fitted) {
    fitted->assign(s.residues.size(), Plane{});
    parallel_for(s.residues.size(), 512, [&](size_t r0, size_t r1, size_t) {
        std::vector<std::array<double, 3>> pts;
        for (size_t r = r0; r < r1; r++) {
            pts.clear();
            for (uint32_t a : s.residues[r].atoms) if (bits[a] & want) pts.push_back({s.x[a], s.y[a], s.z[a]});
            if (pts.size() >= 3) fit_plane(pts, &(*fitted)[r]);
        }
    });
}

// should_compare_residues (complex.rs:94-131) on prepared keys
struct ResKey { int32_t model_serial; uint32_t chain_rank; uint32_t ord; bool in_l, in_r; };
static bool compare_residues(const ResKey &a, const ResKey &b, bool symmetric) {
    if (a.model_serial != b.model_serial) return false;
    if (!((a.in_l && b.in_r) || (b.in_l && a.in_r))) return false;
    if (a.chain_rank == b.chain_rank) {
        if (symmetric) return (b.ord > 1) && (a.ord < b.ord - 1);
        bool neigh = (a.ord == 0) ? (b.ord == a.ord || b.ord == a.ord + 1) : (b.ord == a.ord - 1 || b.ord == a.ord || b.ord == a.ord + 1);
        return !neigh;
    }
    return !(symmetric && a.in_r && b.in_r && a.in_l && b.in_l && a.chain_rank > b.chain_rank);
}

#endif

}  // namespace arp

using namespace arp;
// ---- the device table path (SURVEY.md 8f rows f1 + f2) ------------------------------------------------------------------------
EntityRec arp::atom_entity(const arp_structure &s, size_t a) {
    EntityRec e;
    memcpy(e.chain, s.chain.at(a), 8); memcpy(e.resn, s.res_resn.at(a), 8); memcpy(e.atomn, s.name.at(a), 8);
    memcpy(e.insertion, s.icode.at(a), 4); memcpy(e.altloc, s.altloc.at(a), 4);
    e.resi = s.resi[a]; e.atomi = s.serial[a]; e.atom = (int32_t)a; e.model = (uint32_t)s.model_serial[a];
    return e;
}
EntityRec arp::ring_entity(const PlaneEntry &r) {
    EntityRec e;
    auto put = [](char *dst, size_t cap, const std::string &v) { memset(dst, 0, cap); memcpy(dst, v.data(), std::min(cap - 1, v.size())); };
    put(e.chain, 8, r.chain); put(e.resn, 8, r.resn); put(e.atomn, 8, "Ring"); put(e.insertion, 4, r.icode); put(e.altloc, 4, r.altloc);
    e.resi = r.resi; e.atomi = 0; e.atom = -1; e.model = (uint32_t)r.model_serial;
    return e;
}

TableCache::~TableCache() {
    join_book();
    if (dev.block) { (void)hipSetDevice(dev.device); (void)hipFree(dev.block); if (dev.derived) (void)hipFree(dev.derived); if (dev.rings_block) (void)hipFree(dev.rings_block); }
}

namespace {
void free_table_cache(void *p) { delete (TableCache *)p; }
uint32_t be32(const char *p) { return ((uint32_t)(unsigned char)p[0] << 24) | ((uint32_t)(unsigned char)p[1] << 16) | ((uint32_t)(unsigned char)p[2] << 8) | (uint32_t)(unsigned char)p[3]; }
uint32_t be32s(const std::string &v) { char b[4] = {0, 0, 0, 0}; memcpy(b, v.data(), std::min<size_t>(3, v.size())); return be32(b); }
}  // namespace

TableCache *arp::table_cache_of(arp_structure *s) {
    std::lock_guard<std::mutex> guard(s->table_cache_mu);
    if (s->table_cache) return (TableCache *)s->table_cache;
    std::unique_ptr<TableCache> holder(new TableCache());  // (published at the end: an exception on the way leaks nothing, and its job is joined)
    TableCache *c = holder.get();
    const size_t n = s->n, nr = s->residues.size();
    LapTimer lap("    table cache %-22s %8.3f ms\n");
    plane_atom_bits(*s, &c->plane_bits, &c->has_ring, &c->has_sc);
    lap("plane bits");
    c->res_atom_ptr.assign(nr + 1, 0);
    for (size_t r = 0; r < nr; r++) c->res_atom_ptr[r + 1] = c->res_atom_ptr[r] + (uint32_t)s->residues[r].atoms.size();
    c->res_atom_idx.resize(c->res_atom_ptr[nr]);
    parallel_for(nr, 4096, [&](size_t r0, size_t r1, size_t) {
        for (size_t r = r0; r < r1; r++) std::copy(s->residues[r].atoms.begin(), s->residues[r].atoms.end(), c->res_atom_idx.begin() + c->res_atom_ptr[r]);
    });
    lap("residue CSR");
    build_planes(*s, true, c->has_ring, nullptr, &c->rings, &c->ring_idx, &c->ring_first);
    lap("ring entities");
    // A file with a single model holds one residue per (chain, resi, icode): an entity's side-chain plane can only be its own residue's,
    // and the keyed entries (one per residue and conformer) are needed for multi-model files only.
    c->direct = s->chains.empty() || s->chains.back().model_idx == 0;
    if (!c->direct) build_planes(*s, false, c->has_sc, nullptr, &c->scp, &c->sc_idx, &c->sc_first);
    lap("sc-plane entities");
    // model tables: ordinal -> serial, and the rank of the serial (sort key `model`, mod.rs:122)
    {
        const uint32_t nm = s->chains.empty() ? 1u : s->chains.back().model_idx + 1u;
        c->model_serial_of.assign(nm, 0);
        for (const ChainInfo &ch : s->chains) c->model_serial_of[ch.model_idx] = ch.model_serial;
        std::vector<uint32_t> serials;
        for (int32_t v : c->model_serial_of) serials.push_back((uint32_t)v);  // the column is u32 (mod.rs:143)
        std::sort(serials.begin(), serials.end());
        serials.erase(std::unique(serials.begin(), serials.end()), serials.end());
        c->model_rank.resize(nm);
        for (uint32_t m = 0; m < nm; m++) c->model_rank[m] = (uint32_t)(std::lower_bound(serials.begin(), serials.end(), (uint32_t)c->model_serial_of[m]) - serials.begin());
        c->ring_model_rank.resize(c->rings.size());
        for (size_t k = 0; k < c->rings.size(); k++)
            c->ring_model_rank[k] = (uint32_t)(std::lower_bound(serials.begin(), serials.end(), (uint32_t)c->rings[k].model_serial) - serials.begin());
    }
    // per-atom entity keys and the residue whose side-chain plane applies (the join key of mod.rs:100-110 plus resn, as in collect_sc_stats)
    c->atom_keys.resize(n);
    c->atom_sc_src.assign(n, ARP_NONE);
    parallel_for(n, 1u << 15, [&](size_t a0, size_t a1, size_t) {
        for (size_t a = a0; a < a1; a++) c->atom_keys[a] = EntKey{s->resi[a], be32(s->altloc.at(a)), s->serial[a], be32(s->icode.at(a))};
    });
    parallel_for(nr, 2048, [&](size_t r0, size_t r1, size_t) {
        std::vector<uint32_t> src_of_alt;
        for (size_t r = r0; r < r1; r++) {
            const ResidueInfo &ri = s->residues[r];
            if (ri.atoms.empty()) continue;
            const uint32_t a0 = ri.atoms[0];
            src_of_alt.assign(ri.altlocs.size(), ARP_NONE);
            for (size_t k = 0; k < ri.altlocs.size(); k++) {
                if (c->direct) { if (c->has_sc[r]) src_of_alt[k] = (uint32_t)r; continue; }
                auto f = c->sc_idx.find(plane_key(s->model_serial[a0], s->chain.at(a0), s->resi[a0], s->icode.at(a0), ri.altlocs[k].c_str(), s->res_resn.at(a0)));
                if (f != c->sc_idx.end()) src_of_alt[k] = c->scp[f->second].res;
            }
            for (uint32_t a : ri.atoms)
                for (size_t k = 0; k < ri.altlocs.size(); k++)
                    if (strcmp(s->altloc.at(a), ri.altlocs[k].c_str()) == 0) { c->atom_sc_src[a] = src_of_alt[k]; break; }
        }
    });
    c->ring_sc_src.assign(c->rings.size(), ARP_NONE);
    c->ring_keys.resize(c->rings.size());
    for (size_t k = 0; k < c->rings.size(); k++) {
        const PlaneEntry &r = c->rings[k];
        if (c->direct) { if (c->has_sc[r.res]) c->ring_sc_src[k] = r.res; }  // same residue, same conformer altloc
        else {
            auto f = c->sc_idx.find(plane_key(r.model_serial, r.chain.c_str(), r.resi, r.icode.c_str(), r.altloc.c_str(), r.resn.c_str()));
            if (f != c->sc_idx.end()) c->ring_sc_src[k] = c->scp[f->second].res;
        }
        c->ring_keys[k] = EntKey{r.resi, be32s(r.altloc), 0, be32s(r.icode)};  // complex.rs:334-342: atomi 0
    }
    lap("keys + sc sources");
    // The entity book: names and numbers of every atom and ring, gathered once.  Only the tables' string columns read it, so it is filled
    // by a job of its own while the first call's uploads and kernels run; get_contacts_device waits for it before it hands out a table.
    c->book = std::make_shared<EntityBook>();
    {
        EntityBook *bk = c->book.get();
        bk->n = n + c->rings.size();
        bk->ent.reset(new EntityRec[bk->n]);
        bk->lens.reset(new uint32_t[bk->n]);
        const int workers = host_threads();
        const arp_structure *sp = s;
        const TableCache *cp = c;
        auto fill = [bk, sp, cp, workers]() {
            HostThreadsScope scope(workers);
            const size_t n_atoms = sp->n;
            auto lens_of = [](const EntityRec &e) {
                auto len = [](const char *p, int w) { int k = 0; while (k < w && p[k]) k++; return (uint32_t)k; };
                return len(e.chain, 8) | (len(e.resn, 8) << 4) | (len(e.atomn, 8) << 8) | (len(e.insertion, 4) << 12) | (len(e.altloc, 4) << 16);
            };
            parallel_for(n_atoms, 1u << 14, [&](size_t a0, size_t a1, size_t) {
                for (size_t a = a0; a < a1; a++) { bk->ent[a] = atom_entity(*sp, a); bk->lens[a] = lens_of(bk->ent[a]); }
            });
            for (size_t k = 0; k < cp->rings.size(); k++) { bk->ent[n_atoms + k] = ring_entity(cp->rings[k]); bk->lens[n_atoms + k] = lens_of(bk->ent[n_atoms + k]); }
        };
        // (an exception must not leave the thread's function: it is parked and rethrown by wait_for_book on the thread that asks for the book)
        TableCache *cw = c;
        auto job = [fill, cw]() noexcept { try { fill(); } catch (...) { cw->book_error = std::current_exception(); } };
        try { c->book_job = std::thread(job); } catch (const std::system_error &) { fill(); }  // (no thread to be had: filled here)
    }
    lap("entity book (job started)");
    s->table_cache = holder.release(); s->table_cache_free = free_table_cache;
    return c;
}

namespace {
// the structure's arrays on the context's device: uploaded once; only the attribute words depend on the chain groups
arp_status ensure_resident(arp_context *ctx, arp_structure *s, TableCache *c, const char *groups) {
    DevStructure &d = c->dev;
    const int device = context_device(ctx);
    hipStream_t st = (hipStream_t)context_stream(ctx);
    HIP_TRY(hipSetDevice(device));
    const uint64_t n = s->n, nr = s->residues.size(), nh = s->res_h_idx.size(), nm = c->model_rank.size();
    if (!d.block || d.device != device) {
        if (d.block) { (void)hipSetDevice(d.device); (void)hipFree(d.block); if (d.derived) (void)hipFree(d.derived); if (d.rings_block) (void)hipFree(d.rings_block); (void)hipSetDevice(device); d.block = nullptr; d.derived = nullptr; d.rings_block = nullptr; d.rings_cap = 0; d.rings_host.clear(); }
        struct Seg { const void *src; uint64_t bytes; void **dst; };
        Seg seg[] = {{s->x.data(), n * 8, (void **)&d.x}, {s->y.data(), n * 8, (void **)&d.y}, {s->z.data(), n * 8, (void **)&d.z},
                     {s->attr.data(), n * 4, (void **)&d.attr}, {s->res_ord.data(), n * 4, (void **)&d.res_ord}, {s->res_id.data(), n * 4, (void **)&d.res_id},
                     {s->res_h_ptr.data(), (nr + 1) * 4, (void **)&d.res_h_ptr}, {s->res_h_idx.data(), nh * 4, (void **)&d.res_h_idx},
                     {s->res_cb.data(), nr * 4, (void **)&d.res_cb}, {s->res_sg.data(), nr * 4, (void **)&d.res_sg},
                     {s->chain_rank.data(), n * 4, (void **)&d.chain_rank}, {s->model.data(), n * 4, (void **)&d.model},
                     {c->plane_bits.data(), n, (void **)&d.plane_bits}, {c->res_atom_ptr.data(), (nr + 1) * 4, (void **)&d.res_atom_ptr},
                     {c->res_atom_idx.data(), c->res_atom_idx.size() * 4, (void **)&d.res_atom_idx}, {c->atom_sc_src.data(), n * 4, (void **)&d.atom_sc_src},
                     {c->atom_keys.data(), n * sizeof(EntKey), (void **)&d.ent_key}, {c->model_rank.data(), nm * 4, (void **)&d.model_rank},
                     {c->model_serial_of.data(), nm * 4, (void **)&d.model_serial_of}};
        Carver lay;
        std::vector<uint64_t> offs;
        for (const Seg &g : seg) offs.push_back(lay.take(g.bytes));
        const uint64_t total = std::max<uint64_t>(lay.off, 256);
        LapTimer lap("    resident %-25s %8.3f ms\n");
        HIP_TRY(hipMalloc((void **)&d.block, total));
        lap("device block");
        d.device = device;
        // one pinned staging block, filled by the host workers, one copy across PCIe (pageable arrays cross at ~3 GB/s)
        char *dev_scr = nullptr, *pin = nullptr;
        arp_status stt = context_scratch(ctx, 1, 0, total, &dev_scr, &pin);
        if (stt != ARP_OK) return stt;
        lap("pinned staging block");
        const size_t n_seg = sizeof seg / sizeof seg[0];
        for (size_t k = 0; k < n_seg; k++) *seg[k].dst = d.block + offs[k];
        parallel_for(n_seg * 8, 1, [&](size_t k0, size_t k1, size_t) {  // every segment in 8 slices
            for (size_t k = k0; k < k1; k++) {
                const Seg &g = seg[k / 8];
                const uint64_t lo = g.bytes * (k % 8) / 8, hi = g.bytes * (k % 8 + 1) / 8;
                if (hi > lo) memcpy(pin + offs[k / 8] + lo, (const char *)g.src + lo, hi - lo);
            }
        });
        lap("gather into it");
        HIP_TRY(hipMemcpyAsync(d.block, pin, total, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));  // (the pinned block is scratch: reused by the table pass below)
        lap("H2D");
        d.n = n; d.n_res = nr; d.n_h = nh;
        d.n_chains = (uint32_t)s->chain_ids.size(); d.n_models = (uint32_t)nm;
        d.any_icode = false;
        for (uint64_t a = 1; a < n && !d.any_icode; a++) d.any_icode = c->atom_keys[a].icode != c->atom_keys[0].icode;  // (rings carry their residue's: the same values)
        d.attr_groups = groups;
        lap("insertion-code scan");
    } else if (d.attr_groups != groups) {
        HIP_TRY(hipMemcpyAsync(d.attr, s->attr.data(), n * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        d.attr_groups = groups;
    }
    return ARP_OK;
}

arp_status get_contacts_device(arp_context *ctx, arp_structure *s, const char *groups, double vdw_comp, double dist_cutoff, arp_table **out) {
    LapTimer lap("  get_contacts %-22s %8.3f ms\n");
    TableCache *c = table_cache_of(s);
    std::lock_guard<std::mutex> one_call_per_structure(c->mu);
    {   // InteractionComplex::new (complex.rs:36-68): the ligand / receptor bits of this chain-group spec (a no-op when unchanged)
        const arp_status sg = apply_groups(s, groups);
        if (sg != ARP_OK) return sg;
    }
    if (c->rings.empty()) { set_error("Error building ring positions"); return ARP_ERR_NO_RINGS; }  // complex.rs:50
    lap("entities (cached)");
    arp_status st = ensure_resident(ctx, s, c, groups);
    if (st != ARP_OK) return st;
    lap("resident copy");
    // chain sets of this call (utils.rs:71-115): chains without atoms still belong to them.  Kept per chain-group spec: on a structure
    // with thousands of chains this bookkeeping costs more than the GPU pair pass.
    if (!c->have_rings_dev || c->rings_groups != groups) {
        std::vector<char> chain_l(s->chain_ids.size(), 0), chain_r(s->chain_ids.size(), 0);
        std::unordered_map<std::string, uint32_t> rank;
        for (size_t k = 0; k < s->chain_ids.size(); k++) rank[s->chain_ids[k]] = (uint32_t)k;
        {
            std::vector<std::string> L, R;
            if ((st = parse_groups(s->chain_ids, groups, &L, &R)) != ARP_OK) return st;
            for (auto &ch : L) chain_l[rank[ch]] = 1;
            for (auto &ch : R) chain_r[rank[ch]] = 1;
        }
        c->rings_dev.resize(c->rings.size());
        for (size_t k = 0; k < c->rings_dev.size(); k++) {
            PlaneEntry &e = c->rings[k];
            e.chain_rank = rank[e.chain]; e.in_l = chain_l[e.chain_rank]; e.in_r = chain_r[e.chain_rank];
            c->rings_dev[k] = RingEnt{e.res, e.model_serial, c->ring_model_rank[k], e.chain_rank, (e.in_l ? 1u : 0u) | (e.in_r ? 2u : 0u) | (e.has_ord ? 4u : 0u), e.ord, c->ring_sc_src[k], 0u};
        }
        c->rings_groups = groups; c->have_rings_dev = true;
    }
    const std::vector<RingEnt> &rings = c->rings_dev;
    // get_atomic_contacts (complex.rs:189-299): the GPU hot path, on the resident arrays, list left on the device
    arp_params prm;
    arp_default_params(&prm);
    prm.vdw_comp = vdw_comp; prm.dist_cutoff = dist_cutoff;
    prm.flags |= ARP_FLAG_CONTACTS_ONLY;  // only pairs with an interaction become rows
    DevStructure &d = c->dev;
    arp_atoms dv{};
    dv.n = d.n; dv.x = d.x; dv.y = d.y; dv.z = d.z; dv.attr = d.attr; dv.res_ord = d.res_ord; dv.chain_rank = d.chain_rank; dv.model = d.model;
    dv.res_id = d.res_id; dv.n_res = d.n_res; dv.res_h_ptr = d.res_h_ptr; dv.res_h_idx = d.res_h_idx; dv.res_cb = d.res_cb; dv.res_sg = d.res_sg;
    dv.location = ARP_MEM_DEVICE;
    const arp_pair *pairs = nullptr;  // a view of the context's own buffer: one pass, no allocation
    uint64_t n_pairs = 0;
    if ((st = contacts_atomic_view(ctx, &dv, &prm, &pairs, &n_pairs)) != ARP_OK) return st;
    lap("atomic pairs (GPU)");
    TableRowsHost rows;
    st = device_table(ctx, d, rings, c->ring_keys, pairs, n_pairs, dist_cutoff, &rows);
    if (st != ARP_OK) return st;
    lap("device table");
    // the table keeps the rows as they came back and a reference to the structure's entity book: no per-row host work here
    arp_table *t = new arp_table();
    t->n = rows.n;
    t->rows_owner = std::move(rows.owner); t->rows = rows.rows; t->sc = rows.sc;
    c->wait_for_book();
    t->book = c->book;
    lap("table object");
    *out = t;
    return ARP_OK;
}
}  // namespace

#ifdef ARP_WITH_HOST_TABLE
#include "../../tests/hosttable/table_host.inl"  // test-only: not part of the product library (build.py: build_host_table_library)
#endif

extern "C" arp_status arp_get_contacts(arp_context *ctx, arp_structure *s, const char *groups, double vdw_comp, double dist_cutoff,
                                       arp_table **out) {
    return arp_get_contacts_mt(ctx, s, groups, vdw_comp, dist_cutoff, -1, out);
}

extern "C" arp_status arp_get_contacts_mt(arp_context *ctx, arp_structure *s, const char *groups, double vdw_comp, double dist_cutoff,
                                          int32_t num_threads, arp_table **out) try {
    if (!s || !out || !groups) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    *out = nullptr;
    HostThreadsScope threads(num_threads);  // one worker count for every pass of this call
#ifdef ARP_WITH_HOST_TABLE   // test-only build (tests/hosttable): the round-1 host assembly as a cross-check of the device table
    if (g_debug.table_host) return get_contacts_host(ctx, s, groups, vdw_comp, dist_cutoff, out);
#endif
    return get_contacts_device(ctx, s, groups, vdw_comp, dist_cutoff, out);
} ARP_ABI_CATCH

// The planes the device fits (residues.rs:270-298), per residue of the filtered model in hierarchy order: 12 doubles
// {ring centre, ring normal, sc centre, sc normal}; valid[r] bit 1 = ring plane, bit 2 = side-chain plane.
extern "C" uint64_t arp_structure_n_residues(const arp_structure *s) { return s ? s->residues.size() : 0; }
extern "C" arp_status arp_structure_fit_planes(arp_context *ctx, arp_structure *s, double *planes, uint8_t *valid) try {
    if (!ctx || !s || !planes || !valid) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    arp_atoms view;
    arp_status st = arp_structure_atoms(s, s->groups_valid ? s->groups_applied.c_str() : "/", &view);
    if (st != ARP_OK) return st;
    TableCache *c = table_cache_of(s);
    if ((st = ensure_resident(ctx, s, c, s->groups_applied.c_str())) != ARP_OK) return st;
    std::vector<double> p;
    std::vector<uint8_t> v;
    if ((st = device_planes(ctx, c->dev, &p, &v)) != ARP_OK) return st;
    memcpy(planes, p.data(), p.size() * sizeof(double));
    memcpy(valid, v.data(), v.size());
    return ARP_OK;
} ARP_ABI_CATCH
