// The ensemble entry points -- contact frequencies, their residue level (3.12), timelines (3.13), similarity (3.14),
// autocorrelation (3.16), clusters (3.17) and water bridges (3.19) -- and the host yardsticks of the last four (arp_timeline_stats, arp_bit_gram_host, arp_bit_autocorr_host,
// arp_bit_cluster_host).  One preamble (freq_prepare) checks the call and fills the device job; the device pipelines are freq.inl, timeline.inl,
// similarity.inl, autocorr.inl and cluster.inl; the table they all return is the level's frequency table (table.cpp's columns), with the timeline columns,
// the matrix, the curves or the clusters attached.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "table.h"

// ---- contact frequencies over frames (device pipeline: freq.inl) -------------------------------------------------
namespace arp {
// Model 0 of the structure is the topology: its atoms are the prefix [0, n0) of the structure's atoms and its residues the prefix [0, r0) of the
// residue tables (the hierarchy is built in file order, model by model).  With frames_from_models, every further model must repeat model 0's
// atoms one for one; the frames are then the models' coordinates.
arp_status freq_topology(const arp_structure *s, bool frames_from_models, uint64_t *n0, uint64_t *r0, uint64_t *n_models) {
    uint64_t n = 0;
    while (n < s->n && s->model[n] == 0u) n++;
    uint64_t r = 0;
    while (r < s->residues.size() && s->chains[s->residues[r].chain].model_idx == 0u) r++;
    const uint64_t nm = s->chains.empty() ? 1u : (uint64_t)s->chains.back().model_idx + 1u;
    *n0 = n; *r0 = r; *n_models = nm;
    if (!frames_from_models || nm == 1) return ARP_OK;
    auto serial_of = [&](uint64_t m) { for (const ChainInfo &c : s->chains) if (c.model_idx == m) return c.model_serial; return 0; };
    for (uint64_t m = 1; m < nm; m++) {
        const uint64_t base = m * n;
        uint64_t have = 0;
        while (base + have < s->n && s->model[base + have] == m) have++;
        const uint64_t shared = std::min(have, n);
        for (uint64_t k = 0; k < shared; k++) {
            const uint64_t a = base + k;
            const char *what = nullptr;
            if (memcmp(s->chain.at(a), s->chain.at(k), 8) != 0) what = "chain";
            else if (memcmp(s->resn.at(a), s->resn.at(k), 8) != 0 || memcmp(s->res_resn.at(a), s->res_resn.at(k), 8) != 0) what = "residue name";
            else if (s->resi[a] != s->resi[k]) what = "residue number";
            else if (memcmp(s->icode.at(a), s->icode.at(k), 4) != 0) what = "insertion code";
            else if (memcmp(s->altloc.at(a), s->altloc.at(k), 4) != 0) what = "altloc";
            else if (memcmp(s->name.at(a), s->name.at(k), 8) != 0) what = "atom name";
            else if (s->serial[a] != s->serial[k]) what = "serial number";
            else if (memcmp(s->elem.at(a), s->elem.at(k), 4) != 0) what = "element";
            if (what) {
                set_error("contact frequencies: model %llu (MODEL %d) differs from model 0 at atom %llu: %s (%s %s %d %s serial %d, model 0 has %s %s %d %s serial %d)",
                          (unsigned long long)m, serial_of(m), (unsigned long long)k, what, s->chain.at(a), s->resn.at(a), s->resi[a], s->name.at(a), s->serial[a],
                          s->chain.at(k), s->resn.at(k), s->resi[k], s->name.at(k), s->serial[k]);
                return ARP_ERR_BAD_INPUT;
            }
        }
        if (have != n) {
            set_error("contact frequencies: model %llu (MODEL %d) differs from model 0 at atom %llu: it has %llu atoms, model 0 has %llu",
                      (unsigned long long)m, serial_of(m), (unsigned long long)shared, (unsigned long long)have, (unsigned long long)n);
            return ARP_ERR_BAD_INPUT;
        }
    }
    return ARP_OK;
}
}  // namespace arp

using namespace arp;

namespace {
// The ring entities of the topology (arp_contact_frequencies_ex): those arp_get_contacts builds for model 0 as a single-model structure, from the
// table path's own builder.  A single-model structure's are the cached ones; model 0 of a multi-model file gets its own list (the cached one files
// planes under every model serial: DESIGN.md section 3.7).
struct FreqRingTopo {
    std::vector<PlaneEntry> own;
    const std::vector<PlaneEntry> *ents = nullptr;
    std::vector<RingEnt> rings;        // src_res = slot
    std::vector<uint32_t> slot_res, cand;
};
void freq_ring_entities(arp_structure *s, TableCache *c, uint64_t r0, FreqRingTopo *out) {
    if (c->direct) { out->ents = &c->rings; return; }
    PlaneIndex idx;
    std::vector<int64_t> first;
    build_planes(*s, true, c->has_ring, nullptr, &out->own, &idx, &first, (size_t)r0);
    out->ents = &out->own;
}

// What every ensemble entry point does before the device runs.  First the call's own checks, under its own name `what`: the arguments, the flags it
// allows (ARP_FREQ_RINGS and `own_flags`), the level.  Then the checks of arp_contact_frequencies_ex (nothing here touches the device), the chain
// groups on the topology's attribute words, the ring entities with ARP_FREQ_RINGS, and the device job -- keyed by residue for level 1 -- with the
// capacity knobs.  checked_only: ctx was NULL.
struct FreqPrep {
    uint64_t n0 = 0, r0 = 0, F = 0;
    int32_t level = 0;
    std::vector<double> model_xyz;
    std::vector<uint32_t> attr;
    FreqRingTopo rt;
    std::vector<uint32_t> water, polar;   // ARP_FREQ_WATERS: the topology's water atoms and polar atoms, ascending
    FreqJob job;
    uint64_t timeline_cap = 0, similarity_cap = 0, autocorr_cap = 0;   // bytes the bitmap / the similarity matrix / the autocorrelation matrix may take
    bool checked_only = false;
};
arp_status freq_prepare(const char *what, uint32_t own_flags, int32_t level, arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const char *groups,
                        double vdw_comp, double dist_cutoff, uint32_t flags, arp_table **out, FreqPrep *p) {
    if (!s || !out || !groups) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    *out = nullptr;
    const uint32_t unknown = flags & ~((uint32_t)ARP_FREQ_RINGS | own_flags);
    if (unknown) { set_error("%s: unknown flag bits 0x%x", what, unknown); return ARP_ERR_BAD_INPUT; }
    if (level != 0 && level != 1) { set_error("%s: level must be 0 (atoms) or 1 (residues), got %d", what, (int)level); return ARP_ERR_BAD_INPUT; }
    p->level = level;
    if ((flags & ARP_FREQ_WATERS) && level == 0) {
        set_error("%s: ARP_FREQ_WATERS needs level 1 (residues): a bridge joins two residues through a water; arp_water_bridges lists the atoms of every bridge", what);
        return ARP_ERR_BAD_INPUT;
    }
    // validation: nothing here touches the device
    uint64_t &n0 = p->n0, &r0 = p->r0, nm = 1;
    arp_status st = freq_topology(s, xyz == nullptr, &n0, &r0, &nm);
    if (st != ARP_OK) return st;
    const uint64_t F = p->F = xyz ? n_frames : nm;
    if (F == 0) { set_error("contact frequencies: at least one frame is needed"); return ARP_ERR_BAD_INPUT; }
    if (n0 >= (1ull << 29)) { set_error("contact frequencies: the topology has %llu atoms, at most 2^29 - 1 are supported", (unsigned long long)n0); return ARP_ERR_BAD_INPUT; }
    if (F > (1ull << 40) / std::max<uint64_t>(n0, 1)) { set_error("contact frequencies: too many frames"); return ARP_ERR_BAD_INPUT; }
    std::vector<double> &model_xyz = p->model_xyz;
    if (!xyz) {  // the models' coordinates as F x n0 x 3
        model_xyz.resize(F * n0 * 3);
        for (uint64_t a = 0; a < F * n0; a++) { model_xyz[3 * a] = s->x[a]; model_xyz[3 * a + 1] = s->y[a]; model_xyz[3 * a + 2] = s->z[a]; }
    }
    const double *frames = xyz ? xyz : model_xyz.data();
    {
        const uint64_t nv = F * n0 * 3;
        uint64_t bad = nv;
        for (uint64_t v = 0; v < nv; v++) if (!std::isfinite(frames[v])) { bad = v; break; }
        if (bad != nv) {
            set_error("contact frequencies: non-finite coordinate in frame %llu, atom %llu", (unsigned long long)(bad / (3 * n0)), (unsigned long long)(bad / 3 % n0));
            return ARP_ERR_BAD_INPUT;
        }
    }
    if (std::isnan(vdw_comp) || std::isnan(dist_cutoff)) { set_error("NaN parameter"); return ARP_ERR_BAD_INPUT; }
    // the ligand / receptor bits of this chain-group spec, with the errors of arp_get_contacts (utils.rs:71-115); the structure's own attribute
    // words are left alone (a table call on it may be using them)
    std::vector<uint32_t> &attr = p->attr;
    attr.resize(n0);
    std::vector<uint32_t> bits(s->chain_ids.size(), 0);
    {
        std::vector<std::string> L, R;
        if ((st = parse_groups(s->chain_ids, groups, &L, &R)) != ARP_OK) return st;
        for (size_t k = 0; k < s->chain_ids.size(); k++) {
            if (std::binary_search(L.begin(), L.end(), s->chain_ids[k])) bits[k] |= ARP_ATTR_LIGAND;
            if (std::binary_search(R.begin(), R.end(), s->chain_ids[k])) bits[k] |= ARP_ATTR_RECEPTOR;
        }
        for (uint64_t a = 0; a < n0; a++) attr[a] = s->base_attr[a] | bits[s->chain_rank[a]];
    }
    // ARP_FREQ_RINGS: the topology's ring entities, as entities n0 .. n0 + n_rings - 1 (a topology without rings is the table without rings)
    FreqRingTopo &rt = p->rt;
    TableCache *cache = nullptr;
    uint64_t n_rings = 0;
    if (flags & ARP_FREQ_RINGS) {
        cache = table_cache_of(s);
        freq_ring_entities(s, cache, r0, &rt);
        n_rings = rt.ents->size();
        if (n0 + n_rings >= (1ull << 29)) {
            set_error("contact frequencies: the topology has %llu atoms and %llu rings, at most 2^29 - 1 entities are supported", (unsigned long long)n0, (unsigned long long)n_rings);
            return ARP_ERR_BAD_INPUT;
        }
    }
    // ARP_FREQ_WATERS: water atoms (residue HOH, not hydrogen) and polar atoms (donor or acceptor, not hydrogen); the classes keep them apart
    if (flags & ARP_FREQ_WATERS) {
        for (uint64_t a = 0; a < n0; a++) {
            if (attr[a] & ARP_ATTR_H) continue;
            const bool water = strcmp(s->res_resn.at(a), "HOH") == 0, polar = (attr[a] & (ARP_ATTR_DONOR | ARP_ATTR_ACCEPTOR)) != 0u;
            if (water && polar) {
                set_error("water bridges: atom %llu (%s of HOH %d, chain %s) is a water atom with a donor or acceptor class", (unsigned long long)a, s->name.at(a), s->resi[a], s->chain.at(a));
                return ARP_ERR_BAD_INPUT;
            }
            if (water) p->water.push_back((uint32_t)a);
            else if (polar) p->polar.push_back((uint32_t)a);
        }
    }
    p->checked_only = !ctx;
    if (!ctx) return ARP_OK;  // validation only
    FreqJob &job = p->job;
    job.n = n0; job.n_res = r0; job.n_h = r0 ? s->res_h_ptr[r0] : 0; job.n_frames = F;
    job.attr = attr.data(); job.res_ord = s->res_ord.data(); job.chain_rank = s->chain_rank.data(); job.res_id = s->res_id.data();
    job.res_h_ptr = s->res_h_ptr.data(); job.res_h_idx = s->res_h_idx.data(); job.res_cb = s->res_cb.data(); job.res_sg = s->res_sg.data();
    job.xyz = frames; job.vdw_comp = vdw_comp; job.dist_cutoff = dist_cutoff;
    job.chunk_atoms = g_debug.freq_chunk_atoms > 0 ? (uint64_t)g_debug.freq_chunk_atoms : 0u;
    if (level == 1) {
        job.residue = true;
        job.frame_bits = g_debug.freq_frame_bits > 0 ? (uint32_t)g_debug.freq_frame_bits : 0u;
    }
    p->timeline_cap = g_debug.timeline_cap_bytes > 0 ? (uint64_t)g_debug.timeline_cap_bytes : (1ull << 31);
    p->similarity_cap = g_debug.similarity_cap_bytes > 0 ? (uint64_t)g_debug.similarity_cap_bytes : (1ull << 31);
    p->autocorr_cap = g_debug.autocorr_cap_bytes > 0 ? (uint64_t)g_debug.autocorr_cap_bytes : (1ull << 31);
    job.n_water = p->water.size(); job.n_polar = p->polar.size();
    job.water = p->water.data(); job.polar = p->polar.data();
    if (n_rings) {
        std::unordered_map<std::string, uint32_t> rank;
        for (size_t k = 0; k < s->chain_ids.size(); k++) rank[s->chain_ids[k]] = (uint32_t)k;
        rt.rings.resize(n_rings);
        for (uint64_t k = 0; k < n_rings; k++) {  // (the entities of a residue follow each other: one slot per residue)
            const PlaneEntry &e = (*rt.ents)[k];
            if (rt.slot_res.empty() || rt.slot_res.back() != e.res) rt.slot_res.push_back(e.res);
            const uint32_t cr = rank[e.chain], cb = bits[cr];
            rt.rings[k] = RingEnt{(uint32_t)rt.slot_res.size() - 1u, 0, 0u, cr, ((cb & ARP_ATTR_LIGAND) ? 1u : 0u) | ((cb & ARP_ATTR_RECEPTOR) ? 2u : 0u) | (e.has_ord ? 4u : 0u), e.ord, ARP_NONE, 0u};
        }
        for (uint64_t a = 0; a < n0; a++) if ((attr[a] & ARP_ATTR_POS_RESN) && !(attr[a] & ARP_ATTR_H)) rt.cand.push_back((uint32_t)a);  // what the pair pass's cell list holds of them
        job.n_rings = n_rings; job.n_slots = rt.slot_res.size(); job.n_cand = rt.cand.size();
        job.rings = rt.rings.data(); job.slot_res = rt.slot_res.data(); job.cand = rt.cand.data();
        job.res_atom_ptr = cache->res_atom_ptr.data(); job.res_atom_idx = cache->res_atom_idx.data(); job.plane_bits = cache->plane_bits.data();
    }
    return ARP_OK;
}

// The frequency table of the device's rows at the job's level: the rows' counts and distance extremes as they came back, the identity of both
// entities of a row from the topology.  Atom level: an entity is an atom or (ARP_FREQ_RINGS) a ring; residue level: a residue, shown as its first
// topology atom (what the residue-SASA rows take it from).
std::unique_ptr<arp_table> freq_table(const arp_structure *s, const FreqPrep &prep, FreqRowsHost &rows) {
    const bool residues = prep.level == 1;
    const uint64_t n0 = prep.n0;
    std::vector<uint32_t> first;
    if (residues) {
        first.assign(prep.r0, ARP_NONE);
        for (uint64_t a = n0; a-- > 0;) first[s->res_id[a]] = (uint32_t)a;
    }
    std::unique_ptr<arp_table> t(new arp_table());
    t->n = rows.key.size();
    t->n_frames = std::move(rows.count); t->min_distance = std::move(rows.mn); t->max_distance = std::move(rows.mx);
    frequency_columns(t.get(), residues ? kResidueFreqSide : kAtomFreqSide);
    const uint32_t id_bits = residues ? rows.res_bits : 29u;  // key = from << (id_bits + 5) | to << 5 | code
    auto put = [&](SideCols &side, size_t k, uint32_t id) {
        if (residues) { side.put(k, atom_entity(*s, first.at(id))); side.residue[k] = (int32_t)id; }
        else if (id >= n0) { side.put(k, ring_entity((*prep.rt.ents)[id - n0])); side.ring[k] = (int32_t)(id - n0); }
        else side.put(k, atom_entity(*s, id));
    };
    for (size_t k = 0; k < t->n; k++) {
        const unsigned long long key = rows.key[k];
        t->interaction[k] = (int32_t)(key & 31u);
        t->frequency[k] = (float)((double)t->n_frames[k] / (double)prep.F);
        put(t->from, k, (uint32_t)(key >> (id_bits + 5u)));
        put(t->to, k, (uint32_t)((key >> 5) & ((1ull << id_bits) - 1u)));
    }
    return t;
}
}  // namespace

extern "C" arp_status arp_contact_frequencies(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp,
                                              double dist_cutoff, arp_table **out) {
    return arp_contact_frequencies_ex(ctx, s, n_frames, xyz, groups, vdw_comp, dist_cutoff, 0u, out);
}

namespace {
// both levels of the frequency call (level 1: DESIGN.md section 3.12 -- the device keys the items by residue and counts a frame once per row)
arp_status contact_frequencies(int32_t level, arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp, double dist_cutoff,
                               uint32_t flags, arp_table **out) {
    FreqPrep prep;
    arp_status st = freq_prepare("contact frequencies", level == 1 ? ARP_FREQ_WATERS : 0u, level, ctx, s, n_frames, xyz, groups, vdw_comp, dist_cutoff, flags, out, &prep);
    if (st != ARP_OK || prep.checked_only) return st;
    FreqRowsHost rows;
    if ((st = device_frequencies(ctx, prep.job, &rows)) != ARP_OK) return st;
    *out = freq_table(s, prep, rows).release();
    return ARP_OK;
}
}  // namespace

extern "C" arp_status arp_contact_frequencies_ex(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp,
                                                 double dist_cutoff, uint32_t flags, arp_table **out) try {
    return contact_frequencies(0, ctx, s, n_frames, xyz, groups, vdw_comp, dist_cutoff, flags, out);
} ARP_ABI_CATCH

extern "C" arp_status arp_residue_contact_frequencies(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp,
                                                      double dist_cutoff, uint32_t flags, arp_table **out) try {
    return contact_frequencies(1, ctx, s, n_frames, xyz, groups, vdw_comp, dist_cutoff, flags, out);
} ARP_ABI_CATCH

// ---- contact timelines over frames (device pipeline: timeline.inl) ----------------------------------------------------
extern "C" arp_status arp_contact_timelines(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp,
                                            double dist_cutoff, uint32_t flags, int32_t level, arp_table **out) try {
    FreqPrep prep;
    arp_status st = freq_prepare("contact timelines", ARP_TIMELINE_NO_BITMAP | ARP_FREQ_WATERS, level, ctx, s, n_frames, xyz, groups, vdw_comp, dist_cutoff, flags, out, &prep);
    if (st != ARP_OK || prep.checked_only) return st;
    FreqRowsHost rows;
    TimelineHost tl;
    if ((st = device_timelines(ctx, prep.job, !(flags & ARP_TIMELINE_NO_BITMAP), prep.timeline_cap, &rows, &tl)) != ARP_OK) return st;
    // the frequency columns are the frequency call's own (the same rows through the same table builder), the timeline columns join them
    std::unique_ptr<arp_table> t = freq_table(s, prep, rows);
    t->tl = std::move(tl);
    t->tl_frames = prep.F;
    timeline_columns(t.get());
    for (uint64_t k = 0; k < t->n; k++) t->mean_run[k] = (float)((double)t->n_frames[k] / (double)t->tl.n_events[k]);
    *out = t.release();
    return ARP_OK;
} ARP_ABI_CATCH

// ---- water bridges, frame by frame (device pipeline: freq_water.inl) ----------------------------------------------------------
extern "C" arp_status arp_water_bridges(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const char *groups, arp_table **out) try {
    FreqPrep prep;
    arp_status st = freq_prepare("water bridges", ARP_FREQ_WATERS, 1, ctx, s, n_frames, xyz, groups, 0.1, 6.5, ARP_FREQ_WATERS, out, &prep);
    if (st != ARP_OK || prep.checked_only) return st;
    std::vector<WaterTriple> rows;
    if ((st = device_water_bridges(ctx, prep.job, &rows)) != ARP_OK) return st;
    std::unique_ptr<arp_table> t(new arp_table());
    t->n = rows.size();
    water_bridge_columns(t.get());
    for (size_t k = 0; k < t->n; k++) {
        const WaterTriple &r = rows[k];
        t->frame[k] = r.frame;
        t->from.put(k, atom_entity(*s, r.p)); t->to.put(k, atom_entity(*s, r.q)); t->water.put(k, atom_entity(*s, r.w));
        t->from_distance[k] = r.dp; t->to_distance[k] = r.dq; t->distance[k] = std::max(r.dp, r.dq);
    }
    *out = t.release();
    return ARP_OK;
} ARP_ABI_CATCH

// The definition of the timeline statistics, bit by bit (no device): the yardstick of k_timeline_stats.
extern "C" arp_status arp_timeline_stats(uint64_t rows, uint64_t n_frames, const uint32_t *words, uint32_t *n_present, uint32_t *first, uint32_t *last, uint32_t *n_events,
                                         uint32_t *longest_run) try {
    if ((rows && n_frames && !words) || (rows && (!n_present || !first || !last || !n_events || !longest_run))) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    if (n_frames > 0xFFFFFFF0ull) { set_error("timeline statistics: more than 2^32 frames"); return ARP_ERR_BAD_INPUT; }
    const uint64_t W = (n_frames + 31u) / 32u;
    for (uint64_t r = 0; r < rows; r++) {
        uint32_t present = 0, f_first = ARP_NONE, f_last = ARP_NONE, events = 0, best = 0, run = 0;
        for (uint64_t f = 0; f < n_frames; f++) {
            if (words[r * W + (f >> 5)] >> (f & 31u) & 1u) {
                if (!run) events++;
                run++;
                present++;
                if (f_first == ARP_NONE) f_first = (uint32_t)f;
                f_last = (uint32_t)f;
                if (run > best) best = run;
            } else run = 0;
        }
        n_present[r] = present; first[r] = f_first; last[r] = f_last; n_events[r] = events; longest_run[r] = best;
    }
    return ARP_OK;
} ARP_ABI_CATCH

// ---- contact similarity between frames, contact co-occurrence between rows (device pipeline: similarity.inl) ----------------
extern "C" arp_status arp_contact_similarity(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp,
                                             double dist_cutoff, uint32_t flags, int32_t level, arp_table **out) try {
    FreqPrep prep;
    arp_status st = freq_prepare("contact similarity", ARP_SIM_COUNTS | ARP_SIM_ROWS, level, ctx, s, n_frames, xyz, groups, vdw_comp, dist_cutoff, flags, out, &prep);
    if (st != ARP_OK || prep.checked_only) return st;
    FreqRowsHost rows;
    SimilarityHost sim;
    if ((st = device_similarity(ctx, prep.job, (flags & ARP_SIM_ROWS) != 0, (flags & ARP_SIM_COUNTS) != 0, prep.timeline_cap, prep.similarity_cap, &rows, &sim)) != ARP_OK) return st;
    // the table is the frequency table of the level (the same rows through the same table builder); the matrix rides along
    std::unique_ptr<arp_table> t = freq_table(s, prep, rows);
    t->similarity = true;
    t->sim_flags = flags & (uint32_t)(ARP_SIM_COUNTS | ARP_SIM_ROWS);
    t->sim = std::move(sim);
    *out = t.release();
    return ARP_OK;
} ARP_ABI_CATCH

namespace {
arp_status bit_gram_args(uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, const void *out, const uint32_t *sizes) {
    if (flags & ~(uint32_t)(ARP_SIM_COUNTS | ARP_SIM_ROWS)) { set_error("bit gram: unknown flag bits 0x%x", flags & ~(uint32_t)(ARP_SIM_COUNTS | ARP_SIM_ROWS)); return ARP_ERR_BAD_INPUT; }
    if (n_bits >= (1ull << 32) || rows >= (1ull << 32)) { set_error("bit gram: 2^32 or more %s (the counts are u32)", n_bits >= (1ull << 32) ? "bits" : "rows"); return ARP_ERR_BAD_INPUT; }
    const uint64_t M = (flags & ARP_SIM_ROWS) ? rows : n_bits;
    if (rows && ((n_bits && !words) || (M && (!out || !sizes)))) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}
}  // namespace

// The definition of the matrix on its own (no device): the yardstick of k_bit_transpose / k_bit_sizes / k_bit_gram.  Every bit is looked at one by one
// and filed under its set (a frame's set of rows, or a row's set of frames); |a AND b| is then counted over the sets' words.
extern "C" arp_status arp_bit_gram_host(uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, void *out, uint32_t *sizes) try {
    arp_status st = bit_gram_args(rows, n_bits, words, flags, out, sizes);
    if (st != ARP_OK) return st;
    const bool by_rows = (flags & ARP_SIM_ROWS) != 0, counts = (flags & ARP_SIM_COUNTS) != 0;
    const uint64_t W = (n_bits + 31u) / 32u, M = by_rows ? rows : n_bits, N = by_rows ? n_bits : rows, K = (N + 31u) / 32u;
    if (!rows && (by_rows || !out || !sizes)) return ARP_OK;  // (the frames of a bitmap without rows are n_bits empty sets)
    std::vector<uint32_t> sets(M * K, 0u);
    for (uint64_t r = 0; r < rows; r++)
        for (uint64_t f = 0; f < n_bits; f++)
            if (words[r * W + (f >> 5)] >> (f & 31u) & 1u) {
                const uint64_t a = by_rows ? r : f, e = by_rows ? f : r;
                sets[a * K + (e >> 5)] |= 1u << (e & 31u);
            }
    for (uint64_t a = 0; a < M; a++) {
        uint32_t c = 0;
        for (uint64_t w = 0; w < K; w++) c += (uint32_t)__builtin_popcount(sets[a * K + w]);
        sizes[a] = c;
    }
    for (uint64_t a = 0; a < M; a++)
        for (uint64_t b = 0; b < M; b++) {
            uint32_t inter = 0;
            for (uint64_t w = 0; w < K; w++) inter += (uint32_t)__builtin_popcount(sets[a * K + w] & sets[b * K + w]);
            if (counts) { ((uint32_t *)out)[a * M + b] = inter; continue; }
            const uint64_t uni = (uint64_t)sizes[a] + sizes[b] - inter;
            ((float *)out)[a * M + b] = uni ? (float)((double)inter / (double)uni) : 1.0f;
        }
    return ARP_OK;
} ARP_ABI_CATCH

extern "C" arp_status arp_bit_gram(arp_context *ctx, uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, void *out, uint32_t *sizes) try {
    if (!ctx) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    arp_status st = bit_gram_args(rows, n_bits, words, flags, out, sizes);
    if (st != ARP_OK) return st;
    if (!rows || !n_bits) return arp_bit_gram_host(rows, n_bits, words, flags, out, sizes);  // (no bit to look at: every set is empty)
    const uint64_t cap = g_debug.similarity_cap_bytes > 0 ? (uint64_t)g_debug.similarity_cap_bytes : (1ull << 31);
    return device_bit_gram(ctx, rows, n_bits, words, (flags & ARP_SIM_ROWS) != 0, (flags & ARP_SIM_COUNTS) != 0, cap, out, sizes);
} ARP_ABI_CATCH

// ---- clusters of the frames by their contacts (device pipeline: cluster.inl) ---------------------------------------------------
namespace {
arp_status cluster_args(const char *what, float min_similarity, uint32_t max_clusters) {
    if (!(std::isfinite(min_similarity) && min_similarity >= 0.0f && min_similarity <= 1.0f)) {
        set_error("%s: min_similarity must be a finite value in [0, 1], got %g", what, (double)min_similarity);
        return ARP_ERR_BAD_INPUT;
    }
    if (max_clusters == 0) { set_error("%s: max_clusters must be at least 1 (ARP_NONE: no limit)", what); return ARP_ERR_BAD_INPUT; }
    return ARP_OK;
}
uint64_t cluster_cap() { return g_debug.cluster_cap_bytes > 0 ? (uint64_t)g_debug.cluster_cap_bytes : (1ull << 31); }
}  // namespace

extern "C" arp_status arp_contact_clusters(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp, double dist_cutoff,
                                           uint32_t flags, int32_t level, float min_similarity, uint32_t max_clusters, arp_table **out) try {
    FreqPrep prep;
    arp_status st = freq_prepare("contact clusters", ARP_CLUSTER_NO_COUNTS, level, ctx, s, n_frames, xyz, groups, vdw_comp, dist_cutoff, flags, out, &prep);
    if (st != ARP_OK || (st = cluster_args("contact clusters", min_similarity, max_clusters)) != ARP_OK || prep.checked_only) return st;
    FreqRowsHost rows;
    ClustersHost clusters;
    if ((st = device_clusters(ctx, prep.job, min_similarity, max_clusters, !(flags & ARP_CLUSTER_NO_COUNTS), prep.timeline_cap, cluster_cap(), &rows, &clusters)) != ARP_OK) return st;
    // the table is the frequency table of the level (the same rows through the same table builder); the clusters ride along
    std::unique_ptr<arp_table> t = freq_table(s, prep, rows);
    t->clustered = true;
    t->cluster_flags = flags & (uint32_t)ARP_CLUSTER_NO_COUNTS;
    t->clusters = std::move(clusters);
    *out = t.release();
    return ARP_OK;
} ARP_ABI_CATCH

namespace {
struct BitClusterOut { uint32_t *cluster; float *sim; uint32_t *n_neighbours, *sizes, *centre, *cluster_size, *n_clusters, *counts; };
arp_status bit_cluster_args(uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, float min_similarity, uint32_t max_clusters, const BitClusterOut &o) {
    if (flags & ~(uint32_t)ARP_SIM_ROWS) { set_error("bit cluster: unknown flag bits 0x%x", flags & ~(uint32_t)ARP_SIM_ROWS); return ARP_ERR_BAD_INPUT; }
    if (n_bits >= (1ull << 32) || rows >= (1ull << 32)) { set_error("bit cluster: 2^32 or more %s (the counts are u32)", n_bits >= (1ull << 32) ? "bits" : "rows"); return ARP_ERR_BAD_INPUT; }
    arp_status st = cluster_args("bit cluster", min_similarity, max_clusters);
    if (st != ARP_OK) return st;
    if ((flags & ARP_SIM_ROWS) && o.counts) { set_error("bit cluster: cluster_counts exist for the bit columns only, not with ARP_SIM_ROWS"); return ARP_ERR_BAD_INPUT; }
    const uint64_t M = (flags & ARP_SIM_ROWS) ? rows : n_bits;
    if (!o.n_clusters || (rows && n_bits && !words) || (M && (!o.cluster || !o.sim || !o.n_neighbours || !o.sizes || !o.centre || !o.cluster_size))) {
        set_error("null argument");
        return ARP_ERR_BAD_INPUT;
    }
    return ARP_OK;
}
}  // namespace

// The definition of the clusters on its own (no device): the yardstick of k_bit_adjacency / k_cluster_round / k_cluster_tail / k_cluster_counts.  Every bit is
// filed under its set as in arp_bit_gram_host, every pair of sets gets its f32 Tanimoto value and its neighbour flag, and the rounds recount the alive
// neighbours of every alive set from scratch.
extern "C" arp_status arp_bit_cluster_host(uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, float min_similarity, uint32_t max_clusters, uint32_t *cluster,
                                           float *similarity_to_centre, uint32_t *n_neighbours, uint32_t *sizes, uint32_t *centre, uint32_t *cluster_size, uint32_t *n_clusters,
                                           uint32_t *cluster_counts) try {
    const BitClusterOut o{cluster, similarity_to_centre, n_neighbours, sizes, centre, cluster_size, n_clusters, cluster_counts};
    arp_status st = bit_cluster_args(rows, n_bits, words, flags, min_similarity, max_clusters, o);
    if (st != ARP_OK) return st;
    const bool by_rows = (flags & ARP_SIM_ROWS) != 0;
    const uint64_t W = (n_bits + 31u) / 32u, M = by_rows ? rows : n_bits, N = by_rows ? n_bits : rows, K = (N + 31u) / 32u;
    *n_clusters = 0;
    if (!M) return ARP_OK;
    if (M > 46340u) { set_error("bit cluster: the host definition keeps one byte per pair, %llu sets are too many for it", (unsigned long long)M); return ARP_ERR_CAPACITY; }
    std::vector<uint32_t> sets(M * K, 0u);
    for (uint64_t r = 0; r < rows; r++)
        for (uint64_t f = 0; f < n_bits; f++)
            if (words[r * W + (f >> 5)] >> (f & 31u) & 1u) {
                const uint64_t a = by_rows ? r : f, e = by_rows ? f : r;
                sets[a * K + (e >> 5)] |= 1u << (e & 31u);
            }
    for (uint64_t a = 0; a < M; a++) {
        uint32_t c = 0;
        for (uint64_t w = 0; w < K; w++) c += (uint32_t)__builtin_popcount(sets[a * K + w]);
        sizes[a] = c;
    }
    auto tanimoto = [&](uint64_t a, uint64_t b) {
        uint32_t inter = 0;
        for (uint64_t w = 0; w < K; w++) inter += (uint32_t)__builtin_popcount(sets[a * K + w] & sets[b * K + w]);
        const uint64_t uni = (uint64_t)sizes[a] + sizes[b] - inter;
        return uni ? (float)((double)inter / (double)uni) : 1.0f;
    };
    std::vector<uint8_t> adj(M * M), alive(M, 1);
    for (uint64_t a = 0; a < M; a++) {
        uint32_t n = 0;
        for (uint64_t b = 0; b < M; b++) n += (adj[a * M + b] = tanimoto(a, b) >= min_similarity);
        n_neighbours[a] = n;
    }
    const uint32_t nan_bits = 0x7FC00000u;
    for (uint64_t a = 0; a < M; a++) { cluster[a] = ARP_NONE; memcpy(similarity_to_centre + a, &nan_bits, 4); }
    uint64_t n_alive = M;
    uint32_t k = 0;
    while (n_alive && k < max_clusters) {
        uint64_t c = 0;
        uint32_t best = 0;
        for (uint64_t a = 0; a < M; a++) {
            if (!alive[a]) continue;
            uint32_t n = 0;
            for (uint64_t b = 0; b < M; b++) n += alive[b] & adj[a * M + b];
            if (n > best) { best = n; c = a; }  // (ties: the smallest index stays)
        }
        if (best == 1u) {  // nobody has a neighbour left: the rounds from here on take the alive sets one by one, in index order
            for (uint64_t a = 0; a < M && k < max_clusters; a++)
                if (alive[a]) { alive[a] = 0; cluster[a] = k; similarity_to_centre[a] = 1.0f; centre[k] = (uint32_t)a; cluster_size[k] = 1u; k++; }
            break;
        }
        uint32_t size = 0;
        for (uint64_t b = 0; b < M; b++)
            if (alive[b] && adj[c * M + b]) { alive[b] = 0; cluster[b] = k; similarity_to_centre[b] = tanimoto(b, c); size++; }
        centre[k] = (uint32_t)c; cluster_size[k] = size;
        n_alive -= size;
        k++;
    }
    *n_clusters = k;
    if (cluster_counts) {
        std::fill(cluster_counts, cluster_counts + rows * k, 0u);
        for (uint64_t r = 0; r < rows; r++)
            for (uint64_t f = 0; f < n_bits; f++)
                if ((words[r * W + (f >> 5)] >> (f & 31u) & 1u) && cluster[f] != ARP_NONE) cluster_counts[r * k + cluster[f]]++;
    }
    return ARP_OK;
} ARP_ABI_CATCH

extern "C" arp_status arp_bit_cluster(arp_context *ctx, uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, float min_similarity, uint32_t max_clusters,
                                      uint32_t *cluster, float *similarity_to_centre, uint32_t *n_neighbours, uint32_t *sizes, uint32_t *centre, uint32_t *cluster_size,
                                      uint32_t *n_clusters, uint32_t *cluster_counts) try {
    if (!ctx) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    const BitClusterOut o{cluster, similarity_to_centre, n_neighbours, sizes, centre, cluster_size, n_clusters, cluster_counts};
    arp_status st = bit_cluster_args(rows, n_bits, words, flags, min_similarity, max_clusters, o);
    if (st != ARP_OK) return st;
    if (!rows || !n_bits)  // (no bit to look at: every set is empty)
        return arp_bit_cluster_host(rows, n_bits, words, flags, min_similarity, max_clusters, cluster, similarity_to_centre, n_neighbours, sizes, centre, cluster_size, n_clusters, cluster_counts);
    ClustersHost c;
    if ((st = device_bit_cluster(ctx, rows, n_bits, words, (flags & ARP_SIM_ROWS) != 0, min_similarity, max_clusters, cluster_counts != nullptr, cluster_cap(), &c)) != ARP_OK) return st;
    std::copy(c.cluster.begin(), c.cluster.end(), cluster);
    memcpy(similarity_to_centre, c.sim.data(), c.m * 4u);
    std::copy(c.n_neighbours.begin(), c.n_neighbours.end(), n_neighbours);
    std::copy(c.sizes.begin(), c.sizes.end(), sizes);
    std::copy(c.centre.begin(), c.centre.end(), centre);
    std::copy(c.cluster_size.begin(), c.cluster_size.end(), cluster_size);
    *n_clusters = (uint32_t)c.n_clusters;
    if (cluster_counts) memcpy(cluster_counts, c.counts, rows * c.n_clusters * 4u);
    return ARP_OK;
} ARP_ABI_CATCH

// ---- contact autocorrelation and survival curves across frames (device pipeline: autocorr.inl) ----------------------------------
extern "C" arp_status arp_contact_autocorrelation(arp_context *ctx, arp_structure *s, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp,
                                                  double dist_cutoff, uint32_t flags, int32_t level, uint32_t max_lag, arp_table **out) try {
    FreqPrep prep;
    arp_status st = freq_prepare("contact autocorrelation", ARP_ACF_CONTINUOUS | ARP_ACF_NO_MATRIX, level, ctx, s, n_frames, xyz, groups, vdw_comp, dist_cutoff, flags, out, &prep);
    if (st != ARP_OK) return st;
    const uint64_t F = prep.F;
    if (F > (1ull << 24)) { set_error("contact autocorrelation: F = %llu frames, at most 2^24 are supported (the half-lives are served as f32)", (unsigned long long)F); return ARP_ERR_BAD_INPUT; }
    if (max_lag != ARP_NONE && max_lag >= F) { set_error("contact autocorrelation: max_lag %u is not below the %llu frames", max_lag, (unsigned long long)F); return ARP_ERR_BAD_INPUT; }
    if (prep.checked_only) return ARP_OK;
    const uint64_t L = max_lag == ARP_NONE ? F - 1u : max_lag;
    FreqRowsHost rows;
    AutocorrHost acf;
    if ((st = device_autocorrelation(ctx, prep.job, (flags & ARP_ACF_CONTINUOUS) != 0, !(flags & ARP_ACF_NO_MATRIX), L, prep.timeline_cap, prep.autocorr_cap, &rows, &acf)) != ARP_OK)
        return st;
    // the table is the frequency table of the level (the same rows through the same table builder); half_life joins its columns, the counts ride along
    std::unique_ptr<arp_table> t = freq_table(s, prep, rows);
    t->autocorr = true;
    t->acf_flags = flags & (uint32_t)(ARP_ACF_CONTINUOUS | ARP_ACF_NO_MATRIX);
    t->acf = std::move(acf);
    autocorrelation_columns(t.get());
    *out = t.release();
    return ARP_OK;
} ARP_ABI_CATCH

namespace {
arp_status bit_autocorr_args(uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, uint32_t max_lag, const uint32_t *group, uint32_t n_groups, const uint64_t *sums,
                             const uint32_t *half_life, uint64_t *L) {
    if (flags & ~(uint32_t)ARP_ACF_CONTINUOUS) { set_error("bit autocorrelation: unknown flag bits 0x%x", flags & ~(uint32_t)ARP_ACF_CONTINUOUS); return ARP_ERR_BAD_INPUT; }
    if (n_bits >= (1ull << 32) || rows >= (1ull << 32)) { set_error("bit autocorrelation: 2^32 or more %s (the counts are u32)", n_bits >= (1ull << 32) ? "bits" : "rows"); return ARP_ERR_BAD_INPUT; }
    if (n_bits == 0) { set_error("bit autocorrelation: at least one bit per row is needed"); return ARP_ERR_BAD_INPUT; }
    if (max_lag != ARP_NONE && max_lag >= n_bits) { set_error("bit autocorrelation: max_lag %u is not below the %llu bits", max_lag, (unsigned long long)n_bits); return ARP_ERR_BAD_INPUT; }
    if ((rows && (!words || !half_life)) || (group && n_groups && !sums)) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    if (group)
        for (uint64_t r = 0; r < rows; r++)
            if (group[r] >= n_groups) { set_error("bit autocorrelation: group[%llu] = %u, there are %u groups", (unsigned long long)r, group[r], n_groups); return ARP_ERR_BAD_INPUT; }
    *L = max_lag == ARP_NONE ? n_bits - 1u : max_lag;
    return ARP_OK;
}
}  // namespace

// The definition on its own (no device): every bit is looked at one by one.  Intermittent: per lag, the frames f with bit f and bit f + lag.  Continuous:
// every maximal run of length n adds n - lag to each lag below n.  The half-life is the integer predicate of the header, lag by lag.
extern "C" arp_status arp_bit_autocorr_host(uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, uint32_t max_lag, const uint32_t *group, uint32_t n_groups,
                                            uint32_t *acf, uint64_t *sums, uint32_t *half_life) try {
    uint64_t L = 0;
    arp_status st = bit_autocorr_args(rows, n_bits, words, flags, max_lag, group, n_groups, sums, half_life, &L);
    if (st != ARP_OK) return st;
    const uint64_t W = (n_bits + 31u) / 32u, n_lags = L + 1u;
    if (group && sums) std::fill(sums, sums + (uint64_t)n_groups * n_lags, 0ull);
    std::vector<uint32_t> curve(n_lags);
    for (uint64_t r = 0; r < rows; r++) {
        auto bit = [&](uint64_t f) { return (words[r * W + (f >> 5)] >> (f & 31u) & 1u) != 0; };
        std::fill(curve.begin(), curve.end(), 0u);
        if (flags & ARP_ACF_CONTINUOUS) {
            uint64_t run = 0;
            for (uint64_t f = 0; f <= n_bits; f++) {
                if (f < n_bits && bit(f)) { run++; continue; }
                for (uint64_t lag = 0; lag < run && lag <= L; lag++) curve[lag] += (uint32_t)(run - lag);
                run = 0;
            }
        } else {
            for (uint64_t lag = 0; lag <= L; lag++)
                for (uint64_t f = 0; f + lag < n_bits; f++)
                    if (bit(f) && bit(f + lag)) curve[lag]++;
        }
        uint32_t half = ARP_NONE;
        for (uint64_t lag = 1; lag <= L && half == ARP_NONE; lag++)  // 2 acf F <= acf0 (F - lag): the left product halved instead, so that nothing overflows
            if ((uint64_t)curve[lag] * n_bits <= (((uint64_t)curve[0] * (n_bits - lag)) >> 1)) half = (uint32_t)lag;
        half_life[r] = half;
        if (acf) std::copy(curve.begin(), curve.end(), acf + r * n_lags);
        if (group && sums)
            for (uint64_t lag = 0; lag <= L; lag++) sums[(uint64_t)group[r] * n_lags + lag] += curve[lag];
    }
    return ARP_OK;
} ARP_ABI_CATCH

extern "C" arp_status arp_bit_autocorr(arp_context *ctx, uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, uint32_t max_lag, const uint32_t *group,
                                       uint32_t n_groups, uint32_t *acf, uint64_t *sums, uint32_t *half_life) try {
    if (!ctx) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    uint64_t L = 0;
    arp_status st = bit_autocorr_args(rows, n_bits, words, flags, max_lag, group, n_groups, sums, half_life, &L);
    if (st != ARP_OK) return st;
    if (!rows) return arp_bit_autocorr_host(rows, n_bits, words, flags, max_lag, group, n_groups, acf, sums, half_life);  // (no row: only the sums are zeroed)
    const uint64_t cap = g_debug.autocorr_cap_bytes > 0 ? (uint64_t)g_debug.autocorr_cap_bytes : (1ull << 31);
    return device_bit_autocorr(ctx, rows, n_bits, words, (flags & ARP_ACF_CONTINUOUS) != 0, L, group, n_groups, cap, acf, reinterpret_cast<unsigned long long *>(sums), half_life);
} ARP_ABI_CATCH
