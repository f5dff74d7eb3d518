// The table object (arp_table): the columns of every table kind, the registry arp_table_column looks names up in, and the Arrow C Data
// Interface export (mod.rs:140-214: the DataFrame the reference returns).  Who fills a table: arp_get_contacts (table_cache.cpp) and the
// ensemble entry points (table_ens.cpp).  Nothing here touches the device.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>

#include "table.h"

using namespace arp;

// ---- columns and their registry -------------------------------------------------------------------------------------------------------------
namespace {
struct SideFieldInfo { uint32_t bit; const char *suffix; int32_t width; const char *format; bool in_batch; };
// in the order of a side's columns in TABLE_COLUMNS / FREQ_COLUMNS / RESIDUE_FREQ_COLUMNS (api.py); atom / ring / residue are indices for programs, not part of a batch
const SideFieldInfo kSideFields[] = {
    {kChain, "chain", 8, "u", true}, {kResn, "resn", 8, "u", true}, {kResi, "resi", 4, "i", true}, {kInsertion, "insertion", 4, "u", true}, {kAltloc, "altloc", 4, "u", true},
    {kAtomn, "atomn", 8, "u", true}, {kAtomi, "atomi", 4, "i", true}, {kAtom, "atom", 4, "i", false}, {kRing, "ring", 4, "i", false}, {kResidue, "residue", 4, "i", false}};
constexpr size_t kNSideFields = sizeof kSideFields / sizeof kSideFields[0];
const void *side_data(const SideCols &c, uint32_t bit) {
    switch (bit) {
        case kChain: return c.chain.buf.data();
        case kResn: return c.resn.buf.data();
        case kResi: return c.resi.data();
        case kInsertion: return c.insertion.buf.data();
        case kAltloc: return c.altloc.buf.data();
        case kAtomn: return c.atomn.buf.data();
        case kAtomi: return c.atomi.data();
        case kAtom: return c.atom.data();
        case kRing: return c.ring.data();
        default: return c.residue.data();
    }
}
const char *side_name(int side, size_t field) {  // "from_chain" ... "water_residue": built once, never freed (an exported schema may point at them for ever)
    static const std::vector<std::string> *names = [] {
        auto *v = new std::vector<std::string>();
        for (const char *prefix : {"from_", "to_", "water_"})
            for (const SideFieldInfo &f : kSideFields) v->push_back(std::string(prefix) + f.suffix);
        return v;
    }();
    return (*names)[(size_t)side * kNSideFields + field].c_str();
}
void add_number(arp_table *t, const char *name, const char *format, const void *data, bool in_batch = true) {
    t->columns.push_back(TableColumn{name, 4, format, TableColumn::kNumber, in_batch, data, nullptr});
}
void add_side(arp_table *t, int side, const SideCols &c) {  // side: 0 from, 1 to, 2 water
    for (size_t f = 0; f < kNSideFields; f++) {
        const SideFieldInfo &info = kSideFields[f];
        if (!(c.fields & info.bit)) continue;
        t->columns.push_back(TableColumn{side_name(side, f), info.width, info.format, info.format[0] == 'u' ? TableColumn::kString : TableColumn::kNumber, info.in_batch,
                                         side_data(c, info.bit), nullptr});
    }
}
void add_sides(arp_table *t) { add_side(t, 0, t->from); add_side(t, 1, t->to); }
}  // namespace

void arp::SideCols::resize(size_t n, uint32_t which) {
    fields = which;
    if (which & kChain) chain.resize(n);
    if (which & kResn) resn.resize(n);
    if (which & kResi) resi.resize(n);
    if (which & kInsertion) insertion.resize(n);
    if (which & kAltloc) altloc.resize(n);
    if (which & kAtomn) atomn.resize(n);
    if (which & kAtomi) atomi.resize(n);
    if (which & kAtom) atom.resize(n);
    if (which & kRing) ring.assign(n, -1);
    if (which & kResidue) residue.resize(n);
}

void arp::contact_columns(arp_table *t) {
    const size_t n = t->n;
    t->model.resize(n); t->interaction.resize(n); t->distance.resize(n);
    t->from.resize(n, kContactSide); t->to.resize(n, kContactSide);
    t->sc_dist.resize(n); t->sc_dihedral.resize(n); t->sc_angle.resize(n); t->sc_valid.resize(n);
    add_number(t, "model", "I", t->model.data());
    t->columns.push_back(TableColumn{"interaction", 4, "u", TableColumn::kInteraction, true, t->interaction.data(), nullptr});
    add_number(t, "distance", "f", t->distance.data());
    add_sides(t);
    const std::pair<const char *, const std::vector<float> *> sc[] = {{"sc_centroid_dist", &t->sc_dist}, {"sc_dihedral", &t->sc_dihedral}, {"sc_centroid_angle", &t->sc_angle}};
    for (const auto &c : sc)  // null where either residue has no side-chain plane (mod.rs:100-110 left join)
        t->columns.push_back(TableColumn{c.first, 4, "f", TableColumn::kNullableF32, true, c.second->data(), t->sc_valid.data()});
    t->columns.push_back(TableColumn{"sc_valid", 1, "C", TableColumn::kNumber, false, t->sc_valid.data(), nullptr});
}

void arp::frequency_columns(arp_table *t, uint32_t side) {
    const size_t n = t->n;
    t->interaction.resize(n);
    t->from.resize(n, side); t->to.resize(n, side);
    t->n_frames.resize(n); t->frequency.resize(n); t->min_distance.resize(n); t->max_distance.resize(n);
    t->columns.push_back(TableColumn{"interaction", 4, "u", TableColumn::kInteraction, true, t->interaction.data(), nullptr});
    add_sides(t);
    add_number(t, "n_frames", "I", t->n_frames.data());
    add_number(t, "frequency", "f", t->frequency.data());
    add_number(t, "min_distance", "f", t->min_distance.data());
    add_number(t, "max_distance", "f", t->max_distance.data());
}

void arp::water_bridge_columns(arp_table *t) {
    const size_t n = t->n;
    t->frame.resize(n); t->from_distance.resize(n); t->to_distance.resize(n); t->distance.resize(n);
    t->from.resize(n, kContactSide); t->to.resize(n, kContactSide); t->water.resize(n, kWaterSide);
    add_number(t, "frame", "I", t->frame.data());
    add_sides(t);
    add_side(t, 2, t->water);
    add_number(t, "from_distance", "f", t->from_distance.data());
    add_number(t, "to_distance", "f", t->to_distance.data());
    add_number(t, "distance", "f", t->distance.data());
}

void arp::timeline_columns(arp_table *t) {
    const size_t n = t->n;
    t->tl.first.resize(n); t->tl.last.resize(n); t->tl.n_events.resize(n); t->tl.longest.resize(n); t->mean_run.resize(n);
    add_number(t, "first_frame", "I", t->tl.first.data());
    add_number(t, "last_frame", "I", t->tl.last.data());
    add_number(t, "n_events", "I", t->tl.n_events.data());
    add_number(t, "longest_run", "I", t->tl.longest.data());
    add_number(t, "mean_run", "f", t->mean_run.data());
}

void arp::autocorrelation_columns(arp_table *t) {
    const size_t n = t->n;
    t->acf.half_life.resize(n, ARP_NONE);
    t->half_life.resize(n); t->half_life_valid.resize(n);
    for (size_t k = 0; k < n; k++) {  // (a lag is below 2^24: exact as f32)
        const uint32_t h = t->acf.half_life[k];
        t->half_life_valid[k] = h != ARP_NONE ? 1 : 0;
        t->half_life[k] = h != ARP_NONE ? (float)h : 0.f;
    }
    t->columns.push_back(TableColumn{"half_life", 4, "f", TableColumn::kNullableF32, true, t->half_life.data(), t->half_life_valid.data()});
    t->columns.push_back(TableColumn{"half_life_valid", 1, "C", TableColumn::kNumber, false, t->half_life_valid.data(), nullptr});
}

namespace {
// the fixed-width columns of a device-path table, all at once, on first access
void materialize_columns(arp_table *t) {
    const EntityBook &bk = *t->book;
    contact_columns(t);
    parallel_for(t->n, 1u << 14, [&](size_t k0, size_t k1, size_t) {
        for (size_t k = k0; k < k1; k++) {
            const TableRow &r = t->rows[k];
            const TableSc &c = t->sc[k];
            const EntityRec &f = bk.ent[r.from_ent];
            t->model[k] = f.model; t->interaction[k] = r.interaction; t->distance[k] = r.distance;
            t->from.put(k, f); t->to.put(k, bk.ent[r.to_ent]);
            t->sc_valid[k] = c.valid != 0.f ? 1 : 0; t->sc_dist[k] = c.dist; t->sc_dihedral[k] = c.dihedral; t->sc_angle[k] = c.angle;
        }
    });
}
}  // namespace

extern "C" void arp_table_free(arp_table *t) { delete t; }
extern "C" uint64_t arp_table_rows(const arp_table *t) { return t ? t->n : 0; }
extern "C" const void *arp_table_column(const arp_table *t_const, const char *name, int32_t *width) {
    if (!t_const || !name) return nullptr;
    arp_table *t = const_cast<arp_table *>(t_const);
    if (t->book) std::call_once(t->columns_once, [t]() { materialize_columns(t); });
    for (const TableColumn &c : t->columns)
        if (strcmp(c.name, name) == 0) { if (width) *width = c.width; return c.data; }
    return nullptr;
}

extern "C" const uint32_t *arp_table_timeline(const arp_table *t, uint64_t *words_per_row, uint64_t *n_frames) {
    if (!t || !t->tl.has_bitmap || t->tl.words_per_row == 0) return nullptr;
    if (words_per_row) *words_per_row = t->tl.words_per_row;
    if (n_frames) *n_frames = t->tl_frames;
    static const uint32_t no_rows = 0;
    return t->tl.words.empty() ? &no_rows : t->tl.words.data();  // (a table without rows still has a bitmap: never NULL)
}

extern "C" const void *arp_table_similarity(const arp_table *t, uint64_t *m, uint32_t *flags, const uint32_t **sizes) {
    if (!t || !t->similarity) return nullptr;
    if (m) *m = t->sim.m;
    if (flags) *flags = t->sim_flags;
    static const uint32_t nothing = 0;
    if (sizes) *sizes = t->sim.sizes.empty() ? &nothing : t->sim.sizes.data();
    return t->sim.matrix ? (const void *)t->sim.matrix : (const void *)&nothing;  // (an empty matrix is still a matrix: never NULL)
}

extern "C" const uint32_t *arp_table_autocorrelation(const arp_table *t, uint64_t *n_lags, uint32_t *flags, const uint64_t **sums, uint32_t *n_groups) {
    if (!t || !t->autocorr) return nullptr;
    if (n_lags) *n_lags = t->acf.n_lags;
    if (flags) *flags = t->acf_flags;
    static const uint64_t nothing = 0;
    if (sums) *sums = t->acf.sums.empty() ? &nothing : reinterpret_cast<const uint64_t *>(t->acf.sums.data());
    if (n_groups) *n_groups = t->acf.n_groups;
    if (!t->acf.has_matrix) return nullptr;
    return t->acf.matrix ? t->acf.matrix : reinterpret_cast<const uint32_t *>(&nothing);  // (a matrix without rows is still a matrix)
}

extern "C" const uint32_t *arp_table_clusters(const arp_table *t, uint64_t *n_frames, uint32_t *n_clusters, uint32_t *flags, const float **similarity_to_centre,
                                              const uint32_t **n_neighbours, const uint32_t **sizes, const uint32_t **centre, const uint32_t **cluster_size,
                                              const uint32_t **cluster_counts) {
    if (!t || !t->clustered) return nullptr;
    const ClustersHost &c = t->clusters;
    static const uint32_t nothing = 0;
    auto data = [](const std::vector<uint32_t> &v) { return v.empty() ? &nothing : v.data(); };  // (an empty array is still an array: never NULL)
    if (n_frames) *n_frames = c.m;
    if (n_clusters) *n_clusters = (uint32_t)c.n_clusters;
    if (flags) *flags = t->cluster_flags;
    if (similarity_to_centre) *similarity_to_centre = reinterpret_cast<const float *>(data(c.sim));
    if (n_neighbours) *n_neighbours = data(c.n_neighbours);
    if (sizes) *sizes = data(c.sizes);
    if (centre) *centre = data(c.centre);
    if (cluster_size) *cluster_size = data(c.cluster_size);
    if (cluster_counts) *cluster_counts = !c.has_counts ? nullptr : c.counts ? c.counts : &nothing;
    return data(c.cluster);
}

// ---- Arrow C Data Interface export ----------------------------------------------------------------------------------------------------------
namespace {
constexpr uint64_t kMaxUtf8 = 0x7FFFFFF0ull;  // (rows, or bytes of one string column: the offsets are 32-bit)
arp_status too_large() { set_error("table too large for 32-bit utf8 offsets"); return ARP_ERR_BAD_INPUT; }

// One child of the batch: its field and the buffers it owns -- validity (nullable columns), values or utf8 offsets, utf8 bytes.
struct ArrowColumn {
    const char *name, *format;   // static storage
    bool nullable = false;
    int64_t null_count = 0;
    void *buf[3] = {nullptr, nullptr, nullptr};
    ArrowColumn(const char *name_, const char *format_, bool nullable_) : name(name_), format(format_), nullable(nullable_) {}
    ~ArrowColumn() { for (void *b : buf) free(b); }
    ArrowColumn(const ArrowColumn &) = delete;
    ArrowColumn &operator=(const ArrowColumn &) = delete;
    int64_t n_buffers() const { return format[0] == 'u' ? 3 : 2; }
    // `count` elements of `elem` bytes, never a null pointer, 8 spare bytes behind; a failed allocation is std::bad_alloc (ARP_ERR_OOM at the C ABI)
    template <class T> T *alloc(int which, size_t count, bool zeroed = false) {
        const size_t bytes = std::max<size_t>(count * sizeof(T), 8) + 8;
        free(buf[which]);
        buf[which] = zeroed ? calloc(bytes, 1) : malloc(bytes);
        if (!buf[which]) throw std::bad_alloc();
        return (T *)buf[which];
    }
};
using ArrowColumns = std::vector<std::unique_ptr<ArrowColumn>>;

struct ArrowBatch {  // private data of the struct array
    std::vector<ArrowArray> kids;
    std::vector<ArrowArray *> kid_ptrs;
    const void *bufs[1] = {nullptr};
};
struct ArrowFields {  // private data of the struct schema
    std::vector<ArrowSchema> kids;
    std::vector<ArrowSchema *> kid_ptrs;
};
void release_column(ArrowArray *a) {
    delete (ArrowColumn *)a->private_data;
    a->release = nullptr;
}
void release_batch(ArrowArray *a) {
    ArrowBatch *b = (ArrowBatch *)a->private_data;
    for (ArrowArray &k : b->kids)
        if (k.release) k.release(&k);
    delete b;
    a->release = nullptr;
}
void release_leaf_schema(ArrowSchema *s) { s->release = nullptr; }
void release_fields(ArrowSchema *s) {
    ArrowFields *f = (ArrowFields *)s->private_data;
    for (ArrowSchema &k : f->kids)
        if (k.release) k.release(&k);
    delete f;
    s->release = nullptr;
}

// The struct array of `n` rows over the columns, and its schema: the one place that fills an ArrowArray / ArrowSchema.  The columns pass to the
// array (each child releases its own); until the last line they are the list's, so an exception on the way frees them.
void arrow_struct(ArrowColumns &&cols, int64_t n, ArrowArray *out_array, ArrowSchema *out_schema) {
    std::unique_ptr<ArrowBatch> b(new ArrowBatch());
    std::unique_ptr<ArrowFields> f(new ArrowFields());
    const size_t nc = cols.size();
    b->kids.resize(nc); f->kids.resize(nc); b->kid_ptrs.resize(nc); f->kid_ptrs.resize(nc);
    for (size_t k = 0; k < nc; k++) {
        ArrowColumn &c = *cols[k];
        ArrowArray &a = b->kids[k];
        a = ArrowArray{};
        a.length = n; a.null_count = c.null_count; a.offset = 0;
        a.n_buffers = c.n_buffers(); a.n_children = 0;
        a.buffers = (const void **)c.buf; a.children = nullptr; a.dictionary = nullptr;
        a.release = release_column; a.private_data = &c;
        b->kid_ptrs[k] = &a;
        ArrowSchema &sch = f->kids[k];
        sch = ArrowSchema{};
        sch.format = c.format; sch.name = c.name; sch.metadata = nullptr;
        sch.flags = c.nullable ? 2 /* ARROW_FLAG_NULLABLE */ : 0;
        sch.n_children = 0; sch.children = nullptr; sch.dictionary = nullptr;
        sch.release = release_leaf_schema; sch.private_data = nullptr;
        f->kid_ptrs[k] = &sch;
    }
    *out_array = ArrowArray{};
    out_array->length = n; out_array->null_count = 0; out_array->offset = 0;
    out_array->n_buffers = 1; out_array->buffers = b->bufs;
    out_array->n_children = (int64_t)nc; out_array->children = b->kid_ptrs.data(); out_array->dictionary = nullptr;
    out_array->release = release_batch; out_array->private_data = b.get();
    *out_schema = ArrowSchema{};
    out_schema->format = "+s"; out_schema->name = ""; out_schema->metadata = nullptr; out_schema->flags = 0;
    out_schema->n_children = (int64_t)nc; out_schema->children = f->kid_ptrs.data(); out_schema->dictionary = nullptr;
    out_schema->release = release_fields; out_schema->private_data = f.get();
    b.release(); f.release();
    for (auto &c : cols) c.release();  // (nothing above this line throws once the vectors are sized)
}

// Arrow export of a device-path table: every buffer of the 20 columns straight from the rows and the entity book, in two
// passes over row chunks on the host workers (string bytes per chunk, then the chunk's offsets / bytes / numbers / validity bits).
// No intermediate fixed-width columns, no zero fill, no per-row allocation.
arp_status export_arrow_fast(const arp_table *t, ArrowArray *out_array, ArrowSchema *out_schema) {
    const size_t n = t->n;
    const EntityBook &bk = *t->book;
    constexpr size_t kChunkRows = 1u << 15;  // a multiple of 8: validity bytes are never shared between chunks
    const size_t n_chunks = (n + kChunkRows - 1) / kChunkRows;
    // string columns: 0-4 from_{chain, resn, insertion, altloc, atomn}, 5-9 to_..., 10 interaction
    constexpr int kStr = 11;
    static const int shift_of[5] = {0, 4, 12, 16, 8};  // EntityBook::lens nibbles in the order chain, resn, insertion, altloc, atomn
    uint32_t name_len[ARP_N_INTERACTIONS];
    for (int k = 0; k < ARP_N_INTERACTIONS; k++) name_len[k] = (uint32_t)strlen(arp_interaction_name(k));
    std::vector<uint64_t> bytes((n_chunks + 1) * kStr, 0);
    parallel_for(n_chunks, 1, [&](size_t c0, size_t c1, size_t) {
        for (size_t c = c0; c < c1; c++) {
            uint64_t acc[kStr] = {0};
            const size_t k1 = std::min(n, (c + 1) * kChunkRows);
            for (size_t k = c * kChunkRows; k < k1; k++) {
                const TableRow &r = t->rows[k];
                const uint32_t lf = bk.lens[r.from_ent], lt = bk.lens[r.to_ent];
                for (int q = 0; q < 5; q++) { acc[q] += (lf >> shift_of[q]) & 15u; acc[5 + q] += (lt >> shift_of[q]) & 15u; }
                acc[10] += name_len[r.interaction];
            }
            for (int q = 0; q < kStr; q++) bytes[(c + 1) * kStr + q] = acc[q];
        }
    });
    for (size_t c = 0; c < n_chunks; c++) for (int q = 0; q < kStr; q++) bytes[(c + 1) * kStr + q] += bytes[c * kStr + q];
    for (int q = 0; q < kStr; q++) if (bytes[n_chunks * kStr + q] > kMaxUtf8) return too_large();
    // numeric columns: model u32, distance f32, from_resi, from_atomi, to_resi, to_atomi i32, sc_* f32 with validity
    enum { MODEL, DIST, FRESI, FATOMI, TRESI, TATOMI, SCD, SCDIH, SCANG, N_NUM };
    struct Field { const char *name, *format; bool is_str; int slot; };
    static const Field fields[20] = {
        {"model", "I", false, MODEL}, {"interaction", "u", true, 10}, {"distance", "f", false, DIST},
        {"from_chain", "u", true, 0}, {"from_resn", "u", true, 1}, {"from_resi", "i", false, FRESI},
        {"from_insertion", "u", true, 2}, {"from_altloc", "u", true, 3}, {"from_atomn", "u", true, 4}, {"from_atomi", "i", false, FATOMI},
        {"to_chain", "u", true, 5}, {"to_resn", "u", true, 6}, {"to_resi", "i", false, TRESI},
        {"to_insertion", "u", true, 7}, {"to_altloc", "u", true, 8}, {"to_atomn", "u", true, 9}, {"to_atomi", "i", false, TATOMI},
        {"sc_centroid_dist", "f", false, SCD}, {"sc_dihedral", "f", false, SCDIH}, {"sc_centroid_angle", "f", false, SCANG}};
    ArrowColumns cols;
    int32_t *str_off[kStr]; char *str_bytes[kStr];
    void *num[N_NUM]; uint8_t *validity[N_NUM] = {nullptr};
    for (const Field &fd : fields) {
        cols.emplace_back(new ArrowColumn(fd.name, fd.format, !fd.is_str && fd.slot >= SCD));
        ArrowColumn &c = *cols.back();
        if (fd.is_str) { str_off[fd.slot] = c.alloc<int32_t>(1, n + 1); str_bytes[fd.slot] = c.alloc<char>(2, bytes[n_chunks * kStr + fd.slot]); }
        else {
            num[fd.slot] = c.alloc<uint32_t>(1, n);
            if (c.nullable) validity[fd.slot] = c.alloc<uint8_t>(0, (n + 7) / 8);
        }
    }
    std::vector<uint64_t> nulls(n_chunks, 0);
    parallel_for(n_chunks, 1, [&](size_t c0, size_t c1, size_t) {
        for (size_t c = c0; c < c1; c++) {
            uint64_t off[kStr];
            for (int q = 0; q < kStr; q++) off[q] = bytes[c * kStr + q];
            const size_t k1 = std::min(n, (c + 1) * kChunkRows);
            uint64_t chunk_nulls = 0;
            for (size_t k = c * kChunkRows; k < k1; k++) {
                const TableRow &r = t->rows[k];
                const TableSc &sc = t->sc[k];
                const EntityRec &f = bk.ent[r.from_ent], &o = bk.ent[r.to_ent];
                const uint32_t lf = bk.lens[r.from_ent], lt = bk.lens[r.to_ent];
                const char *fs[5] = {f.chain, f.resn, f.insertion, f.altloc, f.atomn}, *ts[5] = {o.chain, o.resn, o.insertion, o.altloc, o.atomn};
                for (int q = 0; q < 5; q++) {
                    const uint32_t a = (lf >> shift_of[q]) & 15u, b = (lt >> shift_of[q]) & 15u;
                    str_off[q][k] = (int32_t)off[q]; memcpy(str_bytes[q] + off[q], fs[q], a); off[q] += a;
                    str_off[5 + q][k] = (int32_t)off[5 + q]; memcpy(str_bytes[5 + q] + off[5 + q], ts[q], b); off[5 + q] += b;
                }
                str_off[10][k] = (int32_t)off[10];
                memcpy(str_bytes[10] + off[10], arp_interaction_name(r.interaction), name_len[r.interaction]); off[10] += name_len[r.interaction];
                ((uint32_t *)num[MODEL])[k] = f.model; ((float *)num[DIST])[k] = r.distance;
                ((int32_t *)num[FRESI])[k] = f.resi; ((int32_t *)num[FATOMI])[k] = f.atomi;
                ((int32_t *)num[TRESI])[k] = o.resi; ((int32_t *)num[TATOMI])[k] = o.atomi;
                ((float *)num[SCD])[k] = sc.dist; ((float *)num[SCDIH])[k] = sc.dihedral; ((float *)num[SCANG])[k] = sc.angle;
                chunk_nulls += sc.valid == 0.f;
            }
            for (size_t k = c * kChunkRows; k < k1; k += 8) {  // validity bits, one byte per eight rows (null where either residue has no sc plane)
                uint8_t v = 0;
                for (size_t b = 0; b < 8 && k + b < k1; b++) v |= (uint8_t)((t->sc[k + b].valid != 0.f ? 1u : 0u) << b);
                for (int q = SCD; q < N_NUM; q++) validity[q][k >> 3] = v;
            }
            nulls[c] = chunk_nulls;
        }
    });
    for (int q = 0; q < kStr; q++) str_off[q][n] = (int32_t)bytes[n_chunks * kStr + q];
    int64_t sc_nulls = 0;
    for (uint64_t v : nulls) sc_nulls += (int64_t)v;
    for (auto &c : cols) if (c->nullable) c->null_count = sc_nulls;
    arrow_struct(std::move(cols), (int64_t)n, out_array, out_schema);
    return ARP_OK;
}

// utf8 offsets + bytes of n strings: len(i) and text(i) say what string i is
template <class Len, class Text>
bool utf8_fill(ArrowColumn &c, size_t n, Len len, Text text) {
    int32_t *off = c.alloc<int32_t>(1, n + 1);
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) { off[i] = (int32_t)total; total += len(i); if (total > kMaxUtf8) return false; }
    off[n] = (int32_t)total;
    char *bytes = c.alloc<char>(2, total);
    for (size_t i = 0; i < n; i++) memcpy(bytes + off[i], text(i), (size_t)(off[i + 1] - off[i]));
    return true;
}

// Arrow export of a table that holds its columns (every kind but the device contact table): the registry's batch columns in its order
arp_status export_arrow_columns(const arp_table *t, ArrowArray *out_array, ArrowSchema *out_schema) {
    const size_t n = t->n;
    ArrowColumns cols;
    for (const TableColumn &tc : t->columns) {
        if (!tc.in_batch) continue;
        cols.emplace_back(new ArrowColumn(tc.name, tc.format, tc.kind == TableColumn::kNullableF32));
        ArrowColumn &c = *cols.back();
        bool fits = true;
        switch (tc.kind) {
            case TableColumn::kString: {
                const char *p = (const char *)tc.data;
                const size_t W = (size_t)tc.width;
                fits = utf8_fill(c, n, [&](size_t i) { return strnlen(p + i * W, W); }, [&](size_t i) { return p + i * W; });
                break;
            }
            case TableColumn::kInteraction: {  // interaction code -> the reference's Display string (structs.rs:6-51)
                const int32_t *code = (const int32_t *)tc.data;
                fits = utf8_fill(c, n, [&](size_t i) { return strlen(arp_interaction_name(code[i])); }, [&](size_t i) { return arp_interaction_name(code[i]); });
                break;
            }
            case TableColumn::kNullableF32: {
                uint8_t *bits = c.alloc<uint8_t>(0, (n + 7) / 8, true);
                for (size_t i = 0; i < n; i++) {
                    if (tc.valid[i]) bits[i >> 3] |= (uint8_t)(1u << (i & 7));
                    else c.null_count++;
                }
            }
                [[fallthrough]];  // the values
            case TableColumn::kNumber:
                if (n) memcpy(c.alloc<char>(1, n * (size_t)tc.width), tc.data, n * (size_t)tc.width);
                else c.alloc<char>(1, 0);
                break;
        }
        if (!fits) return too_large();
    }
    arrow_struct(std::move(cols), (int64_t)n, out_array, out_schema);
    return ARP_OK;
}
}  // namespace

extern "C" arp_status arp_table_export_arrow(const arp_table *t, ArrowArray *out_array, ArrowSchema *out_schema) try {
    if (!t || !out_array || !out_schema) { set_error("null argument"); return ARP_ERR_BAD_INPUT; }
    if (t->n > kMaxUtf8) return too_large();
    return t->book ? export_arrow_fast(t, out_array, out_schema) : export_arrow_columns(t, out_array, out_schema);
} ARP_ABI_CATCH
