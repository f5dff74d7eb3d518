// What the three host files of the table path share: the table object and its column registry (table.cpp), the per-structure entity cache
// (table_cache.cpp) and what the ensemble entry points (table_ens.cpp) take from both.  No HIP type appears here: table.cpp and table_ens.cpp
// compile without the HIP runtime's headers.
#pragma once
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

#include "host_common.h"
#include "table_dev.h"

// One entity of the output vocabulary (structs.rs:55-70): an atom, or a ring (atomn "Ring", atomi 0: complex.rs:334-342).
// Fixed NUL-padded names (the widths of the table's string columns).  48 bytes: a row touches two of these.
struct EntityRec {
    char chain[8], resn[8], atomn[8], insertion[4], altloc[4];
    int32_t resi, atomi, atom;   // atom: index into the structure's atoms, -1 for a ring
    uint32_t model;              // model serial as the table shows it (mod.rs:143)
};
static_assert(sizeof(EntityRec) == 48, "EntityRec layout");
struct EntityBook {              // every entity a table of this structure can mention; immutable, shared by the tables (which may outlive the structure)
    // (plain arrays, not vectors: 52 bytes per entity that every worker writes once -- a vector would zero them first, on one thread)
    std::unique_ptr<EntityRec[]> ent;  // atoms, then rings
    std::unique_ptr<uint32_t[]> lens;  // string lengths of an entity, 4 bits each: chain, resn, atomn, insertion, altloc
    size_t n = 0;
};

namespace arp {

// The per-entity columns of one side of a row; a table holds them twice, as `from` and `to`.  `fields`: which of them this kind of table has,
// in the order the sides are registered (and appear in an Arrow batch); the others stay empty.
enum SideField : uint32_t { kChain = 1, kResn = 2, kResi = 4, kInsertion = 8, kAltloc = 16, kAtomn = 32, kAtomi = 64, kAtom = 128, kRing = 256, kResidue = 512 };
constexpr uint32_t kContactSide = kChain | kResn | kResi | kInsertion | kAltloc | kAtomn | kAtomi | kAtom;
constexpr uint32_t kAtomFreqSide = kContactSide | kRing;
constexpr uint32_t kResidueFreqSide = kChain | kResn | kResi | kInsertion | kResidue;
constexpr uint32_t kWaterSide = kChain | kResi | kInsertion | kAltloc | kAtomi | kAtom;  // the mediating water of arp_water_bridges ("water_*")
struct SideCols {
    uint32_t fields = 0;
    StrCol<8> chain, resn, atomn;
    StrCol<4> insertion, altloc;
    std::vector<int32_t> resi, atomi, atom;
    std::vector<int32_t> ring;      // ring entity index of the topology, -1 for an atom (arp_contact_frequencies_ex)
    std::vector<int32_t> residue;   // residue ordinal of the topology (arp_residue_contact_frequencies)
    void resize(size_t n, uint32_t which);
    void put(size_t k, const EntityRec &e) {   // row k names entity e: every identity column this side has (ring / residue are the builder's)
        const uint32_t has = fields;           // (a local: the byte copies below could alias the member)
        if (has & kChain) memcpy(chain.at(k), e.chain, 8);
        if (has & kResn) memcpy(resn.at(k), e.resn, 8);
        if (has & kResi) resi[k] = e.resi;
        if (has & kInsertion) memcpy(insertion.at(k), e.insertion, 4);
        if (has & kAltloc) memcpy(altloc.at(k), e.altloc, 4);
        if (has & kAtomn) memcpy(atomn.at(k), e.atomn, 8);
        if (has & kAtomi) atomi[k] = e.atomi;
        if (has & kAtom) atom[k] = e.atom;
    }
};

// One column a table has: what arp_table_column serves under `name`, and how the Arrow batch shows it.  A table's registry lists its columns in
// batch order (the ones with in_batch false are served by arp_table_column alone); a name that is not in it is a column the table does not have.
struct TableColumn {
    enum Kind { kNumber, kString, kInteraction, kNullableF32 };
    const char *name;        // static storage
    int32_t width;           // bytes per element of `data`
    const char *format;      // Arrow format ("I", "i", "f", "u")
    Kind kind;               // kString: NUL-padded `width` bytes -> utf8; kInteraction: i32 codes -> the interactions' names; kNullableF32: `valid` says where
    bool in_batch;
    const void *data;        // n elements, owned by the table
    const uint8_t *valid;    // kNullableF32: one byte per row, 0 = null
};

struct PlaneEntry {
    int32_t model_serial; std::string chain; int32_t resi; std::string icode, altloc, resn;
    Plane plane;
    bool has_ord = false; uint32_t ord = 0;   // res2idx[(model, chain, resi, icode, altloc, resn)]
    uint32_t res = 0, alt_k = 0;              // the residue (and which of its conformer altlocs) the plane was last written from
    uint32_t chain_rank = 0; bool in_l = false, in_r = false;
};
// The identity of an atom (structs.rs:109-119) and of a ring entity (complex.rs:334-342: atomn "Ring", atomi 0, no atom index) as the tables show it.
EntityRec atom_entity(const arp_structure &s, size_t a);
EntityRec ring_entity(const PlaneEntry &r);

}  // namespace arp

struct arp_table {
    uint64_t n = 0;
    // device path: the table as it comes back -- rows of {from entity, to entity, distance, interaction} + side-chain statistics -- and the
    // entity book; the fixed-width columns below are materialised on first access (arp_table_column), the Arrow export reads rows + book
    std::shared_ptr<const EntityBook> book;
    std::shared_ptr<char> rows_owner;          // the pooled pinned block (or heap block) rows and sc live in
    const arp::TableRow *rows = nullptr;
    const arp::TableSc *sc = nullptr;
    std::once_flag columns_once;
    // the columns, each sized by the builder of the kind that has it and listed in `columns`
    std::vector<arp::TableColumn> columns;
    arp::SideCols from, to;
    std::vector<int32_t> interaction;
    std::vector<uint32_t> model;                                          // contact table
    std::vector<float> distance, sc_dist, sc_dihedral, sc_angle;
    std::vector<uint8_t> sc_valid;
    std::vector<uint32_t> n_frames;                                       // frequency tables
    std::vector<float> frequency, min_distance, max_distance;
    // contact-timeline table (arp_contact_timelines): a frequency table of either level with five more columns (tl.first / last / n_events / longest,
    // mean_run) and, unless ARP_TIMELINE_NO_BITMAP, the rows' frame bitmap (arp_table_timeline)
    arp::TimelineHost tl;
    uint64_t tl_frames = 0;
    std::vector<float> mean_run;
    // contact-similarity table (arp_contact_similarity): a frequency table of either level that owns the m x m matrix between frames or rows
    // (arp_table_similarity); the matrix is not a column
    bool similarity = false;
    uint32_t sim_flags = 0;
    arp::SimilarityHost sim;
    // contact-autocorrelation table (arp_contact_autocorrelation): a frequency table of either level with one more column, half_life (null: none), that
    // owns the rows x n_lags counts and the per-interaction sums (arp_table_autocorrelation); the counts are not columns
    bool autocorr = false;
    uint32_t acf_flags = 0;
    arp::AutocorrHost acf;
    std::vector<float> half_life;
    std::vector<uint8_t> half_life_valid;
    // water-bridge table (arp_water_bridges): one row per bridge (from atom, water, to atom) of a frame; `distance` is the longer leg
    arp::SideCols water;
    std::vector<uint32_t> frame;
    std::vector<float> from_distance, to_distance;
    // contact-cluster table (arp_contact_clusters): a frequency table of either level that owns the per-frame and per-cluster arrays and the rows x clusters
    // counts (arp_table_clusters); none of them is a column
    bool clustered = false;
    uint32_t cluster_flags = 0;
    arp::ClustersHost clusters;
};

namespace arp {

// The builders of the table kinds (table.cpp): each sizes the columns of its kind to t->n rows -- a column the caller has already moved in at that
// size keeps its values -- and lists them in t->columns.
void contact_columns(arp_table *t);                        // the 20 columns of arp_get_contacts + sc_valid, from_atom / to_atom
void frequency_columns(arp_table *t, uint32_t side);       // kAtomFreqSide or kResidueFreqSide
void water_bridge_columns(arp_table *t);                   // frame, the from / to / water identities, the two legs and the longer of them
void timeline_columns(arp_table *t);                       // behind frequency_columns: t->tl's statistics + mean_run
void autocorrelation_columns(arp_table *t);                // behind frequency_columns: half_life, from t->acf.half_life (ARP_NONE: null)

// ---- table_cache.cpp: which entities a structure has, kept with the structure ---------------------------------------------------------------
// (model serial, chain id, resi, icode, altloc, resn) with the names packed into integers (ids are <= 7 / 3 characters, the
// widths of the string columns): hashing and comparing keys costs no allocation.
struct PlaneKey {
    int32_t model, resi;
    uint32_t icode, altloc;
    uint64_t chain, resn;
    bool operator==(const PlaneKey &o) const {
        return model == o.model && resi == o.resi && icode == o.icode && altloc == o.altloc && chain == o.chain && resn == o.resn;
    }
};
struct PlaneKeyHash {
    size_t operator()(const PlaneKey &k) const {
        uint64_t h = k.chain * 0x9E3779B97F4A7C15ull ^ k.resn;
        h = (h ^ (h >> 29)) * 0xBF58476D1CE4E5B9ull + (((uint64_t)(uint32_t)k.model << 32) | (uint32_t)k.resi);
        h = (h ^ (h >> 31)) * 0x94D049BB133111EBull + (((uint64_t)k.icode << 32) | k.altloc);
        return (size_t)(h ^ (h >> 32));
    }
};
using PlaneIndex = std::unordered_map<PlaneKey, size_t, PlaneKeyHash>;

// `first_of_res` (single-model structures only, else left empty): entry of (residue r, its altloc k) = first_of_res[r] + k, -1 if r has
// no plane -- one model holds one residue per (chain, resi, icode), so no key can be written twice and no keyed lookup is needed.
// has_plane[r]: the residue has >= 3 plane atoms (residues.rs:273: the only way a fit fails).  fitted == nullptr: the planes
// themselves are fitted on the device (table_dev.hip); the entries then only say WHICH residue's plane an entity uses (e.res).
// n_res_use < the structure's residues: only model 0 (its residues are that prefix), regarded as a single-model structure -- the topology of
// arp_contact_frequencies_ex when the frames are the models of a file.
void build_planes(const arp_structure &s, bool rings, const std::vector<char> &has_plane, const std::vector<Plane> *fitted_in, std::vector<PlaneEntry> *out,
                  PlaneIndex *index, std::vector<int64_t> *first_of_res, size_t n_res_use = SIZE_MAX);

// Host: which entities exist and their names (group-independent parts are kept with the structure, so is the device-resident copy
// of its arrays).  Device (table_dev.hip): plane fits, ring rows, row expansion, the sort, the side-chain plane statistics.
struct TableCache {
    std::vector<uint8_t> plane_bits;
    std::vector<char> has_ring, has_sc;
    std::vector<uint32_t> res_atom_ptr, res_atom_idx, atom_sc_src, model_rank;
    std::vector<int32_t> model_serial_of;
    std::vector<EntKey> atom_keys;
    std::vector<PlaneEntry> rings, scp;       // entities (no planes: those are fitted on the device)
    PlaneIndex ring_idx, sc_idx;
    std::vector<int64_t> ring_first, sc_first;
    bool direct = true;
    std::vector<uint32_t> ring_sc_src;        // per ring entity: residue whose sc plane applies, or ARP_NONE
    std::vector<EntKey> ring_keys;
    std::vector<uint32_t> ring_model_rank;
    std::shared_ptr<EntityBook> book;
    std::thread book_job;                     // fills `book` while the first call's device work runs; joined before a table gets the book
    std::exception_ptr book_error;            // what the job threw, if anything: rethrown on the calling thread by wait_for_book
    void wait_for_book() {
        if (book_job.joinable()) book_job.join();
        if (book_error) { std::exception_ptr e = book_error; book_error = nullptr; std::rethrow_exception(e); }
    }
    void join_book() noexcept { if (book_job.joinable()) book_job.join(); }
    std::mutex mu;                            // held for the whole of a device-table call on this structure
    std::string rings_groups; bool have_rings_dev = false;   // the ring entities as the device wants them, for this chain-group spec
    std::vector<RingEnt> rings_dev;
    DevStructure dev;
    ~TableCache();                            // (joins the job, frees the device blocks)
};
// (Calls on ONE structure are serialised: its cache and its resident device copy are per-structure state.  Different structures run in parallel.)
TableCache *table_cache_of(arp_structure *s);

}  // namespace arp
