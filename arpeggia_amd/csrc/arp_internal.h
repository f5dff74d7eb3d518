// Internal declarations shared by the HIP kernels (kernels.hip) and the host engine (engine.cpp, batch.cpp, sasa_dev.cpp; their own internals: engine.h).
#pragma once
#include <cstdint>
#include <vector>
#include <hip/hip_runtime.h>

#include "../../include/arpeggia_amd.h"
#include "debug_knobs.h"
#include "emit_plan.h"

namespace arp {

// SAP residue table (src/sap.rs:41-101): name, hydrophobicity (Black & Mould, shifted so that glycine is 0), largest side-chain SASA.
// One list for arp_sap_weight (sasa_dev.cpp) and the device weight kernel (sasa.inl): the code of a residue is its position here.
#define ARP_SAP_RESIDUES(X)                                                                                                          \
    X("ALA", 0.616f - 0.501f, 15.395f) X("ARG", 0.000f - 0.501f, 124.338f) X("ASN", 0.236f - 0.501f, 90.303f)                       \
    X("ASP", 0.028f - 0.501f, 87.601f) X("CYS", 0.680f - 0.501f, 46.456f) X("GLU", 0.043f - 0.501f, 95.534f)                        \
    X("GLN", 0.251f - 0.501f, 99.186f) X("GLY", 0.000f, 3.229f) X("HIS", 0.165f - 0.501f, 96.532f) X("ILE", 0.943f - 0.501f, 31.448f) \
    X("LEU", 0.943f - 0.501f, 30.271f) X("LYS", 0.283f - 0.501f, 61.962f) X("MET", 0.738f - 0.501f, 65.233f)                        \
    X("PHE", 1.000f - 0.501f, 67.945f) X("PRO", 0.711f - 0.501f, 17.812f) X("SER", 0.359f - 0.501f, 39.355f)                        \
    X("THR", 0.450f - 0.501f, 42.648f) X("TRP", 0.878f - 0.501f, 101.491f) X("TYR", 0.880f - 0.501f, 94.478f)                       \
    X("VAL", 0.825f - 0.501f, 26.702f)

// Decision constants in SQUARED-distance space.  The reference compares d = sqrt(s) (correctly rounded f64)
// against thresholds T with `<` (vdw.rs:33-41) or `<=` (everything else).  Because rn(sqrt(.)) is monotone,
// {s : sqrt(s) < T} = {s : s < lt(T)} with lt(T) = min{s : sqrt(s) >= T}; likewise d <= T  <=>  s < le(T).
// The host computes lt/le exactly (engine.cpp: bound_lt / bound_le), so the device never needs a sqrt to decide.
struct DevParams {
    double r2;            // squared search radius, inclusive candidate test d^2 <= r2 (rstar locate_within_distance): r2_call, or less with
                          // ARP_FLAG_CONTACTS_ONLY (no rule reaches further than the largest bound of the elements present) -- set by the grid sizing
    double s_ion;         // le(4.0)   ionic.rs:5, hbond.rs:7
    double s_polar;       // le(3.5)   hbond.rs:8
    double s_hphob;       // le(4.5)   hydrophobic.rs:5
    double s_clash[256];  // lt(cov[a]+cov[b] - c)   vdw.rs:33
    double s_cov[256];    // lt(cov[a]+cov[b] + c)   vdw.rs:34
    double s_vdw[256];    // lt(vdw[a]+vdw[b] + c)   vdw.rs:41
    double s_hacc[16];    // le(h_vdw + vdw[acceptor] + c)   hbond.rs:54,98
    double s_cov_max;     // the largest s_cov[] of the element pairs PRESENT: below it a candidate MAY be inside a covalent / clash band (k_emit's short level
                          // count) -- set by the grid sizing
    float r2f;            // prefilter threshold in f32 (r2 + margin), set by the grid sizing
    uint32_t flags;       // arp_params.flags (ARP_FLAG_CONTACTS_ONLY is read by the pair kernels)
    double r2_call;       // dist_cutoff^2 (complex.rs:191) as the caller gave it.  Everything but r2, r2f and s_cov_max is constant for a given
                          // arp_params: the device copy is uploaded when the parameters change, not per call
    uint32_t strip_force; // diagnostics (arp_debug_set "strip_rows"): rows per y strip of the cell order, a power of two; 0 = chosen by input size
    uint32_t pad_;
};

// Uniform grid, written by the device-side setup kernel (no host round trip).
struct GridParams {
    double ox, oy, oz;    // origin = min corner of the heavy atoms
    double inv_edge;      // 1 / cell edge in y and z, edge >= dist_cutoff * (1 + 1e-6)
    double inv_edge_x;    // kx / edge: cells are kx times finer along x (the fastest-running cell index), so that a lane's slot windows
                          // -- x-runs of 2 kx + 1 cells -- hug the search sphere: the same five windows, up to a third fewer tests
    uint32_t kx;          // x cells per cell edge (1, 2 or 4): a neighbour within the cutoff is at most kx cells away along x
    uint32_t nx, ny, nz;  // cells per axis for ONE model
    uint32_t nzt;         // total z layers = n_models * (nz + 1): each model gets its own slab + an empty separator
    uint32_t ncells;      // nx * ny * nzt (ny rounded up to whole strips when sy_shift != 0)
    uint32_t n_heavy;     // atoms in the grid (non-H)
    uint32_t n_tasks;     // ceil(n_heavy / 64): one wave-task per 64 consecutive slots
    uint32_t bad;         // bit 0: non-finite coordinate seen, bit 1: model ids too sparse for the workspace
    float prefilter_margin;
    uint32_t all_both;    // every heavy atom is in the ligand AND the receptor set (groups "/"): orient() takes its short form
    double mx, my, mz;    // box midpoint: the f32 prefilter records are relative to it (halves their magnitude)
    double r2m;           // prefilter threshold on d^2 in f64: r2 + storage margin + dot-form margin
    const double *model_org;  // packed batches: per model {origin xyz, midpoint xyz} -- every member sits in a grid slab of its own
                              // position, however far apart the members are in space; nullptr = one origin for all models
    uint32_t rk_bad;      // k_place met a residue ordinal or chain rank that does not fit the 32-bit residue word (Sorted::rkey): the residue-rule
                          // kernels (k_emit<.., RES>) then reject nothing early -- the exact phase decides on the real keys, as always
    uint32_t sy_shift;    // cell rows run (layer, y) when 0; else in y strips of 2^sy_shift rows: (strip, layer, y inside the strip) -- grid_row
    uint32_t key_unsorted;  // k_place<.., NARROW> met an atom whose key (model, chain rank, residue ordinal) is smaller than its predecessor's in the
                            // input order: the narrow-record kernels then order the two atoms of every pair on the real keys (Xrec, below)
};

// Row of cells (y, layer) -> its place in the cell order; a row's nx cells are consecutive.  Layer-major order keeps a row's neighbours in the
// next layer a whole layer of atoms away: the emit kernel's gathers find them in the XCD's 4 MB L2 only while two layers of records fit there
// (up to ~2 x 10^6 atoms of a compact structure).  Beyond that the rows are ordered in y strips (grid_setup picks the height), and the distance
// is a strip's share of a layer.  ny: the real row count (sy_shift == 0); strips pad it to a multiple of their height with empty rows.
__host__ __device__ inline uint32_t grid_row(uint32_t y, uint32_t layer, uint32_t ny, uint32_t nzt, uint32_t s) {
    return s ? ((((y >> s) * nzt + layer) << s) | (y & ((1u << s) - 1u))) : layer * ny + y;
}
__host__ __device__ inline void grid_row_decode(uint32_t r, uint32_t ny, uint32_t nzt, uint32_t s, uint32_t &y, uint32_t &layer) {
    if (s) { const uint32_t q = r >> s; layer = q % nzt; y = ((q / nzt) << s) | (r & ((1u << s) - 1u)); }
    else { y = r % ny; layer = r / ny; }
}

// Device view of the caller's SoA (all device pointers).
struct DevAtoms {
    uint32_t n;
    const double *x, *y, *z;
    const uint32_t *attr, *res_ord;
    const uint32_t *chain_rank, *model;
    const uint32_t *res_id, *res_h_ptr, *res_h_idx, *res_cb, *res_sg;
    uint32_t n_res;
    uint32_t per_model;   // packed batch: size the grid by the largest member and give every model its own origin
};

// Exact-phase record of one heavy atom, 48 B = three 16-byte parts.  The hot kernels read parts 0 and 1 whole and the first
// half of part 2; `attr` (the caller's word + the residue-has-hydrogens bit) is only read by the deferred probe passes.
//   pw = pair word, built when the atom is placed (grid.inl make_pair_word): element class in bits 0-3 and again in bits 4-7, the class bits the
//   pair rules combine as two bytes P (bits 8-14) and Q (bits 16-22) such that (Pa & Qb) | (Pb & Qa) has one bit per pair
//   predicate, LIGAND / RECEPTOR in bits 24 / 25, residue-has-hydrogens in bit 30.
//   {res_ord, crm} sit side by side: read as one 64-bit word they are the key (model, chain rank, residue ordinal) that orders the two atoms
//   of a pair when every atom is in both chain sets (orient_all_both).
struct __attribute__((aligned(16))) Fat {
    double x, y;
    double z; uint32_t pw, orig /* index into the caller's arrays */;
    uint32_t res_ord, crm /* chain rank (all 32 bits; the model is not in the key: every model owns its own slab of the grid + an empty
                             separator layer, so the windows of an atom only ever hold atoms of its own model, complex.rs:96-98) */, cell /* cell id of the slot */, attr;
};
// The narrow exact record, 32 B = two 16-byte parts: what k_emit's 12-wave kernels gather per survivor and k_place<.., NARROW> scatters per atom
// when the emit plan chose it (emit_plan.h plan_emit); it lives in the memory of Sorted::fat.  `ot` = original index in the HIGH `ib` bits
// (the call's index width, a kernel argument: two records compare like their indices) and below them the low T = 32 - ib bits of the atom's TAG
// (chain rank << kRkOrdBits) + residue ordinal, computed modulo 2^32.  The cell, the attribute word and the chain key of the wide record are not here: a task recomputes its home
// cells from the coordinates (cell_coords, grid.inl), and whoever needs the real chain rank / ordinal / attribute word reads the caller's
// arrays by the original index (the batch's rare branch in exact_finish_e, fat_from_narrow in the probe passes).
struct __attribute__((aligned(16))) Xrec {
    double x, y;
    double z; uint32_t pw, ot;
};
constexpr uint32_t kPwLigand = 1u << 24, kPwReceptor = 1u << 25, kPwResHasH = 1u << 30;  // (bits 26-29 and 31 stay clear: the emit kernel ANDs the word with a table entry's probe bits)

// Cell-sorted copy of the heavy atoms (slot order: x-major cells, atoms of a cell in ascending input index).
struct Sorted {
    float4 *rec;          // {x-mx, y-my, z-mz as f32, |.|^2 of those three}  -- prefilter operand, 16 B
    Fat *fat;
    uint32_t *rkey;       // residue word chain rank << 20 | residue ordinal (kRkOrdBits): two atoms whose words differ by at most 1 are of one residue
                          // or of sequence neighbours in one chain and never pair (complex.rs:108-113) -- k_emit<.., RES> drops such prefilter
                          // survivors before the gathers.  Written by k_place<true> only, valid while GridParams::rk_bad == 0
};
// the residue word: 20 bits of residue ordinal (at most 2^20 - 3, so that the words of two chains are at least 3 apart) + 11 bits of chain rank
// (bit 31 stays clear: the home side disables the rule with a word no neighbour word comes within 2^30 of)
constexpr uint32_t kRkOrdBits = 20, kRkOrdMax = (1u << kRkOrdBits) - 3u, kRkChainMax = (1u << 11) - 1u, kRkOff = 0xC0000000u;

// Same-address (and same-line) device atomics serialise in one L2 channel at ~90 ns each: the task counters of the eight XCD
// groups sit in separate 128-byte lines (measured: sharing one line cost the emit kernel 155 us of hand-out time).
constexpr uint32_t kTaskCtrStride = 32;                       // words
constexpr uint32_t kTaskCtrWords = 4 * 8 * kTaskCtrStride;    // [mode][group]

// The device/host result contract.  Words of Workspace::result that a pair pass publishes (the host reads the first kResultWords of them into
// arp_context::h_result after every pass; the kernels write them, engine.cpp pass_collect reads them): total pairs; status bits (kStat*); emit
// allocator head (64-record units; records in the hole-free sequence); chunks of the deferred-probe list; how many of the first 255 atoms
// carry their predecessor's residue word (k_place: the launcher's hint for the next call).  kSasaTestsWord: the SASA kernel's f32 distance tests.
enum : uint32_t { kResPairs = 0, kResFlags = 1, kResEmitHead = 2, kResDeferred = 3, kResResRuns = 4, kResRare = 5, kResultWords = 6, kSasaTestsWord = 8 };
// kResRare: batches of the narrow-record emit kernels that fetched the real chain keys (exact_finish_e's rare branch) -- arp_pair_rare_batches
// Status bits: the list did not fit the capacity / CYS SG..SG covalent pair whose residue has no CB / non-finite coordinate / the deferred-probe
// list overflowed / k_fixup's hole plan is inconsistent / model ids too sparse for the workspace / the probe pass was skipped on a stale memo
constexpr unsigned long long kStatCapacity = 1, kStatCysNoCb = 2, kStatNonFinite = 4, kStatDeferOverflow = 8, kStatHolePlan = 16,
                             kStatSparseModels = 64, kStatStaleSkip = 128;
// the pinned host block of a context (arp_context::h_result): the kResultWords of the last pair pass, then slots of other calls
constexpr uint32_t kHostSasaTestsSlot = 6, kHostResultWords = 8;

struct Workspace {
    double *partials;        // k_bounds: [256][8] per-block partial results
    uint32_t *tickets;        // self-resetting arrival counters: [0] bounds, [1] cell scan, [2] pair scan
    GridParams *grid;
    DevParams *params;
    uint32_t *cell_of_atom;   // n
    uint32_t *rank_of_atom;   // n: arrival rank inside the cell (returning atomic)
    uint32_t *cell_count;     // ncells_cap + 1
    uint32_t *cell_start;     // ncells_cap + 1
    uint32_t *perm;           // n: slot -> atom (arrival order inside a cell)
    uint32_t *slot_cell;      // n
    Sorted sorted;
    uint32_t *task_count;     // n/64 + 2: candidate pairs per wave-task
    unsigned long long *task_base;  // n/64 + 2
    uint32_t *scan_tmp;       // block sums (1024 + 1)
    unsigned long long *scan_tmp64;
    unsigned long long *result;  // the words kRes* above (+ kSasaTestsWord; from word 32 on the chunk totals of k_scan_single)
    ulonglong2 *hole_list;    // emit mode: one (start, length) per block
    arp_pair *scratch;        // emit mode: home of positions >= the caller's capacity until k_fixup has closed the holes
    unsigned long long scratch_cap;
    uint32_t *task_ctr;       // [4 modes][8 block groups] x kTaskCtrStride words: next wave-task of the group, one counter per 128-B line
    uint2 *defer_list;        // emit mode: candidates whose classification needs a hydrogen / disulfide probe
    unsigned long long defer_cap;
    uint32_t ncells_cap;
    uint32_t n_cap;
    uint32_t *model_box;      // per-model bounding boxes of a packed batch: 65536 x {min xyz, max xyz} as order-preserving f32 codes
    double *model_org;        // 65536 x {origin xyz, midpoint xyz}
};

// Device view of one pack (batch.inl): the members' arrays back to back + the descriptor table {first atom, first residue, first
// hydrogen-list entry, model offset} x (K + 1) and the per-member scratch of the renumbering and of the pair-list split.
struct PackDesc {             // entry m of K + 1 (the last one is the sentinel holding the totals)
    uint32_t first_atom, first_res, first_h, model_off;
};
struct PackArrays {
    uint32_t n, n_res, n_h, K;
    PackDesc *desc;
    uint32_t *model;
    uint32_t *res_id, *res_h_ptr, *res_cb, *res_sg, *res_h_idx;
    uint32_t *n_models, *status;             // K, 1
    unsigned long long *count, *offset, *cursor;  // K, K + 1, K
};

struct Profiler {
    static constexpr int kMax = 32;
    bool enabled = false;
    int n = 0;
    const char *names[kMax];
    hipEvent_t ev0[kMax], ev1[kMax];
    bool created = false;
    void begin(const char *name, hipStream_t st);
    void end(hipStream_t st);
};

// Launch wrappers (kernels.hip / pairs.inl).  All asynchronous on `st`.
// want_rkey, narrow_ib: EmitPlan::res and EmitPlan::narrow_ib of the pass the cell list is built for (k_place writes the residue words / the narrow exact
// record, Xrec, with that many index bits instead of the wide one, Fat)
void launch_grid(const DevAtoms &in, const Workspace &ws, hipStream_t st, Profiler *prof, double cutoff, bool ordered, bool want_rkey = false, uint32_t narrow_ib = 0);
void launch_count(const DevAtoms &in, const Workspace &ws, hipStream_t st, Profiler *prof, unsigned long long capacity, bool have_out, bool contacts_only);
void launch_fill_ordered(const DevAtoms &in, const Workspace &ws, arp_pair *out, unsigned long long capacity, hipStream_t st, Profiler *prof,
                         bool contacts_only);
// the launch sequence of the plan, on a cell list built for it; ARP_ERR_HIP: the plan names a k_emit variant there is none of (an internal error)
arp_status launch_emit(const DevAtoms &in, const Workspace &ws, arp_pair *out, unsigned long long capacity, hipStream_t st, Profiler *prof, const EmitPlan &plan);
unsigned long long emit_scratch_records();
void launch_neighbor_sum(const DevAtoms &in, const Workspace &ws, double radius, double r2, const float *weight, float *out, hipStream_t st, Profiler *prof);
// Atom SASA (sasa.inl): the grid over the atoms without ARP_ATTR_H, then one wave per grid atom.  buried == nullptr: k_sasa; sasa / count hold
// in.n entries.  buried != nullptr: k_sasa_split; the group mask of an atom is ARP_ATTR_LIGAND (group 1) |
// ARP_ATTR_RECEPTOR (group 2) of its attribute word, sasa / count are three planes of in.n entries (complex, group 1, group 2), buried in.n
// entries.  All indexed like the input arrays (atoms outside the grid are not written).  The kernel adds its number of f32 distance tests to
// Workspace::result[kSasaTestsWord].
void launch_sasa(const DevAtoms &in, const Workspace &ws, double cutoff, const float *R, const float *sphere, uint32_t n_points, float r_max,
                 float *sasa, int32_t *count, int32_t *buried, hipStream_t st, Profiler *prof);
// w[j] = arp_sap_weight(ARP_SAP_RESIDUES name code[j], sasa[src[j]]), 0 where src[j] < 0 or code[j] >= 20
void launch_sap_weight(uint32_t n, const uint32_t *code, const int32_t *src, const float *sasa, float *w, hipStream_t st);
void launch_pack_fix(const PackArrays &pa, hipStream_t st);
// SASA / SAP statistics over the frames of an ensemble (ens.inl).  All device pointers.
struct EnsTopo {          // the topology, uploaded once per call: m selected atoms of the n_top atoms a frame's coordinates cover
    uint32_t n_top, m;
    const uint32_t *sel;    // m: topology index of selected atom k
    const float *R;         // m: radius + probe
    const uint32_t *code;   // m: position in ARP_SAP_RESIDUES (>= 20: none); SAP only
    const uint32_t *pattr;  // m: attribute word of the SAP grid (side chain: in the grid; else ARP_ATTR_H: kept out); SAP only
};
struct EnsPack {          // the packed arrays of one pass, frames x m entries each; px == nullptr: no SAP
    double *x, *y, *z, *px, *py, *pz;
    uint32_t *model, *pattr, *code;
    int32_t *src;
    float *R;
};
struct EnsAcc {           // per selected atom, over all frames so far
    unsigned long long *s1, *s2;  // sum of count, sum of count^2
    int32_t *cmin, *cmax;
    double *t1, *t2;              // SAP: sum and sum of squares of the per-frame f32 values, added in frame order
    float *pmin, *pmax;
};
// item f * m + k of the packed arrays = selected atom k of frame f of the pass; xyz: frames x n_top x 3 as uploaded
void launch_ens_tile(uint32_t frames, const double *xyz, const EnsTopo &t, const EnsPack &p, hipStream_t st);
// folds the pass's count / sap ([frame][atom]; sap nullable) into the accumulators (first: they start with this pass) and writes total[f] = the
// f32 of the f64 sum of sasa[f][:] in atom order for every frame of the pass
void launch_ens_reduce(uint32_t frames, uint32_t m, const int32_t *count, const float *sasa, const float *sap, const EnsAcc &a, bool first, float *total,
                       hipStream_t st);
// dSASA over frames (ens.inl).  out[f * m + k] = attr[k]: the attribute words of a pass of packed frames
void launch_bsa_tile_attr(uint32_t frames, uint32_t m, const uint32_t *attr, uint32_t *out, hipStream_t st);
// folds the pass's buried ([frame][atom]) into a.s1 / s2 / cmin / cmax (k_ens_reduce as it is) and into frames_buried (frames with buried > 0),
// and writes total[g][f] = the f32 of the f64 sum of plane g of sasa3 ([3][frame][atom]) over frame f in atom order (k_ens_totals as it is)
void launch_bsa_ens_reduce(uint32_t frames, uint32_t m, const int32_t *buried, const float *sasa3, const EnsAcc &a, uint32_t *frames_buried, bool first,
                           float *const total[3], hipStream_t st);
// Segment sums (seg.inl).  All device pointers.
struct SegCsr {           // n_seg segments over the items of a row: segment s lists item[start[s] .. start[s + 1]) in the order they are added
    uint32_t n_seg, n_long;
    const uint32_t *start, *item;
    const uint32_t *long_ids;  // n_long: the segments with more than 64 items (the wave kernel's), ascending
};
// out[row][s] = f32 of the f64 sum of values[row][item] over segment s in list order (one __dadd_rn per item), rows x n_seg; values: rows x m
void launch_segment_sum(uint64_t rows, uint32_t m, const float *values, const SegCsr &c, float *out, hipStream_t st);
struct SegAcc {           // per residue, over all frames so far: sum and sum of squares of the per-frame f32 values (f64, frame order), extremes
    double *t1, *t2;
    float *vmin, *vmax;
};
// folds the pass's rs ([frame][n_res]) into the accumulators (first: they start with this pass)
void launch_ens_res_reduce(uint32_t frames, uint32_t n_res, const float *rs, const SegAcc &a, bool first, hipStream_t st);
// Shape complementarity (sc.inl).  Dot and probe records as the kernels write them; arp_sc_dots copies from the dots.
struct ScDot {        // 80 B
    double p[3], n[3], area, nn_dist, score;
    uint32_t atom, flags;  // flags: kind (ARP_SC_DOT_*) | ARP_SC_DOT_BURIED | ARP_SC_DOT_TRIMMED
};
struct ScProbe {      // 72 B
    double p[3], alt[3], height;
    uint32_t a[3], i;  // a: the reference's atom_indices; i: the first atom of the pair the probe came from (its burial candidate list)
};
constexpr uint32_t kScErrCoincident = 1, kScErrSubdiv = 2;
struct ScJob {
    uint32_t n;
    const double *x, *y, *z, *r;   // host arrays
    const uint32_t *mol;           // 0 / 1
    const long long *serial;
    double rp, density, band, sep, w;
};
struct ScRunOut {
    std::vector<ScDot> dots[2];    // toroidal, contact, concave: the reference's order
    uint64_t n_toroidal = 0, n_convex = 0, n_concave = 0, n_probes = 0;
    std::vector<uint32_t> att;     // 1: Buried, 0: Far
    uint32_t err = 0, err_i = 0, err_j = 0;  // kScErr*: Coincident (atoms err_i, err_j) or TooManySubdivisions
};
// Runs every device stage on `st` (synchronising for the sizes of the outputs).  ARP_ERR_HIP on a runtime failure; the SC errors in out->err.
arp_status launch_sc(const ScJob &job, hipStream_t st, Profiler *prof, ScRunOut *out);
// The same over the frames of an ensemble (sc_ens.inl).
struct ScEnsFrame {       // one per frame, written on the device and copied back
    uint32_t ok;          // no coincident pair, no subdivision failure, dots on both surfaces
    uint32_t subdiv;      // the sampling limit was exceeded
    uint32_t ci, cj;      // the coincident pair (atoms of the frame; both ~0 when there is none)
    uint32_t att[2];      // Buried atoms per molecule
    uint32_t nT[2], nC[2], nK[2];  // toroidal, contact and concave dots per surface
    uint32_t n_probes;
};
struct ScEnsJob {
    uint32_t n;                    // atoms per frame
    uint64_t n_frames;
    const double *xyz;             // host, [F][n][3]
    const double *r;
    const uint32_t *mol;
    const long long *serial;
    double rp, density, band, sep, w;
    uint32_t frames_per_pass;      // > 0: the knob sc_ens_frames; 0: from the memory budget
};
struct ScEnsOut {                  // host arrays
    arp_sc_surface *surf;          // [F][2]: the dot statistics of each surface (atom counts zero)
    ScEnsFrame *frames;            // [F]
    uint32_t *frames_in_interface; // [n]
    unsigned long long *trimmed_dots;  // [n]
};
arp_status launch_sc_ens(const ScEnsJob &job, hipStream_t st, Profiler *prof, ScEnsOut *out);
// statistics of dot segments (sc_ens.inl k_sc_dot_stats) on host columns, and the host restatement with the same summation order
arp_status launch_sc_dot_stats(uint64_t n_seg, const uint64_t *start, const uint32_t *flags, const double *area, const double *nn, const double *score,
                               const uint32_t *other, arp_sc_surface *out, hipStream_t st);
void sc_dot_stats_host(uint64_t n_seg, const uint64_t *start, const uint32_t *flags, const double *area, const double *nn, const double *score,
                       const uint32_t *other, arp_sc_surface *out);
void launch_pack_split(const PackArrays &pa, const unsigned long long *result, const arp_pair *pairs, unsigned long long capacity, arp_pair *grouped, bool ordered, hipStream_t st);

}  // namespace arp
