// Host-side declarations shared by the host sources (engine.cpp, batch.cpp, sasa_dev.cpp, structure.cpp, table*.cpp, table_dev.hip), and the rule
// by which a block of several arrays is planned and carved (seg_align, Carver, Bump, planned_bytes, carve_block).  It includes no HIP header: the rule is checked in a host program of its own (tests/hostcheck/carve_check.cpp).
#pragma once
#include <array>
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <exception>
#include <mutex>
#include <new>
#include <string>
#include <system_error>
#include <thread>
#include <unordered_set>
#include <vector>

#include "../../include/arpeggia_amd.h"
#include "debug_knobs.h"

namespace arp {

void set_error(const char *fmt, ...);

// A block that holds several arrays is carved into 256-byte aligned segments.  The rule lives here and nowhere else: a block's size is never
// written down, it is what its layout -- the sequence of take() calls that hands out its arrays -- adds up to.  The layout is walked twice: once
// without a block, to plan the bytes to allocate, and once on the block, to carve it (planned_bytes, carve_block).
constexpr uint64_t seg_align(uint64_t bytes) { return (bytes + 255u) & ~255ull; }
struct Carver {  // the offset of the next segment; offsets only: one layout serves a device block and its pinned twin
    uint64_t off = 0;
    uint64_t take(uint64_t bytes) { const uint64_t at = off; off += seg_align(bytes); return at; }
};
struct Bump {  // typed pieces of one block; without a block (base == nullptr) it plans: take() moves the offset on and returns nullptr
    char *base = nullptr; Carver c{};
    template <class T> T *take(uint64_t count) { const uint64_t at = c.take(count * sizeof(T)); return base ? reinterpret_cast<T *>(base + at) : nullptr; }
};
// A layout is a callable void(Bump &) that assigns the pointers of a call.  The bytes a block needs to hold it:
template <class Layout> uint64_t planned_bytes(Layout &&layout) { Bump plan; layout(plan); return plan.c.off; }
// The pointers into `block`, which holds `planned` bytes.  A layout that asks for other sizes on its second walk (one that changes a value it
// reads, say) is an error of the program: a status, and the caller launches nothing.
template <class Layout> arp_status carve_block(char *block, uint64_t planned, Layout &&layout) {
    Bump b{block};
    layout(b);
    if (b.c.off == planned) return ARP_OK;
    set_error("internal error: a block planned at %llu bytes was carved into %llu", (unsigned long long)planned, (unsigned long long)b.c.off);
    return ARP_ERR_HIP;
}

// No exception may cross the C ABI (SURVEY.md 8b "Errors": the reference panics, a C boundary returns a status).  Every status-returning entry
// point that allocates or starts threads is a function-try-block that ends in this: `extern "C" arp_status f(...) try { ... } ARP_ABI_CATCH`.
#define ARP_ABI_CATCH                                                                                                               \
    catch (const std::bad_alloc &) { arp::set_error("out of host memory"); return ARP_ERR_OOM; }                                   \
    catch (const std::exception &e_) { arp::set_error("internal error: %s", e_.what()); return ARP_ERR_HIP; }                       \
    catch (...) { arp::set_error("internal error: unknown exception"); return ARP_ERR_HIP; }

// A failing HIP runtime call ends the calling function with a status (OOM told apart) and a message naming the call.
#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) {                                                                    \
            arp::set_error("HIP error %d (%s) at %s:%d: %s", (int)e_, hipGetErrorString(e_), __FILE__, __LINE__, #expr); \
            return (e_ == hipErrorOutOfMemory) ? ARP_ERR_OOM : ARP_ERR_HIP;                        \
        }                                                                                          \
    } while (0)

// The stage laps of the "timing" switch (arp_debug_set): lap(what) prints the time since the previous lap (or the construction) on stderr through
// `line`, a format that takes the stage's name (%s) and the milliseconds (%f).  Inert unless the switch is set when it is constructed.
struct LapTimer {
    const char *line;
    bool on;
    std::chrono::steady_clock::time_point prev;
    explicit LapTimer(const char *line_format) : line(line_format), on(g_debug.timing != 0), prev(std::chrono::steady_clock::now()) {}
    void operator()(const char *what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, line, what, std::chrono::duration<double, std::milli>(now - prev).count());
        prev = now;
    }
};

// Fixed-width, NUL-padded string column (n x W chars), the layout the C ABI hands to numpy / Rust.
template <int W>
struct StrCol {
    std::vector<char> buf;
    void resize(size_t n) { buf.assign(n * W, 0); }
    size_t size() const { return buf.size() / W; }
    const char *at(size_t i) const { return &buf[i * W]; }
    char *at(size_t i) { return &buf[i * W]; }
    void set(size_t i, const char *s) {
        char *d = at(i);
        int k = 0;
        for (; k < W - 1 && s[k]; k++) d[k] = s[k];
        for (; k < W; k++) d[k] = 0;
    }
    std::string str(size_t i) const { return std::string(at(i)); }
};

struct Plane {
    double c[3], n[3];
};

struct ChainInfo {
    uint32_t model_idx;
    int32_t model_serial;
    std::string id;
};

struct ResidueInfo {
    uint32_t chain;       // index into chains
    int32_t resi;
    std::string icode;
    std::string name;     // Residue::name(): common conformer name
    uint32_t ord;         // positional index inside the chain (complex.rs:411-440)
    std::vector<uint32_t> atoms;         // atom indices in hierarchy order (conformer ordinal, then input order)
    std::vector<std::string> altlocs;    // distinct conformer altlocs in order of appearance
};

}  // namespace arp

// The parsed, filtered model (what `load_model` returns in the reference, utils.rs:51-63), as SoA columns.
struct arp_structure {
    uint64_t n = 0;
    std::vector<double> x, y, z, occ;
    std::vector<int32_t> serial, resi, model_serial;
    arp::StrCol<8> name, resn /* conformer */, res_resn /* residue */, chain;
    arp::StrCol<4> altloc, icode, elem;
    std::vector<uint32_t> res_ord, res_id, base_attr, attr;
    std::vector<uint32_t> chain_rank, model;
    std::vector<uint32_t> atom_chain;  // index into chains
    std::vector<arp::ChainInfo> chains;
    std::vector<arp::ResidueInfo> residues;
    std::vector<std::string> chain_ids;  // distinct ids, byte-wise sorted: chain_rank indexes this
    std::vector<uint32_t> res_h_ptr, res_h_idx, res_cb, res_sg;
    std::string groups_applied;
    bool groups_valid = false;
    // table_cache.cpp: derived per-structure tables of the table path + the device-resident copy (built on the first arp_get_contacts)
    void *table_cache = nullptr;
    std::mutex table_cache_mu;   // guards the creation of table_cache
    void (*table_cache_free)(void *) = nullptr;
    ~arp_structure() { if (table_cache && table_cache_free) table_cache_free(table_cache); }
};

namespace arp {
// The atoms of one SASA run on the device (sasa_dev.cpp), host arrays of n entries: what sasa_run and bsa_run share.
struct SasaAtoms {
    uint64_t n = 0;
    const double *x = nullptr, *y = nullptr, *z = nullptr;  // f64 coordinates: SASA rounds them to f32, the SAP neighbour sum takes them as they are
    const float *R = nullptr;              // radius + probe in f32 (read for the atoms in the grid only)
    const uint32_t *model = nullptr;       // slab of every atom (dSASA runs three selections as three models of one grid); nullptr = all 0
    uint32_t n_points = 0;
    const float *sphere = nullptr;         // n_points x 3 unit vectors (sasa_sphere_points)
};
// Atom SASA (+ the SAP chain): sasa_dev.cpp runs it, arp_atom_sasa and the structure-level entry points (sasa.cpp) fill the job.
struct SasaJob : SasaAtoms {
    const uint8_t *include = nullptr;      // the SASA atoms; the others get sasa 0, count 0
    // SAP (src/sap.rs:137-250), when sidechain != nullptr: weight[j] = arp_sap_weight(residue code[j], sasa[src[j]]) (0 for src[j] < 0),
    // sap[i] = the f32 sum of the weights of the side-chain atoms within sap_radius of side-chain atom i (arp_sap_neighbor_sum)
    const uint8_t *sidechain = nullptr;
    const uint32_t *res_code = nullptr;    // position in ARP_SAP_RESIDUES, >= 20: none
    const int32_t *src = nullptr;
    float sap_radius = 0.0f;
    // segment sums of the SASA values on the device (seg.inl), in the same stream: residue and chain level
    const struct SegJob *segs = nullptr;
    uint32_t n_segs = 0;
};
// One CSR over the atoms of a job / the selected atoms of an ensemble (arp_segment_sum's contract; checked by seg_check) and where its sums go.
struct SegJob {
    uint32_t n_seg = 0;
    const uint32_t *start = nullptr, *item = nullptr;  // n_seg + 1, start[n_seg]
    float *out = nullptr;                  // n_seg (sasa_run); unused by ens_run
};
// ARP_ERR_BAD_INPUT + message unless start is monotone from 0, below 2^31 - 64, and every item is below m
arp_status seg_check(uint64_t m, uint64_t n_seg, const uint32_t *start, const uint32_t *item);
// sasa / count / sap (nullable) receive n entries; one synchronisation at the end.  Inputs are checked by the callers.  With all three null
// only the segment sums come back.
arp_status sasa_run(arp_context *ctx, const SasaJob &job, float *sasa, int32_t *count, float *sap);
// The frames of an ensemble run (sasa_dev.cpp EnsPasses), host arrays: what ens_run and bsa_ens_run share.
struct EnsAtoms {
    uint64_t n_top = 0, m = 0, n_frames = 0;  // atoms a frame's coordinates cover, selected atoms, frames
    const double *xyz = nullptr;           // n_frames x n_top x 3
    const uint32_t *sel = nullptr;         // m topology indices, ascending
    const float *R = nullptr;              // m: radius + probe in f32
    uint32_t n_points = 0;
    const float *sphere = nullptr;
    uint64_t chunk_atoms = 0;              // packed atoms per pass, 0: automatic
};
// SASA / SAP statistics over the frames of an ensemble (arp_sasa_ensemble): sasa_dev.cpp ens_run packs the frames into
// passes and runs them (kernels in ens.inl + the unchanged SASA / SAP kernels); sasa.cpp selects, checks and finishes.
struct EnsJob : EnsAtoms {
    bool with_sap = false;
    const uint8_t *sidechain = nullptr;    // m (SAP)
    const uint32_t *res_code = nullptr;    // m (SAP): position in ARP_SAP_RESIDUES, >= 20: none
    float sap_radius = 0.0f;
    const SegJob *res = nullptr, *chain = nullptr;  // residue level (arp_sasa_ensemble_residues): the CSRs over the m selected atoms, both or none
};
struct EnsOut {                            // m entries each unless noted; the SAP members are written only with EnsJob::with_sap
    unsigned long long *s1 = nullptr, *s2 = nullptr;
    int32_t *cmin = nullptr, *cmax = nullptr;
    double *t1 = nullptr, *t2 = nullptr;
    float *pmin = nullptr, *pmax = nullptr;
    float *total = nullptr;                // n_frames
    int32_t *count = nullptr;              // n_frames x m, nullable
    float *sap = nullptr;                  // n_frames x m, nullable
    // with EnsJob::res: per residue the f64 sums of the per-frame residue SASA and of its square (frame order) and the extremes; per frame the
    // chain sums; the per-frame residue values only when asked for
    double *rt1 = nullptr, *rt2 = nullptr;
    float *rmin = nullptr, *rmax = nullptr;
    float *chain_sasa = nullptr;           // n_frames x chain->n_seg
    float *residue_sasa = nullptr;         // n_frames x res->n_seg, nullable
};
arp_status ens_run(arp_context *ctx, const EnsJob &job, const EnsOut &out);
// Buried surface per atom (sasa.inl k_sasa_split): sasa_dev.cpp bsa_run, sasa_run's staging with the split walk.
struct BsaJob : SasaAtoms {
    const uint8_t *group = nullptr;        // 0: not in the grid; bit 0: in group 1, bit 1: in group 2
    bool per_model = false;                // every model gets its own origin (DevAtoms::per_model)
    const SegJob *seg = nullptr;           // nullable: one CSR over the n atoms; SegJob::out receives 3 x n_seg sums (complex, group 1, group 2)
};
// sasa3 / count3 (nullable): 3 x n (complex, group 1, group 2; 0 where the atom is not in the group); buried (nullable): n.  One synchronisation.
arp_status bsa_run(arp_context *ctx, const BsaJob &job, float *sasa3, int32_t *count3, int32_t *buried);
// dSASA over the frames of an ensemble (arp_dsasa_ensemble): ens_run's passes with k_sasa_split on the pack
struct BsaEnsJob : EnsAtoms {
    const uint8_t *group = nullptr;        // m: 1, 2 or 3
};
struct BsaEnsOut {
    unsigned long long *s1 = nullptr, *s2 = nullptr;  // m: sum of buried, sum of buried^2 over the frames
    int32_t *bmin = nullptr, *bmax = nullptr;         // m
    uint32_t *frames_buried = nullptr;                // m: frames with buried > 0
    float *total[3] = {nullptr, nullptr, nullptr};    // n_frames each: complex, group 1, group 2
    int32_t *buried = nullptr;                        // n_frames x m, nullable
};
arp_status bsa_ens_run(arp_context *ctx, const BsaEnsJob &job, const BsaEnsOut &out);
// table_ens.cpp: model 0 of a structure as the topology of an ensemble (n0 atoms, r0 residues); with frames_from_models every further model must
// repeat model 0's atoms one for one (ARP_ERR_BAD_INPUT naming the first model and atom that differ)
arp_status freq_topology(const arp_structure *s, bool frames_from_models, uint64_t *n0, uint64_t *r0, uint64_t *n_models);
// golden-spiral unit vectors in f64, rounded to f32 (DESIGN.md "Atom SASA")
void sasa_sphere_points(uint32_t n, float *xyz);
uint32_t sap_residue_code(const char *resn);
arp_status sasa_check_params(float probe, int32_t n_points);  // ARP_ERR_BAD_INPUT + message unless 1 <= n_points <= ARP_SASA_MAX_POINTS, probe finite >= 0  // position in ARP_SAP_RESIDUES (case-insensitive, as arp_sap_weight), 20 if none

// sasa.cpp: steps 1-5 of arp_structure_sasa_select (keep: chain ids, empty = all; model_filter: step 4; serial_filter: step 5)
std::vector<uint32_t> select_atoms(const arp_structure *s, const std::unordered_set<std::string> &keep, bool remove_h, bool model_filter,
                                   bool serial_filter, int32_t model_num);
arp_status parse_groups(const std::vector<std::string> &all_chains, const char *groups, std::vector<std::string> *ligand,
                        std::vector<std::string> *receptor);
arp_status apply_groups(arp_structure *s, const char *groups);
bool fit_plane(const std::vector<std::array<double, 3>> &pts, Plane *out);

// Host worker threads for the table path (planes, rows, sort, columns) -- the counterpart of the reference's global rayon pool
// (utils.rs:8-30, python.rs num_threads).  1 = serial (the reference's default), 0 = all hardware threads.
int host_threads();
void set_host_threads(int n);
// Pins the worker count of the calling thread for the lifetime of the scope: n > 0 that many, n == 0 all hardware threads,
// n < 0 a snapshot of the process-wide default.  parallel_for() is only ever called from the thread that owns the scope.
struct HostThreadsScope {
    int prev;
    explicit HostThreadsScope(int n);
    ~HostThreadsScope();
    HostThreadsScope(const HostThreadsScope &) = delete;
    HostThreadsScope &operator=(const HostThreadsScope &) = delete;
};
// fn(begin, end, worker) over [0, n) in contiguous slices, one per worker; serial below `min_per_worker` items per worker.
template <class F>
void parallel_for(size_t n, size_t min_per_worker, F &&fn) {
    size_t workers = (size_t)host_threads();
    if (min_per_worker && n / min_per_worker < workers) workers = n / min_per_worker;
    if (workers <= 1) { fn((size_t)0, n, (size_t)0); return; }
    // An exception must not leave a std::thread's function (std::terminate) nor unwind past joinable threads: a worker parks its exception,
    // the guard joins on every path, and the caller rethrows the first one -- it then reaches the C ABI's catch like any exception of the
    // calling thread.
    std::vector<std::thread> th;
    th.reserve(workers);
    std::exception_ptr first_error;
    std::mutex error_mu;
    auto guarded = [&](size_t w) noexcept {
        try { fn(n * w / workers, n * (w + 1) / workers, w); }
        catch (...) { std::lock_guard<std::mutex> lk(error_mu); if (!first_error) first_error = std::current_exception(); }
    };
    {
        struct JoinAll { std::vector<std::thread> &t; ~JoinAll() { for (auto &x : t) if (x.joinable()) x.join(); } } join_all{th};
        size_t started = 0;  // slices [0, started) run on threads of their own; the caller takes the last one and any that could not get a thread
        for (; started + 1 < workers; started++) {
            const size_t w = started;
            try { th.emplace_back([&guarded, w]() { guarded(w); }); } catch (const std::system_error &) { break; }
        }
        for (size_t w = started; w < workers; w++) guarded(w);
    }
    if (first_error) std::rethrow_exception(first_error);
}
}  // namespace arp
