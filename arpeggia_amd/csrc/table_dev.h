// Device side of the contact table (SURVEY.md 8f rows f1 + f2): plane fits, ring rows, row expansion, the 10-key sort and the
// side-chain plane statistics run as HIP kernels (table_dev.hip); table_cache.cpp keeps the bookkeeping (entity lists, strings).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/arpeggia_amd.h"

namespace arp {

// One ring of the output vocabulary (complex.rs:334-342: entity "Ring", atomi 0), as the device needs it.
struct RingEnt {
    uint32_t src_res;        // residue whose ring atoms define the plane
    int32_t model_serial;    // the model serial the ring is filed under (complex.rs:447-449)
    uint32_t model_rank;     // rank of that serial among the file's serials (sort key `model`)
    uint32_t chain_rank;
    uint32_t flags;          // 1 = chain in the ligand set, 2 = in the receptor set, 4 = resolves to a residue (has an ordinal)
    uint32_t ord;            // positional index of that residue in its chain (complex.rs:411-440)
    uint32_t sc_src;         // residue whose side-chain plane applies to the ring entity, or ARP_NONE
    uint32_t pad;
};

struct EntKey { int32_t resi; uint32_t altloc; int32_t atomi; uint32_t icode; };  // names as big-endian words: unsigned compare == byte-wise order

// Device-resident copy of a structure (kept with the arp_structure, uploaded once): the arp_atoms arrays + what the table kernels need.
struct DevStructure {
    int device = -1;
    char *block = nullptr;               // one allocation
    uint64_t n = 0, n_res = 0, n_h = 0;
    double *x = nullptr, *y = nullptr, *z = nullptr;
    uint32_t *attr = nullptr, *res_ord = nullptr, *res_id = nullptr, *res_h_ptr = nullptr, *res_h_idx = nullptr, *res_cb = nullptr, *res_sg = nullptr;
    uint32_t *chain_rank = nullptr, *model = nullptr;
    uint8_t *plane_bits = nullptr;       // per atom: 1 = ring-plane atom (residues.rs:163-186), 2 = sc-plane atom (residues.rs:188-268)
    uint32_t *res_atom_ptr = nullptr, *res_atom_idx = nullptr;   // residue -> atoms in hierarchy order
    uint32_t *atom_sc_src = nullptr;     // per atom: residue whose sc plane applies, or ARP_NONE
    EntKey *ent_key = nullptr;           // per atom
    uint32_t *model_rank = nullptr;      // per model ordinal
    int32_t *model_serial_of = nullptr;  // per model ordinal
    // derived once per structure by the first device_table call (they depend on the structure alone): the fitted planes and the entity ranks
    char *derived = nullptr;             // one allocation
    void *ring_pl = nullptr, *sc_pl = nullptr; uint8_t *pl_valid = nullptr; uint32_t *ent_rank = nullptr; uint64_t derived_n_ent = 0;
    uint32_t max_ent_rank = 0;           // largest rank of an entity inside its chain (the width of a rank in the rows' sort key)
    uint32_t n_chains = 0, n_models = 0;  // distinct chain ids / models of the structure (widths of the sort keys)
    bool any_icode = false;              // some atom carries an insertion code (otherwise that sort pass is skipped)
    std::string attr_groups;             // the chain groups the resident attr words were built for
    char *rings_block = nullptr;         // the ring entities {RingEnt[], EntKey[]} on the device; sent again when they differ from rings_host (table_dev.hip)
    uint64_t rings_cap = 0;
    std::vector<char> rings_host;
};

struct TableRow { uint32_t from_ent, to_ent; float distance; int32_t interaction; };   // entity = atom index, or n_atoms + ring index
struct TableSc { float dist, dihedral, angle, valid; };                                   // valid != 0: both residues have a side-chain plane
// What comes back: rows in final order.  A large table lands straight in a pooled pinned block (batch.cpp pinned_block) that the table
// then OWNS -- no copy out of a landing buffer; a small one is copied into plain arrays.  `owner` keeps whichever it is alive.
struct TableRowsHost {
    uint64_t n = 0;
    std::shared_ptr<char> owner;
    TableRow *rows = nullptr;
    TableSc *sc = nullptr;
};
std::shared_ptr<char> pinned_block(size_t bytes);   // pooled pinned host memory; the deleter gives the block back to the pool (batch.cpp)

// Runs the whole device pipeline for one structure.  `pairs_dev` = contacts-only pair list on the device (arp_contacts_atomic,
// ARP_MEM_DEVICE).  Returns ARP_ERR_NO_RINGS etc. like arp_get_contacts.
arp_status device_table(arp_context *ctx, DevStructure &ds, const std::vector<RingEnt> &rings, const std::vector<EntKey> &ring_keys,
                        const arp_pair *pairs_dev, uint64_t n_pairs, double dist_cutoff, TableRowsHost *out);
struct TableRoute;
TableRoute table_route_last();  // the route of the process's last device_table call (table_plan.h; arp_debug_get)
// the planes the device fitted, for tests (PHE4 of 1ubq: residues.rs:355-372): 12 doubles per residue {ring c, ring n, sc c, sc n} + validity bits
arp_status device_planes(arp_context *ctx, const DevStructure &ds, std::vector<double> *planes, std::vector<uint8_t> *valid);

// Contact frequencies over frames (freq.inl, arp_contact_frequencies): the topology's arrays (host, the chain groups applied to attr) and
// n_frames x n x 3 f64 coordinates.  Rows come back sorted by key = i << 34 | j << 5 | interaction code (i, j: entities -- atoms, or n + ring).
struct FreqJob {
    uint64_t n = 0, n_res = 0, n_h = 0, n_frames = 0;
    const uint32_t *attr = nullptr, *res_ord = nullptr, *chain_rank = nullptr, *res_id = nullptr, *res_h_ptr = nullptr, *res_h_idx = nullptr,
                   *res_cb = nullptr, *res_sg = nullptr;
    const double *xyz = nullptr;
    double vdw_comp = 0.1, dist_cutoff = 6.5;
    uint64_t chunk_atoms = 0;  // atoms per pass, 0 = automatic (arp_debug_set "freq_chunk_atoms")
    // ARP_FREQ_RINGS (freq_rings.inl), n_rings > 0: the topology's ring entities as entities n .. n + n_rings - 1.  rings[e].src_res is a SLOT:
    // the ring residues in order, slot_res[k] the residue of slot k; res_atom_ptr / res_atom_idx / plane_bits as DevStructure holds them, cut
    // to model 0; cand: the atoms a CationPi row can name (ARP_ATTR_POS_RESN, not ARP_ATTR_H), ascending
    uint64_t n_rings = 0, n_slots = 0, n_cand = 0;
    const RingEnt *rings = nullptr;
    const uint32_t *slot_res = nullptr, *res_atom_ptr = nullptr, *res_atom_idx = nullptr, *cand = nullptr;
    const uint8_t *plane_bits = nullptr;
    // arp_residue_contact_frequencies: rows per (residue of from, residue of to, code), a frame counted once per row; the
    // rows' keys are res(from) << (res_bits + 5) | res(to) << 5 | code.  frame_bits: the knob freq_frame_bits, 0 = automatic
    bool residue = false;
    uint32_t frame_bits = 0;
    // ARP_FREQ_WATERS (freq_water.inl), n_water > 0: the topology's water atoms (residue HOH, not ARP_ATTR_H) and polar atoms
    // (ARP_ATTR_DONOR or ARP_ATTR_ACCEPTOR, not ARP_ATTR_H), both ascending and disjoint; residue level only
    uint64_t n_water = 0, n_polar = 0;
    const uint32_t *water = nullptr, *polar = nullptr;
};
struct FreqRowsHost {
    std::vector<unsigned long long> key;
    std::vector<uint32_t> count;
    std::vector<float> mn, mx;
    uint32_t res_bits = 0;  // residue level: bits of a residue ordinal in the keys
};
arp_status device_frequencies(arp_context *ctx, const FreqJob &job, FreqRowsHost *out);

// Water bridges (freq_water.inl, arp_water_bridges): one record per bridge (p, w, q) of every frame -- topology atom indices,
// the two legs as f32 -- ordered by (frame, p, q, w).  Of the job only the topology's attr / res_ord / chain_rank, the frames and the water and polar
// lists are read.
struct WaterTriple { uint32_t frame, p, q, w; float dp, dq; };
arp_status device_water_bridges(arp_context *ctx, const FreqJob &job, std::vector<WaterTriple> *out);

// Contact timelines (timeline.inl, arp_contact_timelines): the frequency rows of the job (device_frequencies' own result)
// and, per row, the bitmap of the frames that feed it (bit f & 31 of words[r * words_per_row + (f >> 5)]) with its statistics.  want_bitmap false:
// the bitmap stays on the device (words empty).  cap_bytes: the most device memory the bitmap may take (ARP_ERR_CAPACITY beyond).
struct TimelineHost {
    uint64_t words_per_row = 0;
    bool has_bitmap = false;
    std::vector<uint32_t> words, first, last, n_events, longest;
};
arp_status device_timelines(arp_context *ctx, const FreqJob &job, bool want_bitmap, uint64_t cap_bytes, FreqRowsHost *rows, TimelineHost *out);

// Contact similarity (similarity.inl, arp_contact_similarity / arp_bit_gram): the frequency rows of the job and the Gram matrix of
// its timeline bitmap -- between frames (m = F) or, by_rows, between rows (m = R) -- as u32 counts or as the bits of f32 Tanimoto values, with the
// set sizes.  The bitmap never leaves the device.  cap_bytes: the most the matrix may take (ARP_ERR_CAPACITY beyond); timeline_cap_bytes: the bitmap's.
struct SimilarityHost {
    uint64_t m = 0;
    std::shared_ptr<char> owner;         // the block the matrix lives in: pooled pinned memory (batch.cpp pinned_block) from 1 MiB on, the heap below
    uint32_t *matrix = nullptr;          // m x m, row-major
    std::vector<uint32_t> sizes;
};
arp_status device_similarity(arp_context *ctx, const FreqJob &job, bool by_rows, bool counts, uint64_t timeline_cap_bytes, uint64_t cap_bytes, FreqRowsHost *rows,
                             SimilarityHost *out);
// the same kernels on a host bitmap of `rows` rows of ceil(n_bits / 32) words (rows > 0, n_bits > 0): out m x m, sizes m
arp_status device_bit_gram(arp_context *ctx, uint64_t rows, uint64_t n_bits, const uint32_t *words, bool by_rows, bool counts, uint64_t cap_bytes, void *out, uint32_t *sizes);

// Contact autocorrelation (autocorr.inl, arp_contact_autocorrelation / arp_bit_autocorr): the frequency rows of the job and, per row
// and lag 0 .. L, in how many frames the row's contact exists now and L frames on (intermittent), or all the way there (continuous), with the per-
// interaction sums and the rows' half-lives (ARP_NONE: none).  want_matrix false: no rows x (L + 1) buffer exists on either side.  cap_bytes: the most the
// device matrix may take (ARP_ERR_CAPACITY beyond); timeline_cap_bytes: the bitmap's, which never leaves the device.
struct AutocorrHost {
    uint64_t n_lags = 0;
    uint32_t n_groups = 0;
    bool has_matrix = false;
    std::shared_ptr<char> owner;         // the block the matrix lives in: pooled pinned memory from 1 MiB on, the heap below
    uint32_t *matrix = nullptr;          // rows x n_lags, row-major
    std::vector<unsigned long long> sums;  // n_groups x n_lags
    std::vector<uint32_t> half_life;     // per row
};
arp_status device_autocorrelation(arp_context *ctx, const FreqJob &job, bool continuous, bool want_matrix, uint64_t max_lag, uint64_t timeline_cap_bytes, uint64_t cap_bytes,
                                  FreqRowsHost *rows, AutocorrHost *out);
// the same kernels on a host bitmap (rows > 0, max_lag < n_bits): acf rows x (max_lag + 1) (nullable), sums n_groups x (max_lag + 1) (written when group is given), half_life rows
arp_status device_bit_autocorr(arp_context *ctx, uint64_t rows, uint64_t n_bits, const uint32_t *words, bool continuous, uint64_t max_lag, const uint32_t *group, uint64_t n_groups,
                               uint64_t cap_bytes, uint32_t *acf, unsigned long long *sums, uint32_t *half_life);

// Contact clusters (cluster.inl, arp_contact_clusters / arp_bit_cluster): the frequency rows of the job and the gromos clusters of its
// frames on the neighbour relation tanimoto >= min_similarity -- per frame its cluster (ARP_NONE: left over by max_clusters), the bits of its f32 Tanimoto
// value to the cluster's centre, its neighbours in the full graph and its set size; per cluster its centre and size; and, with want_counts, in how many frames
// of each cluster every row is present.  Neither the bitmap nor any frame-by-frame matrix leaves the device.  cap_bytes: the most the neighbour bits, and the
// counts, may take (ARP_ERR_CAPACITY beyond); timeline_cap_bytes: the bitmap's.
struct ClustersHost {
    uint64_t m = 0, n_clusters = 0;
    bool has_counts = false;
    std::vector<uint32_t> cluster, sim, n_neighbours, sizes;   // per frame
    std::vector<uint32_t> centre, cluster_size;                // per cluster
    std::shared_ptr<char> owner;         // the block the counts live in: pooled pinned memory from 1 MiB on, the heap below
    uint32_t *counts = nullptr;          // rows x n_clusters, row-major
};
arp_status device_clusters(arp_context *ctx, const FreqJob &job, float min_similarity, uint32_t max_clusters, bool want_counts, uint64_t timeline_cap_bytes, uint64_t cap_bytes,
                           FreqRowsHost *rows, ClustersHost *out);
// the same kernels on a host bitmap (rows > 0, n_bits > 0); by_rows: the word rows are clustered (m = rows, no counts), else the bit columns (m = n_bits)
arp_status device_bit_cluster(arp_context *ctx, uint64_t rows, uint64_t n_bits, const uint32_t *words, bool by_rows, float min_similarity, uint32_t max_clusters, bool want_counts,
                              uint64_t cap_bytes, ClustersHost *out);

// RMSD between frames (rmsd.inl, arp_rmsd_matrix / arp_rmsd_reference / arp_rmsd_clusters): n_frames x n_atoms x 3 f64 coordinates and
// the n_sel selected atoms, strictly increasing.  kMatrix: out[F x F]; kReference: out[F] against frame ref_frame, or against ref_xyz[n_atoms x 3] when it is
// given; kClusters: the gromos clusters on rmsd <= cutoff into ClustersHost (sim: the bits of the f32 rmsd to the centre; sizes and counts stay empty).  The
// caller has checked the sizes against the capacity knob.
struct RmsdJob {
    enum Kind { kMatrix, kReference, kClusters } kind = kMatrix;
    uint64_t n_atoms = 0, n_frames = 0, n_sel = 0;
    const double *xyz = nullptr;
    const uint32_t *sel = nullptr;
    uint64_t chunk_atoms = 0;  // atoms per upload pass, 0 = automatic (arp_debug_set "rmsd_chunk_atoms")
    const double *ref_xyz = nullptr;
    uint64_t ref_frame = 0;
    float cutoff = 0.0f;
    uint32_t max_clusters = ARP_NONE;
};
constexpr uint64_t rmsd_n_pad(uint64_t n) { return (n + 3u) & ~3ull; }  // atoms of a packed frame: n rounded up to the K step of the f64 MFMA (rmsd.inl kRmsdStep)
arp_status device_rmsd(arp_context *ctx, const RmsdJob &job, float *out, ClustersHost *clusters);
// rmsd.cpp: what every arp_rmsd_* / arp_rmsf call checks before the device is touched (the frame checks of the frequency call, then the selection), and the
// capacity knob "rmsd_cap_bytes"
uint64_t rmsd_cap();
arp_status rmsd_check(const char *what, const arp_structure *s, uint64_t n_frames, const double *xyz, const uint32_t *sel, uint64_t n_sel, std::vector<double> *model_xyz,
                      const double **frames, uint64_t *n0_out, uint64_t *F_out);

// RMSF and the mean structure (rmsf.inl, arp_rmsf): the frames superposed on frame ref_frame, on ref_xyz[n_atoms x 3] when it is given, or
// -- max_rounds > 1 -- on their own iterated mean, fitted on the n_sel atoms of sel and measured on the n_msel atoms of msel (msel == nullptr: on sel, n_msel
// is then n_sel).  The outputs are arp_rmsf's; transforms and aligned may be null.  The caller has checked the sizes against the capacity knob.
struct RmsfJob {
    uint64_t n_atoms = 0, n_frames = 0, n_sel = 0, n_msel = 0;
    const double *xyz = nullptr;
    const uint32_t *sel = nullptr, *msel = nullptr;
    uint64_t chunk_atoms = 0;  // atoms per upload pass, 0 = automatic (arp_debug_set "rmsd_chunk_atoms")
    const double *ref_xyz = nullptr;
    uint64_t ref_frame = 0;
    uint32_t max_rounds = 1;
    double tol = 0.0;
};
struct RmsfOut {
    double *mean = nullptr;        // [m][3]
    float *rmsf = nullptr;         // [m]
    float *frame_rmsd = nullptr;   // [F]
    double *transforms = nullptr;  // [F][12], nullable
    double *aligned = nullptr;     // [F][m][3], nullable
    double *cov = nullptr;         // [3 m][3 m], nullable: arp_covariance (cov.inl, behind the deviations of the same pipeline)
    float *dccm = nullptr;         // [m][m], nullable: arp_covariance
    uint32_t n_rounds = 0;
    double last_change = 0.0;
};
arp_status device_rmsf(arp_context *ctx, const RmsfJob &job, RmsfOut *out);
// rmsf.cpp: what arp_rmsf and arp_covariance check before the device is touched, under the prefix `what`: the checks of the arp_rmsd_* calls, then the
// measured selection, the rounds and the reference
arp_status rmsf_check(const char *what, const arp_structure *s, uint64_t n_frames, const double *xyz, const uint32_t *sel, uint64_t n_sel, const uint32_t *msel, uint64_t n_msel,
                      const double *ref_xyz, uint64_t ref_frame, uint32_t max_rounds, double tol, std::vector<double> *model_xyz, const double **frames, uint64_t *n0_out, uint64_t *F_out);
// rmsf.cpp: the bytes of arp_rmsf's resident state (X, G and, with a measured set of its own, XM) that "rmsd_cap_bytes" limits
uint64_t rmsf_resident_bytes(uint64_t F, uint64_t n_sel, uint64_t m, bool own_msel);

// Covariance, DCCM and projection (cov.inl, arp_covariance / arp_project).  The Gram kernel walks 32 x 32 tiles of the upper triangle of
// an L x L product (L = 3 m_pad coordinates, or m_pad atoms for the DCCM) and splits the frames into slabs so that a small triangle still fills the chip:
// about kCovGridTarget workgroups, a slab never shorter than kCovSlabMin frames and always whole chunks.  The plan is a function of (F, L) alone.
constexpr uint32_t kCovTile = 32;           // coordinates of a workgroup tile edge: 2 x 2 waves of 16 x 16
constexpr uint32_t kCovChunk = 16;          // contraction rows staged through LDS per step of the tile loop
constexpr uint32_t kCovSlabMin = 64;        // frames of the shortest slab
constexpr uint32_t kCovGridTarget = 1024;   // workgroups wanted: four per CU of the 256
struct CovPlan {
    uint64_t L = 0, T = 0, tri = 0, slab_frames = 0, slabs = 0;
    uint64_t part_items() const { return slabs * tri * kCovTile * kCovTile; }  // doubles of partial[slab][tile][32][32]
};
inline CovPlan cov_plan(uint64_t F, uint64_t L) {
    CovPlan p;
    p.L = L;
    p.T = (L + kCovTile - 1u) / kCovTile;
    p.tri = p.T * (p.T + 1u) / 2u;
    const uint64_t want = (kCovGridTarget + p.tri - 1u) / p.tri, per = (F + want - 1u) / want;
    p.slab_frames = std::max<uint64_t>(kCovSlabMin, (per + kCovChunk - 1u) / kCovChunk * kCovChunk);
    p.slabs = (F + p.slab_frames - 1u) / p.slab_frames;
    return p;
}
// what arp_covariance adds to arp_rmsf's resident bytes: the deviations, the requested outputs at their padded sizes and the slab partials
inline uint64_t cov_extra_bytes(uint64_t F, uint64_t m, bool cov, bool dccm) {
    const uint64_t m_pad = rmsd_n_pad(m);
    return F * 3u * m_pad * 8u + (cov ? 9u * m_pad * m_pad * 8u : 0u) + (dccm ? m_pad * m_pad * 4u : 0u) +
           std::max(cov ? cov_plan(F, 3u * m_pad).part_items() : 0u, dccm ? cov_plan(F, m_pad).part_items() : 0u) * 8u;
}
struct ProjectJob {
    uint64_t n_atoms = 0, n_frames = 0, n_msel = 0, k = 0;
    const double *xyz = nullptr;         // [F][N][3]
    const uint32_t *msel = nullptr;      // [m]
    uint64_t chunk_atoms = 0;            // atoms per upload pass, 0 = automatic (arp_debug_set "rmsd_chunk_atoms")
    const double *transforms = nullptr;  // [F][12], nullable: identity
    const double *mean = nullptr;        // [m][3]
    const double *modes = nullptr;       // [k][3 m]
};
arp_status device_project(arp_context *ctx, const ProjectJob &job, double *proj);

// Secondary structure (dssp.inl, arp_dssp).  The constants of the definition, written once: the host twin (dssp.cpp) and the kernels
// read these.
constexpr double kDsspCos70 = 0.3420201433256687;  // cos 70 deg: a bend where cos kappa is below it
constexpr double kDsspBreak = 2.5;                 // A: |C[r-1] - N[r]| above it breaks the chain
constexpr double kDsspCaCut = 9.0;                 // A: pairs with |CA - CA| below it get an energy
constexpr double kDsspMinDist = 0.5;               // A: a distance below it gives kDsspMinEnergy
constexpr double kDsspMinEnergy = -9.9;
constexpr double kDsspCoupling = 27.888;           // kcal A / mol: 332 x 0.42 x 0.20
constexpr double kDsspHbond = -0.5;                // kcal / mol: a bond where E is below it
constexpr uint64_t kDsspMaxRes = 1ull << 28;
struct DsspJob {
    uint64_t n_atoms = 0, n_frames = 0, n_res = 0;
    const double *xyz = nullptr;     // [F][N][3]
    const uint32_t *bb = nullptr;    // [R][4]: N, CA, C, O
    const uint8_t *flags = nullptr;  // [R]
    uint64_t chunk_atoms = 0;        // atoms per upload pass, 0 = automatic (arp_debug_set "rmsd_chunk_atoms")
};
struct DsspOut {
    uint8_t *codes = nullptr;         // [F][R], nullable
    uint32_t *counts = nullptr;       // [R][8]
    uint32_t *frame_counts = nullptr; // [F][8], nullable
    uint32_t *hb_acceptor = nullptr;  // [F][R][2], nullable
    float *hb_energy = nullptr;       // [F][R][2], nullable
};
arp_status device_dssp(arp_context *ctx, const DsspJob &job, DsspOut *out);
// rmsd.cpp: the frame half of rmsd_check (topology, frame count, finite coordinates), for the calls that take no selection
arp_status rmsd_frames_check(const arp_structure *s, uint64_t n_frames, const double *xyz, std::vector<double> *model_xyz, const double **frames, uint64_t *n0_out, uint64_t *F_out);

// Torsion angles and Ramachandran maps (torsion.inl, arp_torsions).  The definition, written once: the host twin (torsion.cpp) and the
// kernels call these two functions.  Every expression is f64 in the order of include/arpeggia_amd.h (the library is built with -ffp-contract=off).
#if defined(__HIPCC__)
#define ARP_HOST_DEVICE __host__ __device__
#else
#define ARP_HOST_DEVICE   // (a stand-alone host build of the twin under the sanitizers compiles this header as plain C++)
#endif
constexpr double kTorsionDeg = 57.29577951308232;   // 180 / pi
constexpr uint32_t kTorsionMaxBins = 360;
constexpr uint32_t kTorsionNanBits = 0x7FC00000u;   // angles of an undefined torsion
constexpr uint16_t kTorsionNoBin = 0xFFFFu;
struct Torsion {
    double c, s, a;   // cos, sin, degrees in (-180, 180]; 0, 0, 0 where undefined
    uint8_t state;    // 0 undefined, 1 g+, 2 t, 3 g-
};
ARP_HOST_DEVICE inline Torsion torsion_eval(const double *p0, const double *p1, const double *p2, const double *p3) {
    const double b1x = p1[0] - p0[0], b1y = p1[1] - p0[1], b1z = p1[2] - p0[2];
    const double b2x = p2[0] - p1[0], b2y = p2[1] - p1[1], b2z = p2[2] - p1[2];
    const double b3x = p3[0] - p2[0], b3y = p3[1] - p2[1], b3z = p3[2] - p2[2];
    const double n1x = b1y * b2z - b1z * b2y, n1y = b1z * b2x - b1x * b2z, n1z = b1x * b2y - b1y * b2x;
    const double n2x = b2y * b3z - b2z * b3y, n2y = b2z * b3x - b2x * b3z, n2z = b2x * b3y - b2y * b3x;
    const double x = (n1x * n2x + n1y * n2y) + n1z * n2z;
    const double y = sqrt((b2x * b2x + b2y * b2y) + b2z * b2z) * ((b1x * n2x + b1y * n2y) + b1z * n2z);
    const double h = sqrt(x * x + y * y);
    Torsion t{0.0, 0.0, 0.0, 0u};
    if (!(h > 0.0) || !(h < INFINITY)) return t;
    t.c = x / h; t.s = y / h;
    t.a = atan2(y, x) * kTorsionDeg;
    t.state = t.c <= -0.5 ? 2u : t.s >= 0.0 ? 1u : 3u;
    return t;
}
// the bin of a defined angle, B = n_bins > 0: floor((a + 180) / (360 / B)), B wraps to 0 (+180 falls into bin 0).  atan2 gives -pi for y = -0, x < 0: should
// the product with 180 / pi round below -180, the negative quotient counts as bin 0, where -180 itself falls; the result is below B whatever a is.
ARP_HOST_DEVICE inline uint32_t torsion_bin(double a, uint32_t B) {
    const double w = 360.0 / (double)B, q = floor((a + 180.0) / w);
    uint32_t k = q > 0.0 ? (uint32_t)q : 0u;
    if (k >= B) k -= B;
    return k < B ? k : B - 1u;
}
struct TorsionJob {
    uint64_t n_atoms = 0, n_frames = 0, n_tors = 0, n_pairs = 0;
    uint32_t n_bins = 0, n_groups = 0;
    const double *xyz = nullptr;      // [F][N][3]
    const uint32_t *quads = nullptr;  // [D][4]
    const uint32_t *pairs = nullptr;  // [P][3]: torsion a, torsion b, group
    uint64_t chunk_atoms = 0;         // atoms per upload pass, 0 = automatic (arp_debug_set "rmsd_chunk_atoms")
    int hist2_route = 0;              // arp_debug_set "torsion_hist2_route"
};
struct TorsionOut {
    float *angles = nullptr;           // [F][D], nullable
    double *cossin = nullptr;          // [F][D][2], nullable
    uint8_t *states = nullptr;         // [F][D], nullable
    double *sums = nullptr;            // [D][2]
    uint32_t *n_defined = nullptr;     // [D]
    uint32_t *state_counts = nullptr;  // [D][4]
    uint32_t *n_transitions = nullptr; // [D]
    uint32_t *hist = nullptr;          // [D][B], nullable
    uint32_t *hist2 = nullptr;         // [G][B][B], nullable
};
// The resident device bytes of arp_torsions that "rmsd_cap_bytes" limits: the state bytes, the slab sums and the two histograms (torsion.inl kTorsionSlab = 32).
inline uint64_t torsion_resident_bytes(uint64_t F, uint64_t D, uint64_t B, uint64_t G, bool hist, bool hist2) {
    return F * D + (F + 31u) / 32u * D * 16u + (hist ? D * B * 4u : 0u) + (hist2 ? G * B * B * 4u : 0u);
}
arp_status device_torsions(arp_context *ctx, const TorsionJob &job, TorsionOut *out);

// engine.cpp: the context's stream / device and grow-only scratch (device and pinned host)
void *context_stream(arp_context *ctx);
int context_device(arp_context *ctx);
// engine.cpp: the table path's pair pass -- device-resident inputs, *data = a view of the context's own pair buffer (valid until its next call)
arp_status contacts_atomic_view(arp_context *ctx, const arp_atoms *atoms, const arp_params *params, const arp_pair **data, uint64_t *n);
struct GridParams;
struct Fat;
// the cell list the most recent pair pass of this context built -- valid only if that pass ran on exactly these arrays (x, n)
bool context_grid(arp_context *ctx, const double *x, uint64_t n, const GridParams **grid, const uint32_t **cell_start, const Fat **fat);
arp_status context_scratch(arp_context *ctx, int slot, uint64_t dev_bytes, uint64_t pinned_bytes, char **dev, char **pinned);  // slot 0 / 1: two independent grow-only blocks

}  // namespace arp
