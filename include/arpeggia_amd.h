/*
 * arpeggia_amd.h -- C ABI of the MI355X-native contact engine (libarpeggia_amd.so).
 *
 * Drop-in boundary for ONE path of y1zhou/arpeggia v0.8.0: `arpeggia::get_contacts`
 * (src/contacts/mod.rs:61, re-exported src/lib.rs:28) and, inside it, the hot loop
 * `Interactions::get_atomic_contacts` (src/contacts/complex.rs:189-299).  The reference has no FFI of its
 * own (pure Rust); these are the entry points a Rust `extern "C"` block / ctypes stub binds -- see
 * INTEGRATION.md for the exact reference-side stubs.  Plain pointers and sizes only, no torch/HIP types:
 * a HIP stream crosses as `void*`.
 *
 * Every function returns an arp_status and never unwinds across the boundary (the reference panics instead:
 * utils.rs:77,109; complex.rs:50; vdw.rs:58-69).  arp_last_error() gives the thread-local message, which
 * reproduces the reference's panic strings where its tests pin them (utils.rs:215,223).
 */
#ifndef ARPEGGIA_AMD_H
#define ARPEGGIA_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ARP_API_VERSION 2   /* v2 (round 4): arp_atoms.chain_rank and arp_atoms.model are 32-bit (v1: uint16_t, at most 65 535 chains / models) */

typedef int32_t arp_status;
enum {
    ARP_OK = 0,
    ARP_ERR_BAD_GROUPS = 1,   /* utils.rs:77  "Invalid chain groups format! Use '/' for all-to-all comparisons." */
    ARP_ERR_EMPTY_GROUPS = 2, /* utils.rs:109 "Empty chain groups!" */
    ARP_ERR_NO_RINGS = 3,     /* complex.rs:50 "Error building ring positions" (no HIS/PHE/TYR/TRP ring at all) */
    ARP_ERR_BAD_INPUT = 4,    /* malformed arrays / unsupported element / CYS without CB (vdw.rs:58 unwrap) ... */
    ARP_ERR_HIP = 5,          /* a HIP runtime call failed */
    ARP_ERR_OOM = 6,
    ARP_ERR_NO_DEVICE = 7,    /* no gfx950 device visible: the engine has NO CPU fallback */
    ARP_ERR_IO = 8,
    ARP_ERR_CAPACITY = 9      /* caller-provided pair buffer too small; required size reported */
};

/* ---- interaction vocabulary: bit k of arp_pair.kind <=> variant k of the reference enum (structs.rs:6-51) ---- */
enum {
    ARP_StericClash = 0, ARP_CovalentBond, ARP_Disulfide, ARP_VanDerWaalsContact, ARP_IonicBond, ARP_HydrogenBond,
    ARP_WeakHydrogenBond, ARP_PolarContact, ARP_WeakPolarContact, ARP_IonicRepulsion, ARP_SaltBridge,
    ARP_PiDisplacedStacking, ARP_PiTStacking, ARP_PiSandwichStacking, ARP_PiParallelInPlaneStacking,
    ARP_PiTiltedStacking, ARP_PiLStacking, ARP_CationPi, ARP_HydrophobicContact, ARP_N_INTERACTIONS
};
/* A row code of the ensemble tables only (ARP_FREQ_WATERS below), never a bit of arp_pair.kind and not a variant of the reference enum: it stays
 * outside the enum, ARP_N_INTERACTIONS stays 19, and arp_interaction_name returns "WaterBridge" for it. */
#define ARP_WaterBridge 19

/* ---- per-atom attribute word (arp_atoms.attr) ---- */
#define ARP_ATTR_ELEM_MASK   0x0000000Fu /* element class: index into arp_params.cov_radius / vdw_radius            */
#define ARP_ATTR_DONOR       0x00000010u /* hbond.rs:160-178 is_hydrogen_donor (conformer name, atom name)          */
#define ARP_ATTR_ACCEPTOR    0x00000020u /* hbond.rs:137-157 is_hydrogen_acceptor                                    */
#define ARP_ATTR_WEAK_DONOR  0x00000040u /* hbond.rs:204-207 element C and name != "C"                               */
#define ARP_ATTR_POS         0x00000080u /* ionic.rs:84-91 (conformer name)                                          */
#define ARP_ATTR_NEG         0x00000100u /* ionic.rs:94-99                                                           */
#define ARP_ATTR_HYDROPHOBIC 0x00000200u /* hydrophobic.rs:27-45 (residue name)                                      */
#define ARP_ATTR_CYS_SG      0x00000400u /* vdw.rs:50-53: residue CYS and atom SG                                    */
#define ARP_ATTR_H           0x00000800u /* element H: never a candidate (complex.rs:83-87,201), only an H-bond probe */
#define ARP_ATTR_LIGAND      0x00001000u /* chain in the ligand set   (utils.rs:71-115)                              */
#define ARP_ATTR_RECEPTOR    0x00002000u /* chain in the receptor set                                                */
#define ARP_ATTR_POS_RESN    0x00004000u /* ionic.rs:84-91 keyed by RESIDUE name (cation-pi, aromatic.rs:18)         */

#define ARP_NONE 0xFFFFFFFFu

enum { ARP_MEM_HOST = 0, ARP_MEM_DEVICE = 1 };

/* SoA view of one structure, borrowed for the duration of a call (the reference borrows &PDB: mod.rs:61).
 * All arrays have n entries unless noted.  `location` says where EVERY pointer lives. */
typedef struct arp_atoms {
    uint64_t n;                  /* atoms, hydrogens included                                                 */
    const double *x, *y, *z;     /* f64 coordinates (pdbtbx Atom::pos)                                        */
    const uint32_t *attr;        /* ARP_ATTR_* bits                                                           */
    const uint32_t *res_ord;     /* positional index of the residue in its chain (complex.rs:411-440)         */
    const uint32_t *chain_rank;  /* rank of the chain id under byte-wise string order (complex.rs:129); the reference keys on the id
                                  * STRING (complex.rs:19-21): any number of chains                                     */
    const uint32_t *model;       /* model ordinal 0, 1, 2, ... (complex.rs:96-98 same-model test); dense: every model owns a
                                  * slab of the cell grid, the largest ordinal is bounded by the grid (~4 per atom)             */
    /* tables for the rare data-dependent rules; may be NULL when n_res == 0 (then no H probes, no disulfides) */
    const uint32_t *res_id;      /* per atom: global residue ordinal                                          */
    uint64_t n_res;
    const uint32_t *res_h_ptr;   /* n_res+1: CSR residue -> hydrogen atoms (hbond.rs:38-42 scans the residue) */
    const uint32_t *res_h_idx;   /* atom indices of the hydrogens                                             */
    const uint32_t *res_cb;      /* n_res: first CB of the residue or ARP_NONE (vdw.rs:55-58)                 */
    const uint32_t *res_sg;      /* n_res: first SG of the residue or ARP_NONE (vdw.rs:59-63)                 */
    int32_t location;            /* ARP_MEM_HOST | ARP_MEM_DEVICE                                             */
    int32_t reserved;
} arp_atoms;

/* arp_params.flags.  By default pairs are emitted in one pass in an unspecified order (like the reference, whose order is
 * that of an R*-tree walk + rayon, complex.rs:194-298).  DETERMINISTIC selects the two-pass count/scan/fill emitter
 * whose output order is a function of the input only (about 2x slower: 0.54 against 0.26 ms on 10^6 atoms).
 * CONTACTS_ONLY drops the candidates no rule matched (kind == 0) on the device: what is left is exactly the set of
 * pairs get_atomic_contacts turns into ResultEntry rows (complex.rs:208-297), typically 5-10% of the candidates, so the
 * copy to the host and the table assembly shrink by that factor.  arp_get_contacts uses it. */
#define ARP_FLAG_DETERMINISTIC 0x1u
#define ARP_FLAG_CONTACTS_ONLY 0x2u
/* NO_SPECULATION (arp_contacts_atomic_enqueue): the single-pass emitter normally skips the launch of the probe pass (hydrogen-bond angles,
 * disulfide dihedrals) when the previous call on the same arrays needed none, checks the guess on the device, and lets
 * arp_contacts_atomic_result repeat the whole call when the guess was wrong -- until then the records a probe decides sit in `out` with
 * kind 0 (inputs below ~20 000 atoms run their probes inside the emitter: nothing is speculated there; between ~20 000 and ~131 000 atoms the same
 * guess also selects a launch sequence without the hole fix-up -- if it was wrong nothing of that call's output is valid until the repeat has run).  With this flag the probe pass is always launched behind the emitter, on the same stream: work the caller orders on that stream
 * after the enqueue sees final records.  (One repeat remains possible, for either setting: a deferred-probe list that overflows -- an input
 * with more than ~16 probe candidates per atom -- is grown by arp_contacts_atomic_result and the call run again; it then returns only after
 * the repeat, and what ran on the stream in between has seen an incomplete list.  ARP_FLAG_DETERMINISTIC never speculates.) */
#define ARP_FLAG_NO_SPECULATION 0x4u
/* RESIDUE_RUNS / NO_RESIDUE_RUNS: a hint about the input, never a change of the result.  The reference never pairs two atoms of one residue or
 * of sequence neighbours in one chain (complex.rs:108-113); in an input whose residues are runs of atoms (every protein) a third of an atom's
 * geometric neighbours are such atoms, and the single-pass emitter has kernels that drop them before the exact phase.  They cost a little on an
 * input of one-atom residues (a synthetic cloud), so the engine picks them from a sample of the PREVIOUS call's atoms on the same context
 * (how many of the first 255 atoms continue their predecessor's residue).  RESIDUE_RUNS asks for them outright (a first call, mixed workloads),
 * NO_RESIDUE_RUNS rules them out.  Both kernels emit the same list. */
#define ARP_FLAG_RESIDUE_RUNS 0x8u
#define ARP_FLAG_NO_RESIDUE_RUNS 0x10u

typedef struct arp_params {
    double vdw_comp;             /* mod.rs:61 vdw_comp    (default 0.1) */
    double dist_cutoff;          /* mod.rs:61 dist_cutoff (default 6.5) */
    double cov_radius[16];       /* by element class: pdbtbx covalent_single  (vdw.rs:24-28) */
    double vdw_radius[16];       /* by element class: pdbtbx van_der_waals                   */
    double h_vdw_radius;         /* Element::H van_der_waals (hbond.rs:52)                   */
    uint32_t flags;              /* ARP_FLAG_* */
    uint32_t reserved;
} arp_params;

/* One classified candidate pair = one element of `ligand_neighbors` (complex.rs:194-213) after the per-pair
 * rules (complex.rs:215-298).  i = ligand atom x, j = receptor atom y (indices into arp_atoms).  Pairs with
 * kind == 0 are candidates that produced no row. */
typedef struct arp_pair {
    uint32_t i, j;
    float dist;                  /* (f32) Atom::distance, as the table stores it (mod.rs:148) */
    uint32_t kind;               /* bit set over ARP_* interaction codes */
} arp_pair;

typedef struct arp_pairs {
    uint64_t n;
    arp_pair *data;              /* owned by the library until arp_pairs_free */
    int32_t location;            /* where data lives */
    int32_t reserved;
} arp_pairs;

typedef struct arp_context arp_context;     /* one per (device, stream); owns the reusable workspace */
typedef struct arp_structure arp_structure; /* parsed + filtered model (utils.rs:51-63 load_model)   */
typedef struct arp_table arp_table;         /* the 20-column contact table (mod.rs:140-214)          */

/* ---- library / device ---- */
/* Diagnostics -- not part of the reference's surface.  The library reads ONE environment variable, ARPEGGIA_AMD_HOST_POOL_MB (idle pinned host
 * memory kept for the next batch / table, default 4096); every other switch is set here, process-wide:
 *   "timing"        1: stage laps of the table, batch and ingest paths on stderr
 *   "emit_kernel"   1: the single-pass emitter runs its alternative kernel (both operands gathered; the route of inputs beyond 2^24 slots), so that
 *                      the parity suite can check it on ordinary inputs; 0 (default): chosen by input size
 *   "defer_entries" N > 0: entries of the deferred-probe list of workspaces allocated from now on (a tiny list makes the grow-and-repeat path run)
 *   "strip_rows"    N = a power of two: the cell rows of single-model inputs are ordered in y strips of N rows (chosen by input size when 0, the default:
 *                      strips only from ~2.5 x 10^6 atoms of a compact structure on), for parameter blocks built from now on -- lets the parity suite run the strip order on small inputs
 *   "index_bits"    the narrow (32-byte) exact record of the single-pass emitter: 0 (default): its index width follows the input size; N = 1 .. 20: N index bits
 *                      (an input whose last index does not fit them keeps the wide record); N < 0: the wide record always.  Same list either way -- lets the
 *                      suite run the wide-index fallback on small inputs
 *   "scan_kernel"   the scan of the cell counts: 0 (default): chosen by input size; 1: the look-back scan of large inputs on 256 blocks; 2: the same on
 *                      1024 blocks (the shape of packs and of inputs beyond 2^20 atoms).  Same grid either way -- lets the suite run it on small inputs
 *   "table_host"    1: only in the test library built with -DARP_WITH_HOST_TABLE (tests/hosttable): arp_get_contacts assembles the table on the host
 *   "freq_chunk_atoms" N > 0: arp_contact_frequencies runs its frames in passes of N atoms (whole frames, at least one per pass), so that tests can
 *                      force several passes; 0 (default): about 2 x 10^6 atoms per pass
 *   "freq_cap_items" N > 0: the first buffers of arp_contact_frequencies hold N items (aggregate + one pass's items) instead of max(65536, 2 x pairs),
 *                      so that tests can make the grow-and-repeat path run; 0 (default): automatic
 *   "freq_frame_bits" k in 1 .. 17: the device keys of arp_residue_contact_frequencies carry k frame bits, so a pass holds at most 2^k - 1 frames and
 *                      tiny inputs reach the frame cap; 0 (default): automatic (17, fewer only beyond 2^21 residues)
 *   "ens_chunk_atoms" N > 0: arp_sasa_ensemble runs its frames in passes of N packed atoms (frames x selected atoms; whole frames, at least one per
 *                      pass), so that tests can force several passes; 0 (default): about 2 x 10^6 atoms per pass
 *   "sc_ens_frames" N in 1 .. 2^20: arp_sc_ensemble runs N whole frames per pass, so that tests reach pass edges at tiny shapes; 0 (default): as many
 *                      as the pass's memory budget allows.  The results do not depend on it
 *   "timeline_cap_bytes" N > 0: arp_contact_timelines refuses a device bitmap of more than N bytes (ARP_ERR_CAPACITY), so that tests reach the limit on
 *                      tiny inputs; 0 (default): 2^31 bytes
 *   "similarity_cap_bytes" N > 0: arp_contact_similarity and arp_bit_gram refuse a matrix of more than N bytes (ARP_ERR_CAPACITY), so that tests reach
 *                      the limit on tiny inputs; 0 (default): 2^31 bytes
 *   "autocorr_cap_bytes" N > 0: arp_contact_autocorrelation and arp_bit_autocorr refuse a device matrix of more than N bytes (ARP_ERR_CAPACITY), so that
 *                      tests reach the limit on tiny inputs; 0 (default): 2^31 bytes
 *   "cluster_cap_bytes" N > 0: arp_contact_clusters and arp_bit_cluster refuse neighbour bits, or cluster counts, of more than N bytes (ARP_ERR_CAPACITY), so
 *                      that tests reach the limit on tiny inputs; 0 (default): 2^31 bytes
 *   "rmsd_chunk_atoms" N > 0: the arp_rmsd_* calls upload their frames in passes of N atoms (whole frames, at least one per pass), so that tests can force
 *                      several passes; 0 (default): about 2 x 10^6 atoms per pass.  The results do not depend on it
 *   "rmsd_cap_bytes" N > 0: arp_rmsd_matrix refuses a matrix, arp_rmsd_clusters neighbour bits, and every arp_rmsd_* call packed coordinates of more than N
 *                      bytes (ARP_ERR_CAPACITY), so that tests reach the limit on tiny inputs; 0 (default): 2^31 bytes
 *   "table_key_bits" N in 6 .. 64: N stands for the 64 bits of the key word when the contact table chooses its sort passes (one merged key, two or three
 *                      passes) and decides whether the one-launch path may run, so that small inputs reach the plans of wide keys; the passes themselves sort
 *                      on their real widths, and the table's bytes do not change.  0 (default): 64.  Anything else is ARP_ERR_BAD_INPUT (6 is the narrowest pass any structure can
 *                      have, not the widest pass of the structure at hand: the knob is set before a structure is known, and a value below a real pass is harmless)
 *   "torsion_hist2_route" how arp_torsions adds up its Ramachandran maps: 0 (default) per-workgroup LDS tables where n_groups x n_bins^2 x 4 bytes fit 64 KiB,
 *                      wave-matched global adds otherwise; 1 the LDS tables where they fit; 2 the wave-matched adds always; 3 one global add per sample
 *                      (measurements).  The results do not depend on it
 * Unknown keys return ARP_ERR_BAD_INPUT. */
arp_status arp_debug_set(const char *key, int64_t value);
/* The read-only twin: what the last contact-table call of the process (arp_get_contacts) did.
 *   "table_small"     the one-launch path: -1 not tried (more than 2048 pairs), 0 it finished the table, 1 / 2 / 3 it gave up (more than 4096 rows / a run of
 *                     64 or more rows with equal sort keys / more ring rows than reserved, after the one repeat) and the general path ran, 4 not tried
 *                     because the keys and a row index do not fit one word
 *   "table_pairs"     contact pairs the table was built from;  "table_atom_rows" / "table_ring_rows"  its rows
 *   "table_plan"      the radix passes of the general path as decimal digits: 6, 25 or 234; 0 when it did not sort
 *   "table_long_way"  1: the general path sorted a second time with the tie-breaking keys as passes of their own
 *   "table_ring_cap"  ring rows reserved when the call ended (64 x rings + 1024, or what the counter reported when that was too few)
 * Unknown keys return ARP_ERR_BAD_INPUT. */
arp_status arp_debug_get(const char *key, int64_t *value);
int32_t arp_api_version(void);
/* A binder compiled against this header calls arp_check_api_version(ARP_API_VERSION) once: ARP_OK when the library lays out arp_atoms /
 * arp_params / arp_pair as that version of the header does, ARP_ERR_BAD_INPUT (+ arp_last_error) otherwise -- a v1 caller (16-bit chain
 * ranks and models) would otherwise hand over arrays the v2 kernels read 4 bytes per atom. */
arp_status arp_check_api_version(int32_t header_version);
const char *arp_strerror(arp_status s);
const char *arp_last_error(void);
int32_t arp_device_count(void);             /* gfx950 devices visible; 0 => every compute call fails with ARP_ERR_NO_DEVICE */
const char *arp_interaction_name(int32_t code); /* structs.rs:151-157 Display == variant name */
void arp_default_params(arp_params *p);     /* 0.1 / 6.5 and the radii of the built-in element classes */
int32_t arp_element_class(const char *symbol); /* class index used by arp_default_params, -1 if unsupported */

/* ---- context ---- */
arp_status arp_context_create(int32_t device, arp_context **out);
void arp_context_destroy(arp_context *ctx);
/* Launch on a caller-owned HIP stream (hipStream_t passed as void*; NULL = the legacy default stream).  A new context
 * starts on a private non-blocking stream of its own. */
arp_status arp_context_set_stream(arp_context *ctx, void *hip_stream);
arp_status arp_context_synchronize(arp_context *ctx);

/* ---- the hot path: replaces Interactions::get_atomic_contacts (complex.rs:189-299) ---- */
/* Synchronous.  Inputs may be host or device arrays; output is library-allocated where `out_location` says. */
arp_status arp_contacts_atomic(arp_context *ctx, const arp_atoms *atoms, const arp_params *params,
                               int32_t out_location, arp_pairs *out);
void arp_pairs_free(arp_pairs *pairs);

/* Asynchronous, allocation-free form for resident data (inputs MUST be ARP_MEM_DEVICE): enqueues the whole
 * pipeline on the context's stream and returns.  `out` is a device buffer of `capacity` pairs.
 * arp_contacts_atomic_result() synchronises the stream and returns the pair count (ARP_ERR_CAPACITY + the required
 * count when the buffer was too small; nothing is written past `capacity`).
 * CONTRACT: the contents of `out` (and the count) are DEFINED ONLY AFTER arp_contacts_atomic_result HAS RETURNED ARP_OK.  Between the
 * two calls the buffer is speculative: the result call may run the enqueued work a second time (see ARP_FLAG_NO_SPECULATION), so
 * stream work ordered between enqueue and result must not consume `out` unless that flag is set -- and `atoms`, `params`' arrays and
 * `out` must stay alive and unchanged until the result call returns. */
arp_status arp_contacts_atomic_enqueue(arp_context *ctx, const arp_atoms *atoms, const arp_params *params,
                                       arp_pair *out, uint64_t capacity);
arp_status arp_contacts_atomic_result(arp_context *ctx, uint64_t *n_pairs);

/* Batch of independent structures sharded over devices (no collective).  ctxs[d] is a context on
 * device d; structure k goes to a device by longest-processing-time-first on its atom count; one host thread
 * per device; with ARP_FLAG_CONTACTS_ONLY small structures of a device's share are packed into shared launches.
 * outs[k] is filled like arp_contacts_atomic (host memory).  The lists of structures that shared a pack are views into ONE pinned block
 * (one PCIe copy per pack, no copy per member): release every outs[k] with arp_pairs_free as usual -- the block is reference-counted and
 * goes back to a pool when its last list is freed; do not free() the pointers yourself. */
arp_status arp_contacts_atomic_batch(arp_context *const *ctxs, int32_t n_ctx, const arp_atoms *const *atoms,
                                     int32_t n_structures, const arp_params *params, arp_pairs *outs);
/* Pinned host blocks whose last pair list or table has been freed are kept for the next batch / table (pinning memory costs far more than
 * the copy it saves; at most 4 GiB stay pooled -- ARPEGGIA_AMD_HOST_POOL_MB in the environment sets another limit, 0 keeps nothing -- and a
 * request only reuses a pooled block of at most twice its size).  This returns the idle ones to the system; blocks still referenced are untouched.
 * Returns the number of bytes released. */
uint64_t arp_release_host_pool(void);

/* ---- SAP neighbour sum: the radius sum of src/sap.rs:155-204 on the same cell list ----
 * out[i] = sum over the atoms j with sidechain[j] != 0 and |r_j - r_i|^2 <= f64(sap_radius * sap_radius) (inclusive, i itself included) of
 * weight[j], accumulated in f32, for every atom i with sidechain[i] != 0; 0 for the others.  Host arrays.  The per-atom SASA behind the
 * weights (src/sasa.rs, rust-sasa) is the caller's: arp_sap_weight gives hydrophobicity(resn) * clamp(sasa / max_sc_asa(resn), 0, 1) as the
 * reference forms it (sap.rs:41-101,198-209). */
float arp_sap_weight(const char *resn, float sasa);
arp_status arp_sap_neighbor_sum(arp_context *ctx, uint64_t n, const double *x, const double *y, const double *z,
                                const uint8_t *sidechain, const float *weight, float sap_radius, float *out);

/* ---- atom SASA: Shrake-Rupley on the same cell list (reference src/sasa.rs:174-247, get_atom_sasa through rust-sasa) ----
 * Numerical contract (DESIGN.md "Atom SASA"; tests/sasa_restatement.py restates it in numpy bit for bit):
 *   inputs as the reference casts them (sasa.rs:193-210): c_i = f32 coordinates, R_i = f32(radius_i + probe) with radius_i the f32
 *   pdbtbx van_der_waals radius (arp_params.vdw_radius of the element class at the structure level);
 *   sphere points s_k, k < n_points: arp_sasa_sphere_points (golden spiral, computed in f64 and rounded to f32 -- believed to be rust-sasa's
 *   formula; that crate is not part of the reference's tree, so this is an assumption);
 *   point k of atom i is BURIED iff some other selected atom j (self excluded by index) has d^2 < R_j^2 (strict), where
 *   d^2 = tx^2 + ty^2 + tz^2 evaluated left to right in f64 without contraction, t = (c_i - c_j) + s_k R_i per axis from the f32 values;
 *   count_i = number of points not buried (exact integer); sasa_i = f32(((4 pi R_i) R_i count_i) / n_points) evaluated in f64.
 * n_points must be 1..ARP_SASA_MAX_POINTS and probe finite and >= 0, else ARP_ERR_BAD_INPUT (so is a radius that is not finite and >= 0). */
#define ARP_SASA_MAX_POINTS 4096
/* xyz: 3 n floats, the unit vectors of the contract. */
arp_status arp_sasa_sphere_points(uint32_t n, float *xyz);
/* Raw arrays (host), like arp_sap_neighbor_sum.  include[i] != 0 selects atom i (NULL: all); the others neither bury nor get a value
 * (sasa 0, count 0).  out_count may be NULL.  Synchronous. */
arp_status arp_atom_sasa(arp_context *ctx, uint64_t n, const double *x, const double *y, const double *z, const float *radius,
                         const uint8_t *include, float probe, int32_t n_points, float *out_sasa, int32_t *out_count);
/* Diagnostics: f32 distance tests (point x list entry) the kernel of the most recent SASA call on ctx made. */
uint64_t arp_sasa_tests(const arp_context *ctx);
/* Diagnostics: how many 64-pair batches of the most recent collected pair pass on ctx decided their pair filter on the residue ordinals and chain
 * ranks read from the input arrays instead of on the tags of the narrow exact record (0 when the pass ran on the wide record).
 * (A diagnostics entry point like arp_sasa_tests: ARP_API_VERSION names the layout of arp_atoms / arp_params / arp_pair and does not move.) */
uint64_t arp_pair_rare_batches(const arp_context *ctx);

/* Structure level.  The atom selection is the reference's prepare_pdb_for_sasa + filter_pdb_by_model (sasa.rs:27-135, 183-195), in order:
 *   1. chains: a comma-separated list, entries trimmed, empty entries dropped; empty = all chains;
 *   2. remove_hydrogens: drop element H;
 *   3. drop whole residues named HOH H2O D2O WAT TIP TIP3 TIP4 SPC NA CL K CA MG ZN FE MN CU CO NI CD SO4 PO4 NO3 ACE NH2;
 *   4. only when the structure has more than one model: keep the model whose serial is model_num (the first one for 0 or no match);
 *   5. keep the atoms whose MODEL serial equals model_num.
 * Step 5 is the reference's quirk, kept on purpose: a file with MODEL 1..N records and the default model_num 0 selects NO atom, and
 * model_num 1 on a file without MODEL records (serial 0) selects none either.
 * out_atoms (n_atoms entries, arp_structure_n_atoms) receives the selected structure atom indices in structure order. */
arp_status arp_structure_sasa_select(const arp_structure *s, const char *chains, int32_t model_num, int32_t remove_hydrogens,
                                     uint64_t *n_out, uint32_t *out_atoms);
/* get_atom_sasa (sasa.rs:174): one row per selected atom, sorted by serial number (atomi; structure order among equal serials).
 * Every out_* array holds arp_structure_n_atoms(s) entries (an upper bound); *n_rows says how many were written.  out_count may be NULL. */
arp_status arp_structure_atom_sasa(arp_context *ctx, const arp_structure *s, const char *chains, int32_t model_num, int32_t remove_hydrogens,
                                   float probe, int32_t n_points, uint64_t *n_rows, uint32_t *out_atoms, float *out_sasa, int32_t *out_count);
/* get_per_atom_sap_score (sap.rs:137-259): SASA, weights and the neighbour sum on one stream with one synchronisation.  The rows are the
 * atom-SASA rows (above, hydrogens removed) whose serial is that of a non-backbone atom of the whole structure; sap = the f32 sum, over the
 * side-chain atoms of the structure after steps 1-3 (NO model filter, all models) within sap_radius (inclusive) of the row's atom with that
 * serial, of arp_sap_weight(resn, atom SASA of the neighbour's serial), 0 for a neighbour whose serial has no SASA row.  Backbone = atom
 * names N CA C O OXT (pdbtbx's is_backbone; an assumption).  Arrays and *n_rows as arp_structure_atom_sasa. */
arp_status arp_structure_sap_score(arp_context *ctx, const arp_structure *s, const char *chains, int32_t model_num, float probe,
                                   int32_t n_points, float sap_radius, uint64_t *n_rows, uint32_t *out_atoms, float *out_sasa, float *out_sap);
/* get_dsasa (sasa.rs:400-451) from ATOM-level SASA: groups are parsed as arp_get_contacts does (its errors); each of complex (both groups),
 * group 1 and group 2 is selected by steps 2-4 above (no step 5: the reference sums chain-level SASA here) and the three run as three
 * models of one grid in one launch.  *out = f32(g1 + g2 - complex) of the three f32 totals (each summed in f64, rounded once); no halving.
 * A negative result is written and ARP_ERR_BAD_INPUT returned (python.rs:177-188 raises). */
arp_status arp_structure_dsasa(arp_context *ctx, const arp_structure *s, const char *groups, float probe, int32_t n_points, int32_t model_num,
                               float *out);

/* ---- residue- and chain-level SASA, relative SASA, segment sums -- DESIGN.md section 3.9 ----
 * Radius tables.  ARP_RADII_VDW: the element's van der Waals radius (arp_params.vdw_radius), what arp_structure_atom_sasa, arp_structure_dsasa
 * and arp_sasa_ensemble use.  ARP_RADII_PROTOR: the ProtOr radii of Tsai et al. 1999 by (residue name, atom name), then (ANY, atom name) for the
 * backbone and CB, then the element's van der Waals radius.  The reference computes its residue and chain levels through rust-sasa with
 * with_allow_vdw_fallback(true); ProtOr is the table that reproduces the reference's own chain-level pin on 1ubq (4813 A^2).  ASSUMPTIONS, since
 * rust-sasa is not part of the reference's tree: which element table its fallback uses (here: arp_params.vdw_radius); its list of polar residues
 * (here: ARG ASN ASP GLN GLU HIS LYS SER THR TYR); its rule that "only the first altloc is considered" at the residue level (not restated: all
 * selected atoms take part, as at the atom level and in arp_structure_dsasa). */
#define ARP_RADII_VDW 0
#define ARP_RADII_PROTOR 1
/* *out = the radius in f32 (the probe is added in f32 by the callers).  The residue name is matched case-insensitively, the atom name exactly.
 * ARP_ERR_BAD_INPUT: an unknown table, or no table entry and an element without a van der Waals radius.  Host only. */
arp_status arp_sasa_radius(const char *resn, const char *atomn, const char *element, int32_t table, float *out);
/* MaxASA of Tien et al. 2013 (the reference's get_max_asa, sasa.rs:460-483), residue name matched case-insensitively; 0 = none.  Host only. */
float arp_max_asa(const char *resn);
/* 1 for ARG ASN ASP GLN GLU HIS LYS SER THR TYR (case-insensitive; an assumption, see above), else 0.  Host only. */
int32_t arp_residue_is_polar(const char *resn);
/* Segment sums on the device.  values: rows x m finite, non-negative f32 (host, C order).  n_seg segments as a CSR: seg_start[n_seg + 1]
 * (seg_start[0] = 0, monotone, at most 2^31 - 65 items in all) and seg_item[seg_start[n_seg]], every entry an index below m; a segment lists
 * its items in the order they are added -- they need not be contiguous, ascending or disjoint.
 * out[row][s] (rows x n_seg, host) = f32(acc), acc = 0.0; acc = acc + (double)values[row][seg_item[q]] for q = seg_start[s] .. seg_start[s + 1) - 1
 * in that order, every addition one IEEE f64 round-to-nearest add: the bytes of that sequential chain for every input; an empty segment gives
 * 0.0f.  No atomics: two calls give the same bytes.  rows == 0, n_seg == 0 or m == 0: ARP_OK, nothing written.  ARP_ERR_BAD_INPUT before the
 * device is touched: an item >= m, a seg_start that is not monotone from 0, sizes out of range.  ctx == NULL runs only these checks.  Synchronous. */
arp_status arp_segment_sum(arp_context *ctx, uint64_t rows, uint64_t m, const float *values, uint64_t n_seg, const uint32_t *seg_start,
                           const uint32_t *seg_item, float *out);
/* arp_structure_atom_sasa / arp_structure_dsasa with the radii of `table` (ARP_RADII_VDW: the same bytes as those). */
arp_status arp_structure_atom_sasa_radii(arp_context *ctx, const arp_structure *s, const char *chains, int32_t model_num, int32_t remove_hydrogens,
                                         float probe, int32_t n_points, int32_t table, uint64_t *n_rows, uint32_t *out_atoms, float *out_sasa,
                                         int32_t *out_count);
arp_status arp_structure_dsasa_radii(arp_context *ctx, const arp_structure *s, const char *groups, float probe, int32_t n_points, int32_t model_num,
                                     int32_t table, float *out);
/* get_residue_sasa (sasa.rs:284-318).  Selection: steps 1-4 of arp_structure_sasa_select with hydrogens removed (NO step 5: the reference has no
 * serial filter here).  Per-atom SASA: what arp_atom_sasa gives the selected atoms with the radii of `table`.  One row per residue of the selection
 * -- the atoms sharing the ingest's residue (chain, resi, insertion) --, sasa = the segment sum (above) of its atoms' values in selection order,
 * summed on the device behind the SASA kernel; only the sums come back.  Rows sorted stably by (chain as a byte string, resi, insertion).
 * out_atoms[r]: the first selected atom of the row's residue (its chain, resn, resi and insertion are the row's identity); out_is_polar[r]:
 * arp_residue_is_polar of its residue name (nullable).  Every out_* array holds arp_structure_n_atoms(s) entries (an upper bound). */
arp_status arp_structure_residue_sasa(arp_context *ctx, const arp_structure *s, const char *chains, int32_t model_num, float probe, int32_t n_points,
                                      int32_t table, uint64_t *n_rows, uint32_t *out_atoms, float *out_sasa, uint8_t *out_is_polar);
/* get_chain_sasa (sasa.rs:352-382): the same selection, one row per chain id (a chain need not be one run of the selection), sorted by chain id. */
arp_status arp_structure_chain_sasa(arp_context *ctx, const arp_structure *s, const char *chains, int32_t model_num, float probe, int32_t n_points,
                                    int32_t table, uint64_t *n_rows, uint32_t *out_atoms, float *out_sasa);
/* get_relative_sasa (sasa.rs:520-561, its code: no altloc and no max_sasa column): the residue rows plus out_relative[r] = sasa / arp_max_asa
 * (one f32 division) with out_valid[r] = 1, or NaN with out_valid[r] = 0 (null) where the residue has no MaxASA. */
arp_status arp_structure_relative_sasa(arp_context *ctx, const arp_structure *s, const char *chains, int32_t model_num, float probe, int32_t n_points,
                                       int32_t table, uint64_t *n_rows, uint32_t *out_atoms, float *out_sasa, uint8_t *out_is_polar, float *out_relative,
                                       uint8_t *out_valid);

/* ---- shape complementarity (Lawrence & Colman 1993; reference src/sc/, get_sc) -- DESIGN.md section 3.6 ----
 * Every quantity is f64 and follows the reference's rules and order; sums run in dot order; of two nearest dots at equal distance the
 * lower index wins; same-molecule neighbours at equal distance are ordered by atom index. */
typedef struct arp_sc_settings {
    double probe_radius;       /* rp, 1.7 (must be > 0) */
    double dot_density;        /* dots per A^2, 15 */
    double peripheral_band;    /* A, 1.5 */
    double separation_cutoff;  /* A, 8 */
    double gaussian_w;         /* A^-2, 0.5 */
} arp_sc_settings;
void arp_sc_default_settings(arp_sc_settings *out);
typedef struct arp_sc_surface {
    uint64_t n_atoms, n_buried_atoms, n_far_atoms, n_all_dots, n_trimmed_dots;
    double trimmed_area, d_mean, d_median, s_mean, s_median;
} arp_sc_surface;
typedef struct arp_sc_results {
    arp_sc_surface surface[2];
    arp_sc_surface combined;   /* counts and area: sums; means and medians: midpoints of the two surfaces */
    uint64_t n_convex, n_toroidal, n_concave, n_probes;
    double sc, distance, area; /* combined s_median, d_median, trimmed_area */
} arp_sc_results;
/* The Lawrence & Colman radius of (residue, atom name) from the reference's table (first match, '*' wildcards), else the element's
 * van der Waals radius (arp_params.vdw_radius); 0 when neither exists.  Host only. */
double arp_sc_radius(const char *resn, const char *atomn, const char *element);
/* Raw arrays (host): molecule[i] is 0 or 1; serial NULL = the index (serials must be distinct: the reference keys its maps by them);
 * radius > 0.  settings NULL = the defaults.  Errors (ARP_ERR_BAD_INPUT, arp_last_error holds the reference's text): "No atoms defined",
 * "Failed to read radii: No atoms for chain group 1", "Overlapping atoms detected: ...", "Sampling limit exceeded",
 * "Failed to read radii: No molecular dots generated".  Synchronous. */
arp_status arp_sc(arp_context *ctx, uint64_t n, const double *x, const double *y, const double *z, const double *radius, const uint8_t *molecule,
                  const int64_t *serial, const arp_sc_settings *settings, arp_sc_results *out);
/* get_sc (src/sc/mod.rs:51-80): groups parsed as arp_get_contacts does (its errors); the atoms are steps 1-4 of arp_structure_sasa_select
 * (hydrogens removed, chains = both groups, NO step 5) with molecule 0 for a chain of group 1, else 1; radii from arp_sc_radius (an atom
 * without one is refused).  Duplicate serial numbers among the selected atoms are refused. */
arp_status arp_structure_sc(arp_context *ctx, const arp_structure *s, const char *groups, int32_t model_num, arp_sc_results *out);
/* The selection of arp_structure_sc without running it: out_atoms / out_molecule hold arp_structure_n_atoms(s) entries; *n_out are written. */
arp_status arp_structure_sc_select(const arp_structure *s, const char *groups, int32_t model_num, uint64_t *n_out, uint32_t *out_atoms,
                                   uint8_t *out_molecule);
/* The dots of surface 0 / 1 of the context's last successful SC call, in the reference's order (toroidal by pair (i, j), ring point,
 * side i then j, arc point; then contact by atom, latitude, point; then concave by probe).  *n = the count; the arrays are written when
 * cap >= *n (any may be NULL): xyz and normal 3 per dot; flags = kind | ARP_SC_DOT_BURIED | ARP_SC_DOT_TRIMMED; nn_dist and score are
 * set on trimmed dots (0 elsewhere). */
#define ARP_SC_DOT_CONVEX 0
#define ARP_SC_DOT_TOROIDAL 1
#define ARP_SC_DOT_CONCAVE 2
#define ARP_SC_DOT_BURIED 4
#define ARP_SC_DOT_TRIMMED 8
arp_status arp_sc_dots(arp_context *ctx, int32_t surface, uint64_t cap, uint64_t *n, double *xyz, double *normal, double *area, uint32_t *flags,
                       double *nn_dist, double *score);
/* The owner atom of each of those dots (an index into the atoms of the call), same order and cap convention. */
arp_status arp_sc_dot_atoms(arp_context *ctx, int32_t surface, uint64_t cap, uint64_t *n, uint32_t *atom);

/* ---- shape complementarity across the frames of an ensemble -- DESIGN.md section 3.18 ----
 * F frames of one topology (n atoms; radius, molecule, serial and settings as arp_sc; xyz [F][n][3]) run through the device in passes of whole
 * frames (as many as a memory budget allows; arp_debug_set "sc_ens_frames" fixes the number).  No relation crosses a frame: every frame's
 * dots, flags, distances and scores are those of arp_sc on that frame, bit for bit.  Per frame, results[f] and status[f]:
 *   ARP_SC_FRAME_OK          results[f] as arp_sc fills it.  Integer fields, medians, sc and distance equal arp_sc's; trimmed_area, d_mean,
 *                            s_mean and area are sums of the same terms in another (fixed) order, see arp_sc_dot_stats
 *   ARP_SC_FRAME_NO_DOTS     "No molecular dots generated": atom counts, kind and probe counts and n_all_dots filled, the rest zero
 *   ARP_SC_FRAME_COINCIDENT  "Overlapping atoms detected": err_atoms[2 f], [2 f + 1] (nullable) name the pair arp_sc's message names (indices
 *                            into the n atoms, ~0 for every other frame); atom counts filled, the rest zero
 *   ARP_SC_FRAME_SUBDIV      "Sampling limit exceeded": atom counts filled, the rest zero
 * A frame's status is not a call failure: the call returns ARP_OK when the inputs were valid, and a failed frame leaves the others unchanged.
 * Per atom, over the frames with status OK: frames_in_interface[i] = the frames in which atom i owns a trimmed dot, trimmed_dots[i] = the sum of
 * its trimmed dots.  Input errors (ARP_ERR_BAD_INPUT before any device work): null pointers, n_frames == 0, a non-finite coordinate (the message
 * names the first such frame), and radii, molecule ids, serials and settings as arp_sc refuses them.  ctx == NULL runs only these checks.
 * The dots arp_sc_dots returns are not touched.  Synchronous. */
#define ARP_SC_FRAME_OK 0
#define ARP_SC_FRAME_NO_DOTS 1
#define ARP_SC_FRAME_COINCIDENT 2
#define ARP_SC_FRAME_SUBDIV 3
arp_status arp_sc_ensemble(arp_context *ctx, uint64_t n, uint64_t n_frames, const double *xyz, const double *radius, const uint8_t *molecule,
                           const int64_t *serial, const arp_sc_settings *settings, arp_sc_results *results, uint32_t *status, uint32_t *err_atoms,
                           uint32_t *frames_in_interface, uint64_t *trimmed_dots);
/* The same on a structure: the selection, molecule ids and radii of arp_structure_sc on model 0 (the topology); the frames are xyz, n_frames x
 * N x 3 coordinates of model 0's N atoms, or with xyz == NULL the structure's models (arp_dsasa_ensemble's convention and its topology
 * errors).  *n_rows selected atoms: out_atoms (structure index) and out_molecule hold arp_structure_n_atoms entries at most, as do
 * frames_in_interface and trimmed_dots; results, status and err_atoms (2 per frame, indices into the rows; nullable) hold *frames_used frames.
 * ctx == NULL runs only the checks and writes *n_rows, *frames_used and (when given) out_atoms, out_molecule. */
arp_status arp_structure_sc_ensemble(arp_context *ctx, const arp_structure *topology, uint64_t n_frames, const double *xyz, const char *groups,
                                     uint64_t *n_rows, uint64_t *frames_used, uint32_t *out_atoms, uint8_t *out_molecule, arp_sc_results *results,
                                     uint32_t *status, uint32_t *err_atoms, uint32_t *frames_in_interface, uint64_t *trimmed_dots);
/* The statistics kernel of the ensemble call on the caller's dot columns (host arrays), and its host restatement: the twins are bit-identical.
 * Segment s holds the dots [seg_start[s], seg_start[s + 1]) (seg_start[0] = 0); a dot counts when flags has ARP_SC_DOT_TRIMMED.  out[s]:
 * n_all_dots = the segment's length, n_trimmed_dots = k, trimmed_area, and -- zero when k = 0 or segment other[s] has no trimmed dot --
 * d_mean, s_mean (= -(sum of -score) / k), d_median and s_median = element k / 2 in ascending order of the trimmed dots' nn_dist / score (no
 * averaging; -0 sorts before +0).  Each sum is taken in a fixed order that depends on the segment alone: lane t of 256 adds the trimmed dots at
 * positions t, t + 256, ... of the segment in increasing position, starting from +0; the 256 partial sums are folded p[t] += p[t + h] for
 * h = 128, 64, ..., 1.  The atom counts of out[s] are zero. */
arp_status arp_sc_dot_stats_host(uint64_t n_seg, const uint64_t *seg_start, const uint32_t *flags, const double *area, const double *nn_dist,
                                 const double *score, const uint32_t *other, arp_sc_surface *out);
arp_status arp_sc_dot_stats(arp_context *ctx, uint64_t n_seg, const uint64_t *seg_start, const uint32_t *flags, const double *area,
                            const double *nn_dist, const double *score, const uint32_t *other, arp_sc_surface *out);

/* Per-kernel device timing of the most recent call (HIP events on the context's stream).  Enable, run, then read.
 * names[k] points to a static string.  Returns the number of kernels recorded (<= cap). */
arp_status arp_profile_enable(arp_context *ctx, int32_t on);
int32_t arp_profile_read(arp_context *ctx, const char **names, float *milliseconds, int32_t cap);

/* ---- structure ingest: replaces utils.rs:51-63 load_model (+ python.rs:45-47) ---- */
arp_status arp_structure_load(const char *path, int32_t ignore_zero_occupancy, arp_structure **out);
/* Build from flat per-atom records (fixed-width, NUL-padded strings).  hierarchy == 0: derive the
 * Model>Chain>Residue>Conformer hierarchy the way pdbtbx does and apply the load_model residue filter.
 * hierarchy == 1: take res_ord / res_id as given (synthetic SoA inputs). */
typedef struct arp_records {
    uint64_t n;
    const double *x, *y, *z, *occupancy;
    const int32_t *serial, *resi, *model_serial;
    const char *name;      /* n x 8  atom name          */
    const char *resn;      /* n x 8  conformer name     */
    const char *chain;     /* n x 8  chain id           */
    const char *altloc;    /* n x 4                     */
    const char *icode;     /* n x 4  insertion code     */
    const char *element;   /* n x 4                     */
    const uint32_t *res_ord; /* hierarchy == 1 only */
    const uint32_t *res_id;  /* hierarchy == 1 only */
} arp_records;
arp_status arp_structure_from_records(const arp_records *rec, int32_t hierarchy, arp_structure **out);
void arp_structure_free(arp_structure *s);
uint64_t arp_structure_n_atoms(const arp_structure *s);
/* Host SoA view for a given chain grouping (utils.rs:71-115 parse_groups sets the LIGAND/RECEPTOR bits).
 * The view stays valid until the next arp_structure_atoms call on `s` or arp_structure_free. */
arp_status arp_structure_atoms(arp_structure *s, const char *groups, arp_atoms *view);
/* Per-atom identity columns, n x width fixed-width strings / n ints (valid while `s` lives). */
const char *arp_structure_strings(const arp_structure *s, const char *column, int32_t *width);
const int32_t *arp_structure_ints(const arp_structure *s, const char *column);

/* Host worker threads of the table path (entity bookkeeping, copies out of pinned memory, column / Arrow materialisation -- the plane
 * fits, ring rows, row assembly and sort run on the device): the reference's global rayon pool (utils.rs:8-30; `num_threads` of
 * python.rs:31).  1 = serial (default, as in the reference), 0 = all hardware threads.  The table is identical for every count. */
void arp_set_num_threads(int32_t n);
int32_t arp_get_num_threads(void);

/* ---- the table: replaces arpeggia::get_contacts (mod.rs:61-137) ----
 * The structure is kept resident on the context's device (uploaded once, with its fitted planes and entity ranks); calls on ONE
 * arp_structure are serialised inside the library, different structures (on different contexts) run in parallel. */
arp_status arp_get_contacts(arp_context *ctx, arp_structure *s, const char *groups, double vdw_comp,
                            double dist_cutoff, arp_table **out);
/* The same with the host worker count of THIS call given explicitly (the reference sizes a scoped rayon pool per call,
 * utils.rs:8-30): num_threads > 0 that many, 0 all hardware threads, < 0 the process-wide default of arp_set_num_threads.
 * Concurrent calls with different counts do not interfere. */
arp_status arp_get_contacts_mt(arp_context *ctx, arp_structure *s, const char *groups, double vdw_comp,
                               double dist_cutoff, int32_t num_threads, arp_table **out);
/* The ring / side-chain planes as the device fits them (residues.rs:270-298), per residue of the filtered model in
 * hierarchy order: planes = n_residues x 12 doubles {ring centre, ring normal, sc centre, sc normal}; valid[r] bit 1 = the residue has a
 * ring plane, bit 2 = a side-chain plane. */
uint64_t arp_structure_n_residues(const arp_structure *s);
arp_status arp_structure_fit_planes(arp_context *ctx, arp_structure *s, double *planes, uint8_t *valid);
void arp_table_free(arp_table *t);
uint64_t arp_table_rows(const arp_table *t);
/* Column by reference name (mod.rs:140-181,209-211): "model" u32; "interaction" i32 code; "distance" f32;
 * "from_resi"/"from_atomi"/"to_resi"/"to_atomi" i32; "sc_centroid_dist"/"sc_dihedral"/"sc_centroid_angle" f32
 * (+ "sc_valid" u8: 0 => null); string columns are rows x width fixed-width NUL-padded chars.  Also
 * "from_atom"/"to_atom" i32 atom indices (-1 for a "Ring" entity). */
const void *arp_table_column(const arp_table *t, const char *name, int32_t *width);

/* ---- contact frequencies over the frames of an ensemble (NMR models, MD snapshots, conformers of one topology) -- DESIGN.md section 3.7 ----
 * The topology is model 0 of `topology` (after load_model's filtering), N atoms.  Frame f is the topology with its coordinates replaced by
 * xyz[f] (n_frames x N x 3 f64, host, C order); xyz == NULL: the structure's models are the frames (n_frames is ignored), and every model must list
 * model 0's atoms in the same order -- equal chain, residue name, resi, insertion code, altloc, atom name, serial and element -- else
 * ARP_ERR_BAD_INPUT naming the first model and atom that differ.  The atom-atom pairs of a frame are those of arp_contacts_atomic (groups,
 * vdw_comp, dist_cutoff as for arp_get_contacts, with its group errors); every set bit of a pair's kind is one (i, j, interaction) item.
 * The table has one row per distinct (i, j, interaction) of at least one frame, i / j topology atom indices, ordered by (i, j, interaction):
 *   "interaction" i32 code; "from_chain" "from_resn" "from_insertion" "from_altloc" "from_atomn" fixed-width strings, "from_resi" "from_atomi" i32,
 *   the same seven "to_*" columns, "from_atom" / "to_atom" i32 (i, j); "n_frames" u32 (frames with the row); "frequency" f32 = f32(n_frames / F)
 *   divided in f64; "min_distance" / "max_distance" f32 over those frames.  No ring rows (CationPi, Pi*: arp_contact_frequencies_ex adds them) and no sc_* columns; no ring is required.
 * The result does not depend on the order the device produces pairs in: two calls give identical bytes.  arp_table_rows / arp_table_column /
 * arp_table_export_arrow serve this column set (the Arrow batch has the columns above in that order, without from_atom / to_atom).
 * Errors before the device is touched (ARP_ERR_BAD_INPUT unless noted): n_frames == 0 with xyz, a non-finite coordinate, N >= 2^29, the
 * model check, the chain groups (ARP_ERR_BAD_GROUPS / ARP_ERR_EMPTY_GROUPS).  ctx == NULL runs only these checks (ARP_OK, *out = NULL).
 * Frames run through the device in passes of about 2 x 10^6 atoms (arp_debug_set "freq_chunk_atoms"); memory grows with the distinct rows, not F. */
arp_status arp_contact_frequencies(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp,
                                   double dist_cutoff, arp_table **out);

/* arp_contact_frequencies with flags.  flags == 0 is arp_contact_frequencies: the same checks, the same bytes.  An unknown
 * flag bit is ARP_ERR_BAD_INPUT.
 * ARP_FREQ_RINGS adds the ring rows -- CationPi and the six Pi* stackings.  Definition: let S_f be the SINGLE-MODEL structure that holds model 0's
 * atoms, in order, with frame f's coordinates (the same f64 values; nothing is parsed again).  The ring entities of the topology are the ring
 * entities arp_get_contacts builds for S_0, in its order: one per altloc of every residue with at least 3 ring-plane atoms, in residue order; all
 * entities of a residue share that residue's plane.  There are n_rings of them; entity numbers are 0 .. N - 1 for atoms and N + e for ring e.
 * Frame f contributes, besides its atom-atom items, one item (from entity, to entity, code, f32 distance) for every row with a ring entity that
 * arp_get_contacts(S_f, groups, vdw_comp, dist_cutoff) returns: CationPi rows ring -> atom, the six Pi* rows ring -> ring.  Ring-ring rows do NOT
 * depend on dist_cutoff; ring-atom rows do (candidates: d^2 <= dist_cutoff^2 from the ring centre, inclusive, in f64).  Items are aggregated like
 * atom items: one row per distinct (from, to, code) with n_frames, frequency, min_distance / max_distance; the same ring pair under different
 * codes in different frames gives different rows.  Row order stays (from entity, to entity, code): every ring row has a ring as `from`, so all
 * ring rows follow all atom-atom rows, and the atom-atom rows are byte for byte the table without rings.
 * A ring entity's columns: chain, resn, resi, insertion, altloc of the entity, atomn "Ring", atomi 0 (what arp_get_contacts writes);
 * "from_atom" / "to_atom" are -1.  arp_table_column also serves "from_ring" / "to_ring" i32 on frequency tables: the ring entity index, -1 for
 * an atom.  The Arrow batch keeps its column set.
 * A topology without any ring is not an error: ARP_OK and the table without rings (arp_get_contacts' ARP_ERR_NO_RINGS does not apply).
 * With the frames taken from a multi-model FILE (xyz == NULL) the rings are still those of model 0 regarded as a single-model structure -- NOT what
 * arp_get_contacts files for the multi-model file, which keeps ring planes under every model serial.
 * One more check before the device is touched: N + n_rings < 2^29 (ARP_ERR_BAD_INPUT).  The sc_* statistics stay out of scope. */
#define ARP_FREQ_RINGS 0x1u
arp_status arp_contact_frequencies_ex(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp,
                                      double dist_cutoff, uint32_t flags, arp_table **out);

/* ---- residue-level contact frequencies over the frames of an ensemble -- DESIGN.md section 3.12 ----
 * Topology, N, F frames, xyz, groups, vdw_comp and dist_cutoff exactly as arp_contact_frequencies_ex defines them.  For frame f let items(f) be
 * the items that call defines for the same flags: (from entity, to entity, code, f32 distance) -- the atom-atom items, plus the ring items with
 * ARP_FREQ_RINGS.  Every entity maps to a residue of the topology: atom a to the ingest's residue ordinal res_id[a] (a residue is one (chain,
 * resi, insertion); all altlocs of a residue are the same residue; ordinals run 0 .. n_res - 1 in hierarchy order), ring entity e to the residue
 * of its plane (the altloc entities of one ring residue are the same residue).
 * The table has one row per distinct (A = res(from), B = res(to), code) over all frames, ordered by (A, B, code).  A residue pair is in contact
 * in a frame when ANY of its items is, so this table cannot be derived from the atom-level one:
 *   "n_frames" u32      the number of DISTINCT frames with at least one item of the row
 *   "frequency" f32     f32((double)n_frames / F)
 *   "min_distance" f32  the minimum over those frames of c_f, c_f = the smallest f32 distance among the row's items in frame f (the frame's
 *                       closest approach under that interaction)
 *   "max_distance" f32  the maximum over those frames of c_f -- NOT the maximum over all items
 * Orientation is the items' own, nothing is symmetrised: (A, B, code) and (B, A, code) are different rows if both occur.
 * Further columns: "interaction" i32 code; "from_chain" "from_resn" "from_insertion" fixed-width strings and "from_resi" i32, taken from the first
 * topology atom of the residue (as the residue-level SASA rows take them), the same four "to_*" columns, and "from_residue" / "to_residue" i32
 * (the ordinals A, B).  The table has no atom, altloc, atomn, atomi or ring columns: arp_table_column returns NULL for them.  The Arrow batch has
 * the 13 columns interaction, from_chain, from_resn, from_resi, from_insertion, to_chain, to_resn, to_resi, to_insertion, n_frames, frequency,
 * min_distance, max_distance, in that order.
 * The bytes do not depend on the pass size (arp_debug_set "freq_chunk_atoms"), the frame bits of the device keys ("freq_frame_bits"), the first
 * buffer capacity ("freq_cap_items") or the order in which the device produced pairs or ran atomics: two calls give identical bytes.
 * flags accepts ARP_FREQ_RINGS and ARP_FREQ_WATERS (below); any other bit is ARP_ERR_BAD_INPUT.  Errors and checks are arp_contact_frequencies_ex's,
 * with the same statuses and messages, before the device is touched; ctx == NULL runs only them (ARP_OK, *out = NULL).  No new size limit: a huge
 * topology only gets smaller passes. */
arp_status arp_residue_contact_frequencies(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp,
                                           double dist_cutoff, uint32_t flags, arp_table **out);

/* ---- water bridges: water-mediated contacts per frame and across frames -- DESIGN.md section 3.19 ----
 * Topology, N, F frames, xyz and groups exactly as arp_contact_frequencies_ex defines them.  The topology is classified once per call:
 *   water atom   residue name HOH and not ARP_ATTR_H
 *   polar atom   attr & (ARP_ATTR_DONOR | ARP_ATTR_ACCEPTOR) non-zero and not ARP_ATTR_H.  No water atom is polar (the attribute tables give a water
 *                oxygen neither class; an input that breaks this is ARP_ERR_BAD_INPUT).  Hydrogens play no part: the rule is geometric on heavy
 *                atoms, like PolarContact.
 * In frame f:
 *   leg (w, p)        holds iff d2 = dx*dx + dy*dy + dz*dz <= 12.25, evaluated in f64 in that order, inclusive (12.25 = 3.5^2, the PolarContact
 *                     distance, exactly representable)
 *   bridge (p, w, q)  holds iff p != q are polar, both legs hold, attr[p] & ARP_ATTR_LIGAND, attr[q] & ARP_ATTR_RECEPTOR, and the residue rule of
 *                     the contact table in its symmetric form accepts (residue of p, residue of q): on one chain ord(q) >= ord(p) + 2, and two
 *                     chains that are both in the ligand and in the receptor set are listed once, by chain order.  One orientation per residue pair.
 * The water's own chain and groups play no part (a water filed under a third chain still mediates), and a bridge depends on neither vdw_comp nor
 * dist_cutoff: the bridged atoms may be up to 7 A apart.
 * ARP_FREQ_WATERS on arp_residue_contact_frequencies, and on arp_contact_timelines at level 1, adds one item per bridge:
 *   (A = res_id[p], B = res_id[q], code ARP_WaterBridge, frame f, dist = (float)sqrt(max(d2p, d2q)), the longer leg)
 * so the closest approach of a frame is its tightest bridge, and a row's "min_distance" <= T says the pair is bridged at leg length T in some frame.
 * The rows with any other code are byte for byte the table without the flag; without the flag nothing changes.  ARP_FREQ_RINGS may be combined.
 * At level 0 (arp_contact_frequencies_ex never accepts the bit; arp_contact_timelines with level 0) the flag is ARP_ERR_BAD_INPUT.  The similarity,
 * autocorrelation and cluster calls reject the bit as unknown: arp_bit_gram, arp_bit_autocorr and arp_bit_cluster on the timeline's bitmap serve meanwhile.
 * Capacity: a water with more than 32 polar atoms within 3.5 A in any frame fails the whole call with ARP_ERR_CAPACITY and a message saying so,
 * never a shorter table (real structures have 4 to 8).  The sweep is brute force, waters x polar atoms per frame. */
#define ARP_FREQ_WATERS 0x100u
/* The bridges themselves, one row per (frame, p, q, w), ordered by those four (topology atom indices).  Same frame convention and checks as the
 * frequency calls; ctx == NULL runs only the checks (ARP_OK, *out = NULL).  No pair pass runs.  Columns (arp_table_column; the Arrow batch has them in
 * this order): "frame" u32; "from_chain" "from_resn" "from_resi" "from_insertion" "from_altloc" "from_atomn" "from_atomi" (atom p) and the same seven
 * "to_*" (atom q); "water_chain" "water_resi" "water_insertion" "water_altloc" "water_atomi"; "from_distance" "to_distance" f32 (the legs) and
 * "distance" f32 (the longer leg).  "from_atom" / "water_atom" / "to_atom" i32 (topology indices) are served by arp_table_column only.  Grouping the
 * rows by (res_id[p], res_id[q]) gives the ARP_WaterBridge rows of arp_residue_contact_frequencies exactly.  More than 2^31 rows: ARP_ERR_CAPACITY. */
arp_status arp_water_bridges(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const char *groups, arp_table **out);

/* ---- contact timelines over the frames of an ensemble: which frames, how many events, how long -- DESIGN.md section 3.13 ----
 * Topology, n_frames, xyz, groups, vdw_comp and dist_cutoff exactly as arp_contact_frequencies_ex (level 0) or arp_residue_contact_frequencies
 * (level 1) define them.  The rows are exactly the rows that call returns for the same arguments (flags & ARP_FREQ_RINGS), in its order, and the
 * table serves every column of that frequency table with identical bytes.  On top of them, with F the number of frames:
 *   present[r][f] = 1 iff frame f contributes at least one item to row r.  At atom level the item is (from entity, to entity, code); at residue level
 *   it is any item whose entities map to (A, B, code) -- several items of one frame set the same bit.
 * Per row, over f = 0 .. F - 1 (arp_table_column, all 4 bytes wide):
 *   "first_frame" "last_frame" u32   the smallest / largest f with the bit set
 *   "n_events" u32                   the number of maximal runs of consecutive set bits
 *   "longest_run" u32                the length of the longest such run, in frames
 *   "mean_run" f32                   f32((double)n_frames / n_events)
 * The bitmap itself (arp_table_timeline): words[r][w] u32, W = ceil(F / 32) words per row, row-major; frame f is bit f & 31 of word f >> 5; the unused
 * high bits of a row's last word are zero.  The popcount of a row equals the row's "n_frames"; should it ever not, the call fails with ARP_ERR_HIP and
 * an "internal error" message instead of returning a table.
 * arp_table_export_arrow appends the five columns behind the frequency columns of the level; the bitmap is not part of the Arrow batch.
 * flags: ARP_FREQ_RINGS (the ring rows, as in the frequency calls), ARP_FREQ_WATERS (level 1 only: the water-bridge rows; at level 0 it is
 * ARP_ERR_BAD_INPUT with a message that names level 1 and arp_water_bridges) and ARP_TIMELINE_NO_BITMAP (the statistics are computed, the bitmap is not copied
 * to the host: arp_table_timeline returns NULL); any other bit, or a level outside {0, 1}, is ARP_ERR_BAD_INPUT.  Every check, status and message of the frequency
 * calls runs before the device is touched; ctx == NULL runs only the checks (ARP_OK, *out = NULL).
 * Device memory: the frequency call's, plus rows x W x 4 bytes for the bitmap.  A bitmap above 2^31 bytes (arp_debug_set "timeline_cap_bytes") is
 * ARP_ERR_CAPACITY, with a message that names rows, frames and bytes.  The bytes do not depend on the pass size or on the order in which the device
 * produced pairs or ran atomics: two calls give identical bytes.  Synchronous; the frames cross the device twice (rows, then marks). */
#define ARP_TIMELINE_NO_BITMAP 0x2u
arp_status arp_contact_timelines(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp,
                                 double dist_cutoff, uint32_t flags, int32_t level, arp_table **out);
/* The host bitmap of a timeline table (owned by the table): *words_per_row = W, *n_frames = F (both nullable).  NULL for every other table and for a
 * table built with ARP_TIMELINE_NO_BITMAP. */
const uint32_t *arp_table_timeline(const arp_table *t, uint64_t *words_per_row, uint64_t *n_frames);
/* The definition above on its own (no device), a plain loop over the bits of `rows` rows of ceil(n_frames / 32) words: n_present = the popcount over
 * frames 0 .. n_frames - 1 (bits past n_frames are ignored), first / last, n_events, longest_run as above; a row without any set bit gets first = last =
 * ARP_NONE and zeros.  For anyone who post-processes a bitmap (a frame window, an AND of two rows), and the yardstick of the device kernel. */
arp_status arp_timeline_stats(uint64_t rows, uint64_t n_frames, const uint32_t *words, uint32_t *n_present, uint32_t *first, uint32_t *last, uint32_t *n_events,
                              uint32_t *longest_run);

/* ---- contact similarity between frames, contact co-occurrence between rows -- DESIGN.md section 3.14 ----
 * Topology, n_frames, xyz, groups, vdw_comp, dist_cutoff and level exactly as arp_contact_timelines defines them, and present[r][f] is that call's:
 * the same rows in the same order, either level, with or without ARP_FREQ_RINGS.  With F frames and R rows:
 *   axis "frames" (default)  S_f = { r : present[r][f] };  inter[f][g] = |S_f AND S_g|;  sizes[f] = |S_f|;  M = F
 *   axis "rows" (ARP_SIM_ROWS)  T_r = { f : present[r][f] };  inter[r][s] = |T_r AND T_s|;  sizes[r] = |T_r| = the row's "n_frames";  M = R
 *   metric "tanimoto" (default)  f32((double)inter / (double)(sizes_a + sizes_b - inter)), 1.0f when the union is empty (two empty sets are
 *                             identical), so the diagonal is 1.0 everywhere; one IEEE f64 divide and one rounding to f32
 *   metric "count" (ARP_SIM_COUNTS)  inter as u32
 * The matrix is full, symmetric, M x M, row-major.  No contact in any frame (R = 0): on axis "frames" the counts are 0, the Tanimoto values 1.0 and
 * the sizes 0; on axis "rows" the matrix is empty.
 * The returned table is the frequency table of the level: every column and the Arrow export have the bytes of arp_contact_frequencies_ex /
 * arp_residue_contact_frequencies for the same arguments; the matrix is not part of the batch (arp_table_similarity).
 * flags: ARP_FREQ_RINGS, ARP_SIM_COUNTS, ARP_SIM_ROWS; any other bit, or a level outside {0, 1}, is ARP_ERR_BAD_INPUT.  Every check, status and message
 * of the frequency calls runs before the device is touched; ctx == NULL runs only the checks (ARP_OK, *out = NULL).
 * Device memory: the timeline call's (its bitmap limit applies, and the bitmap is never copied to the host), plus M x M x 4 bytes for the matrix and,
 * on axis "frames", the transposed bitmap.  A matrix above 2^31 bytes (arp_debug_set "similarity_cap_bytes") is ARP_ERR_CAPACITY, with a message that
 * names M, the axis and the bytes; the check runs as soon as R is known, before anything is allocated for the matrix.  The bytes do not depend on the
 * pass size, on the order in which the device produced pairs, or on tile scheduling: two calls give identical bytes.  Synchronous. */
#define ARP_SIM_COUNTS 0x4u
#define ARP_SIM_ROWS 0x8u
arp_status arp_contact_similarity(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp,
                                  double dist_cutoff, uint32_t flags, int32_t level, arp_table **out);
/* The host matrix of a similarity table (owned by the table): *m = M, *flags = the call's ARP_SIM_* bits (f32 values unless ARP_SIM_COUNTS: u32),
 * *sizes = the M set sizes (all three nullable).  Never NULL for a similarity table, M = 0 included; NULL for every other table. */
const void *arp_table_similarity(const arp_table *t, uint64_t *m, uint32_t *flags, const uint32_t **sizes);
/* The definition above on any bitmap of the timeline layout (`rows` rows of ceil(n_bits / 32) words), bit by bit, without a device: ARP_SIM_ROWS
 * clear compares the bit columns (the frames of a timeline bitmap: M = n_bits), set compares the word rows (M = rows); ARP_SIM_COUNTS as above.  out:
 * M x M f32 or u32, sizes: M u32.  Bits past n_bits in a row's last word are ignored.  n_bits or rows of 2^32 and more, an unknown flag, or a null
 * pointer with rows > 0 are ARP_ERR_BAD_INPUT.  The CPU yardstick of the device kernels, and a tool for post-processed bitmaps. */
arp_status arp_bit_gram_host(uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, void *out, uint32_t *sizes);
/* The same on the device for a host bitmap: upload, the kernels of arp_contact_similarity, download.  Identical bytes.  The matrix limit of
 * arp_contact_similarity applies (ARP_ERR_CAPACITY). */
arp_status arp_bit_gram(arp_context *ctx, uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, void *out, uint32_t *sizes);

/* ---- contact autocorrelation and survival curves across frames: how long a contact lives -- DESIGN.md section 3.16 ----
 * Topology, n_frames, xyz, groups, vdw_comp, dist_cutoff and level exactly as arp_contact_timelines defines them, and present[r][f] is that call's:
 * the same rows in the same order, either level, with or without ARP_FREQ_RINGS.  With F frames, R rows and lags t = 0 .. L, L = max_lag:
 *   intermittent (default)           acf[r][t] = #{ f : 0 <= f < F - t, present[r][f] and present[r][f + t] }
 *   continuous (ARP_ACF_CONTINUOUS)  acf[r][t] = #{ f : 0 <= f < F - t, present[r][f] and present[r][f + 1] and ... and present[r][f + t] }
 *                                    = the sum over the row's maximal runs of max(0, run length - t)
 * acf[r][0] is the row's "n_frames"; continuous <= intermittent; continuous is 0 from the row's longest run on.
 *   sums[c][t] = the sum of acf[r][t] over the rows with interaction code c (u64; ARP_N_INTERACTIONS codes)
 *   half-life of row r = the smallest t in 1 .. L with 2 acf[r][t] F <= acf[r][0] (F - t): where the window-corrected estimator
 *   C(t) = (acf[t] / (F - t)) / (acf[0] / F) has fallen to one half; none when no lag passes (an always-present row has C = 1 throughout).
 * max_lag: ARP_NONE means F - 1; a max_lag >= F is ARP_ERR_BAD_INPUT; 0 is legal (one column equal to "n_frames", no half-life).  F > 2^24 is
 * ARP_ERR_BAD_INPUT with a message that names F (the half-lives are served as f32).
 * The returned table is the frequency table of the level -- every column has the bytes of arp_contact_frequencies_ex / arp_residue_contact_frequencies for
 * the same arguments -- plus one column "half_life" (f32, the integral lag; null where there is none), which arp_table_export_arrow appends behind the
 * frequency columns.  The counts are not columns (arp_table_autocorrelation).
 * flags: ARP_FREQ_RINGS, ARP_ACF_CONTINUOUS, ARP_ACF_NO_MATRIX (the rows' curves are neither stored on the device nor copied: the sums and the half-lives
 * only); any other bit -- ARP_TIMELINE_NO_BITMAP too: the bitmap never leaves the device here --, or a level outside {0, 1}, is ARP_ERR_BAD_INPUT.  Every
 * check, status and message of the frequency calls runs before the device is touched; ctx == NULL runs only the checks, those on max_lag and F included
 * (ARP_OK, *out = NULL).
 * Device memory: the timeline call's (its bitmap limit applies), plus R x (L + 1) x 4 bytes for the matrix unless ARP_ACF_NO_MATRIX, and with
 * ARP_ACF_CONTINUOUS 4 bytes per run of the bitmap (a run list above 2^31 bytes is ARP_ERR_CAPACITY too, and so
 * are more than 2^24 - 1 lag tiles, rows x ceil((L + 1) / 256): what one launch takes, with or without the matrix).  A matrix above 2^31
 * bytes (arp_debug_set "autocorr_cap_bytes") is ARP_ERR_CAPACITY, with a message that names rows, lags and bytes; the check runs as soon as R is known,
 * before anything is allocated for the matrix.  Should acf[r][0] ever differ from the row's "n_frames", the call fails with ARP_ERR_HIP and an "internal
 * error" message instead of returning a table.  Integer sums and minima only: two calls give identical bytes, whatever the pass size.  Synchronous. */
#define ARP_ACF_CONTINUOUS 0x10u
#define ARP_ACF_NO_MATRIX 0x20u
arp_status arp_contact_autocorrelation(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp,
                                       double dist_cutoff, uint32_t flags, int32_t level, uint32_t max_lag, arp_table **out);
/* The host counts of an autocorrelation table (owned by the table): u32, rows x *n_lags, row-major, *n_lags = L + 1; *flags = the call's ARP_ACF_* bits;
 * *sums = the u64 sums, *n_groups x *n_lags (all four nullable, and filled for every autocorrelation table).  Returns NULL for a table built with
 * ARP_ACF_NO_MATRIX and for every other table; never NULL otherwise, a table without rows included. */
const uint32_t *arp_table_autocorrelation(const arp_table *t, uint64_t *n_lags, uint32_t *flags, const uint64_t **sums, uint32_t *n_groups);
/* The definition above on any bitmap of the timeline layout (`rows` rows of ceil(n_bits / 32) words), a plain loop over the bits, without a device.
 * flags: ARP_ACF_CONTINUOUS only.  max_lag as above (ARP_NONE: n_bits - 1).  group (nullable): group[r] < n_groups files row r's counts under sums[group[r]]
 * (u64, n_groups x (L + 1), zeroed first; not written without group); acf (nullable): u32 rows x (L + 1); half_life: u32 per row, ARP_NONE for none.
 * Bits past n_bits in a row's last word are ignored.  A null words / half_life with rows > 0, an unknown flag, a max_lag >= n_bits, a group[r] >= n_groups,
 * and n_bits or rows of 2^32 and more are ARP_ERR_BAD_INPUT.  The CPU yardstick of the device kernels, and a tool for post-processed bitmaps (a frame
 * window, the AND of two rows). */
arp_status arp_bit_autocorr_host(uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, uint32_t max_lag, const uint32_t *group, uint32_t n_groups,
                                 uint32_t *acf, uint64_t *sums, uint32_t *half_life);
/* The same on the device for a host bitmap: upload, the kernels of arp_contact_autocorrelation, download.  Identical bytes.  The matrix limit of
 * arp_contact_autocorrelation applies when acf is given (ARP_ERR_CAPACITY).  rows == 0 is answered by the host function. */
arp_status arp_bit_autocorr(arp_context *ctx, uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, uint32_t max_lag, const uint32_t *group,
                            uint32_t n_groups, uint32_t *acf, uint64_t *sums, uint32_t *half_life);

/* ---- clusters of the frames by their contacts: which states there are, which frame stands for each, which contacts tell them apart -- DESIGN.md section 3.17 ----
 * Topology, n_frames, xyz, groups, vdw_comp, dist_cutoff and level exactly as arp_contact_similarity defines them on axis "frames", and present[r][f] is that
 * call's: the same rows in the same order, either level, with or without ARP_FREQ_RINGS.  With F frames and R rows:
 *   S_f = { r : present[r][f] };  sizes[f] = |S_f|;  tan(f, g) = the f32 Tanimoto value of arp_contact_similarity, bit for bit (1.0f for an empty union)
 *   neighbours  adj[f][g] <=> tan(f, g) >= min_similarity, compared as f32 values: symmetric, adj[f][f] always -- what the matrix of arp_contact_similarity
 *               gives when it is compared with min_similarity
 *   clusters (the method MD users know as gromos: Daura et al. 1999)  all F frames alive, k = 0; while a frame is alive and k < max_clusters:
 *               n[f] = #{ g alive : adj[f][g] } for every alive f (f itself included; over the frames alive NOW); c = the alive frame with the largest n[f], the
 *               smallest index among equals; cluster k = { g alive : adj[c][g] } with centre c; its members leave the alive set; k += 1.  C = the final k; the
 *               cluster sizes do not increase with k.
 * min_similarity must be finite and in [0, 1]; max_clusters: ARP_NONE means no limit, 0 is ARP_ERR_BAD_INPUT.
 * Results (arp_table_clusters; none of them is a column): cluster[f] u32 (ARP_NONE for the frames left over when max_clusters ended the loop),
 * similarity_to_centre[f] f32 = tan(f, centre of its cluster) (1.0f for a centre, the bits 0x7FC00000 for a left-over frame), n_neighbours[f] u32 = n[f] of the
 * first round (the degree in the full graph, f included), sizes[f] u32, centre[k] and cluster_size[k] u32 (C entries), and cluster_counts[r][k] u32, R x C,
 * row-major = #{ f : cluster[f] = k and present[r][f] } -- the numerator of row r's frequency inside state k; not computed with ARP_CLUSTER_NO_COUNTS.
 * No contact in any frame (R = 0): every frame is the empty set, all are mutual neighbours: one cluster with centre 0.
 * The returned table is the frequency table of the level: every column and the Arrow export have the bytes of arp_contact_frequencies_ex /
 * arp_residue_contact_frequencies for the same arguments.
 * flags: ARP_FREQ_RINGS, ARP_CLUSTER_NO_COUNTS; any other bit -- ARP_SIM_ROWS, ARP_SIM_COUNTS and ARP_TIMELINE_NO_BITMAP too --, or a level outside {0, 1}, is
 * ARP_ERR_BAD_INPUT.  Every check, status and message of the frequency calls runs before the device is touched; ctx == NULL runs only the checks, those on
 * min_similarity and max_clusters included (ARP_OK, *out = NULL).
 * Device memory: the timeline call's (its bitmap limit applies; the bitmap is never copied to the host), the transposed bitmap, F x ceil(F / 32) x 4 bytes of
 * neighbour bits, a few vectors of F entries, and R x C x 4 bytes for the counts.  No F x F matrix of values exists on either side, and the limit of
 * arp_contact_similarity ("similarity_cap_bytes") does not apply: 10^5 frames are 1.25 GB of neighbour bits.  Neighbour bits above 2^31 bytes
 * (arp_debug_set "cluster_cap_bytes") are ARP_ERR_CAPACITY, with a message that names F and the bytes; the check runs as soon as R is known, before anything
 * is allocated for them.  Counts above the same limit are ARP_ERR_CAPACITY too, once C is known and before they are allocated.  Should the cluster sizes not
 * add up to the assigned frames, or -- with every frame assigned -- a row's counts not add up to its "n_frames", the call fails with ARP_ERR_HIP and an
 * "internal error" message instead of returning a table.  Integer work and the one IEEE divide: two calls give identical bytes, whatever the pass size.
 * Synchronous. */
#define ARP_CLUSTER_NO_COUNTS 0x40u
arp_status arp_contact_clusters(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const char *groups, double vdw_comp,
                                double dist_cutoff, uint32_t flags, int32_t level, float min_similarity, uint32_t max_clusters, arp_table **out);
/* The host arrays of a cluster table (owned by the table).  Returns cluster[F]; *n_frames = F, *n_clusters = C, *flags = the call's ARP_CLUSTER_* bits, and the
 * arrays described above: F entries each for similarity_to_centre, n_neighbours and sizes, C for centre and cluster_size, R x C for cluster_counts (every out
 * pointer nullable).  *cluster_counts is NULL for a table built with ARP_CLUSTER_NO_COUNTS; nothing else is ever NULL for a cluster table.  Returns NULL
 * for every other table. */
const uint32_t *arp_table_clusters(const arp_table *t, uint64_t *n_frames, uint32_t *n_clusters, uint32_t *flags, const float **similarity_to_centre,
                                   const uint32_t **n_neighbours, const uint32_t **sizes, const uint32_t **centre, const uint32_t **cluster_size,
                                   const uint32_t **cluster_counts);
/* The definition above on any bitmap of the timeline layout (`rows` rows of ceil(n_bits / 32) words), bit by bit, without a device: ARP_SIM_ROWS clear
 * clusters the bit columns (the frames of a timeline bitmap: M = n_bits), set clusters the word rows (M = rows).  cluster, similarity_to_centre, n_neighbours
 * and sizes take M entries; centre and cluster_size take min(M, max_clusters); *n_clusters = C.  cluster_counts (nullable; the bit columns only) takes
 * rows x min(M, max_clusters) entries and is written as rows x C, row-major.  Bits past n_bits in a row's last word are ignored.  n_bits or rows of 2^32 and
 * more, any flag but ARP_SIM_ROWS, a min_similarity or max_clusters the call above refuses, cluster_counts with ARP_SIM_ROWS, a null n_clusters, or a null
 * words or result pointer with M > 0 are ARP_ERR_BAD_INPUT.  The CPU yardstick of the device kernels (one byte per pair: more than 46340 sets are
 * ARP_ERR_CAPACITY), and a tool for post-processed bitmaps. */
arp_status arp_bit_cluster_host(uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, float min_similarity, uint32_t max_clusters, uint32_t *cluster,
                                float *similarity_to_centre, uint32_t *n_neighbours, uint32_t *sizes, uint32_t *centre, uint32_t *cluster_size, uint32_t *n_clusters,
                                uint32_t *cluster_counts);
/* The same on the device for a host bitmap: upload, the kernels of arp_contact_clusters, download.  Identical bytes.  The limits of arp_contact_clusters
 * apply (ARP_ERR_CAPACITY).  rows == 0 and n_bits == 0 are answered by the host function. */
arp_status arp_bit_cluster(arp_context *ctx, uint64_t rows, uint64_t n_bits, const uint32_t *words, uint32_t flags, float min_similarity, uint32_t max_clusters,
                           uint32_t *cluster, float *similarity_to_centre, uint32_t *n_neighbours, uint32_t *sizes, uint32_t *centre, uint32_t *cluster_size,
                           uint32_t *n_clusters, uint32_t *cluster_counts);

/* ---- RMSD between the frames of an ensemble after optimal superposition: how far each frame is from a reference, which frames are the same conformation --
 * DESIGN.md section 3.20 ----
 * Frames exactly as arp_contact_frequencies defines them: model 0 of `topology` is the topology, N atoms; xyz is n_frames x N x 3 f64 on the host, C order;
 * xyz == NULL: the structure's models are the frames, with that call's one-for-one model check and its messages.
 * Selection: sel[n_sel], u32 topology atom indices, strictly increasing (which also rules out duplicates); all atoms have weight 1; n = n_sel.
 * Per frame f:  c_f = the f64 centroid of the selected atoms;  x_f,i = coordinate - c_f (centring happens before any product is formed);  G_f = sum_i |x_f,i|^2.
 * Per pair (f, g):  S = sum_i x_f,i x_g,i^T, 3 x 3 (Sab: component a of f with component b of g), and K(S) is Horn's symmetric 4 x 4 matrix
 *     |  Sxx + Syy + Szz    Syz - Szy          Szx - Sxz          Sxy - Syx        |
 *     |  Syz - Szy          Sxx - Syy - Szz    Sxy + Syx          Szx + Sxz        |
 *     |  Szx - Sxz          Sxy + Syx         -Sxx + Syy - Szz    Syz + Szy        |
 *     |  Sxy - Syx          Szx + Sxz          Syz + Szy         -Sxx - Syy + Szz  |
 *   lambda = its largest eigenvalue: the optimum over proper rotations only -- a mirror image does not superpose.  Then
 *   msd(f, g) = max(0, (G_f + G_g - 2 lambda) / n);  rmsd(f, g) = (float)sqrt(msd), one rounding to f32, as the tables' distances are f32.
 *   rmsd(f, f) is 0.0f by definition: written, never computed.  rmsd(f, g) and rmsd(g, f) are the same bits.  Two identical but distinct frames give a value
 *   near 0, not necessarily 0.
 *   neighbours  adj[f][g] <=> rmsd(f, g) <= cutoff, compared as f32 and inclusive: exactly what comparing the matrix with cutoff gives
 *   clusters    the loop written out under arp_contact_clusters (gromos: Daura et al. 1999, who define it on this rmsd) with this adj: the largest alive
 *               neighbour count wins, the smallest index among equals, the counts are retaken every round; max_clusters as there.
 * Checks, all before the device is touched, ARP_ERR_BAD_INPUT: the frame checks of the frequency call with its statuses and messages; n_sel == 0; an index
 * >= N; sel not strictly increasing; ref_frame >= F (without ref_xyz); a non-finite ref_xyz; a cutoff that is not finite or < 0; max_clusters == 0 (ARP_NONE:
 * no limit).  ctx == NULL runs only the checks (ARP_OK).
 * Device memory: the packed centred coordinates, F x 3 x n_pad x 8 bytes (n_pad: n rounded up to 4), stay resident for the call; above 2^31 bytes
 * (arp_debug_set "rmsd_cap_bytes") the call is ARP_ERR_CAPACITY with a message that names F, n and the bytes.  The eigenvalue is found by cyclic Jacobi
 * rotations, which lose no accuracy when the top eigenvalue is double (planar, collinear, mirror-image and n <= 3 selections).  A pair's products are summed in
 * the order of the atoms wherever the pair is computed: two calls give identical bytes, whatever the pass size ("rmsd_chunk_atoms").  Synchronous.
 *
 * arp_rmsd_matrix: out[F x F], row-major, caller-owned.  A matrix above 2^31 bytes ("rmsd_cap_bytes") is ARP_ERR_CAPACITY. */
arp_status arp_rmsd_matrix(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const uint32_t *sel, uint64_t n_sel, float *out);
/* out[F] = rmsd(reference, f).  ref_xyz == NULL: the reference is frame ref_frame; out[ref_frame] is 0.0f and every other entry equals the matrix row bit
 * for bit.  Otherwise ref_xyz is N x 3 f64 (the topology's atoms; the selection applies to it), ref_frame is ignored and every entry is computed: a reference
 * equal to frame k gives the matrix row's bits except out[k], which is near 0. */
arp_status arp_rmsd_reference(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const uint32_t *sel, uint64_t n_sel, const double *ref_xyz,
                              uint64_t ref_frame, float *out);
/* The clusters.  cluster[f] u32 (ARP_NONE for the frames left over when max_clusters ended the loop), rmsd_to_centre[f] f32 = the matrix entry (f, centre of
 * its cluster) bit for bit (0.0f for a centre, the bits 0x7FC00000 for a left-over frame), n_neighbours[f] u32 = the degree in the full graph, f included: F
 * entries each; centre[k] and cluster_size[k] u32 take min(F, max_clusters) entries, *n_clusters = C of them are written.  The matrix is never formed: the
 * limit is the neighbour bits, F x ceil(F / 32) x 4 bytes against "rmsd_cap_bytes" (ARP_ERR_CAPACITY) -- 10^5 frames are legal here, where the matrix is
 * not.  Should the cluster sizes not add up to the assigned frames the call fails with ARP_ERR_HIP and an "internal error" message. */
arp_status arp_rmsd_clusters(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const uint32_t *sel, uint64_t n_sel, float cutoff,
                             uint32_t max_clusters, uint32_t *cluster, float *rmsd_to_centre, uint32_t *n_neighbours, uint32_t *centre, uint32_t *cluster_size,
                             uint32_t *n_clusters);
/* The definition above in plain sequential C++, without a device: f64 throughout, the sums in the order of the atoms, cyclic Jacobi on K(S).  xyz_sel is
 * n_frames x n x 3 f64 -- the selected atoms only --, out n_frames x n_frames.  n == 0 or a non-finite coordinate is ARP_ERR_BAD_INPUT, more than 46340
 * frames ARP_ERR_CAPACITY.  The CPU yardstick of the device kernels: they agree with it within the rounding of the sums, not bit for bit. */
arp_status arp_rmsd_host(uint64_t n_frames, uint64_t n, const double *xyz_sel, float *out);

/* ---- RMSF and the mean structure: the frames superposed on a reference or on their own average, how much each atom moves about it -- DESIGN.md section
 * 3.21 ----
 * Frames, topology and sel[n] (the fit atoms) as for the arp_rmsd_* calls above, with their checks and messages.  msel[m]: the measured atoms, u32 topology
 * indices, strictly increasing; msel == NULL: the fit atoms are measured (m = n, n_msel is not looked at).  Weights are 1.
 * Centring.  Per frame c_f = the f64 centroid of the fit atoms; x_f,i = coordinate - c_f, for the fit atoms and the measured atoms alike.  The centroid is
 *   taken in two steps -- the mean, then the mean of what is left after subtracting it, subtracted again -- so that a frame 10^5 A from the origin is
 *   centred to the rounding of its centred coordinates, not of its absolute ones.
 * Starting target.  T_1 = the centred fit atoms of frame ref_frame, or of ref_xyz[N][3] when that is given (ref_frame is then ignored); c_T = that reference's
 * fit centroid, fixed for the call.
 * Round j = 1, 2, ..:  per frame S_f = sum_i x_f,i T_j,i^T over the fit atoms, K(S_f) as written out above, q_f = (w, x, y, z) a unit eigenvector of its
 *   largest eigenvalue, R_f the proper rotation of q_f,
 *     |  w^2 + x^2 - y^2 - z^2    2 (x y - w z)            2 (x z + w y)          |
 *     |  2 (y x + w z)            w^2 - x^2 + y^2 - z^2    2 (y z - w x)          |
 *     |  2 (z x - w y)            2 (z y + w x)            w^2 - x^2 - y^2 + z^2  |
 *   the rotation that minimises sum_i |R x_f,i - T_j,i|^2 over proper rotations (a mirror image stays unsuperposed);  Y_f,i = R_f x_f,i;
 *   M_j = (1 / F) sum_f Y_f over the fit atoms;  change_j = sqrt((1 / n) sum_i |M_j,i - T_j,i|^2).
 *   The call stops after round j when j == max_rounds or change_j <= tol; otherwise T_j+1 = M_j.  max_rounds = 1 is the classic fit to a fixed reference.
 * Outputs, all under the last round's R_f; quantities over the fit atoms use M over the fit set, quantities over the measured atoms the mean over the
 * measured set:
 *   mean[m][3]         f64  the mean of Y over the frames, plus c_T
 *   rmsf[m]            f32  sqrt((1 / F) sum_f |Y_f,i - mean_i|^2): summed as deviations from the finished mean, never as E[y^2] - E[y]^2; one rounding to f32
 *   frame_rmsd[F]      f32  sqrt((1 / n) sum_{i in sel} |Y_f,i - M_i|^2), no re-fit
 *   transforms[F][12]  f64, may be NULL: R_f row-major, then t_f = c_T - R_f c_f, so that y = R x + t maps absolute frame coordinates onto the reference's
 *   aligned[F][m][3]   f64, may be NULL: R x + t of the measured atoms, formed as R_f x_f,i + c_T
 *   *n_rounds u32, *last_change f64: the rounds done and the final change; last_change > tol says that the cap max_rounds ended the call.
 * Eigenvector choice.  Where the top eigenvalue of K is double (collinear fit atoms in either structure, n <= 2) any top eigenvector is allowed; it is chosen
 * deterministically: the Jacobi column of the largest diagonal entry, the lowest index on ties.
 * Checks, all before the device is touched, ARP_ERR_BAD_INPUT: those of the arp_rmsd_* calls (prefix "rmsf"); msel given and empty, with an index >= N or
 * not strictly increasing; max_rounds == 0; a tol that is not finite or < 0; ref_frame >= F (without ref_xyz); a non-finite ref_xyz.  ctx == NULL runs only
 * the checks (ARP_OK).
 * Device memory: both packed sets, F x 3 x (n_pad + m_pad) x 8 bytes (m_pad only with msel), stay resident and are checked against "rmsd_cap_bytes" before
 * anything is allocated: ARP_ERR_CAPACITY with a message that names F, n, m and the bytes.  No floating-point atomic is used and the order of every sum is a
 * function of (F, n, m) alone: two calls give identical bytes, whatever the pass size ("rmsd_chunk_atoms").  Synchronous; one 8-byte read-back per round. */
arp_status arp_rmsf(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const uint32_t *sel, uint64_t n_sel, const uint32_t *msel,
                    uint64_t n_msel, const double *ref_xyz, uint64_t ref_frame, uint32_t max_rounds, double tol, double *mean, float *rmsf, float *frame_rmsd,
                    double *transforms, double *aligned, uint32_t *n_rounds, double *last_change);
/* The definition above in plain sequential C++ on already-selected coordinates, without a device: xyz_sel n_frames x n x 3 (the fit atoms), xyz_msel
 * n_frames x m x 3 (the measured atoms; NULL: the fit atoms, m must equal n), ref_sel n x 3 (the reference's fit atoms; NULL: frame ref_frame).  f64
 * throughout, every sum in the order of its index.  The outputs are arp_rmsf's.  n_frames, n or m == 0, max_rounds == 0, a bad tol or ref_frame and a
 * non-finite coordinate are ARP_ERR_BAD_INPUT.  The CPU yardstick of the device kernels: they agree within the rounding of the sums, not bit for bit. */
arp_status arp_rmsf_host(uint64_t n_frames, uint64_t n, uint64_t m, const double *xyz_sel, const double *xyz_msel, const double *ref_sel, uint64_t ref_frame,
                         uint32_t max_rounds, double tol, double *mean, float *rmsf, float *frame_rmsd, double *transforms, double *aligned, uint32_t *n_rounds,
                         double *last_change);

/* ---- Covariance, DCCM and principal components of an ensemble's motions -- DESIGN.md section 3.22 ----
 * Which atoms move together, and along which collective directions: the second moments of the superposed coordinates.  Frames, topology, sel[n] (the fit
 * atoms), msel[m] (the measured atoms; NULL: the fit atoms), ref_xyz / ref_frame, max_rounds and tol mean exactly what they mean for arp_rmsf, and the
 * superposition is that call's.  Under its last rotations, for the measured atoms: Y_f,i = R_f x_f,i, mean_i their mean over the frames, and
 *   d_f,a = Y_f,i,k - mean_i,k      with the coordinate index a = 3 i + k (atom-major; k = x, y, z).
 * Outputs:
 *   cov[3 m][3 m]  f64 row-major, may be NULL: cov[a][b] = (1 / F) sum_f d_f,a d_f,b.  The divisor is F, as in rmsf, so the trace of atom i's 3 x 3 block is
 *                  rmsf_i^2.  cov[a][b] and cov[b][a] are the same bits: the mirror is written from the same value.
 *   dccm[m][m]     f32 row-major, may be NULL: t_ij = (1 / F) sum_f sum_k d_f,(i,k) d_f,(j,k), v_i = t_ii, dccm[i][j] = clamp(t_ij / sqrt(v_i v_j), -1, 1),
 *                  formed in f64 and rounded once to f32.  The diagonal is written 1.0f, never computed; an off-diagonal entry with v_i == 0 or v_j == 0 is
 *                  0.0f; the matrix is symmetric in its bits, and its bytes do not depend on whether cov is asked for.
 *   mean, rmsf, frame_rmsd, transforms (may be NULL), *n_rounds, *last_change: arp_rmsf's, byte for byte.  (aligned is not offered here.)
 * Checks, all before the device is touched, ARP_ERR_BAD_INPUT: those of arp_rmsf under the prefix "covariance".  ctx == NULL runs only those checks
 * (ARP_OK); with a context, cov == NULL and dccm == NULL together are ARP_ERR_BAD_INPUT.
 * Device memory, checked against "rmsd_cap_bytes" before anything is allocated: what arp_rmsf keeps resident, the deviations F x 3 x m_pad x 8 bytes, the
 * requested outputs at their padded sizes (3 m_pad)^2 x 8 and m_pad^2 x 4, and the partial sums of the frame slabs: ARP_ERR_CAPACITY with a message that
 * names F, m and the bytes.  No floating-point atomic is used; the frames are summed in slabs whose count is a function of (F, m) alone, in a fixed order: two
 * calls give identical bytes, whatever the pass size ("rmsd_chunk_atoms").  Synchronous.
 * The eigen-decomposition of cov (principal components, "essential dynamics") is left to the caller; the Python layer's pca uses LAPACK on the host. */
arp_status arp_covariance(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const uint32_t *sel, uint64_t n_sel, const uint32_t *msel,
                          uint64_t n_msel, const double *ref_xyz, uint64_t ref_frame, uint32_t max_rounds, double tol, double *cov, float *dccm, double *mean, float *rmsf,
                          float *frame_rmsd, double *transforms, uint32_t *n_rounds, double *last_change);
/* Projection of frames onto given directions: proj[F][k] f64, proj[f][j] = sum_a d_f,a V[j][a] in the order of a, for the caller's modes V[k][3 m] (f64,
 * atom-major rows, not required to be orthonormal), with d_f,(i,.) = R_f p_f,i + t_f - mean_i formed from the ABSOLUTE coordinates p of the measured atoms
 * msel[m] (strictly increasing, required), the caller's transforms[F][12] (R row-major, then t, as arp_rmsf returns them; NULL: the identity -- the frames are
 * already superposed) and mean[m][3].  No fit is repeated: new frames, once arp_rmsf has fitted them to the mean structure, project onto old modes.
 * Frames and topology as for arp_rmsf; they are uploaded in the same passes ("rmsd_chunk_atoms") and each pass is projected where it is staged.
 * Checks, all before the device is touched, ARP_ERR_BAD_INPUT: the frame checks of the arp_rmsd_* calls and their selection checks on msel (prefix "project");
 * k == 0; k > 3 m; a non-finite mean, modes or transforms.  ctx == NULL runs only the checks.  The transforms, the modes and the projections are checked
 * against "rmsd_cap_bytes": ARP_ERR_CAPACITY (the staging buffer of one upload pass, which "rmsd_chunk_atoms" sizes, is not counted, as in the arp_rmsd_* calls).  Plain f64 multiply-adds, one sum per projection: identical bytes for any pass size. */
arp_status arp_project(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const uint32_t *msel, uint64_t n_msel, const double *transforms,
                       const double *mean, const double *modes, uint64_t k, double *proj);
/* The two definitions above in plain sequential C++, without a device, every sum in the order of its index.  arp_covariance_host: aligned n_frames x m x 3
 * (superposed coordinates, as arp_rmsf's aligned) and mean m x 3 give d = aligned - mean; cov and dccm as above, each may be NULL, not both.
 * arp_project_host: xyz_msel n_frames x m x 3 are the absolute coordinates of the measured atoms; transforms may be NULL.  n_frames or m == 0, k == 0,
 * k > 3 m and a non-finite value are ARP_ERR_BAD_INPUT.  The CPU yardsticks of the device kernels: they agree within the rounding of the sums. */
arp_status arp_covariance_host(uint64_t n_frames, uint64_t m, const double *aligned, const double *mean, double *cov, float *dccm);
arp_status arp_project_host(uint64_t n_frames, uint64_t m, const double *xyz_msel, const double *transforms, const double *mean, const double *modes, uint64_t k, double *proj);

/* ---- Secondary structure (DSSP, Kabsch & Sander 1983) per frame and across the frames of an ensemble -- DESIGN.md section 3.23 ----
 * Where the helices and strands are, and in what share of the frames.  Frames and topology as for the arp_rmsd_* calls (xyz == NULL: the structure's models
 * are the frames).  The caller names the residues: bb[n_res][4] u32 are the topology atom indices of N, CA, C, O of residue r = 0 .. R - 1 in chain order,
 * flags[n_res] u8 carry ARP_DSSP_CHAIN_START (bit 0: r == 0, or r's chain differs from r - 1's) and ARP_DSSP_NO_H (bit 1: no amide hydrogen, proline).
 * All arithmetic is f64 in the order written; every distance is sqrt((dx dx + dy dy) + dz dz).  Per frame:
 *   brk[r]   = r == 0, or CHAIN_START, or |C[r-1] - N[r]| > 2.5.  cont(a, b), a <= b: 0 <= a, b < R and no brk in a + 1 .. b.
 *   H[r]     = N[r] + (C[r-1] - O[r-1]) / |C[r-1] - O[r-1]| (per component) where !brk[r] and not NO_H; any other residue donates nothing.
 *   E(i, j)  for acceptor i (its C=O) and donor j (its N-H), i != j, i != j - 1, |CA[i] - CA[j]| < 9.0:
 *            27.888 * (((1 / d(O_i, N_j) + 1 / d(C_i, H_j)) - 1 / d(O_i, H_j)) - 1 / d(C_i, N_j)); -9.9 where one of the four distances is < 0.5.
 *            E is NOT rounded to three decimals (mkdssp rounds; a pair within 5e-4 of the threshold can differ from it).
 *   best[j]  the two acceptors of donor j with the lowest E, the lower i on equal E;  hb(i, j) = i is one of them and E(i, j) < -0.5.
 *   turn_n(i), n = 3, 4, 5 = cont(i, i + n) and hb(i, i + n).
 *   A bridge is considered for |i - j| >= 3, cont(i - 1, i + 1) and cont(j - 1, j + 1):
 *     par(i, j)  = [hb(i-1, j) and hb(j, i+1)] or [hb(j-1, i) and hb(i, j+1)];   anti(i, j) = [hb(i, j) and hb(j, i)] or [hb(i-1, j+1) and hb(j-1, i+1)].
 *   States, codes 0 .. 7 of the string "-HBEGITS", assigned in this order:
 *     B  i has a bridge.   E  par(i, j) and (par(i-1, j-1) or par(i+1, j+1)), or anti(i, j) and (anti(i-1, j+1) or anti(i+1, j-1)), for some j.  Ladders are
 *        NOT linked across beta bulges (mkdssp links them: a bulge residue it calls E stays B or loop here).
 *     H  turn_4(i-1) and turn_4(i) set i .. i+3, over B and E.
 *     G  for i ascending, turn_3(i-1) and turn_3(i) set i .. i+2 when all three are '-' or G at that moment: all three or none.   I  the same with turn_5, i .. i+4.
 *     T  k still '-' and some turn_n(i) with i < k < i + n.
 *     S  k still '-', cont(k-2, k+2) and cos of the angle between CA[k] - CA[k-2] and CA[k+2] - CA[k] < cos 70 deg = 0.3420201433256687 (the dot product
 *        (x x' + y y') + z z' over the product of the two lengths).
 * Outputs: codes[F][R] u8 (may be NULL); counts[R][8] u32, in how many frames residue r has each code; frame_counts[F][8] u32 (may be NULL); hb_acceptor[F][R][2]
 * u32 (may be NULL): best[j], ARP_NONE where there is none; hb_energy[F][R][2] f32 (may be NULL): their E rounded once, 0 where there is none.
 * Checks, all before the device is touched, ARP_ERR_BAD_INPUT: the frame checks of the arp_rmsd_* calls; n_res == 0; n_res >= 2^28; a bb index >= N; a flag
 * bit other than the two (all under the prefix "dssp").  ctx == NULL runs only the checks (ARP_OK).
 * The frames go through the device in the upload passes of the arp_rmsd_* calls ("rmsd_chunk_atoms"); no frame depends on another, so device memory is one
 * pass plus counts, whatever F is.  The only atomics are u32 additions: two calls give identical bytes, for any pass size.  Synchronous. */
#define ARP_DSSP_CHAIN_START 1u
#define ARP_DSSP_NO_H 2u
arp_status arp_dssp(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const uint32_t *bb, const uint8_t *flags, uint64_t n_res,
                    uint8_t *codes, uint32_t *counts, uint32_t *frame_counts, uint32_t *hb_acceptor, float *hb_energy);
/* The definition above in plain sequential C++ without a device, on already-gathered coordinates bb_xyz n_frames x n_res x 4 (N, CA, C, O) x 3 f64; bridges are
 * found by trying every j.  The outputs are arp_dssp's (counts required, the others may be NULL).  n_frames or n_res == 0, a flag bit other than the two and a
 * non-finite coordinate are ARP_ERR_BAD_INPUT.  The CPU yardstick of the device kernels: codes, counts and acceptors agree exactly wherever no comparison of the
 * definition is within rounding of its threshold. */
arp_status arp_dssp_host(uint64_t n_frames, uint64_t n_res, const double *bb_xyz, const uint8_t *flags, uint8_t *codes, uint32_t *counts, uint32_t *frame_counts,
                         uint32_t *hb_acceptor, float *hb_energy);

/* ---- Torsion angles, rotamer states and Ramachandran maps across the frames of an ensemble -- DESIGN.md section 3.24 ----
 * What phi, psi, omega and the chi angles are in every frame, in which well each sits and how often it jumps, and the two-dimensional histogram of (phi, psi).
 * Frames and topology as for arp_dssp (xyz == NULL: the structure's models are the frames).  The caller names the torsions: quads[n_tors][4] u32 are topology
 * atom indices p0 .. p3 of torsion d = 0 .. D - 1 (the Python layer's torsion_select builds them); quads may repeat and overlap.
 * One torsion, all f64 in the order written (the library is built with -ffp-contract=off):
 *   b1 = p1 - p0, b2 = p2 - p1, b3 = p3 - p2;  n1 = b1 x b2, n2 = b2 x b3, cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x)
 *   x = (n1.x n2.x + n1.y n2.y) + n1.z n2.z
 *   y = sqrt((b2.x b2.x + b2.y b2.y) + b2.z b2.z) * ((b1.x n2.x + b1.y n2.y) + b1.z n2.z)
 *   h = sqrt(x x + y y).  The torsion is defined in this frame iff h > 0 and h is finite (a repeated atom or a collinear triple leaves it undefined).
 *   c = x / h, s = y / h;  a = atan2(y, x) * (180 / pi) in (-180, 180], IUPAC sign: p0 = (1,0,0), p1 = 0, p2 = (0,0,1), p3 = (cos t, sin t, 1) has a = t.
 *   state u8: 0 undefined; 2 (t) where c <= -0.5; 1 (g+) where not t and s >= 0; 3 (g-) otherwise -- the wells |a| >= 120, [0, 120), (-120, 0), decided from c
 *     and s alone, which are correctly rounded on the device and on the host: both agree bit for bit on c, s and the state.
 *   bin, n_bins = B > 0, w = 360 / B: k = floor((a + 180) / w), k -= B if k >= B (+180 falls into bin 0; a quotient below 0, which only the rounding of
 *     atan2(-0, x < 0) * (180 / pi) = -180 could give, counts as 0).  The one place where atan2 decides an integer.
 * Over the frames, per torsion d: n_defined[d]; state_counts[d][4], the frames in each state; n_transitions[d], the f in 1 .. F - 1 whose states at f - 1 and f
 * are both non-zero and differ; sums[d][2] = (sum c, sum s) over the defined frames -- slabs of 32 frames, each summed in frame order, wave j of four sums the
 * slabs j, j + 4, .., the four meet in a fixed tree: a function of F alone, no floating-point atomic; hist[d][B] u32, the frames per bin.
 * Ramachandran maps: pairs[n_pairs][3] u32 = (torsion a, torsion b, group), group < n_groups; hist2[G][B][B] u32 gets + 1 at [group][bin(a)][bin(b)] for every
 * frame in which both are defined.  The caller chooses the groups (the Python layer: four residue classes, or one group per residue).
 * Outputs: angles[F][D] f32 (may be NULL; undefined: the bits 0x7FC00000), cossin[F][D][2] f64 (may be NULL; undefined: 0, 0), states[F][D] u8 (may be NULL),
 * sums, n_defined, state_counts, n_transitions (required with a context), hist (may be NULL), hist2 (may be NULL; pairs are read only with it).
 * Checks, all before the device is touched: the frame checks of the arp_rmsd_* calls with their messages; then ARP_ERR_BAD_INPUT under the prefix "torsions:" for
 * n_tors == 0, an atom index >= N, n_bins > 360, hist or hist2 with n_bins == 0, hist2 with n_groups == 0 or n_pairs == 0, a pair's torsion >= D or group >= G.
 * The device keeps one state byte per (frame, torsion), the slab sums (D x 16 bytes per 32 frames) and the two histograms resident: their bytes against
 * "rmsd_cap_bytes" are ARP_ERR_CAPACITY.  ctx == NULL runs only the checks (ARP_OK).
 * The frames go through the device in the upload passes of the arp_rmsd_* calls ("rmsd_chunk_atoms").  Transitions are counted from the state bytes after the last
 * pass; the only atomics are u32 additions: two calls give identical bytes for every output, for any pass size.  Synchronous. */
arp_status arp_torsions(arp_context *ctx, arp_structure *topology, uint64_t n_frames, const double *xyz, const uint32_t *quads, uint64_t n_tors, uint32_t n_bins,
                        const uint32_t *pairs, uint64_t n_pairs, uint32_t n_groups, float *angles, double *cossin, uint8_t *states, double *sums, uint32_t *n_defined,
                        uint32_t *state_counts, uint32_t *n_transitions, uint32_t *hist, uint32_t *hist2);
/* The definition above in plain sequential C++ without a device, on already-gathered coordinates quad_xyz n_frames x n_tors x 4 x 3 f64.  The outputs are
 * arp_torsions' (sums, n_defined, state_counts and n_transitions required).  sums run in frame order: they agree with the device within the reordering of at most F
 * terms of magnitude <= 1; everything else agrees exactly, except that angles may differ in the last bits of atan2 (and a bin where an angle is within that of an
 * edge).  n_frames == 0, a non-finite coordinate and the shape checks above are ARP_ERR_BAD_INPUT. */
arp_status arp_torsions_host(uint64_t n_frames, uint64_t n_tors, const double *quad_xyz, uint32_t n_bins, const uint32_t *pairs, uint64_t n_pairs, uint32_t n_groups,
                             float *angles, double *cossin, uint8_t *states, double *sums, uint32_t *n_defined, uint32_t *state_counts, uint32_t *n_transitions,
                             uint32_t *hist, uint32_t *hist2);

/* ---- SASA and SAP statistics over the frames of an ensemble (MD snapshots, NMR models, conformers of one topology) -- DESIGN.md section 3.8 ----
 * Topology, N, frames and xyz exactly as arp_contact_frequencies defines them: model 0 of `topology` is the topology, frame f is xyz[f]
 * (n_frames x N x 3 f64, host, C order); xyz == NULL: the structure's models are the frames, with the same one-for-one model check and its error.
 * Selection: steps 1-3 of arp_structure_sasa_select (chain filter, hydrogens out, solvent / ion residues out) on model 0's atoms -- no step 4 / 5:
 * the models are the frames here.  m selected atoms, in structure order; R_k = f32(van der Waals radius) + probe as arp_structure_atom_sasa
 * (an element without a radius is its error).
 * Per frame f, by definition:
 *   count[f][k], sasa[f][k] = what arp_atom_sasa returns for the m selected atoms with frame f's coordinates, their van der Waals radii (f32), `probe`, include all ones
 *     (counts are integers: exact, whatever the pass size).
 *   with_sap: w[f][k] = arp_sap_weight(residue name of k, sasa[f][k]) (bit for bit); sap[f][k] = arp_sap_neighbor_sum over the side-chain atoms
 *     of the selection (atom name not N CA C O OXT) with frame f's f64 coordinates, the weights w[f][:] and sap_radius; 0 for backbone atoms.
 *     The f32 additions of a neighbour sum run in the order of the cell list the frame sits in, and that list depends on what the pass holds
 *     (every frame of a pass is a model of one packed grid, sized by the largest frame; one z layer or one cell row per wave by task count):
 *     sap[f][k] may differ in its last bits from the per-frame call and between pass sizes.  Two calls with the same inputs and the same
 *     pass size give identical bytes in every output; SASA outputs are identical for every pass size.
 * Per selected atom k, over the F frames (independent of pass boundaries given the per-frame values):
 *   S1 = sum count, S2 = sum count^2 (u64), cmin, cmax; b = (4 pi R_k) R_k in f64, left to right (4 pi = 4.0 * the double nearest pi);
 *   mean_sasa = f32(b * S1 / n_points / F), min_sasa = f32(b * cmin / n_points), max_sasa = f32(b * cmax / n_points) -- the last two are the
 *   per-frame sasa values of those counts --, std_sasa = f32(b * sqrt(D) / n_points / F) with D = F S2 - S1^2 formed exactly in 128-bit integers
 *   and converted to f64 once (population standard deviation); every expression is one f64 chain evaluated left to right, rounded to f32 once.
 *   with_sap: T1 = sum of (f64) sap[f][k], T2 = sum of (f64) sap[f][k]^2, both added in f64 in frame order 0 .. F - 1; mu = T1 / F;
 *   mean_sap = f32(mu), std_sap = f32(sqrt(max(T2 / F - mu * mu, 0))), min_sap / max_sap over the frames.
 * Per frame: total_sasa[f] = f32 of the f64 sum of sasa[f][k] over k in atom order.
 * Outputs: *n_rows = m, *frames_used = F, out_atoms[m] structure atom indices; the per-atom arrays hold m entries (arp_structure_n_atoms entries
 * always suffice); total_sasa holds F; the *_sap arrays are written only with with_sap (else they may be NULL); out_count (i32) / out_sap (f32),
 * both F x m in C order and both nullable, are only copied back when given (out_sap needs with_sap).
 * Errors before the device is touched (ARP_ERR_BAD_INPUT): the model check, n_frames == 0 with xyz, N >= 2^29, n_points / probe as
 * arp_atom_sasa, sap_radius < 0 or NaN, an element without a radius, a non-finite coordinate of a selected atom.  ctx == NULL runs only these
 * checks and writes *n_rows, *frames_used and (when given) out_atoms.  An empty selection is ARP_OK with 0 rows and zero totals.
 * Frames run through the device in passes of about 2 x 10^6 packed atoms (arp_debug_set "ens_chunk_atoms"), at most 65535 frames each; device
 * memory is one pass plus the per-atom accumulators, whatever F is.  Synchronous. */
arp_status arp_sasa_ensemble(arp_context *ctx, const arp_structure *topology, uint64_t n_frames, const double *xyz, const char *chains, float probe,
                             int32_t n_points, int32_t with_sap, float sap_radius, uint64_t *n_rows, uint64_t *frames_used, uint32_t *out_atoms,
                             float *mean_sasa, float *std_sasa, float *min_sasa, float *max_sasa, float *mean_sap, float *std_sap, float *min_sap,
                             float *max_sap, float *total_sasa, int32_t *out_count, float *out_sap);
/* The host-side finishing of arp_sasa_ensemble on its own (no device): the formulas above from the accumulators of m atoms; R = radius + probe.
 * t1 / t2 / mean_sap / std_sap are given together or all NULL. */
arp_status arp_sasa_ensemble_stats(uint64_t n_frames, uint64_t m, const float *R, int32_t n_points, const uint64_t *s1, const uint64_t *s2,
                                   const int32_t *cmin, const int32_t *cmax, const double *t1, const double *t2, float *mean_sasa, float *std_sasa,
                                   float *min_sasa, float *max_sasa, float *mean_sap, float *std_sap);

/* arp_sasa_ensemble without SAP, with the radii of `table` (ARP_RADII_VDW: the same bytes). */
arp_status arp_sasa_ensemble_radii(arp_context *ctx, const arp_structure *topology, uint64_t n_frames, const double *xyz, const char *chains, float probe,
                                   int32_t n_points, int32_t table, uint64_t *n_rows, uint64_t *frames_used, uint32_t *out_atoms, float *mean_sasa,
                                   float *std_sasa, float *min_sasa, float *max_sasa, float *total_sasa, int32_t *out_count);
/* Residue level across the frames of an ensemble.  Topology, frames, selection (m atoms), checks, NULL-context mode, pass
 * sizing and the memory bound are arp_sasa_ensemble's; radii from `table`.  The residues and chains of the selection and their order are those
 * of arp_structure_residue_sasa / arp_structure_chain_sasa.  Per frame f: rs[f][r] and chain_sasa[f][c] are the segment sums (arp_segment_sum)
 * of frame f's per-atom SASA values -- what the single-structure calls give for that frame, for every pass size.  Per residue over the frames:
 * T1 = sum rs, T2 = sum rs^2 (f64, frame order 0 .. F - 1 whatever the pass size), mu = T1 / F, mean_sasa = f32(mu),
 * std_sasa = f32(sqrt(max(T2 / F - mu * mu, 0))), min_sasa / max_sasa over the frames; mean_relative = mean_sasa / arp_max_asa (f32) with
 * relative_valid = 1, or NaN / 0 without a MaxASA.
 * Outputs: *n_rows residues, *n_chains chains, *frames_used = F; out_res_atoms / out_chain_atoms: the first selected atom of every residue /
 * chain; the per-residue arrays and out_*_atoms hold arp_structure_n_atoms entries at most; chain_sasa holds F x n_chains (C order);
 * residue_sasa (F x n_rows, nullable) is copied back only when given.  ctx == NULL runs only the checks and writes the three counts and (when
 * given) out_res_atoms / out_chain_atoms: the way to size chain_sasa.  An empty selection is ARP_OK with 0 rows and 0 chains.  Synchronous. */
arp_status arp_sasa_ensemble_residues(arp_context *ctx, const arp_structure *topology, uint64_t n_frames, const double *xyz, const char *chains, float probe,
                                      int32_t n_points, int32_t table, uint64_t *n_rows, uint64_t *n_chains, uint64_t *frames_used, uint32_t *out_res_atoms,
                                      uint8_t *out_is_polar, float *mean_sasa, float *std_sasa, float *min_sasa, float *max_sasa, float *mean_relative,
                                      uint8_t *relative_valid, uint32_t *out_chain_atoms, float *chain_sasa, float *residue_sasa);

/* ---- buried surface per atom and residue, dSASA over the frames of an ensemble (no counterpart in the reference) ----
 * Every atom carries a group mask: 0 = not in the calculation, bit 0 = in group 1, bit 1 = in group 2 (3 = in both).  With the burial test of
 * arp_atom_sasa unchanged, one kernel walk gives atom i three counts of open points: against every other atom with a non-zero mask (the
 * complex), against the other atoms of group 1, and against the other atoms of group 2; a group count is 0 where the atom is not in that
 * group.  Areas are f32(4 pi R_i^2 count / n_points) as in arp_atom_sasa, and buried = the atom's own group counts minus its complex count,
 * in points, >= 0.  The complex count equals arp_atom_sasa's on the union, a group count equals arp_atom_sasa's on that group alone, exactly.
 * out_count / out_sasa: three planes of n entries (complex, group 1, group 2); out_buried: n.  Masks above 3 and a negative or non-finite radius
 * of an atom with a non-zero mask are ARP_ERR_BAD_INPUT (checked before the device is touched), as is a call on a context with an uncollected
 * enqueued call.  The atom limit is arp_atom_sasa's.  Synchronous. */
arp_status arp_atom_sasa_groups(arp_context *ctx, uint64_t n, const double *x, const double *y, const double *z, const float *radius,
                                const uint8_t *group, float probe, int32_t n_points, int32_t *out_count, float *out_sasa, int32_t *out_buried);
/* The same on a structure, for the `groups` of arp_structure_dsasa (same selection, same group errors, the named radius table).  Rows: the atoms
 * of the two groups' union in arp_structure_atom_sasa's order (by serial, stable); out_atoms (structure index), out_group (1, 2, 3), out_buried hold
 * *n_rows entries, out_sasa / out_count three planes of *n_rows entries (complex, group 1, group 2).  Residue rows (arp_structure_residue_sasa's
 * rows and order, over the union): out_res_atoms (first selected atom), out_res_sasa three planes of *n_res_rows sums (every sum the f64 chain
 * of arp_segment_sum), out_res_buried_atoms (atoms of the residue with buried > 0).  out_totals[4]: complex, group 1, group 2 (each the f64
 * sum in selection order rounded to f32 once) and group 1 + group 2 - complex in f32, which equals arp_structure_dsasa_radii on the same
 * arguments bit for bit; a negative value is the same error.  Every array holds arp_structure_n_atoms entries (x 3 for the planes) at most.
 * The checks that need no device (null arguments, n_points, probe, table, groups) run first, with ctx == NULL as well. */
arp_status arp_structure_buried_sasa(arp_context *ctx, const arp_structure *s, const char *groups, float probe, int32_t n_points, int32_t model_num,
                                     int32_t table, uint64_t *n_rows, uint32_t *out_atoms, uint8_t *out_group, float *out_sasa, int32_t *out_count,
                                     int32_t *out_buried, uint64_t *n_res_rows, uint32_t *out_res_atoms, float *out_res_sasa,
                                     uint32_t *out_res_buried_atoms, float *out_totals);
/* The scalar of arp_structure_dsasa from its three totals: *out = total_g1 + total_g2 - total_complex in f32 (sasa.rs:450); a negative value
 * is ARP_ERR_BAD_INPUT with the reference's message (*out is written all the same).  No device. */
arp_status arp_dsasa_total(float total_complex, float total_g1, float total_g2, float *out);
/* dSASA over the frames of an ensemble, frames packed on the device as in arp_sasa_ensemble (topology, n_frames, xyz, the pass size knob
 * ens_chunk_atoms: as there; the selection is steps 1-3 of arp_structure_sasa_select on the union of the two groups).  Per selected atom:
 * out_atoms, out_group, out_R (radius + probe), and over the frames in frame order the integer accumulators of buried (in points):
 * sum_buried, sum_buried_sq, min_buried, max_buried, frames_buried (frames with buried > 0) -- arp_sasa_ensemble_stats turns the first four
 * into areas.  Per frame: total_complex, total_g1, total_g2 (the f64 sum over the selection rounded to f32 once) and dsasa = g1 + g2 - complex
 * in f32; a negative frame value is returned as it is.  out_buried (n_frames x *n_rows, nullable) is copied back per pass when given.
 * ctx == NULL runs only the checks and writes *n_rows, *frames_used and (when given) out_atoms, out_group, out_R.  Synchronous. */
arp_status arp_dsasa_ensemble(arp_context *ctx, const arp_structure *topology, uint64_t n_frames, const double *xyz, const char *groups, float probe,
                              int32_t n_points, int32_t table, uint64_t *n_rows, uint64_t *frames_used, uint32_t *out_atoms, uint8_t *out_group,
                              float *out_R, uint64_t *sum_buried, uint64_t *sum_buried_sq, int32_t *min_buried, int32_t *max_buried,
                              uint32_t *frames_buried, float *total_complex, float *total_g1, float *total_g2, float *dsasa, int32_t *out_buried);

/* The same 20 columns through the Arrow C Data Interface (a struct array = one record batch; utf8 strings, nullable
 * f32 sc_* columns): what pyo3-polars hands to Python in the reference (python.rs:55, mod.rs:140-214), importable with
 * zero per-row work by pyarrow / polars / arrow-rs (`FFI_ArrowArray`).  The exported arrays own copies of the columns:
 * the table may be freed before they are released.  Struct layout per the Arrow specification (ABI-stable). */
#ifndef ARROW_C_DATA_INTERFACE
#define ARROW_C_DATA_INTERFACE
struct ArrowSchema {
    const char *format, *name, *metadata;
    int64_t flags, n_children;
    struct ArrowSchema **children, *dictionary;
    void (*release)(struct ArrowSchema *);
    void *private_data;
};
struct ArrowArray {
    int64_t length, null_count, offset, n_buffers, n_children;
    const void **buffers;
    struct ArrowArray **children, *dictionary;
    void (*release)(struct ArrowArray *);
    void *private_data;
};
#endif
arp_status arp_table_export_arrow(const arp_table *t, struct ArrowArray *out_array, struct ArrowSchema *out_schema);

#ifdef __cplusplus
}
#endif
#endif
