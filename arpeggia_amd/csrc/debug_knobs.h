// The library's diagnostic switches (arp_debug_set, include/arpeggia_amd.h).  Shared by the kernel launchers and the host sources.
#pragma once
namespace arp {
// Set through arp_debug_set: the library reads no switch from the environment.
struct DebugKnobs {
    int timing;          // stage laps of the table / batch / ingest paths on stderr
    int emit_kernel;     // 1: the single-pass emitter runs k_pairs<kEmit> (both operands gathered: the route of inputs beyond 2^24 slots) -- parity suite
    long defer_entries;  // > 0: entries of the deferred-probe list of workspaces allocated from now on (tests: a tiny list makes the grow-and-repeat path run)
    int strip_rows;      // > 0: rows per y strip of the cell order (a power of two) for parameter blocks built from now on; 0: chosen by input size (grid.inl grid_setup)
    int index_bits;      // the narrow exact record of the single-pass emitter (emit_plan.h plan_emit): 0: index width chosen by input size; 1 .. 20: that width
                         // (an input whose last index does not fit keeps the wide record); < 0: the wide record always
    int table_host;      // test-only library (-DARP_WITH_HOST_TABLE): arp_get_contacts assembles the table on the host
    long freq_chunk_atoms;  // > 0: atoms per pass of arp_contact_frequencies (whole frames, at least one); 0: automatic (freq.inl kFreqAutoAtoms)
    long freq_cap_items;    // > 0: items of the first aggregate + item buffers of arp_contact_frequencies (tests: a tiny buffer makes the grow-and-repeat path run); 0: max(65536, 2 x pairs)
    long freq_frame_bits;   // > 0: frame-tag bits of the keys of arp_residue_contact_frequencies (at most 2^k - 1 frames per pass; tests: tiny inputs reach the frame cap); 0: automatic (freq.inl)
    long ens_chunk_atoms;   // > 0: packed atoms per pass of arp_sasa_ensemble (whole frames, at least one); 0: automatic (sasa_dev.cpp kEnsAutoAtoms)
    long long timeline_cap_bytes;  // > 0: the most device memory the bitmap of arp_contact_timelines may take (tests: the capacity error on tiny inputs); 0: 2^31 bytes
    long long similarity_cap_bytes;  // > 0: the most bytes the matrix of arp_contact_similarity / arp_bit_gram may take (tests: the capacity error on tiny inputs); 0: 2^31 bytes
    long long autocorr_cap_bytes;  // > 0: the most bytes the device matrix of arp_contact_autocorrelation / arp_bit_autocorr may take (tests: the capacity error on tiny inputs); 0: 2^31 bytes
    long long cluster_cap_bytes;  // > 0: the most bytes the neighbour bits, and the counts, of arp_contact_clusters / arp_bit_cluster may take (tests: the capacity error on tiny inputs); 0: 2^31 bytes
    long rmsd_chunk_atoms;  // > 0: atoms per upload pass of the arp_rmsd_* calls (whole frames, at least one; tests: several passes on tiny inputs); 0: automatic (freq.inl kFreqAutoAtoms)
    long long rmsd_cap_bytes;  // > 0: the most bytes the matrix of arp_rmsd_matrix, the neighbour bits of arp_rmsd_clusters and the packed frames of either may take (tests: the capacity error on tiny inputs); 0: 2^31 bytes
    long sc_ens_frames;    // > 0: frames per pass of arp_sc_ensemble (tests: pass edges at tiny shapes); 0: from the memory budget (sc_ens.inl launch_sc_ens)
    int scan_kernel;    // the cell scan (pairs.inl launch_grid): 0: chosen by input size; 1: the look-back scan k_scan_single on 256 blocks; 2: on 1 024 blocks (tests: small inputs reach it)
    int table_key_bits;  // > 0: stands for the 64 of the table plan's three width tests (table_plan.h plan_table; tests: small inputs reach the plans of wide keys); 0: 64
    int torsion_hist2_route;  // the Ramachandran maps of arp_torsions (torsion.inl): 0: chosen by G B^2; 1: per-workgroup LDS tables (falls back to 2 where they do not fit); 2: wave-matched global adds; 3: one global add per sample (measurements)
};
extern DebugKnobs g_debug;

}  // namespace arp
