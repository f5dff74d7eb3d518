"""arpeggia_amd: MI355X-native drop-in for the `contacts` path of y1zhou/arpeggia.

Public surface mirrors the reference (src/lib.rs:20-34, src/python.rs:31-56) for this one path:
contacts(), get_contacts(), load_model(), parse_groups(); and sasa(), relative_sasa(), sap_score(), dsasa(), buried_sasa(); and sc(); and
contact_frequencies(), contact_timelines(), contact_similarity(), contact_autocorrelation(), contact_clusters(), rmsd(), rmsd_matrix(), rmsd_clusters(), rmsf(), covariance(), dccm(), pca(), secondary_structure(), torsions(), sasa_ensemble(), sap_ensemble(), dsasa_ensemble() and sc_ensemble() across the frames of an ensemble (no counterpart in the reference).  Importing this package loads libarpeggia_amd.so and
fails loudly if the HIP extension has not been built -- there is no CPU fallback.
"""
from .api import (  # noqa: F401
    ArpeggiaError, Context, Structure, PAIR_DTYPE, TABLE_COLUMNS, atomic_contacts_batch, atoms_from_arrays, contacts, contacts_batch, debug_get, debug_set, default_params,
    device_count, get_contacts, load_model, parse_groups, sap_neighbor_sum, sap_weight,
)
from .api import (  # noqa: F401  atom SASA, SAP score, dSASA (reference src/sasa.rs, src/sap.rs)
    atom_sasa, dsasa, get_atom_sasa, get_dsasa, get_per_atom_sap_score, get_per_residue_sap_score, sap_score, sasa, sasa_select,
    sasa_sphere_points, sasa_tests,
)
from .api import (  # noqa: F401  residue- and chain-level SASA, relative SASA (src/sasa.rs:284-382, 520-561), segment sums on the device
    CHAIN_SASA_COLUMNS, RELATIVE_SASA_COLUMNS, RESIDUE_ENSEMBLE_SASA_COLUMNS, RESIDUE_SASA_COLUMNS, get_chain_sasa, get_relative_sasa, get_residue_sasa,
    get_residue_sasa_ensemble, max_asa, relative_sasa, sasa_radius, segment_sum,
)
from .api import get_sc, get_sc_results, sc, sc_arrays, sc_dots, sc_radius, sc_select  # noqa: F401  shape complementarity (src/sc/)
from .api import (  # noqa: F401  shape complementarity across the frames of an ensemble
    SC_ENSEMBLE_COLUMNS, SC_FRAME_COLUMNS, SC_FRAME_STATUS, SC_RESULTS_DTYPE, get_sc_ensemble, sc_arrays_ensemble, sc_dot_atoms, sc_dot_stats, sc_ensemble,
    sc_frame_table,
)
from .api import FREQ_COLUMNS, RESIDUE_FREQ_COLUMNS, contact_frequencies, get_contact_frequencies  # noqa: F401  contact frequencies across the frames of an ensemble
from .api import WATER_BRIDGE_COLUMNS, get_water_bridges, water_bridges  # noqa: F401  water-mediated contacts, bridge by bridge
from .api import TIMELINE_COLUMNS, contact_timelines, get_contact_timelines, timeline_stats, unpack_timeline  # noqa: F401  which frames each contact exists in
from .api import bit_gram, contact_similarity, get_contact_similarity  # noqa: F401  which frames look alike, which contacts come and go together
from .api import bit_cluster, contact_clusters, get_contact_clusters  # noqa: F401  which states there are, which frame stands for each, which contacts tell them apart
from .api import get_rmsd, get_rmsd_clusters, get_rmsd_matrix, rmsd, rmsd_clusters, rmsd_host, rmsd_matrix, rmsd_select  # noqa: F401  how far each frame is from a reference, which frames are the same conformation
from .api import RMSF_COLUMNS, RMSF_RESIDUE_COLUMNS, get_rmsf, rmsf, rmsf_host, rmsf_residues, rmsf_table  # noqa: F401  how much each atom moves about the mean structure
from .api import DCCM_COLUMNS, covariance, covariance_host, dccm, dccm_table, get_covariance, get_dccm, get_pca, get_projection, pca, pca_modes, project_host  # noqa: F401  which atoms move together, and along which collective directions
from .api import (  # noqa: F401  where the helices and strands are, and in what share of the frames
    SS_CODES, SS_COLUMNS, backbone_select, get_secondary_structure, secondary_structure, secondary_structure_host, secondary_structure_table, ss_consensus, ss_string,
)
from .api import (  # noqa: F401  what phi, psi, omega and chi are, which rotamer each side chain sits in, the Ramachandran map of the ensemble
    CHI_ATOMS, RAMA_CLASSES, TORSION_COLUMNS, TORSION_KINDS, get_torsions, torsion_select, torsion_table, torsions, torsions_host,
)
from .api import bit_autocorrelation, contact_autocorrelation, get_contact_autocorrelation  # noqa: F401  how long a contact lives, how fast it decays
from .api import (  # noqa: F401  SASA / SAP statistics across the frames of an ensemble
    ENSEMBLE_SAP_COLUMNS, ENSEMBLE_SASA_COLUMNS, RESIDUE_ENSEMBLE_SAP_COLUMNS, get_residue_sap_ensemble, get_sap_ensemble, get_sasa_ensemble,
    sap_ensemble, sasa_ensemble, sasa_ensemble_stats,
)
from .api import (  # noqa: F401  buried surface per atom and residue, dSASA across the frames of an ensemble
    BURIED_ATOM_COLUMNS, BURIED_RESIDUE_COLUMNS, DSASA_ENSEMBLE_COLUMNS, DSASA_FRAME_COLUMNS, atom_sasa_groups, buried_sasa, dsasa_ensemble,
    dsasa_ensemble_stats, dsasa_total, get_buried_sasa, get_dsasa_ensemble,
)
from ._lib import ATTR, INTERACTIONS  # noqa: F401

__version__ = "0.1.0"
