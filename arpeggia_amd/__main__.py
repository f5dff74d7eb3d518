"""Command-line driver: `python -m arpeggia_amd contacts -i model.pdb -o out/` -- the flags and defaults of the reference's
`arpeggia contacts` (src/cli/contacts.rs:9-52) over the MI355X engine; it writes <output>/<filename>.<format> like cli/contacts.rs:108-137.
`sasa`, `relative-sasa`, `sap`, `dsasa` and `sc` take the flags and defaults of src/cli/{sasa,relative_sasa,sap,dsasa,sc}.rs; `sasa`, `dsasa` and
`sasa-ensemble` also take --radii {vdw,protor}: the radius table, which the residue and chain levels of `sasa` need (see arpeggia_amd/api.py).
`contact-frequency` (no counterpart in the reference) takes the flags and defaults of `contacts`; the models of the input file are the frames, and
--rings adds the ring rows (CationPi, Pi* stackings) of every model regarded as a single-model structure; --level residue writes one row per
residue pair and interaction (a model counts once however many of the residues' atoms are in contact).
`contact-timeline` (no counterpart either) takes the flags of `contact-frequency` and writes its table with five more columns per row -- first_frame,
last_frame, n_events, longest_run, mean_run: when the contact exists across the models -- and, with --bitmap FILE.npy, the rows' frame bitmap.
Both take --waters (with --level residue): the WaterBridge rows.  `water-bridges` (no counterpart either) writes every water bridge of every model.
`contact-similarity` (no counterpart either) takes the flags of `contact-timeline` without --bitmap, plus --axis frames|rows and --metric tanimoto|count:
it writes `contact-frequency`'s table and, with --matrix FILE.npy, the matrix between the models (or between the rows).
`contact-autocorrelation` (no counterpart either) takes the flags of `contact-timeline` without --bitmap, plus --mode intermittent|continuous and --max-lag N:
it writes `contact-frequency`'s table with one more column, half_life, and, with --matrix FILE.npy, the per-row counts, with --curves FILE.csv the curves.
`contact-clusters` (no counterpart either) takes the flags of `contact-timeline` without --bitmap, plus --min-similarity X (required) and --max-clusters N: it
writes `contact-frequency`'s table and, with --assignments FILE.csv, one line per model, with --cluster-counts FILE.npy the per-row counts inside each cluster.
`rmsd`, `rmsd-matrix` and `rmsd-clusters` (no counterpart either) superpose the models on --atoms ca|backbone|heavy|all of the chains -c: `rmsd` writes frame, rmsd
against --reference K; `rmsd-matrix` the matrix to --matrix FILE.npy; `rmsd-clusters` the gromos clusters at --cutoff X (required) with the --max-clusters and
--assignments of `contact-clusters`.
`rmsf` (no counterpart either) superposes the models on --fit ca|backbone|heavy|all onto --reference mean (the iterated mean structure, --max-rounds N, --tol X)
or model K, and writes per --atoms atom (default: the --fit atoms) or, with -l residue, per residue the mean position, rmsf and B-factor; --frames FILE.csv: each
model's rmsd to the mean; --aligned FILE.npy: the superposed coordinates.
`dccm` and `pca` (no counterpart either) take `rmsf`'s --fit, --atoms, -c, --reference, --max-rounds and --tol: `dccm` writes the dynamic cross-correlation map of
the measured atoms to --matrix FILE.npy and, with -o (and -f, -t), in long form; `pca` takes --modes K and writes --eigenvalues FILE.csv, --modes-file FILE.npy,
--projections FILE.csv and --covariance FILE.npy (the eigen-solve runs on the host).
`secondary-structure` (no counterpart either) assigns DSSP states (Kabsch & Sander) to the residues of the chains -c in every model and writes, with -o (and -f,
-t), per residue the share of the models in each state and the consensus state; --codes FILE.npy: the codes, uint8 [models, residues]; --strings FILE.txt: one line
of "-HBEGITS" characters per model.
`torsions` (no counterpart either) measures phi, psi, omega and chi1 .. chi5 (--kinds) of the residues of the chains -c in every model and writes, with -o (and
-f, -t), per torsion the circular mean, resultant and standard deviation, the shares of the models in g+, t and g- and the number of transitions; --angles
FILE.npy: the angles, float32 [models, torsions]; --rama-file FILE.npy: the Ramachandran maps, uint32 [groups, --bins, --bins], --rama class|residue.
`sasa-ensemble` and `sap-ensemble` (no counterpart either) take the flags and defaults of `sasa` / `sap` without --model: statistics over the models.
`dsasa --level atom|residue` writes the interface row by row (default `total`: the reference's scalar); `dsasa-ensemble` takes the flags of
`sasa-ensemble` and -g: dSASA per model and the per-atom statistics of the buried surface.
`sc-ensemble` (no counterpart either) takes -i, -g, -o, -f, -t: shape complementarity of every model, and with --atoms how often each atom owns a
trimmed dot of the interface.
"""
from __future__ import annotations

import argparse
import json
import logging
import sys
from pathlib import Path

FORMATS = ("csv", "parquet", "json", "ndjson")  # utils.rs:148-167 DataFrameFileType

RADII_HELP = "Radius table: vdw (element radii) or protor (ProtOr, Tsai et al. 1999); the residue and chain levels of sasa need one"

log = logging.getLogger("arpeggia_amd")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="arpeggia_amd", description="Interatomic contacts on MI355X (arpeggia-compatible)")
    sub = ap.add_subparsers(dest="command", required=True)
    c = sub.add_parser("contacts", help="atomic and ring contacts of a PDB / mmCIF model (cli/contacts.rs)")
    c.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file to be analyzed")
    c.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    c.add_argument("-g", "--groups", default="/", help="Chain groups, e.g. A,B/C,D ('/' = all against all)")
    c.add_argument("-f", "--filename", default="contacts", help="Name of the output file")
    c.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type")
    c.add_argument("-c", "--vdw-comp", default=0.1, type=float, help="Compensation factor for VdW radii dependent interaction types")
    c.add_argument("-d", "--dist-cutoff", default=6.5, type=float, help="Distance cutoff when searching for neighboring atoms")
    c.add_argument("-j", "--num-threads", default=1, type=int, help="Host threads of the table path (0 = all cores); the search runs on the GPU")
    c.add_argument("--ignore-zero-occupancy", action="store_true", help="Ignore atoms with zero occupancy")
    q = sub.add_parser("contact-frequency", help="how often each atom-atom contact occurs across the models of a multi-model file")
    q.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
    q.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    q.add_argument("-g", "--groups", default="/", help="Chain groups, e.g. A,B/C,D ('/' = all against all)")
    q.add_argument("-f", "--filename", default="contact_frequency", help="Name of the output file")
    q.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type")
    q.add_argument("-c", "--vdw-comp", default=0.1, type=float, help="Compensation factor for VdW radii dependent interaction types")
    q.add_argument("-d", "--dist-cutoff", default=6.5, type=float, help="Distance cutoff when searching for neighboring atoms")
    q.add_argument("-j", "--num-threads", default=1, type=int, help="Number of threads (accepted; the computation runs on the GPU)")
    q.add_argument("--ignore-zero-occupancy", action="store_true", help="Ignore atoms with zero occupancy")
    q.add_argument("--rings", action="store_true", help="Add the ring rows (CationPi, Pi stackings) of every model; ring-ring rows do not depend on --dist-cutoff")
    q.add_argument("-l", "--level", default="atom", choices=("atom", "residue"),
                   help="Rows per atom pair, or per residue pair (a model counts once however many of the residues' atoms are in contact)")
    q.add_argument("--waters", action="store_true", help="Add the WaterBridge rows: residue pairs joined through a water within 3.5 A of a polar atom of each (needs -l residue)")
    tl = sub.add_parser("contact-timeline", help="in which models each contact exists: first / last model, events, longest run (contact-frequency's rows)")
    tl.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
    tl.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    tl.add_argument("-g", "--groups", default="/", help="Chain groups, e.g. A,B/C,D ('/' = all against all)")
    tl.add_argument("-f", "--filename", default="contact_timeline", help="Name of the output file")
    tl.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type")
    tl.add_argument("-c", "--vdw-comp", default=0.1, type=float, help="Compensation factor for VdW radii dependent interaction types")
    tl.add_argument("-d", "--dist-cutoff", default=6.5, type=float, help="Distance cutoff when searching for neighboring atoms")
    tl.add_argument("-j", "--num-threads", default=1, type=int, help="Number of threads (accepted; the computation runs on the GPU)")
    tl.add_argument("--ignore-zero-occupancy", action="store_true", help="Ignore atoms with zero occupancy")
    tl.add_argument("--rings", action="store_true", help="Add the ring rows (CationPi, Pi stackings) of every model; ring-ring rows do not depend on --dist-cutoff")
    tl.add_argument("-l", "--level", default="atom", choices=("atom", "residue"),
                    help="Rows per atom pair, or per residue pair (a model counts once however many of the residues' atoms are in contact)")
    tl.add_argument("--waters", action="store_true", help="Add the WaterBridge rows: residue pairs joined through a water within 3.5 A of a polar atom of each (needs -l residue)")
    tl.add_argument("--bitmap", default=None, type=Path, metavar="FILE.npy",
                    help="Also write the rows' frame bitmap: uint32 [rows, ceil(models / 32)], model f = bit f %% 32 of word f // 32")
    wb = sub.add_parser("water-bridges", help="every water bridge of every model: the two bridged atoms, the water, both legs")
    wb.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
    wb.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    wb.add_argument("-g", "--groups", default="/", help="Chain groups, e.g. A,B/C,D ('/' = all against all)")
    wb.add_argument("-f", "--filename", default="water_bridges", help="Name of the output file")
    wb.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type")
    wb.add_argument("--ignore-zero-occupancy", action="store_true", help="Ignore atoms with zero occupancy")
    sm = sub.add_parser("contact-similarity", help="which models have the same contacts (Tanimoto matrix), or which contacts exist in the same models")
    sm.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
    sm.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    sm.add_argument("-g", "--groups", default="/", help="Chain groups, e.g. A,B/C,D ('/' = all against all)")
    sm.add_argument("-f", "--filename", default="contact_similarity", help="Name of the output file")
    sm.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type")
    sm.add_argument("-c", "--vdw-comp", default=0.1, type=float, help="Compensation factor for VdW radii dependent interaction types")
    sm.add_argument("-d", "--dist-cutoff", default=6.5, type=float, help="Distance cutoff when searching for neighboring atoms")
    sm.add_argument("-j", "--num-threads", default=1, type=int, help="Number of threads (accepted; the computation runs on the GPU)")
    sm.add_argument("--ignore-zero-occupancy", action="store_true", help="Ignore atoms with zero occupancy")
    sm.add_argument("--rings", action="store_true", help="Add the ring rows (CationPi, Pi stackings) of every model; ring-ring rows do not depend on --dist-cutoff")
    sm.add_argument("-l", "--level", default="atom", choices=("atom", "residue"),
                    help="Rows per atom pair, or per residue pair (a model counts once however many of the residues' atoms are in contact)")
    sm.add_argument("--axis", default="frames", choices=("frames", "rows"), help="Compare the models with each other (frames), or the table's rows (rows)")
    sm.add_argument("--metric", default="tanimoto", choices=("tanimoto", "count"), help="Tanimoto coefficient (float32), or the size of the intersection (uint32)")
    sm.add_argument("--matrix", default=None, type=Path, metavar="FILE.npy", help="Write the [M, M] matrix: M = models (--axis frames) or rows of the table (--axis rows)")
    ac = sub.add_parser("contact-autocorrelation", help="how long each contact lives across the models: autocorrelation / survival counts per lag, half-lives")
    ac.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
    ac.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    ac.add_argument("-g", "--groups", default="/", help="Chain groups, e.g. A,B/C,D ('/' = all against all)")
    ac.add_argument("-f", "--filename", default="contact_autocorrelation", help="Name of the output file")
    ac.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type")
    ac.add_argument("-c", "--vdw-comp", default=0.1, type=float, help="Compensation factor for VdW radii dependent interaction types")
    ac.add_argument("-d", "--dist-cutoff", default=6.5, type=float, help="Distance cutoff when searching for neighboring atoms")
    ac.add_argument("-j", "--num-threads", default=1, type=int, help="Number of threads (accepted; the computation runs on the GPU)")
    ac.add_argument("--ignore-zero-occupancy", action="store_true", help="Ignore atoms with zero occupancy")
    ac.add_argument("--rings", action="store_true", help="Add the ring rows (CationPi, Pi stackings) of every model; ring-ring rows do not depend on --dist-cutoff")
    ac.add_argument("-l", "--level", default="atom", choices=("atom", "residue"),
                    help="Rows per atom pair, or per residue pair (a model counts once however many of the residues' atoms are in contact)")
    ac.add_argument("--mode", default="intermittent", choices=("intermittent", "continuous"),
                    help="Count the models f where the contact exists in f and in f + lag (intermittent), or in every model from f to f + lag (continuous)")
    ac.add_argument("--max-lag", default=None, type=int, metavar="N", help="Largest lag (default: models - 1)")
    ac.add_argument("--matrix", default=None, type=Path, metavar="FILE.npy", help="Write the per-row counts: uint32 [rows, max lag + 1]")
    ac.add_argument("--curves", default=None, type=Path, metavar="FILE.csv", help="Write the window-corrected curve per interaction: lag, one column per interaction present")
    cl = sub.add_parser("contact-clusters", help="which states the models fall into by their contacts (gromos clusters on the Tanimoto similarity), and each state's centre")
    cl.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
    cl.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    cl.add_argument("-g", "--groups", default="/", help="Chain groups, e.g. A,B/C,D ('/' = all against all)")
    cl.add_argument("-f", "--filename", default="contact_clusters", help="Name of the output file")
    cl.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type")
    cl.add_argument("-c", "--vdw-comp", default=0.1, type=float, help="Compensation factor for VdW radii dependent interaction types")
    cl.add_argument("-d", "--dist-cutoff", default=6.5, type=float, help="Distance cutoff when searching for neighboring atoms")
    cl.add_argument("-j", "--num-threads", default=1, type=int, help="Number of threads (accepted; the computation runs on the GPU)")
    cl.add_argument("--ignore-zero-occupancy", action="store_true", help="Ignore atoms with zero occupancy")
    cl.add_argument("--rings", action="store_true", help="Add the ring rows (CationPi, Pi stackings) of every model; ring-ring rows do not depend on --dist-cutoff")
    cl.add_argument("-l", "--level", default="atom", choices=("atom", "residue"),
                    help="Rows per atom pair, or per residue pair (a model counts once however many of the residues' atoms are in contact)")
    cl.add_argument("--min-similarity", required=True, type=float, metavar="X", help="Two models are neighbours when their Tanimoto similarity is at least X (0 .. 1)")
    cl.add_argument("--max-clusters", default=None, type=int, metavar="N", help="Stop after N clusters; the models left over stay unassigned (default: no limit)")
    cl.add_argument("--assignments", default=None, type=Path, metavar="FILE.csv",
                    help="Write one line per model: frame, cluster, is_centre, similarity_to_centre, n_neighbours, size")
    cl.add_argument("--cluster-counts", default=None, type=Path, metavar="FILE.npy", help="Write in how many models of each cluster a row's contact exists: uint32 [rows, clusters]")
    for name, hlp in (("rmsd", "how far each model is from a reference model after optimal superposition: frame, rmsd"),
                      ("rmsd-matrix", "the rmsd between every two models after optimal superposition"),
                      ("rmsd-clusters", "which models are the same conformation (gromos clusters on rmsd <= cutoff), and each cluster's centre")):
        rm = sub.add_parser(name, help=hlp)
        rm.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
        rm.add_argument("--atoms", default="ca", choices=("ca", "backbone", "heavy", "all"), help="Atoms to superpose on (residue HOH is never among them)")
        rm.add_argument("-c", "--chains", default="", help="Comma-separated chain IDs to include (empty: all)")
        rm.add_argument("--ignore-zero-occupancy", action="store_true", help="Ignore atoms with zero occupancy")
        if name == "rmsd-matrix":
            rm.add_argument("--matrix", required=True, type=Path, metavar="FILE.npy", help="Write the matrix: float32 [models, models]")
            continue
        rm.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
        rm.add_argument("-f", "--filename", default=name.replace("-", "_"), help="Name of the output file (.csv)")
        if name == "rmsd":
            rm.add_argument("--reference", default=0, type=int, metavar="K", help="The reference model (0: the first)")
        else:
            rm.add_argument("--cutoff", required=True, type=float, metavar="X", help="Two models are neighbours when their rmsd is at most X Angstroms")
            rm.add_argument("--max-clusters", default=None, type=int, metavar="N", help="Stop after N clusters; the models left over stay unassigned (default: no limit)")
            rm.add_argument("--assignments", default=None, type=Path, metavar="FILE.csv", help="Write one line per model: frame, cluster, is_centre, rmsd_to_centre, n_neighbours")
    rf = sub.add_parser("rmsf", help="how much each atom moves across the models: superpose them on their mean structure (or on one model), average, and report the "
                                     "fluctuation of every atom or residue about the average")
    rf.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
    rf.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    rf.add_argument("-f", "--filename", default="rmsf", help="Name of the output file (.csv)")
    rf.add_argument("--fit", default="ca", choices=("ca", "backbone", "heavy", "all"), help="Atoms to superpose on (residue HOH is never among them)")
    rf.add_argument("--atoms", default=None, choices=("ca", "backbone", "heavy", "all"), help="Atoms to measure (default: the atoms of --fit)")
    rf.add_argument("-c", "--chains", default="", help="Comma-separated chain IDs to include (empty: all)")
    rf.add_argument("--reference", default="mean", type=_rmsf_reference_arg, metavar="mean|K", help="Superpose on the iterated mean structure, or on model K (0: the first)")
    rf.add_argument("--max-rounds", default=50, type=int, metavar="N", help="With --reference mean: at most N rounds of superposing and averaging")
    rf.add_argument("--tol", default=1e-4, type=float, metavar="X", help="With --reference mean: stop when the mean moves by at most X Angstroms (rms over the fit atoms)")
    rf.add_argument("-l", "--level", default="atom", choices=("atom", "residue"), help="Rows per measured atom, or per residue of the measured atoms")
    rf.add_argument("--frames", default=None, type=Path, metavar="FILE.csv", help="Write one line per model: frame, rmsd (to the mean, over the --fit atoms)")
    rf.add_argument("--aligned", default=None, type=Path, metavar="FILE.npy", help="Write the superposed coordinates of the measured atoms: float64 [models, atoms, 3]")
    rf.add_argument("--ignore-zero-occupancy", action="store_true", help="Ignore atoms with zero occupancy")
    for name in ("dccm", "pca"):
        cv = sub.add_parser(name, help="which atoms move together across the models: the dynamic cross-correlation map after rmsf's superposition" if name == "dccm" else
                            "along which collective directions the models move: principal components of the covariance of the superposed coordinates")
        cv.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
        cv.add_argument("--fit", default="ca", choices=("ca", "backbone", "heavy", "all"), help="Atoms to superpose on (residue HOH is never among them)")
        cv.add_argument("--atoms", default=None, choices=("ca", "backbone", "heavy", "all"), help="Atoms to measure (default: the atoms of --fit)")
        cv.add_argument("-c", "--chains", default="", help="Comma-separated chain IDs to include (empty: all)")
        cv.add_argument("--reference", default="mean", type=_rmsf_reference_arg, metavar="mean|K", help="Superpose on the iterated mean structure, or on model K (0: the first)")
        cv.add_argument("--max-rounds", default=50, type=int, metavar="N", help="With --reference mean: at most N rounds of superposing and averaging")
        cv.add_argument("--tol", default=1e-4, type=float, metavar="X", help="With --reference mean: stop when the mean moves by at most X Angstroms (rms over the fit atoms)")
        cv.add_argument("--ignore-zero-occupancy", action="store_true", help="Ignore atoms with zero occupancy")
        if name == "dccm":
            cv.add_argument("--matrix", default=None, type=Path, metavar="FILE.npy", help="Write the map: float32 [atoms, atoms]")
            cv.add_argument("-o", "--output", default=None, type=Path, help="Output directory of the long-form table (one row per pair of atoms)")
            cv.add_argument("-f", "--filename", default="dccm", help="Name of the long-form table")
            cv.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type of the long-form table")
        else:
            cv.add_argument("--modes", default=10, type=int, metavar="K", help="Principal components to keep")
            cv.add_argument("--eigenvalues", default=None, type=Path, metavar="FILE.csv", help="Write one line per kept mode: mode, eigenvalue, explained, cumulative")
            cv.add_argument("--modes-file", default=None, type=Path, metavar="FILE.npy", help="Write the modes: float64 [K, 3 atoms], atom-major rows")
            cv.add_argument("--projections", default=None, type=Path, metavar="FILE.csv", help="Write one line per model: frame, pc1 .. pcK")
            cv.add_argument("--covariance", default=None, type=Path, metavar="FILE.npy", help="Write the covariance matrix: float64 [3 atoms, 3 atoms]")
    ss = sub.add_parser("secondary-structure", help="where the helices and strands are: DSSP states of every residue in every model, and each residue's share of the "
                                                    "models in every state")
    ss.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
    ss.add_argument("-c", "--chains", default="", help="Comma-separated chain IDs to include (empty: all)")
    ss.add_argument("-o", "--output", default=None, type=Path, help="Output directory of the per-residue table")
    ss.add_argument("-f", "--filename", default="secondary_structure", help="Name of the per-residue table")
    ss.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type of the per-residue table")
    ss.add_argument("--codes", default=None, type=Path, metavar="FILE.npy", help="Write the codes (indices into '-HBEGITS'): uint8 [models, residues]")
    ss.add_argument("--strings", default=None, type=Path, metavar="FILE.txt", help="Write one line per model: the states of its residues as '-HBEGITS' characters")
    ss.add_argument("--ignore-zero-occupancy", action="store_true", help="Ignore atoms with zero occupancy")
    tr = sub.add_parser("torsions", help="what phi, psi, omega and the chi angles are in every model: means, rotamer states and transitions per torsion, and the "
                                         "Ramachandran map of the models")
    tr.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
    tr.add_argument("-c", "--chains", default="", help="Comma-separated chain IDs to include (empty: all)")
    tr.add_argument("--kinds", default="phi,psi,omega,chi", help="Comma-separated torsions to include: phi, psi, omega, chi (all five) or chi1 .. chi5")
    tr.add_argument("--bins", default=36, type=int, metavar="N", help="Bins of the histograms over (-180, 180] (at most 360)")
    tr.add_argument("--rama", default="class", choices=("class", "residue"), help="Groups of the Ramachandran maps: the four residue classes (general, GLY, PRO, "
                                                                                   "pre-PRO) or one map per residue")
    tr.add_argument("-o", "--output", default=None, type=Path, help="Output directory of the per-torsion table")
    tr.add_argument("-f", "--filename", default="torsions", help="Name of the per-torsion table")
    tr.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type of the per-torsion table")
    tr.add_argument("--angles", default=None, type=Path, metavar="FILE.npy", help="Write the angles in degrees: float32 [models, torsions], NaN where undefined")
    tr.add_argument("--rama-file", default=None, type=Path, metavar="FILE.npy", help="Write the Ramachandran maps: uint32 [groups, N, N], rows phi, columns psi")
    tr.add_argument("--ignore-zero-occupancy", action="store_true", help="Ignore atoms with zero occupancy")
    common = dict(model=("-m", "--model", 0, int, "Model number to analyze (0: the first model)"),
                  probe=("-r", "--probe-radius", 1.4, float, "Probe radius in Angstroms"),
                  points=("-n", "--num-points", 100, int, "Number of points for surface calculation"),
                  threads=("-j", "--num-threads", 1, int, "Number of threads (accepted; the computation runs on the GPU)"))

    def add(p, *keys):
        for k in keys:
            short, long_, default, typ, hlp = common[k]
            p.add_argument(short, long_, default=default, type=typ, help=hlp, dest={"model": "model_num", "points": "n_points"}.get(k))

    a = sub.add_parser("sasa", help="solvent accessible surface area per atom (cli/sasa.rs)")
    a.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file to be analyzed")
    a.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    a.add_argument("-f", "--filename", default="sasa", help="Name of the output file")
    a.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type")
    add(a, "model", "probe", "points", "threads")
    a.add_argument("-l", "--level", default="atom", type=str.lower, choices=("atom", "residue", "chain"), help="Aggregation level (residue and chain need --radii)")
    a.add_argument("-c", "--chains", default="", help="Comma-separated chain IDs to include (empty: all)")
    a.add_argument("--radii", default=None, type=str.lower, choices=("vdw", "protor"), help=RADII_HELP)
    rs = sub.add_parser("relative-sasa", help="relative solvent accessible surface area per residue (cli/relative_sasa.rs)")
    rs.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file to be analyzed")
    rs.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    rs.add_argument("-f", "--filename", default="relative_sasa", help="Name of the output file")
    rs.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type")
    add(rs, "model", "probe", "points", "threads")
    rs.add_argument("-c", "--chains", default="", help="Comma-separated chain IDs to include (empty: all)")
    p = sub.add_parser("sap", help="spatial aggregation propensity per atom or residue (cli/sap.rs)")
    p.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file to be analyzed")
    p.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    p.add_argument("-f", "--filename", default="sap", help="Name of the output file")
    p.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type")
    add(p, "model", "probe", "points")
    p.add_argument("-s", "--sap-radius", default=5.0, type=float, help="Radius in Angstroms for the neighbour search")
    add(p, "threads")
    p.add_argument("-l", "--level", default="residue", type=str.lower, choices=("atom", "residue"), help="Aggregation level")
    p.add_argument("-c", "--chains", default="", help="Comma-separated chain IDs to include (empty: all)")
    ea = sub.add_parser("sasa-ensemble", help="per-atom SASA mean / spread / extremes across the models of a multi-model file")
    ea.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
    ea.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    ea.add_argument("-f", "--filename", default="sasa_ensemble", help="Name of the output file")
    ea.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type")
    add(ea, "probe", "points", "threads")
    ea.add_argument("-l", "--level", default="atom", type=str.lower, choices=("atom", "residue", "chain"), help="Aggregation level (residue and chain need --radii)")
    ea.add_argument("-c", "--chains", default="", help="Comma-separated chain IDs to include (empty: all)")
    ea.add_argument("--radii", default=None, type=str.lower, choices=("vdw", "protor"), help=RADII_HELP)
    ep = sub.add_parser("sap-ensemble", help="spatial aggregation propensity averaged across the models of a multi-model file, per atom or residue")
    ep.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
    ep.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    ep.add_argument("-f", "--filename", default="sap_ensemble", help="Name of the output file")
    ep.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type")
    add(ep, "probe", "points")
    ep.add_argument("-s", "--sap-radius", default=5.0, type=float, help="Radius in Angstroms for the neighbour search")
    add(ep, "threads")
    ep.add_argument("-l", "--level", default="residue", type=str.lower, choices=("atom", "residue"), help="Aggregation level")
    ep.add_argument("-c", "--chains", default="", help="Comma-separated chain IDs to include (empty: all)")
    d = sub.add_parser("dsasa", help="buried surface area between two chain groups (cli/dsasa.rs)")
    d.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file to be analyzed")
    d.add_argument("-g", "--groups", required=True, help="Chain groups, e.g. A,B/C,D")
    add(d, "model", "probe", "points", "threads")
    d.add_argument("--radii", default=None, type=str.lower, choices=("vdw", "protor"), help=RADII_HELP)
    d.add_argument("-l", "--level", default="total", type=str.lower, choices=("total", "atom", "residue"),
                   help="total: the scalar (cli/dsasa.rs); atom / residue: the interface row by row, written to --output")
    d.add_argument("-o", "--output", default=None, type=Path, help="Output directory (levels atom and residue)")
    d.add_argument("-f", "--filename", default="dsasa", help="Name of the output file (levels atom and residue)")
    d.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type (levels atom and residue)")
    de = sub.add_parser("dsasa-ensemble", help="dSASA of every model of a multi-model file and how often each atom sits in the interface")
    de.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
    de.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    de.add_argument("-g", "--groups", required=True, help="Chain groups, e.g. A,B/C,D")
    de.add_argument("-f", "--filename", default="dsasa_ensemble", help="Name of the per-atom output file; the per-frame table goes to <filename>_frames")
    de.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type")
    add(de, "probe", "points", "threads")
    de.add_argument("--radii", default=None, type=str.lower, choices=("vdw", "protor"), help=RADII_HELP)
    g = sub.add_parser("sc", help="shape complementarity of two chain groups (cli/sc.rs)")
    g.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file to be analyzed")
    g.add_argument("-g", "--groups", required=True, help="Chain groups, e.g. A,B/C,D: both surfaces must be given")
    g.add_argument("-m", "--model", default=0, type=int, dest="model_num", help="Model number to analyze (0: the first model)")
    g.add_argument("-j", "--num-threads", default=0, type=int, help="Number of threads (accepted; the computation runs on the GPU)")
    ge = sub.add_parser("sc-ensemble", help="shape complementarity of every model of a multi-model file, all models in one pass on the device")
    ge.add_argument("-i", "--input", required=True, type=Path, help="Path to the PDB or mmCIF file whose models are the frames")
    ge.add_argument("-g", "--groups", required=True, help="Chain groups, e.g. A,B/C,D: both surfaces must be given")
    ge.add_argument("-o", "--output", required=True, type=Path, help="Output directory")
    ge.add_argument("-f", "--filename", default="sc_ensemble", help="Name of the per-frame output file; with --atoms the per-atom table goes to <filename>_atoms")
    ge.add_argument("-t", "--output-format", default="csv", type=str.lower, choices=FORMATS, help="Output file type")
    ge.add_argument("--atoms", action="store_true", help="Also write the per-atom table: in how many frames each atom owns a trimmed dot")
    return ap


def run_sc_ensemble(args) -> int:
    """sc-ensemble: one row per model (SC_FRAME_COLUMNS); a model whose SC fails is a row with its status, not a failure of the command."""
    import arpeggia_amd as aa

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    if "/" not in args.groups:
        log.error("Groups must be specified as 'A,B/C,D' with both surfaces defined")
        return 2
    try:
        frames, atoms = aa.sc_ensemble(str(args.input.resolve()), args.groups)
    except aa.ArpeggiaError as e:
        log.error("SC calculation failed: %s", e)
        return 1
    args.output.mkdir(parents=True, exist_ok=True)
    out = (args.output / args.filename).with_suffix("." + args.output_format)
    write_table(frames, out, args.output_format)
    if args.atoms:
        write_table(atoms, (args.output / (args.filename + "_atoms")).with_suffix("." + args.output_format), args.output_format)
    log.info("SC of %d frames saved to %s", len(frames), out)
    return 0


def run_sc(args) -> int:
    """cli/sc.rs: the groups must contain '/'; logs `SC: {:.4}`; a failure is logged and exits nonzero."""
    import arpeggia_amd as aa

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    if "/" not in args.groups:
        log.error("Groups must be specified as 'A,B/C,D' with both surfaces defined")
        return 2
    try:
        v = aa.get_sc(aa.Structure.load(str(args.input.resolve())), args.groups, args.model_num)
    except aa.ArpeggiaError as e:
        log.error("SC calculation failed: %s", e)
        return 1
    log.info("SC: %.4f", v)
    return 0


def run_surface(args) -> int:
    """sasa / relative-sasa / sap / dsasa (cli/sasa.rs, cli/relative_sasa.rs, cli/sap.rs, cli/dsasa.rs)."""
    import arpeggia_amd as aa

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    s = aa.Structure.load(str(args.input.resolve()))
    if args.command == "dsasa" and args.level != "total":
        if args.output is None:
            log.error("dsasa level '%s' writes a table: add --output", args.level)
            return 2
        table, v = aa.get_buried_sasa(s, args.groups, args.level, args.probe_radius, args.n_points, args.model_num, args.radii)
        log.info("Buried surface area (dSASA) at the interface between chains [%s]: %.2f A^2", args.groups, v)
        what = "atoms" if args.level == "atom" else "residues"
    elif args.command == "dsasa":
        v = aa.get_dsasa(s, args.groups, args.probe_radius, args.n_points, args.model_num, radii=args.radii)
        log.info("Buried surface area (dSASA) at the interface between chains [%s]: %.2f A^2", args.groups, v)
        return 0
    elif args.command == "sasa":
        if args.level != "atom" and args.radii is None:
            log.error("sasa level '%s' needs a named radius table (the reference's rust-sasa table is not part of its tree): add --radii protor, or use --level atom", args.level)
            return 2
        if args.level == "atom":
            table = aa.get_atom_sasa(s, args.probe_radius, args.n_points, args.model_num, True, args.chains, radii=args.radii)
        else:
            f = aa.get_residue_sasa if args.level == "residue" else aa.get_chain_sasa
            table = f(s, args.probe_radius, args.n_points, args.model_num, args.chains, args.radii)
        what = {"atom": "atoms", "residue": "residues", "chain": "chains"}[args.level]
    elif args.command == "relative-sasa":
        table = aa.get_relative_sasa(s, args.probe_radius, args.n_points, args.model_num, args.chains)
        what = "residues"
    else:
        f = aa.get_per_atom_sap_score if args.level == "atom" else aa.get_per_residue_sap_score
        table = f(s, args.probe_radius, args.n_points, args.model_num, args.sap_radius, args.chains)
        what = "atoms" if args.level == "atom" else "residues"
    if len(table) == 0:
        log.error("No data found in the input file. Please check the provided arguments, especially the model number.")
        return 1
    args.output.mkdir(parents=True, exist_ok=True)
    out = (args.output / args.filename).with_suffix("." + args.output_format)
    write_table(table, out, args.output_format)
    log.info("Results for %d %s saved to %s", len(table), what, out)
    return 0


def run_ensemble(args) -> int:
    """sasa-ensemble / sap-ensemble / dsasa-ensemble: the models of the input file are the frames."""
    import arpeggia_amd as aa

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    if args.command == "dsasa-ensemble":
        try:
            frames, table = aa.dsasa_ensemble(str(args.input.resolve()), args.groups, args.probe_radius, args.n_points, args.radii)
        except aa.ArpeggiaError as e:
            log.error("Ensemble statistics failed: %s", e)
            return 1
        args.output.mkdir(parents=True, exist_ok=True)
        out = (args.output / args.filename).with_suffix("." + args.output_format)
        write_table(table, out, args.output_format)
        write_table(frames, (args.output / (args.filename + "_frames")).with_suffix("." + args.output_format), args.output_format)
        log.info("Results for %d atoms over %d frames saved to %s", len(table), len(frames), out)
        return 0
    if args.command == "sasa-ensemble" and args.level != "atom" and args.radii is None:
        log.error("sasa level '%s' needs a named radius table (the reference's rust-sasa table is not part of its tree): add --radii protor, or use --level atom", args.level)
        return 2
    try:
        if args.command == "sasa-ensemble":
            table = aa.sasa_ensemble(str(args.input.resolve()), args.probe_radius, args.n_points, args.chains, args.level, args.radii)
        else:
            s = aa.Structure.load(str(args.input.resolve()))
            f = aa.get_sap_ensemble if args.level == "atom" else aa.get_residue_sap_ensemble
            table = f(s, None, args.chains, args.probe_radius, args.n_points, args.sap_radius)
    except aa.ArpeggiaError as e:
        log.error("Ensemble statistics failed: %s", e)
        return 1
    if len(table) == 0:
        log.error("No data found in the input file. Please check the provided arguments.")
        return 1
    args.output.mkdir(parents=True, exist_ok=True)
    out = (args.output / args.filename).with_suffix("." + args.output_format)
    write_table(table, out, args.output_format)
    log.info("Results for %d %s saved to %s", len(table), {"atom": "atoms", "residue": "residues", "chain": "chains"}[getattr(args, "level", "atom")], out)
    return 0


def write_table(table, path: Path, fmt: str) -> None:
    """write_df_to_file (utils.rs:117-146): csv / parquet / json (one array) / ndjson (one object per line)."""
    import pyarrow as pa

    if not isinstance(table, pa.Table):
        table = table.to_arrow()  # polars.DataFrame
    if fmt == "csv":
        import pyarrow.csv as pacsv

        pacsv.write_csv(table, str(path))
    elif fmt == "parquet":
        import pyarrow.parquet as pq

        pq.write_table(table, str(path))
    else:
        rows = table.to_pylist()
        with open(path, "w") as f:
            if fmt == "json":
                json.dump(rows, f)
            else:
                for r in rows:
                    f.write(json.dumps(r) + "\n")


def run_contacts(args) -> int:
    import arpeggia_amd as aa
    from arpeggia_amd import _lib

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)  # cli/contacts.rs:58-64
        return 1
    _lib.lib.arp_set_num_threads(int(args.num_threads))
    s = aa.Structure.load(str(args.input.resolve()), args.ignore_zero_occupancy)
    if not (s.soa("/")["attr"] & _lib.ATTR["H"]).any():
        log.warning("No hydrogen atoms found in the structure. This may affect the accuracy of the results.")  # :91-100
    table = aa.get_contacts(s, args.groups, args.vdw_comp, args.dist_cutoff)
    args.output.mkdir(parents=True, exist_ok=True)
    out = (args.output / args.filename).with_suffix("." + args.output_format)
    arrow = table if hasattr(table, "column") and not hasattr(table, "to_arrow") else table.to_arrow()
    n_clash = sum(1 for v in arrow.column("interaction").to_pylist() if v == "StericClash")
    if n_clash:
        log.warning("Found %d steric %s", n_clash, "clash" if n_clash == 1 else "clashes")  # :117-132
    write_table(table, out, args.output_format)
    log.info("Results saved to %s", out)
    return 0


def run_contact_frequency(args) -> int:
    import arpeggia_amd as aa

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    if args.waters and args.level != "residue":
        log.error("--waters needs --level residue (water-bridges lists the atoms of every bridge)")
        return 1
    try:
        table = aa.contact_frequencies(str(args.input.resolve()), args.groups, args.vdw_comp, args.dist_cutoff, args.ignore_zero_occupancy, rings=args.rings, level=args.level,
                                       waters=args.waters)
    except aa.ArpeggiaError as e:
        log.error("Contact frequencies failed: %s", e)
        return 1
    args.output.mkdir(parents=True, exist_ok=True)
    out = (args.output / args.filename).with_suffix("." + args.output_format)
    write_table(table, out, args.output_format)
    log.info("Results for %d contacts saved to %s", len(table), out)
    return 0


def run_contact_timeline(args) -> int:
    import numpy as np

    import arpeggia_amd as aa
    from arpeggia_amd import api

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    if args.waters and args.level != "residue":
        log.error("--waters needs --level residue (water-bridges lists the atoms of every bridge)")
        return 1
    try:
        table, words = api._contact_timelines_arrow(str(args.input.resolve()), args.groups, args.vdw_comp, args.dist_cutoff, args.ignore_zero_occupancy, args.rings,
                                                    args.level, args.bitmap is not None, args.waters)
    except aa.ArpeggiaError as e:
        log.error("Contact timelines failed: %s", e)
        return 1
    args.output.mkdir(parents=True, exist_ok=True)
    out = (args.output / args.filename).with_suffix("." + args.output_format)
    write_table(table, out, args.output_format)
    if args.bitmap is not None:
        args.bitmap.parent.mkdir(parents=True, exist_ok=True)
        with open(args.bitmap, "wb") as f:  # (np.save on a name would append .npy to any other suffix)
            np.save(f, words)
    log.info("Results for %d contacts saved to %s", len(table), out)
    return 0


def run_water_bridges(args) -> int:
    import arpeggia_amd as aa

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    try:
        table = aa.water_bridges(str(args.input.resolve()), args.groups, args.ignore_zero_occupancy)
    except aa.ArpeggiaError as e:
        log.error("Water bridges failed: %s", e)
        return 1
    args.output.mkdir(parents=True, exist_ok=True)
    out = (args.output / args.filename).with_suffix("." + args.output_format)
    write_table(table, out, args.output_format)
    log.info("Results for %d water bridges saved to %s", len(table), out)
    return 0


def run_contact_similarity(args) -> int:
    import numpy as np

    import arpeggia_amd as aa
    from arpeggia_amd import api

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    try:
        table, matrix = api._contact_similarity_arrow(str(args.input.resolve()), args.groups, args.vdw_comp, args.dist_cutoff, args.ignore_zero_occupancy, args.rings,
                                                      args.level, args.axis, args.metric)
    except aa.ArpeggiaError as e:
        log.error("Contact similarity failed: %s", e)
        return 1
    args.output.mkdir(parents=True, exist_ok=True)
    out = (args.output / args.filename).with_suffix("." + args.output_format)
    write_table(table, out, args.output_format)
    if args.matrix is not None:
        args.matrix.parent.mkdir(parents=True, exist_ok=True)
        with open(args.matrix, "wb") as f:  # (np.save on a name would append .npy to any other suffix)
            np.save(f, matrix)
    log.info("Results for %d contacts saved to %s", len(table), out)
    return 0


def run_contact_autocorrelation(args) -> int:
    import numpy as np

    import arpeggia_amd as aa
    from arpeggia_amd import api

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    try:
        table, cols = api._contact_autocorrelation_arrow(str(args.input.resolve()), args.groups, args.vdw_comp, args.dist_cutoff, args.ignore_zero_occupancy, args.rings,
                                                         args.level, args.mode, args.max_lag, args.matrix is not None)
    except (aa.ArpeggiaError, ValueError) as e:
        log.error("Contact autocorrelation failed: %s", e)
        return 1
    args.output.mkdir(parents=True, exist_ok=True)
    out = (args.output / args.filename).with_suffix("." + args.output_format)
    write_table(table, out, args.output_format)
    if args.matrix is not None:
        args.matrix.parent.mkdir(parents=True, exist_ok=True)
        with open(args.matrix, "wb") as f:  # (np.save on a name would append .npy to any other suffix)
            np.save(f, cols["autocorrelation"])
    if args.curves is not None:
        args.curves.parent.mkdir(parents=True, exist_ok=True)
        names = list(cols["by_interaction"])
        with open(args.curves, "w") as f:
            f.write(",".join(["lag"] + names) + "\n")
            for k, lag in enumerate(cols["lags"]):
                f.write(",".join([str(int(lag))] + [repr(float(cols["by_interaction"][n]["curve"][k])) for n in names]) + "\n")
    log.info("Results for %d contacts saved to %s", len(table), out)
    return 0


def run_contact_clusters(args) -> int:
    import numpy as np

    import arpeggia_amd as aa
    from arpeggia_amd import api

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    try:
        table, cols = api._contact_clusters_arrow(str(args.input.resolve()), args.groups, args.vdw_comp, args.dist_cutoff, args.ignore_zero_occupancy, args.rings,
                                                  args.level, args.min_similarity, args.max_clusters, args.cluster_counts is not None)
    except (aa.ArpeggiaError, ValueError) as e:
        log.error("Contact clusters failed: %s", e)
        return 1
    args.output.mkdir(parents=True, exist_ok=True)
    out = (args.output / args.filename).with_suffix("." + args.output_format)
    write_table(table, out, args.output_format)
    if args.assignments is not None:
        args.assignments.parent.mkdir(parents=True, exist_ok=True)
        centres = set(int(c) for c in cols["centre"])
        with open(args.assignments, "w") as f:
            f.write("frame,cluster,is_centre,similarity_to_centre,n_neighbours,size\n")
            for k in range(cols["n_total_frames"]):
                left = int(cols["cluster"][k]) == 0xFFFFFFFF
                f.write(",".join([str(k), "" if left else str(int(cols["cluster"][k])), "1" if k in centres else "0",
                                  "" if left else repr(float(cols["similarity_to_centre"][k])), str(int(cols["n_neighbours"][k])), str(int(cols["sizes"][k]))]) + "\n")
    if args.cluster_counts is not None:
        args.cluster_counts.parent.mkdir(parents=True, exist_ok=True)
        with open(args.cluster_counts, "wb") as f:  # (np.save on a name would append .npy to any other suffix)
            np.save(f, cols["cluster_counts"])
    log.info("Results for %d contacts in %d clusters saved to %s", len(table), cols["n_clusters"], out)
    return 0


def _rmsf_reference_arg(text: str):
    """--reference of rmsf: the word mean, or a model index."""
    if text == "mean":
        return text
    try:
        k = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"expected 'mean' or a model index, got {text!r}")
    if k < 0:
        raise argparse.ArgumentTypeError(f"expected 'mean' or a model index, got {text!r}")
    return k


def run_rmsf(args) -> int:
    import numpy as np

    import arpeggia_amd as aa

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    try:
        structure = aa.Structure.load(str(args.input.resolve()), args.ignore_zero_occupancy)
        res = aa.get_rmsf(structure, None, args.fit, args.atoms, args.chains, args.reference, args.max_rounds, args.tol, args.level, aligned=args.aligned is not None)
    except (aa.ArpeggiaError, ValueError) as e:
        log.error("RMSF failed: %s", e)
        return 1
    names = aa.RMSF_COLUMNS if args.level == "atom" else aa.RMSF_RESIDUE_COLUMNS
    rows = res if args.level == "atom" else res["residue"]
    idx = rows["atom"]
    ident = {k: [b.decode() for b in structure.strings(k)[idx]] for k in ("chain", "resn", "insertion", "altloc", "atomn")}
    ident["resi"], ident["atomi"] = [str(int(v)) for v in structure.ints("resi")[idx]], [str(int(v)) for v in structure.ints("atomi")[idx]]
    values = {"rmsf": [repr(float(v)) for v in rows["rmsf"]], "bfactor": [repr(float(v)) for v in rows["bfactor"]]}
    if args.level == "atom":
        values.update({name: [repr(float(v)) for v in res["mean"][:, k]] for k, name in enumerate(("mean_x", "mean_y", "mean_z"))})
    else:
        values["n_atoms"] = [str(int(v)) for v in rows["n_atoms"]]
    args.output.mkdir(parents=True, exist_ok=True)
    out = (args.output / args.filename).with_suffix(".csv")
    with open(out, "w") as f:
        f.write(",".join(names) + "\n")
        for k in range(len(idx)):
            f.write(",".join(ident[c][k] if c in ident else values[c][k] for c in names) + "\n")
    if args.frames is not None:
        args.frames.parent.mkdir(parents=True, exist_ok=True)
        with open(args.frames, "w") as f:
            f.write("frame,rmsd\n")
            for k, v in enumerate(res["frame_rmsd"]):
                f.write(f"{k},{float(v)!r}\n")
    if args.aligned is not None:
        args.aligned.parent.mkdir(parents=True, exist_ok=True)
        with open(args.aligned, "wb") as f:  # (np.save on a name would append .npy to any other suffix)
            np.save(f, res["aligned"])
    if args.reference == "mean" and not res["converged"]:
        log.warning("The mean structure still moved by %.3g A after %d rounds (--tol %g): --max-rounds ended the iteration", res["last_change"], res["n_rounds"], args.tol)
    log.info("RMSF of %d %s over %d models (%d rounds) saved to %s", len(idx), "atoms" if args.level == "atom" else "residues", len(res["frame_rmsd"]), res["n_rounds"], out)
    return 0


def _save_npy(path: Path, array):
    import numpy as np

    path.parent.mkdir(parents=True, exist_ok=True)
    with open(path, "wb") as f:  # (np.save on a name would append .npy to any other suffix)
        np.save(f, array)


def run_dccm(args) -> int:
    import arpeggia_amd as aa

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    if args.matrix is None and args.output is None:
        log.error("DCCM: nothing to write, give --matrix FILE.npy and / or -o DIR")
        return 1
    try:
        structure = aa.Structure.load(str(args.input.resolve()), args.ignore_zero_occupancy)
        res = aa.get_dccm(structure, None, args.fit, args.atoms, args.chains, args.reference, args.max_rounds, args.tol)
    except (aa.ArpeggiaError, ValueError) as e:
        log.error("DCCM failed: %s", e)
        return 1
    if args.matrix is not None:
        _save_npy(args.matrix, res["dccm"])
    if args.output is not None:
        args.output.mkdir(parents=True, exist_ok=True)
        out = (args.output / args.filename).with_suffix("." + args.output_format)
        write_table(aa.dccm_table(structure, res), out, args.output_format)
    if args.reference == "mean" and not res["converged"]:
        log.warning("The mean structure still moved by %.3g A after %d rounds (--tol %g): --max-rounds ended the iteration", res["last_change"], res["n_rounds"], args.tol)
    log.info("DCCM of %d atoms over %d models (%d rounds) saved", len(res["atom"]), len(res["frame_rmsd"]), res["n_rounds"])
    return 0


def run_secondary_structure(args) -> int:
    import arpeggia_amd as aa

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    if args.output is None and args.codes is None and args.strings is None:
        log.error("Secondary structure: nothing to write, give -o DIR, --codes FILE.npy and / or --strings FILE.txt")
        return 1
    try:
        structure = aa.Structure.load(str(args.input.resolve()), args.ignore_zero_occupancy)
        res = aa.get_secondary_structure(structure, None, args.chains)
    except (aa.ArpeggiaError, ValueError) as e:
        log.error("Secondary structure failed: %s", e)
        return 1
    if args.output is not None:
        args.output.mkdir(parents=True, exist_ok=True)
        out = (args.output / args.filename).with_suffix("." + args.output_format)
        write_table(aa.secondary_structure_table(structure, res), out, args.output_format)
    if args.codes is not None:
        _save_npy(args.codes, res["codes"])
    if args.strings is not None:
        args.strings.parent.mkdir(parents=True, exist_ok=True)
        with open(args.strings, "w") as f:
            for row in res["codes"]:
                f.write(aa.ss_string(row) + "\n")
    log.info("Secondary structure of %d residues over %d models saved", len(res["residue"]), len(res["frame_counts"]))
    return 0


def run_torsions(args) -> int:
    import arpeggia_amd as aa

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    if args.output is None and args.angles is None and args.rama_file is None:
        log.error("Torsions: nothing to write, give -o DIR, --angles FILE.npy and / or --rama-file FILE.npy")
        return 1
    try:
        structure = aa.Structure.load(str(args.input.resolve()), args.ignore_zero_occupancy)
        res = aa.get_torsions(structure, None, args.chains, args.kinds, args.bins, args.rama, angles=args.angles is not None)
    except (aa.ArpeggiaError, ValueError) as e:
        log.error("Torsions failed: %s", e)
        return 1
    if args.rama_file is not None and "hist2" not in res:
        log.error("Torsions: no Ramachandran map to write (--kinds leaves no residue with both phi and psi, or --bins is 0)")
        return 1
    if args.output is not None:
        args.output.mkdir(parents=True, exist_ok=True)
        out = (args.output / args.filename).with_suffix("." + args.output_format)
        write_table(aa.torsion_table(structure, res), out, args.output_format)
    if args.angles is not None:
        _save_npy(args.angles, res["angles"])
    if args.rama_file is not None:
        _save_npy(args.rama_file, res["hist2"])
    log.info("%d torsions of %d residues saved", len(res["kind"]), res["n_rows"])
    return 0


def run_pca(args) -> int:
    import arpeggia_amd as aa

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    try:
        structure = aa.Structure.load(str(args.input.resolve()), args.ignore_zero_occupancy)
        res = aa.get_pca(structure, None, args.fit, args.atoms, args.chains, args.reference, args.max_rounds, args.tol, args.modes)
    except (aa.ArpeggiaError, ValueError) as e:
        log.error("PCA failed: %s", e)
        return 1
    k = len(res["modes"])
    if args.eigenvalues is not None:
        args.eigenvalues.parent.mkdir(parents=True, exist_ok=True)
        with open(args.eigenvalues, "w") as f:
            f.write("mode,eigenvalue,explained,cumulative\n")
            for j in range(k):
                f.write(f"{j + 1},{float(res['eigenvalues'][j])!r},{float(res['explained'][j])!r},{float(res['cumulative'][j])!r}\n")
    if args.modes_file is not None:
        _save_npy(args.modes_file, res["modes"])
    if args.covariance is not None:
        _save_npy(args.covariance, res["covariance"])
    if args.projections is not None:
        args.projections.parent.mkdir(parents=True, exist_ok=True)
        with open(args.projections, "w") as f:
            f.write(",".join(["frame"] + [f"pc{j + 1}" for j in range(k)]) + "\n")
            for frame, row in enumerate(res["projections"]):
                f.write(",".join([str(frame)] + [repr(float(v)) for v in row]) + "\n")
    if args.reference == "mean" and not res["converged"]:
        log.warning("The mean structure still moved by %.3g A after %d rounds (--tol %g): --max-rounds ended the iteration", res["last_change"], res["n_rounds"], args.tol)
    log.info("%d principal components of %d atoms over %d models: %.1f %% of the variance", k, len(res["atom"]), len(res["frame_rmsd"]),
             100.0 * float(res["cumulative"][-1]))
    return 0


def run_rmsd(args) -> int:
    import numpy as np

    import arpeggia_amd as aa

    if not args.input.exists():
        log.error("Failed to retrieve input file: %s", args.input)
        return 1
    path = str(args.input.resolve())
    try:
        if args.command == "rmsd":
            values = aa.rmsd(path, args.reference, args.atoms, args.chains, args.ignore_zero_occupancy)
        elif args.command == "rmsd-matrix":
            values = aa.rmsd_matrix(path, args.atoms, args.chains, args.ignore_zero_occupancy)
        else:
            cols = aa.rmsd_clusters(path, args.atoms, args.chains, args.ignore_zero_occupancy, cutoff=args.cutoff, max_clusters=args.max_clusters)
    except (aa.ArpeggiaError, ValueError) as e:
        log.error("RMSD failed: %s", e)
        return 1
    if args.command == "rmsd-matrix":
        args.matrix.parent.mkdir(parents=True, exist_ok=True)
        with open(args.matrix, "wb") as f:  # (np.save on a name would append .npy to any other suffix)
            np.save(f, values)
        log.info("RMSD matrix of %d models saved to %s", len(values), args.matrix)
        return 0
    args.output.mkdir(parents=True, exist_ok=True)
    out = (args.output / args.filename).with_suffix(".csv")
    with open(out, "w") as f:
        if args.command == "rmsd":
            f.write("frame,rmsd\n")
            for k, v in enumerate(values):
                f.write(f"{k},{float(v)!r}\n")
        else:
            f.write("cluster,centre,size\n")
            for k in range(cols["n_clusters"]):
                f.write(f"{k},{int(cols['centre'][k])},{int(cols['cluster_size'][k])}\n")
    if args.command == "rmsd-clusters" and args.assignments is not None:
        args.assignments.parent.mkdir(parents=True, exist_ok=True)
        centres = set(int(c) for c in cols["centre"])
        with open(args.assignments, "w") as f:
            f.write("frame,cluster,is_centre,rmsd_to_centre,n_neighbours\n")
            for k in range(len(cols["cluster"])):
                left = int(cols["cluster"][k]) == 0xFFFFFFFF
                f.write(",".join([str(k), "" if left else str(int(cols["cluster"][k])), "1" if k in centres else "0",
                                  "" if left else repr(float(cols["rmsd_to_centre"][k])), str(int(cols["n_neighbours"][k]))]) + "\n")
    log.info("Results saved to %s", out)
    return 0


def main(argv=None) -> int:
    logging.basicConfig(level=logging.INFO, format="%(levelname)s %(message)s", stream=sys.stderr)
    args = build_parser().parse_args(argv)
    if args.command in ("rmsd", "rmsd-matrix", "rmsd-clusters"):
        return run_rmsd(args)
    if args.command == "rmsf":
        return run_rmsf(args)
    if args.command == "dccm":
        return run_dccm(args)
    if args.command == "secondary-structure":
        return run_secondary_structure(args)
    if args.command == "torsions":
        return run_torsions(args)
    if args.command == "pca":
        return run_pca(args)
    if args.command == "sc":
        return run_sc(args)
    if args.command == "sc-ensemble":
        return run_sc_ensemble(args)
    if args.command in ("sasa-ensemble", "sap-ensemble", "dsasa-ensemble"):
        return run_ensemble(args)
    if args.command == "contact-frequency":
        return run_contact_frequency(args)
    if args.command == "contact-timeline":
        return run_contact_timeline(args)
    if args.command == "water-bridges":
        return run_water_bridges(args)
    if args.command == "contact-similarity":
        return run_contact_similarity(args)
    if args.command == "contact-autocorrelation":
        return run_contact_autocorrelation(args)
    if args.command == "contact-clusters":
        return run_contact_clusters(args)
    return run_contacts(args) if args.command == "contacts" else run_surface(args)


if __name__ == "__main__":
    raise SystemExit(main())
