"""Python surface of the MI355X-native contact engine.

Mirrors the reference's PyO3 module for the one path this repo replaces:
`arpeggia.contacts(input_file, groups="/", vdw_comp=0.1, dist_cutoff=6.5, ignore_zero_occupancy=False, num_threads=1)`
(reference: src/python.rs:31-56, stubs python/arpeggia/arpeggia.pyi:7-33) plus the Rust-level pieces it is made of
(`load_model` utils.rs:51, `parse_groups` utils.rs:71, `get_contacts` contacts/mod.rs:61).

Everything numeric happens in libarpeggia_amd.so on a gfx950 device; this file only marshals pointers.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import lib

PAIR_DTYPE = np.dtype([("i", "<u4"), ("j", "<u4"), ("dist", "<f4"), ("kind", "<u4")])

TABLE_COLUMNS = [  # mod.rs:140-181 + 209-211, in the reference's order with its dtypes
    ("model", "u4"), ("interaction", "str"), ("distance", "f4"),
    ("from_chain", "str"), ("from_resn", "str"), ("from_resi", "i4"), ("from_insertion", "str"), ("from_altloc", "str"),
    ("from_atomn", "str"), ("from_atomi", "i4"),
    ("to_chain", "str"), ("to_resn", "str"), ("to_resi", "i4"), ("to_insertion", "str"), ("to_altloc", "str"),
    ("to_atomn", "str"), ("to_atomi", "i4"),
    ("sc_centroid_dist", "f4"), ("sc_dihedral", "f4"), ("sc_centroid_angle", "f4"),
]

FREQ_COLUMNS = [  # arp_contact_frequencies (include/arpeggia_amd.h): one row per distinct (from atom, to atom, interaction) over the frames
    ("interaction", "str"),
    ("from_chain", "str"), ("from_resn", "str"), ("from_resi", "i4"), ("from_insertion", "str"), ("from_altloc", "str"),
    ("from_atomn", "str"), ("from_atomi", "i4"),
    ("to_chain", "str"), ("to_resn", "str"), ("to_resi", "i4"), ("to_insertion", "str"), ("to_altloc", "str"),
    ("to_atomn", "str"), ("to_atomi", "i4"),
    ("n_frames", "u4"), ("frequency", "f4"), ("min_distance", "f4"), ("max_distance", "f4"),
]

RESIDUE_FREQ_COLUMNS = [  # arp_residue_contact_frequencies: one row per distinct (residue of from, residue of to, interaction) over the frames
    ("interaction", "str"),
    ("from_chain", "str"), ("from_resn", "str"), ("from_resi", "i4"), ("from_insertion", "str"),
    ("to_chain", "str"), ("to_resn", "str"), ("to_resi", "i4"), ("to_insertion", "str"),
    ("n_frames", "u4"), ("frequency", "f4"), ("min_distance", "f4"), ("max_distance", "f4"),
]
WATER_BRIDGE_COLUMNS = [  # arp_water_bridges: one row per bridge (from atom, water, to atom) of a frame, ordered by (frame, from_atom, to_atom, water_atom)
    ("frame", "u4"),
    ("from_chain", "str"), ("from_resn", "str"), ("from_resi", "i4"), ("from_insertion", "str"), ("from_altloc", "str"),
    ("from_atomn", "str"), ("from_atomi", "i4"),
    ("to_chain", "str"), ("to_resn", "str"), ("to_resi", "i4"), ("to_insertion", "str"), ("to_altloc", "str"),
    ("to_atomn", "str"), ("to_atomi", "i4"),
    ("water_chain", "str"), ("water_resi", "i4"), ("water_insertion", "str"), ("water_altloc", "str"), ("water_atomi", "i4"),
    ("from_distance", "f4"), ("to_distance", "f4"), ("distance", "f4"),
]
TIMELINE_COLUMNS = [  # arp_contact_timelines: behind the frequency columns of the level (FREQ_COLUMNS / RESIDUE_FREQ_COLUMNS)
    ("first_frame", "u4"), ("last_frame", "u4"), ("n_events", "u4"), ("longest_run", "u4"), ("mean_run", "f4"),
]


class ArpeggiaError(RuntimeError):
    """Raised where the reference panics (pyo3_runtime.PanicException) or a HIP call fails."""

    def __init__(self, status: int, message: str):
        super().__init__(message)
        self.status = status


def _check(status: int):
    if status != _lib.ARP_OK:
        msg = lib.arp_last_error().decode() or lib.arp_strerror(status).decode()
        raise ArpeggiaError(status, msg)


def device_count() -> int:
    return int(lib.arp_device_count())


def default_params(vdw_comp: float = 0.1, dist_cutoff: float = 6.5, deterministic: bool = False, contacts_only: bool = False,
                   no_speculation: bool = False, residue_runs: bool | None = None) -> _lib.arp_params:
    """deterministic=True selects the two-pass ordered emitter (ARP_FLAG_DETERMINISTIC): identical bytes run to run.
    contacts_only=True drops candidates without any interaction on the device (ARP_FLAG_CONTACTS_ONLY).
    no_speculation=True (ARP_FLAG_NO_SPECULATION): Context.enqueue always launches the probe pass, so that work ordered on the stream behind
    the enqueue sees final records (include/arpeggia_amd.h).
    residue_runs: a hint about the input, never a change of the result -- True asks for the kernels that apply the reference's residue rule
    (complex.rs:108-113) before the exact phase (ARP_FLAG_RESIDUE_RUNS), False rules them out (ARP_FLAG_NO_RESIDUE_RUNS), None lets the
    engine choose from a sample of the previous call's atoms."""
    p = _lib.arp_params()
    lib.arp_default_params(C.byref(p))
    p.vdw_comp = vdw_comp
    p.dist_cutoff = dist_cutoff
    p.flags = ((_lib.ARP_FLAG_DETERMINISTIC if deterministic else 0) | (_lib.ARP_FLAG_CONTACTS_ONLY if contacts_only else 0)
               | (_lib.ARP_FLAG_NO_SPECULATION if no_speculation else 0)
               | (0 if residue_runs is None else (_lib.ARP_FLAG_RESIDUE_RUNS if residue_runs else _lib.ARP_FLAG_NO_RESIDUE_RUNS)))
    return p


def debug_set(key: str, value: int):
    """arp_debug_set: the library's diagnostic switches ("timing", "emit_kernel", "defer_entries", "table_host", "freq_chunk_atoms", "freq_cap_items", "freq_frame_bits", "timeline_cap_bytes", "similarity_cap_bytes", "autocorr_cap_bytes", "cluster_cap_bytes", "table_key_bits", ...; include/arpeggia_amd.h)."""
    _check(lib.arp_debug_set(key.encode(), int(value)))


def debug_get(key: str) -> int:
    """arp_debug_get: what the last contact-table call of the process did ("table_small", "table_pairs", "table_atom_rows", "table_ring_rows", "table_plan", "table_long_way", "table_ring_cap"; include/arpeggia_amd.h)."""
    v = C.c_int64(0)
    _check(lib.arp_debug_get(key.encode(), C.byref(v)))
    return int(v.value)


def parse_groups(all_chains, groups: str):
    """utils.rs:71-115 on a throw-away structure with one atom per chain (keeps ONE implementation, in C++)."""
    chains = sorted(set(all_chains))
    n = len(chains)
    rec = {
        "x": np.zeros(n), "y": np.zeros(n), "z": np.arange(n, dtype=np.float64) * 100.0,
        "serial": np.arange(1, n + 1, dtype=np.int32), "resi": np.ones(n, dtype=np.int32),
        "name": np.array([b"CA"] * n, dtype="S8"), "resn": np.array([b"GLY"] * n, dtype="S8"),
        "chain": np.array([c.encode() for c in chains], dtype="S8"), "element": np.array([b"C"] * n, dtype="S4"),
    }
    s = Structure.from_records(rec)
    soa = s.soa(groups)
    lig = {chains[k] for k in range(n) if soa["attr"][k] & _lib.ATTR["LIGAND"]}
    recp = {chains[k] for k in range(n) if soa["attr"][k] & _lib.ATTR["RECEPTOR"]}
    return lig, recp


def _np_from(ptr, n, dtype):
    if not ptr or n == 0:
        return np.zeros(0, dtype=dtype)
    dt = np.dtype(dtype)
    buf = (C.c_char * (n * dt.itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dt, count=n).copy()


class _PairsOwner:
    """Keeps a library-allocated pair list alive for the numpy view over it; frees it with the last reference."""

    def __init__(self, pairs):
        self.pairs = pairs

    def __del__(self):
        if self.pairs is not None and lib is not None:
            lib.arp_pairs_free(C.byref(self.pairs))
            self.pairs = None


def _adopt_pairs(out) -> np.ndarray:
    """Zero-copy numpy view of an arp_pairs in host memory (copying a 460 MB list costs 200 ms of page faults)."""
    n = int(out.n)
    if not out.data or n == 0:
        lib.arp_pairs_free(C.byref(out))
        return np.zeros(0, dtype=PAIR_DTYPE)
    owner = _PairsOwner(out)
    buf = (C.c_char * (n * PAIR_DTYPE.itemsize)).from_address(out.data)
    buf._owner = owner  # the ctypes buffer is the array's base: the owner lives exactly as long as the array (and its views)
    return np.frombuffer(buf, dtype=PAIR_DTYPE, count=n)


class Structure:
    """A parsed, filtered model: what `load_model` (utils.rs:51-63) returns in the reference."""

    def __init__(self, handle):
        self._h = handle
        self._keep = None

    def __del__(self):
        if getattr(self, "_h", None):
            lib.arp_structure_free(self._h)
            self._h = None

    @classmethod
    def load(cls, path, ignore_zero_occupancy: bool = False) -> "Structure":
        h = C.c_void_p()
        _check(lib.arp_structure_load(os.fsencode(str(path)), int(ignore_zero_occupancy), C.byref(h)))
        return cls(h)

    @classmethod
    def from_records(cls, rec: dict, hierarchy: bool = False) -> "Structure":
        """rec: columns x,y,z f64; serial,resi i32; name,resn,chain S8; element S4; optional occupancy f64, model_serial i32,
        altloc/icode S4; with hierarchy=True also res_ord,res_id u32 (synthetic inputs)."""
        n = len(rec["x"])
        keep = {}

        def col(name, dtype, required=True):
            if name not in rec or rec[name] is None:
                if required:
                    raise KeyError(name)
                return None
            a = np.ascontiguousarray(rec[name], dtype=dtype)
            assert len(a) == n, name
            keep[name] = a
            return a.ctypes.data

        r = _lib.arp_records()
        r.n = n
        r.x, r.y, r.z = col("x", "<f8"), col("y", "<f8"), col("z", "<f8")
        r.occupancy = col("occupancy", "<f8", False)
        r.serial, r.resi = col("serial", "<i4"), col("resi", "<i4")
        r.model_serial = col("model_serial", "<i4", False)
        r.name, r.resn, r.chain = col("name", "S8"), col("resn", "S8"), col("chain", "S8")
        r.altloc, r.icode = col("altloc", "S4", False), col("icode", "S4", False)
        r.element = col("element", "S4")
        r.res_ord, r.res_id = col("res_ord", "<u4", hierarchy), col("res_id", "<u4", hierarchy)
        h = C.c_void_p()
        _check(lib.arp_structure_from_records(C.byref(r), int(hierarchy), C.byref(h)))
        return cls(h)

    @property
    def n_atoms(self) -> int:
        return int(lib.arp_structure_n_atoms(self._h))

    def strings(self, column: str) -> np.ndarray:
        w = C.c_int32()
        p = lib.arp_structure_strings(self._h, column.encode(), C.byref(w))
        if not p:
            raise KeyError(column)
        return _np_from(p, self.n_atoms, f"S{w.value}")

    def ints(self, column: str) -> np.ndarray:
        p = lib.arp_structure_ints(self._h, column.encode())
        if not p:
            raise KeyError(column)
        return _np_from(p, self.n_atoms, "<i4")

    def view(self, groups: str = "/") -> _lib.arp_atoms:
        """Borrowed host SoA view (valid until the next view()/soa() call on this structure)."""
        v = _lib.arp_atoms()
        _check(lib.arp_structure_atoms(self._h, groups.encode(), C.byref(v)))
        return v

    def soa(self, groups: str = "/") -> dict:
        """Copy of the SoA columns the GPU path consumes (include/arpeggia_amd.h: arp_atoms)."""
        v = self.view(groups)
        n, nr = int(v.n), int(v.n_res)
        out = {
            "x": _np_from(v.x, n, "<f8"), "y": _np_from(v.y, n, "<f8"), "z": _np_from(v.z, n, "<f8"),
            "attr": _np_from(v.attr, n, "<u4"), "res_ord": _np_from(v.res_ord, n, "<u4"),
            "chain_rank": _np_from(v.chain_rank, n, "<u4"), "model": _np_from(v.model, n, "<u4"),
            "res_id": _np_from(v.res_id, n, "<u4"),
            "res_h_ptr": _np_from(v.res_h_ptr, nr + 1 if nr else 0, "<u4"),
            "res_cb": _np_from(v.res_cb, nr, "<u4"), "res_sg": _np_from(v.res_sg, nr, "<u4"),
        }
        nh = int(out["res_h_ptr"][-1]) if nr else 0
        out["res_h_idx"] = _np_from(v.res_h_idx, nh, "<u4")
        return out


def atoms_from_arrays(soa: dict, location: int = _lib.ARP_MEM_HOST, keep: list | None = None) -> _lib.arp_atoms:
    """Build an arp_atoms from numpy arrays (host) or from objects with .data_ptr() (device tensors)."""
    v = _lib.arp_atoms()

    def ptr(name, dtype):
        a = soa.get(name)
        if a is None:
            return None
        if hasattr(a, "data_ptr"):
            # a device tensor is handed over as a raw address: its element size and layout are all that can be checked here, and they must be
            # what arp_atoms declares (API v2: 32-bit chain ranks and models -- a v1-style int16 tensor would be read 4 bytes per atom)
            want = np.dtype(dtype).itemsize
            if a.element_size() != want or not a.is_contiguous():
                raise ArpeggiaError(_lib.ARP_ERR_BAD_INPUT, f"arp_atoms.{name}: needs a contiguous tensor of {want}-byte elements ({dtype}), "
                                    f"got element size {a.element_size()}, contiguous={a.is_contiguous()}")
            if keep is not None:
                keep.append(a)
            return a.data_ptr() if a.numel() else None
        a = np.ascontiguousarray(a, dtype=dtype)
        if keep is not None:
            keep.append(a)
        return a.ctypes.data if a.size else None

    x = soa["x"]
    v.n = int(x.numel() if hasattr(x, "numel") else len(x))
    v.x, v.y, v.z = ptr("x", "<f8"), ptr("y", "<f8"), ptr("z", "<f8")
    v.attr, v.res_ord = ptr("attr", "<u4"), ptr("res_ord", "<u4")
    v.chain_rank, v.model = ptr("chain_rank", "<u4"), ptr("model", "<u4")
    rcb = soa.get("res_cb")
    v.n_res = int((rcb.numel() if hasattr(rcb, "numel") else len(rcb))) if rcb is not None else 0
    if v.n_res:
        v.res_id = ptr("res_id", "<u4")
        v.res_h_ptr, v.res_h_idx = ptr("res_h_ptr", "<u4"), ptr("res_h_idx", "<u4")
        v.res_cb, v.res_sg = ptr("res_cb", "<u4"), ptr("res_sg", "<u4")
    v.location = location
    return v


class Context:
    """One engine context = one device + one stream + a reusable workspace (arp_context)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        h = C.c_void_p()
        _check(lib.arp_context_create(device, C.byref(h)))
        self._h = h
        self._keep = []
        if stream is not None:
            self.set_stream(stream)

    def __del__(self):
        if getattr(self, "_h", None):
            lib.arp_context_destroy(self._h)
            self._h = None

    def set_stream(self, hip_stream: int | None):
        _check(lib.arp_context_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def synchronize(self):
        _check(lib.arp_context_synchronize(self._h))

    def atomic_contacts(self, atoms, params: _lib.arp_params | None = None) -> np.ndarray:
        """Synchronous hot path (complex.rs:189-299).  atoms: Structure view / arp_atoms / dict of numpy arrays."""
        keep = []
        if isinstance(atoms, dict):
            atoms = atoms_from_arrays(atoms, keep=keep)
        params = params or default_params()
        out = _lib.arp_pairs()
        _check(lib.arp_contacts_atomic(self._h, C.byref(atoms), C.byref(params), _lib.ARP_MEM_HOST, C.byref(out)))
        return _adopt_pairs(out)

    def enqueue(self, atoms: _lib.arp_atoms, params: _lib.arp_params, out_ptr: int, capacity: int):
        """Asynchronous, allocation-free form on device-resident data (arp_contacts_atomic_enqueue)."""
        _check(lib.arp_contacts_atomic_enqueue(self._h, C.byref(atoms), C.byref(params), C.c_void_p(out_ptr), capacity))

    def count(self, atoms: _lib.arp_atoms, params: _lib.arp_params) -> int:
        """Number of classified pairs without writing any (sizes the buffer for enqueue)."""
        self.enqueue(atoms, params, 0, 0)
        n = C.c_uint64()
        st = lib.arp_contacts_atomic_result(self._h, C.byref(n))
        if st not in (_lib.ARP_OK, _lib.ARP_ERR_CAPACITY):
            _check(st)
        return int(n.value)

    def result(self) -> int:
        n = C.c_uint64()
        st = lib.arp_contacts_atomic_result(self._h, C.byref(n))
        if st == _lib.ARP_ERR_CAPACITY:
            raise ArpeggiaError(st, f"pair buffer too small: {n.value} pairs needed")
        _check(st)
        return int(n.value)

    def rare_batches(self) -> int:
        """arp_pair_rare_batches: batches of the last collected pair pass that decided on the real residue keys (diagnostics)."""
        return int(lib.arp_pair_rare_batches(self._h))

    def profile(self, on: bool):
        _check(lib.arp_profile_enable(self._h, int(on)))

    def profile_read(self) -> dict:
        names = (C.c_char_p * 32)()
        ms = (C.c_float * 32)()
        k = lib.arp_profile_read(self._h, names, ms, 32)
        return {names[i].decode(): float(ms[i]) for i in range(k)}

    def get_contacts(self, structure: Structure, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5) -> dict:
        """`arpeggia::get_contacts` (mod.rs:61-137): the sorted 20-column table as a dict of numpy columns."""
        t = C.c_void_p()
        _check(lib.arp_get_contacts(self._h, structure._h, groups.encode(), vdw_comp, dist_cutoff, C.byref(t)))
        try:
            cols = _read_columns(t, TABLE_COLUMNS, (("sc_valid", "u1"), ("from_atom", "i4"), ("to_atom", "i4")))
            cols["sc_valid"] = cols["sc_valid"].astype(bool)
            return cols
        finally:
            lib.arp_table_free(t)

    def contact_frequencies(self, structure: Structure, frames=None, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, rings: bool = False,
                            waters: bool = False, level: str = "atom") -> dict:
        """arp_contact_frequencies_ex as a dict of numpy columns (FREQ_COLUMNS + from_atom / to_atom).  frames: [F, N, 3] f64 coordinates of the
        topology's N atoms (model 0 of `structure`); None: the structure's models are the frames.  rings=True (ARP_FREQ_RINGS) adds the ring rows
        (CationPi, Pi* stackings) behind the atom rows, and the columns from_ring / to_ring (ring entity index, -1 for an atom; from_atom /
        to_atom are -1 for a ring).  level="residue": arp_residue_contact_frequencies -- one row per (residue, residue, interaction), a frame
        counted once per row however many of the residues' atom pairs (and, with rings, ring entities) are in contact; the columns are
        RESIDUE_FREQ_COLUMNS + from_residue / to_residue (residue ordinals of the topology).  waters=True (ARP_FREQ_WATERS, level="residue" only): the
        water-bridge rows (interaction code _lib.WATER_BRIDGE) join the table; see get_contact_frequencies."""
        t = _freq_table(self, structure, frames, groups, vdw_comp, dist_cutoff, rings, level, waters)
        try:
            return _freq_columns(t, rings, level)
        finally:
            lib.arp_table_free(t)

    def contact_timelines(self, structure: Structure, frames=None, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, rings: bool = False,
                          level: str = "atom", bitmap: bool = True, waters: bool = False) -> dict:
        """arp_contact_timelines as a dict of numpy columns: every column contact_frequencies returns for the same arguments (identical bytes), plus
        first_frame / last_frame / n_events / longest_run (u4) and mean_run (f4) per row (TIMELINE_COLUMNS): the first and last frame in which the
        row's contact exists, its number of uninterrupted stretches, the longest of them in frames, and n_frames / n_events.  bitmap=True adds
        timeline_words [rows, ceil(F / 32)] <u4 -- frame f is bit f & 31 of word f >> 5 (unpack_timeline makes it a bool [rows, F]) -- and
        n_total_frames = F; bitmap=False (ARP_TIMELINE_NO_BITMAP) leaves the bitmap on the device."""
        t = _timeline_table(self, structure, frames, groups, vdw_comp, dist_cutoff, rings, level, bitmap, waters)
        try:
            return _timeline_columns(t, rings, level)
        finally:
            lib.arp_table_free(t)

    def water_bridges(self, structure: Structure, frames=None, groups: str = "/") -> dict:
        """arp_water_bridges as a dict of numpy columns: WATER_BRIDGE_COLUMNS + from_atom / water_atom / to_atom (topology atom indices).  See
        get_water_bridges."""
        t = _water_bridge_table(self, structure, frames, groups)
        try:
            return _read_columns(t, WATER_BRIDGE_COLUMNS, (("from_atom", "i4"), ("water_atom", "i4"), ("to_atom", "i4")))
        finally:
            lib.arp_table_free(t)

    def contact_similarity(self, structure: Structure, frames=None, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, rings: bool = False,
                           level: str = "atom", axis: str = "frames", metric: str = "tanimoto") -> dict:
        """arp_contact_similarity as a dict: every column contact_frequencies returns for the same arguments (identical bytes), plus the [M, M] matrix
        between the frames (axis "frames", M = F: which frames have the same contacts) or between the rows (axis "rows", M = rows: which contacts exist
        in the same frames) -- `similarity` <f4 (metric "tanimoto": |a AND b| / |a OR b|, 1.0 for two empty sets) or `intersection` <u4 (metric
        "count": |a AND b|) -- and `sizes` [M] <u4 (contacts per frame, or frames per row), `axis` and `n_total_frames` = F."""
        owner = _TableOwner(_similarity_table(self, structure, frames, groups, vdw_comp, dist_cutoff, rings, level, axis, metric))
        return _similarity_columns(owner, rings, level, structure, frames)  # (a large matrix is a view of the table's: the table lives as long as it)

    def contact_autocorrelation(self, structure: Structure, frames=None, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, rings: bool = False,
                                level: str = "atom", mode: str = "intermittent", max_lag: int | None = None, matrix: bool = True) -> dict:
        """arp_contact_autocorrelation as a dict: every column contact_frequencies returns for the same arguments (identical bytes), plus `half_life` <f4
        per row (the smallest lag at which the window-corrected survival has fallen to one half; NaN: none), `autocorrelation` <u4 [rows, L + 1] (a view
        of the table's block, absent with matrix=False) -- in how many frames the row's contact exists now and `lag` frames on (mode "intermittent"), or
        without a gap all the way there (mode "continuous") --, `lags` = 0 .. L, `by_interaction` {interaction name: {"counts": <u8 [L + 1], "curve":
        <f8 [L + 1]}} for the interactions that have rows (curve = counts F / (counts[0] (F - lags))), `mode` and `n_total_frames` = F.  max_lag None: F - 1."""
        owner = _TableOwner(_autocorr_table(self, structure, frames, groups, vdw_comp, dist_cutoff, rings, level, mode, max_lag, matrix))
        return _autocorr_columns(owner, rings, level, structure, frames)

    def contact_clusters(self, structure: Structure, frames=None, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, rings: bool = False,
                         level: str = "atom", *, min_similarity: float, max_clusters: int | None = None, counts: bool = True) -> dict:
        """arp_contact_clusters as a dict: every column contact_frequencies returns for the same arguments (identical bytes), plus the gromos clusters of the
        frames on the neighbour relation tanimoto >= min_similarity -- per frame `cluster` <u4 (0xFFFFFFFF: left over by max_clusters),
        `similarity_to_centre` <f4 (NaN for a left-over frame), `n_neighbours` <u4 (the frame's neighbours in the full graph, itself included) and `sizes`
        <u4 (contacts per frame); per cluster `centre` and `cluster_size` <u4; `cluster_counts` <u4 [rows, n_clusters] (in how many frames of each cluster a
        row is present; absent with counts=False), `n_clusters` and `n_total_frames` = F.  The frame-by-frame matrix never exists: the call also takes the
        ensembles contact_similarity refuses."""
        owner = _TableOwner(_cluster_table(self, structure, frames, groups, vdw_comp, dist_cutoff, rings, level, min_similarity, max_clusters, counts))
        return _cluster_columns(owner, rings, level)

    def rmsd(self, structure: Structure, frames=None, reference=0, atoms="ca", chains: str = "") -> np.ndarray:
        """arp_rmsd_reference: <f4 [F], the rmsd of every frame to `reference` after optimal superposition (proper rotations only) on the atoms of
        rmsd_select(structure, atoms, chains).  reference: a frame index (that entry is 0.0, the others are the bytes of rmsd_matrix's row) or an [N, 3]
        array of the topology's atoms.  frames: [F, N, 3] f64; None: the structure's models."""
        return _rmsd_reference(self, structure, frames, reference, atoms, chains)

    def rmsd_matrix(self, structure: Structure, frames=None, atoms="ca", chains: str = "") -> np.ndarray:
        """arp_rmsd_matrix: <f4 [F, F], the rmsd between every two frames; exactly symmetric, the diagonal exactly 0."""
        return _rmsd_matrix(self, structure, frames, atoms, chains)

    def rmsd_clusters(self, structure: Structure, frames=None, atoms="ca", chains: str = "", *, cutoff: float, max_clusters: int | None = None) -> dict:
        """arp_rmsd_clusters as a dict: the gromos clusters of the frames on the neighbour relation rmsd <= cutoff (f32, inclusive) -- per frame `cluster`
        <u4 (0xFFFFFFFF: left over by max_clusters), `rmsd_to_centre` <f4 (the matrix entry's bytes; 0.0 for a centre, NaN for a left-over frame) and
        `n_neighbours` <u4 (itself included); per cluster `centre` and `cluster_size` <u4; `n_clusters`.  The matrix never exists."""
        return _rmsd_clusters(self, structure, frames, atoms, chains, cutoff, max_clusters)

    def rmsf(self, structure: Structure, frames=None, fit="ca", atoms=None, chains: str = "", reference="mean", max_rounds: int = 50, tol: float = 1e-4, level: str = "atom",
             aligned: bool = False, transforms: bool = False) -> dict:
        """arp_rmsf as a dict: the frames superposed on the atoms `fit` onto `reference` ("mean": the iterated mean structure from frame 0; a frame index or
        an [N, 3] array: one fit to it), their mean and each measured atom's fluctuation about it -- `atom`, `mean`, `rmsf`, `bfactor`, `frame_rmsd`,
        `n_rounds`, `last_change`, `converged`, on request `aligned` and `transforms`, with level="residue" also `residue` (get_rmsf)."""
        return _rmsf(self, structure, frames, fit, atoms, chains, reference, max_rounds, tol, level, aligned, transforms)

    def covariance(self, structure: Structure, frames=None, fit="ca", atoms=None, chains: str = "", reference="mean", max_rounds: int = 50, tol: float = 1e-4, cov: bool = True,
                   dccm: bool = False, transforms: bool = False) -> dict:
        """arp_covariance as a dict: rmsf's keys (the same superposition, byte for byte) plus `covariance` <f8 [3m, 3m] (cov=True: the second moments of the
        superposed coordinates about their mean, atom-major, divisor F) and / or `dccm` <f4 [m, m] (dccm=True: the dynamic cross-correlation map)."""
        return _covariance(self, structure, frames, fit, atoms, chains, reference, max_rounds, tol, cov, dccm, transforms)

    def dccm(self, structure: Structure, frames=None, fit="ca", atoms=None, chains: str = "", reference="mean", max_rounds: int = 50, tol: float = 1e-4,
             transforms: bool = False) -> dict:
        """covariance() with the `dccm` output only."""
        return _covariance(self, structure, frames, fit, atoms, chains, reference, max_rounds, tol, False, True, transforms)

    def project(self, structure: Structure, frames, atoms, mean, modes, transforms=None) -> np.ndarray:
        """arp_project: <f8 [F, k], the deviations of the measured atoms from `mean` [m, 3] along `modes` [k, 3m] (atom-major rows).  transforms [F, 12]
        (as rmsf returns them) are applied to the frames' absolute coordinates first; None: the frames are already superposed.  No fit is repeated."""
        return _project(self, structure, frames, atoms, mean, modes, transforms)

    def pca(self, structure: Structure, frames=None, fit="ca", atoms=None, chains: str = "", reference="mean", max_rounds: int = 50, tol: float = 1e-4, n_modes: int = 10) -> dict:
        """Principal components of the superposed coordinates ("essential dynamics"): covariance() on the device, numpy.linalg.eigh on the HOST (the eigen-solve
        is not on the device), project() on the device.  See get_pca for the keys."""
        return _pca(self, structure, frames, fit, atoms, chains, reference, max_rounds, tol, n_modes)

    def secondary_structure(self, structure: Structure, frames=None, chains: str = "", codes: bool = True, hbonds: bool = False) -> dict:
        """arp_dssp as a dict: the secondary structure (Kabsch & Sander) of every frame and each residue's share of the frames in every state -- `residue`,
        `counts`, `fraction`, `frame_counts`, with codes=True `codes`, with hbonds=True `hb_acceptor` and `hb_energy` (get_secondary_structure)."""
        return _secondary_structure(self, structure, frames, chains, codes, hbonds)

    def torsions(self, structure: Structure, frames=None, chains: str = "", kinds=("phi", "psi", "omega", "chi"), bins: int = 36, rama="class", angles: bool = True,
                 cossin: bool = False, states: bool = False) -> dict:
        """arp_torsions as a dict: phi, psi, omega and chi of every frame, their rotamer states, transitions, circular statistics, histograms and the
        Ramachandran maps of the ensemble (get_torsions)."""
        return _torsions(self, structure, frames, chains, kinds, bins, rama, angles, cossin, states)

    def sc_ensemble(self, structure: Structure, frames=None, groups: str = "/") -> dict:
        """arp_structure_sc_ensemble as a dict: shape complementarity of every frame of an ensemble (the selection and radii of get_sc on model 0).
        frames: [F, N, 3] f64 coordinates of the N atoms of model 0; None: the structure's models.  Keys: atoms (u32 structure indices of the m
        selected atoms), molecule [m], n_frames, results (F arp_sc_results as a structured array, SC_RESULTS_DTYPE), status [F] (indices into
        SC_FRAME_STATUS), err_atoms [F, 2] (rows of the coincident pair, ~0 elsewhere), frames_in_interface [m] u32, trimmed_dots [m] u64."""
        return _sc_ensemble(self, structure, frames, groups)

    def sasa_ensemble(self, structure: Structure, frames=None, chains: str = "", probe_radius: float = 1.4, n_points: int = 100, sap_radius: float | None = None,
                      per_frame: bool = False, radii=None) -> dict:
        """arp_sasa_ensemble as a dict of numpy arrays: per-atom SASA statistics over the frames of an ensemble, and SAP statistics when
        sap_radius is given.  frames: [F, N, 3] f64 coordinates of the topology's N atoms (model 0 of `structure`); None: the structure's models
        are the frames.  Keys: atoms (u32 structure indices of the m selected atoms), n_frames, mean_sasa / std_sasa / min_sasa / max_sasa [m],
        total_sasa [F], with SAP mean_sap / std_sap / min_sap / max_sap [m]; per_frame adds count [F, m] i32 and, with SAP, sap [F, m] f32."""
        return _sasa_ensemble(self, structure, frames, chains, probe_radius, n_points, sap_radius, per_frame, radii)

    def residue_sasa_ensemble(self, structure: Structure, frames=None, chains: str = "", probe_radius: float = 1.4, n_points: int = 100,
                              radii: str = "protor", per_frame: bool = False) -> dict:
        """arp_sasa_ensemble_residues as a dict of numpy arrays: residue-level SASA statistics over the frames of an ensemble, summed on the
        device.  Keys: res_atoms / chain_atoms (u32: the first selected atom of every residue / chain), n_frames, is_polar [n_res] bool,
        mean_sasa / std_sasa / min_sasa / max_sasa [n_res], mean_relative_sasa [n_res] (NaN where relative_valid is False), chain_sasa
        [F, n_chains]; per_frame adds residue_sasa [F, n_res]."""
        return _residue_sasa_ensemble(self, structure, frames, chains, probe_radius, n_points, radii, per_frame)

    def buried_sasa(self, structure: Structure, groups: str, probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, radii=None) -> dict:
        """arp_structure_buried_sasa as a dict of numpy arrays: the interface of two chain groups atom by atom and residue by residue, from one
        walk of the split kernel.  Keys: atoms (u32 structure indices, by serial), group (u8: 1, 2, 3), sasa [3, m] f32 and count [3, m] i32
        (complex, group 1, group 2; 0 where the atom is not in the group), buried [m] i32 (points), res_atoms, res_sasa [3, n_res] f32,
        res_buried_atoms [n_res] u32, totals [4] f32 (complex, group 1, group 2, dSASA), dsasa (float)."""
        return _buried_sasa(self, structure, groups, probe_radius, n_points, model_num, radii)

    def dsasa_ensemble(self, structure: Structure, frames=None, groups: str = "/", probe_radius: float = 1.4, n_points: int = 100, radii=None,
                       per_frame: bool = False) -> dict:
        """arp_dsasa_ensemble as a dict of numpy arrays: dSASA of every frame and the per-atom statistics of the buried points over the frames.
        Keys: atoms, group, R (radius + probe) [m], n_frames, sum_buried / sum_buried_sq (u64), min_buried / max_buried (i32), frames_buried (u32)
        [m], total_complex / total_g1 / total_g2 / dsasa [F] f32; per_frame adds buried [F, m] i32."""
        return _dsasa_ensemble(self, structure, frames, groups, probe_radius, n_points, radii, per_frame)


def _check_level(level: str):
    if level not in ("atom", "residue"):
        raise ValueError(f"level must be 'atom' or 'residue', got {level!r}")


def _check_waters(waters: bool, level: str):
    if not isinstance(waters, (bool, np.bool_)):  # (a level passed by position would land here: pass level by keyword)
        raise TypeError(f"waters must be a bool, got {waters!r}")
    if waters and level != "residue":
        raise ValueError("waters=True needs level='residue' (a bridge joins two residues through a water); get_water_bridges lists the atoms of every bridge")


def _read_columns(t, spec, extra=()) -> dict:
    """The numpy columns of a table handle (copies), read through arp_table_column.  spec: (name, kind) pairs as the *_COLUMNS lists hold them --
    "str": NUL-padded bytes of the column's width; interaction: the i4 codes (the names are the Arrow batch's); else the dtype.  extra: more such
    pairs behind them.  A column the table does not have is a KeyError (a table without rows serves none)."""
    n = int(lib.arp_table_rows(t))
    cols = {}
    for name, kind in list(spec) + list(extra):
        w = C.c_int32()
        p = lib.arp_table_column(t, name.encode(), C.byref(w))
        if not p and n:
            raise KeyError(name)
        cols[name] = _np_from(p, n, "<i4" if name == "interaction" else f"S{max(w.value, 1)}" if kind == "str" else "<" + kind)
    return cols


def _arrow_of(t):
    """arp_table_export_arrow of a table handle as a pyarrow.Table (the batch owns copies: the handle may be freed)."""
    import pyarrow as pa

    arr, sch = _lib.ArrowArray(), _lib.ArrowSchema()
    _check(lib.arp_table_export_arrow(t, C.byref(arr), C.byref(sch)))
    return pa.Table.from_batches([pa.RecordBatch._import_from_c(C.addressof(arr), C.addressof(sch))])


def _frame_of(table):
    """What the reference returns (python.rs:55): a polars.DataFrame over the same Arrow buffers when polars is importable, else the pyarrow.Table."""
    try:
        import polars as pl

        return pl.from_arrow(table)
    except ImportError:
        return table


def _with_context(device: int, validate) -> "Context":
    """The default context of `device`.  Without a device, validate() -- the same call with ctx None, which only checks the inputs -- runs first: an
    input error takes precedence over the missing device."""
    try:
        return _context(device)
    except ArpeggiaError:
        validate()
        raise


def _topology_atoms(structure: Structure) -> int:
    """Atoms of model 0 (the topology of arp_contact_frequencies): the leading run of the first MODEL serial."""
    m = structure.ints("model")
    if len(m) == 0:
        return 0
    other = np.flatnonzero(m != m[0])
    return int(other[0]) if len(other) else len(m)


def _freq_table(ctx: "Context | None", structure: Structure, frames, groups: str, vdw_comp: float, dist_cutoff: float, rings: bool = False, level: str = "atom",
                waters: bool = False):
    """arp_contact_frequencies_ex (level "atom") or arp_residue_contact_frequencies ("residue") -> table handle (the caller frees it).  ctx None:
    the inputs are only checked (raises their error, else returns None)."""
    _check_level(level)
    _check_waters(waters, level)
    n_frames, ptr, keep = _frames_arg(structure, frames, "contact frequencies")
    t = C.c_void_p()
    call = lib.arp_residue_contact_frequencies if level == "residue" else lib.arp_contact_frequencies_ex
    _check(call(ctx._h if ctx is not None else None, structure._h, int(n_frames), ptr, groups.encode(), float(vdw_comp),
                float(dist_cutoff), (_lib.ARP_FREQ_RINGS if rings else 0) | (_lib.ARP_FREQ_WATERS if waters else 0), C.byref(t)))
    return t if ctx is not None else None


def _water_bridge_table(ctx: "Context | None", structure: Structure, frames, groups: str):
    """arp_water_bridges -> table handle (the caller frees it).  ctx None: the inputs are only checked (raises their error, else returns None)."""
    n_frames, ptr, keep = _frames_arg(structure, frames, "water bridges")
    t = C.c_void_p()
    _check(lib.arp_water_bridges(ctx._h if ctx is not None else None, structure._h, int(n_frames), ptr, groups.encode(), C.byref(t)))
    return t if ctx is not None else None


def _freq_columns(t, rings: bool, level: str) -> dict:
    """The numpy columns of a frequency table handle (copies): FREQ_COLUMNS + from_atom / to_atom (+ from_ring / to_ring with rings), or
    RESIDUE_FREQ_COLUMNS + from_residue / to_residue."""
    if level == "residue":
        return _read_columns(t, RESIDUE_FREQ_COLUMNS, (("from_residue", "i4"), ("to_residue", "i4")))
    return _read_columns(t, FREQ_COLUMNS, (("from_atom", "i4"), ("to_atom", "i4")) + ((("from_ring", "i4"), ("to_ring", "i4")) if rings else ()))


def _timeline_table(ctx: "Context | None", structure: Structure, frames, groups: str, vdw_comp: float, dist_cutoff: float, rings: bool, level: str, bitmap: bool,
                    waters: bool = False):
    """arp_contact_timelines -> table handle (the caller frees it).  ctx None: the inputs are only checked (raises their error, else returns None)."""
    _check_level(level)
    _check_waters(waters, level)
    n_frames, ptr, keep = _frames_arg(structure, frames, "contact timelines")
    t = C.c_void_p()
    flags = (_lib.ARP_FREQ_RINGS if rings else 0) | (0 if bitmap else _lib.ARP_TIMELINE_NO_BITMAP) | (_lib.ARP_FREQ_WATERS if waters else 0)
    _check(lib.arp_contact_timelines(ctx._h if ctx is not None else None, structure._h, int(n_frames), ptr, groups.encode(), float(vdw_comp), float(dist_cutoff),
                                     flags, 1 if level == "residue" else 0, C.byref(t)))
    return t if ctx is not None else None


def _timeline_columns(t, rings: bool, level: str) -> dict:
    """The frequency columns of a timeline table handle, TIMELINE_COLUMNS and, when the table holds its bitmap, timeline_words + n_total_frames (copies)."""
    cols = _freq_columns(t, rings, level)
    cols.update(_read_columns(t, TIMELINE_COLUMNS))
    n = int(lib.arp_table_rows(t))
    wpr, nf = C.c_uint64(), C.c_uint64()
    p = lib.arp_table_timeline(t, C.byref(wpr), C.byref(nf))
    if p:
        cols["timeline_words"] = _np_from(p, n * wpr.value, "<u4").reshape(n, wpr.value)
        cols["n_total_frames"] = int(nf.value)
    return cols


def unpack_timeline(words, n_frames: int) -> np.ndarray:
    """timeline_words [rows, ceil(F / 32)] <u4 -> bool [rows, F]: present[r, f] = bit f & 31 of words[r, f >> 5]."""
    words = np.ascontiguousarray(words, dtype="<u4")
    if words.ndim != 2 or words.shape[1] != (int(n_frames) + 31) // 32:
        raise ValueError(f"words must have shape [rows, {(int(n_frames) + 31) // 32}] for {n_frames} frames, got {list(words.shape)}")
    return np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")[:, :int(n_frames)].astype(bool)


def timeline_stats(words, n_frames: int) -> dict:
    """arp_timeline_stats (host only, no device): the definition of the timeline statistics, bit by bit, on any bitmap of the timeline_words layout
    -- e.g. a frame window or the AND of two rows.  Returns n_present, first_frame, last_frame (0xFFFFFFFF for a row without a set bit), n_events,
    longest_run, each [rows] <u4."""
    words = np.ascontiguousarray(words, dtype="<u4")
    W = (int(n_frames) + 31) // 32
    if words.ndim != 2 or words.shape[1] != W:
        raise ValueError(f"words must have shape [rows, {W}] for {n_frames} frames, got {list(words.shape)}")
    rows = words.shape[0]
    out = {k: np.zeros(rows, "<u4") for k in ("n_present", "first_frame", "last_frame", "n_events", "longest_run")}
    u32p = C.POINTER(C.c_uint32)
    src = words if words.size else np.zeros(1, "<u4")
    _check(lib.arp_timeline_stats(rows, int(n_frames), src.ctypes.data_as(u32p), *[(v if rows else np.zeros(1, "<u4")).ctypes.data_as(u32p) for v in out.values()]))
    return out


def _similarity_flags(axis: str, metric: str) -> int:
    if axis not in ("frames", "rows"):
        raise ValueError(f"axis must be 'frames' or 'rows', got {axis!r}")
    if metric not in ("tanimoto", "count"):
        raise ValueError(f"metric must be 'tanimoto' or 'count', got {metric!r}")
    return (_lib.ARP_SIM_ROWS if axis == "rows" else 0) | (_lib.ARP_SIM_COUNTS if metric == "count" else 0)


def _similarity_table(ctx: "Context | None", structure: Structure, frames, groups: str, vdw_comp: float, dist_cutoff: float, rings: bool, level: str, axis: str,
                      metric: str):
    """arp_contact_similarity -> table handle (the caller frees it).  ctx None: the inputs are only checked (raises their error, else returns None)."""
    _check_level(level)
    flags = _similarity_flags(axis, metric) | (_lib.ARP_FREQ_RINGS if rings else 0)
    n_frames, ptr, keep = _frames_arg(structure, frames, "contact similarity")
    t = C.c_void_p()
    _check(lib.arp_contact_similarity(ctx._h if ctx is not None else None, structure._h, int(n_frames), ptr, groups.encode(), float(vdw_comp), float(dist_cutoff),
                                      flags, 1 if level == "residue" else 0, C.byref(t)))
    return t if ctx is not None else None


class _TableOwner:
    """Keeps a table handle alive for a numpy view into it; frees it with the last reference."""

    def __init__(self, handle):
        self.t = handle

    def __del__(self):
        if self.t is not None and lib is not None:
            lib.arp_table_free(self.t)
            self.t = None


def _similarity_matrix(owner: _TableOwner) -> dict:
    """similarity / intersection, sizes and axis of a similarity table.  A matrix of 1 MiB and more is a zero-copy view that keeps the table alive (at
    10^4 frames it is 400 MB: a copy would cost more than the kernels); everything else is copied."""
    m, flags, sizes = C.c_uint64(), C.c_uint32(), C.POINTER(C.c_uint32)()
    p = lib.arp_table_similarity(owner.t, C.byref(m), C.byref(flags), C.byref(sizes))
    if not p:
        raise KeyError("similarity")
    M = int(m.value)
    counts = bool(flags.value & _lib.ARP_SIM_COUNTS)
    dtype = "<u4" if counts else "<f4"
    if M * M * 4 >= 1 << 20:
        buf = (C.c_char * (M * M * 4)).from_address(p)
        buf._owner = owner  # the ctypes buffer is the array's base: the table lives exactly as long as the array (and its views)
        matrix = np.frombuffer(buf, dtype=dtype, count=M * M).reshape(M, M)
    else:
        matrix = _np_from(p, M * M, dtype).reshape(M, M)
    out = {"intersection" if counts else "similarity": matrix}
    out["sizes"] = _np_from(C.cast(sizes, C.c_void_p).value, M, "<u4")
    out["axis"] = "rows" if flags.value & _lib.ARP_SIM_ROWS else "frames"
    return out


def _similarity_columns(owner: _TableOwner, rings: bool, level: str, structure: Structure, frames) -> dict:
    cols = _freq_columns(owner.t, rings, level)
    cols.update(_similarity_matrix(owner))
    if frames is not None:
        cols["n_total_frames"] = int(np.asarray(frames).shape[0])
    else:
        cols["n_total_frames"] = len(structure.ints("model")) // max(_topology_atoms(structure), 1)
    return cols


def bit_gram(words, n_bits: int, axis: str = "frames", metric: str = "tanimoto", device: int | None = None) -> tuple:
    """(matrix, sizes) of a bitmap of the timeline_words layout, [rows, ceil(n_bits / 32)] <u4: the Tanimoto values (<f4) or intersection counts (<u4,
    metric "count") between its bit columns (axis "frames": M = n_bits) or its rows (axis "rows": M = rows), and the M set sizes (<u4) -- the
    definitions of Context.contact_similarity.  Bits past n_bits are ignored.  device None: arp_bit_gram_host, a plain loop on the CPU (the yardstick);
    a device number: arp_bit_gram, the same kernels contact_similarity runs.  For bitmaps that were post-processed on the host (a frame window, a
    subset of rows)."""
    flags = _similarity_flags(axis, metric)
    words = np.ascontiguousarray(words, dtype="<u4")
    W = (int(n_bits) + 31) // 32
    if words.ndim != 2 or words.shape[1] != W:
        raise ValueError(f"words must have shape [rows, {W}] for {n_bits} bits, got {list(words.shape)}")
    rows = words.shape[0]
    M = rows if axis == "rows" else int(n_bits)
    out = np.zeros((M, M), "<u4" if metric == "count" else "<f4")
    sizes = np.zeros(M, "<u4")
    u32p = C.POINTER(C.c_uint32)
    ptr = lambda a: (a if a.size else np.zeros(1, a.dtype)).ctypes
    args = (rows, int(n_bits), ptr(words).data_as(u32p), flags, ptr(out).data_as(C.c_void_p), ptr(sizes).data_as(u32p))
    if device is None:
        _check(lib.arp_bit_gram_host(*args))
    else:
        _check(lib.arp_bit_gram(_context(int(device))._h, *args))
    return out, sizes


def _max_clusters_arg(max_clusters) -> int:
    if max_clusters is None:
        return _lib.ARP_NONE
    if int(max_clusters) < 0 or int(max_clusters) >= _lib.ARP_NONE:
        raise ValueError(f"max_clusters must be None or 1 .. 2^32 - 2, got {max_clusters!r}")
    return int(max_clusters)  # (0 is the library's to refuse)


def _cluster_table(ctx: "Context | None", structure: Structure, frames, groups: str, vdw_comp: float, dist_cutoff: float, rings: bool, level: str, min_similarity: float,
                   max_clusters, counts: bool):
    """arp_contact_clusters -> table handle (the caller frees it).  ctx None: the inputs are only checked (raises their error, else returns None)."""
    _check_level(level)
    flags = (_lib.ARP_FREQ_RINGS if rings else 0) | (0 if counts else _lib.ARP_CLUSTER_NO_COUNTS)
    n_frames, ptr, keep = _frames_arg(structure, frames, "contact clusters")
    t = C.c_void_p()
    _check(lib.arp_contact_clusters(ctx._h if ctx is not None else None, structure._h, int(n_frames), ptr, groups.encode(), float(vdw_comp), float(dist_cutoff),
                                    flags, 1 if level == "residue" else 0, float(min_similarity), _max_clusters_arg(max_clusters), C.byref(t)))
    return t if ctx is not None else None


def _cluster_arrays(owner: _TableOwner) -> dict:
    """The per-frame and per-cluster arrays of a cluster table (copies) and its counts: a zero-copy view that keeps the table alive from 1 MiB on."""
    u32p = C.POINTER(C.c_uint32)
    m, n, flags, sim = C.c_uint64(), C.c_uint32(), C.c_uint32(), C.POINTER(C.c_float)()
    nn, sizes, centre, csize, counts = u32p(), u32p(), u32p(), u32p(), u32p()
    p = lib.arp_table_clusters(owner.t, C.byref(m), C.byref(n), C.byref(flags), C.byref(sim), C.byref(nn), C.byref(sizes), C.byref(centre), C.byref(csize), C.byref(counts))
    if not p:
        raise KeyError("cluster")
    F, K, R = int(m.value), int(n.value), int(lib.arp_table_rows(owner.t))
    addr = lambda q: C.cast(q, C.c_void_p).value
    out = {"cluster": _np_from(p, F, "<u4"), "similarity_to_centre": _np_from(addr(sim), F, "<f4"), "n_neighbours": _np_from(addr(nn), F, "<u4"),
           "sizes": _np_from(addr(sizes), F, "<u4"), "centre": _np_from(addr(centre), K, "<u4"), "cluster_size": _np_from(addr(csize), K, "<u4")}
    if addr(counts):
        if R * K * 4 >= 1 << 20:
            buf = (C.c_char * (R * K * 4)).from_address(addr(counts))
            buf._owner = owner  # the ctypes buffer is the array's base: the table lives exactly as long as the array (and its views)
            out["cluster_counts"] = np.frombuffer(buf, dtype="<u4", count=R * K).reshape(R, K)
        else:
            out["cluster_counts"] = _np_from(addr(counts), R * K, "<u4").reshape(R, K)
    out["n_clusters"] = K
    out["n_total_frames"] = F
    return out


def _cluster_columns(owner: _TableOwner, rings: bool, level: str) -> dict:
    cols = _freq_columns(owner.t, rings, level)
    cols.update(_cluster_arrays(owner))
    return cols


def bit_cluster(words, n_bits: int, min_similarity: float, axis: str = "frames", max_clusters: int | None = None, device: int | None = None) -> dict:
    """The gromos clusters of a bitmap of the timeline_words layout, [rows, ceil(n_bits / 32)] <u4, by the definitions of Context.contact_clusters: its bit
    columns (axis "frames": M = n_bits) or its rows (axis "rows": M = rows) are the sets.  Returns cluster, similarity_to_centre, n_neighbours, sizes [M],
    centre, cluster_size [n_clusters], n_clusters and, on axis "frames", cluster_counts [rows, n_clusters].  Bits past n_bits are ignored.  device None:
    arp_bit_cluster_host, plain loops on the CPU (the yardstick); a device number: arp_bit_cluster, the same kernels contact_clusters runs."""
    flags = _similarity_flags(axis, "tanimoto")
    words = np.ascontiguousarray(words, dtype="<u4")
    W = (int(n_bits) + 31) // 32
    if words.ndim != 2 or words.shape[1] != W:
        raise ValueError(f"words must have shape [rows, {W}] for {n_bits} bits, got {list(words.shape)}")
    rows = words.shape[0]
    M = rows if axis == "rows" else int(n_bits)
    cap = min(M, _max_clusters_arg(max_clusters))
    out = {"cluster": np.zeros(M, "<u4"), "similarity_to_centre": np.zeros(M, "<f4"), "n_neighbours": np.zeros(M, "<u4"), "sizes": np.zeros(M, "<u4"),
           "centre": np.zeros(cap, "<u4"), "cluster_size": np.zeros(cap, "<u4")}
    n = np.zeros(1, "<u4")
    counts = np.zeros(rows * cap, "<u4") if axis == "frames" else None
    u32p = C.POINTER(C.c_uint32)
    ptr = lambda a, t=u32p: (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(t)
    args = (rows, int(n_bits), ptr(words), flags, float(min_similarity), _max_clusters_arg(max_clusters), ptr(out["cluster"]),
            ptr(out["similarity_to_centre"], C.POINTER(C.c_float)), ptr(out["n_neighbours"]), ptr(out["sizes"]), ptr(out["centre"]), ptr(out["cluster_size"]), ptr(n),
            ptr(counts) if counts is not None else None)
    if device is None:
        _check(lib.arp_bit_cluster_host(*args))
    else:
        _check(lib.arp_bit_cluster(_context(int(device))._h, *args))
    K = int(n[0])
    out["centre"] = out["centre"][:K].copy()
    out["cluster_size"] = out["cluster_size"][:K].copy()
    out["n_clusters"] = K
    if counts is not None:
        out["cluster_counts"] = counts[:rows * K].reshape(rows, K).copy()
    return out


def _autocorr_flags(mode: str, matrix: bool = True) -> int:
    if mode not in ("intermittent", "continuous"):
        raise ValueError(f"mode must be 'intermittent' or 'continuous', got {mode!r}")
    return (_lib.ARP_ACF_CONTINUOUS if mode == "continuous" else 0) | (0 if matrix else _lib.ARP_ACF_NO_MATRIX)


def _max_lag_arg(max_lag) -> int:
    if max_lag is None:
        return _lib.ARP_NONE
    if int(max_lag) < 0 or int(max_lag) >= _lib.ARP_NONE:
        raise ValueError(f"max_lag must be None or 0 .. 2^32 - 2, got {max_lag!r}")
    return int(max_lag)


def _autocorr_table(ctx: "Context | None", structure: Structure, frames, groups: str, vdw_comp: float, dist_cutoff: float, rings: bool, level: str, mode: str,
                    max_lag, matrix: bool):
    """arp_contact_autocorrelation -> table handle (the caller frees it).  ctx None: the inputs are only checked (raises their error, else returns None)."""
    _check_level(level)
    flags = _autocorr_flags(mode, matrix) | (_lib.ARP_FREQ_RINGS if rings else 0)
    n_frames, ptr, keep = _frames_arg(structure, frames, "contact autocorrelation")
    t = C.c_void_p()
    _check(lib.arp_contact_autocorrelation(ctx._h if ctx is not None else None, structure._h, int(n_frames), ptr, groups.encode(), float(vdw_comp), float(dist_cutoff),
                                           flags, 1 if level == "residue" else 0, _max_lag_arg(max_lag), C.byref(t)))
    return t if ctx is not None else None


def _interaction_curves(sums: np.ndarray, n_frames: int) -> dict:
    """{interaction name: {"counts", "curve"}} of the u64 [n_groups, L + 1] sums, for the interactions with rows (counts[0] > 0): the window-corrected
    estimator C(lag) = (counts[lag] / (F - lag)) / (counts[0] / F)."""
    lags = np.arange(sums.shape[1], dtype=np.float64)
    out = {}
    for c in range(min(sums.shape[0], len(_lib.INTERACTIONS))):
        counts = sums[c]
        if counts[0]:
            out[_lib.INTERACTIONS[c]] = {"counts": counts.copy(), "curve": counts.astype(np.float64) * n_frames / (counts[0].astype(np.float64) * (n_frames - lags))}
    return out


def _autocorr_arrays(owner: _TableOwner) -> dict:
    """autocorrelation (a view that keeps the table alive; absent for a table built without its matrix), lags, the sums and the mode of an autocorrelation table."""
    n_lags, flags, sums, n_groups = C.c_uint64(), C.c_uint32(), C.POINTER(C.c_uint64)(), C.c_uint32()
    p = lib.arp_table_autocorrelation(owner.t, C.byref(n_lags), C.byref(flags), C.byref(sums), C.byref(n_groups))
    if not n_lags.value:
        raise KeyError("autocorrelation")
    R, K = int(lib.arp_table_rows(owner.t)), int(n_lags.value)
    out = {"lags": np.arange(K, dtype="<u4"), "mode": "continuous" if flags.value & _lib.ARP_ACF_CONTINUOUS else "intermittent",
           "sums": _np_from(C.cast(sums, C.c_void_p).value, n_groups.value * K, "<u8").reshape(n_groups.value, K)}
    if p:
        if R:
            buf = (C.c_char * (R * K * 4)).from_address(p)
            buf._owner = owner  # the ctypes buffer is the array's base: the table lives exactly as long as the array (and its views)
            out["autocorrelation"] = np.frombuffer(buf, dtype="<u4", count=R * K).reshape(R, K)
        else:
            out["autocorrelation"] = np.zeros((0, K), "<u4")
    return out


def _autocorr_columns(owner: _TableOwner, rings: bool, level: str, structure: Structure, frames) -> dict:
    cols = _freq_columns(owner.t, rings, level)
    hl = _read_columns(owner.t, (("half_life", "f4"), ("half_life_valid", "u1")))
    cols["half_life"] = np.where(hl["half_life_valid"] != 0, hl["half_life"], np.float32(np.nan)).astype("<f4")
    arrays = _autocorr_arrays(owner)
    F = int(np.asarray(frames).shape[0]) if frames is not None else len(structure.ints("model")) // max(_topology_atoms(structure), 1)
    cols["by_interaction"] = _interaction_curves(arrays.pop("sums"), F)
    cols.update(arrays)
    cols["n_total_frames"] = F
    return cols


def bit_autocorrelation(words, n_bits: int, max_lag: int | None = None, mode: str = "intermittent", group=None, n_groups: int = 0, device: int | None = None,
                        matrix: bool = True) -> dict:
    """The autocorrelation of a bitmap of the timeline_words layout, [rows, ceil(n_bits / 32)] <u4, by the definitions of Context.contact_autocorrelation:
    {"autocorrelation": <u4 [rows, L + 1] (absent with matrix=False), "half_life": <u4 [rows] (0xFFFFFFFF: none), "lags", and with `group` (one group
    number below n_groups per row) "sums": <u8 [n_groups, L + 1]}.  Bits past n_bits are ignored; max_lag None: n_bits - 1.  device None:
    arp_bit_autocorr_host, a plain loop on the CPU (the yardstick); a device number: arp_bit_autocorr, the same kernels contact_autocorrelation runs.  For
    bitmaps that were post-processed on the host (a frame window, the AND of two rows)."""
    flags = _autocorr_flags(mode)
    words = np.ascontiguousarray(words, dtype="<u4")
    W = (int(n_bits) + 31) // 32
    if words.ndim != 2 or words.shape[1] != W:
        raise ValueError(f"words must have shape [rows, {W}] for {n_bits} bits, got {list(words.shape)}")
    rows = words.shape[0]
    lag_arg = _max_lag_arg(max_lag)
    L = max(int(n_bits) - 1, 0) if max_lag is None else int(max_lag)
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    ptr = lambda a: (a if a.size else np.zeros(1, a.dtype)).ctypes
    acf = np.zeros((rows, L + 1), "<u4") if matrix else None
    half = np.zeros(rows, "<u4")
    if group is not None:
        group = np.ascontiguousarray(group, dtype="<u4")
        if group.shape != (rows,):
            raise ValueError(f"group must have shape [{rows}], got {list(group.shape)}")
        sums = np.zeros((int(n_groups), L + 1), "<u8")
    args = (rows, int(n_bits), ptr(words).data_as(u32p), flags, lag_arg, ptr(group).data_as(u32p) if group is not None else None, int(n_groups),
            ptr(acf).data_as(u32p) if matrix else None, ptr(sums).data_as(u64p) if group is not None else None, ptr(half).data_as(u32p))
    if device is None:
        _check(lib.arp_bit_autocorr_host(*args))
    else:
        _check(lib.arp_bit_autocorr(_context(int(device))._h, *args))
    out = {"half_life": half, "lags": np.arange(L + 1, dtype="<u4")}
    if matrix:
        out["autocorrelation"] = acf
    if group is not None:
        out["sums"] = sums
    return out


def _frames_arg(structure: Structure, frames, what: str):
    """(n_frames, pointer, keep-alive array) of an optional [F, N, 3] coordinate array; N = the atoms of model 0."""
    if frames is None:
        return 0, None, None
    keep = np.ascontiguousarray(frames, dtype="<f8")
    n = _topology_atoms(structure)
    if keep.ndim != 3 or keep.shape[1:] != (n, 3):
        raise ArpeggiaError(_lib.ARP_ERR_BAD_INPUT, f"{what}: frames must have shape [F, {n}, 3] (the topology's atoms), got {list(keep.shape)}")
    n_frames = keep.shape[0]
    if keep.size == 0:
        keep = np.zeros(1, dtype="<f8")  # (a valid pointer; n_frames == 0 is refused by the library)
    return n_frames, keep.ctypes.data_as(C.POINTER(C.c_double)), keep


def _sasa_ensemble(ctx: "Context | None", structure: Structure, frames, chains: str, probe_radius: float, n_points: int, sap_radius, per_frame: bool,
                   radii=None) -> dict:
    """arp_sasa_ensemble.  ctx None: the inputs are only checked (raises their error); the result then holds atoms and n_frames only.
    radii: a table name runs arp_sasa_ensemble_radii (SASA only: the SAP score is defined on the van der Waals radii)."""
    if radii is not None:
        return _sasa_ensemble_radii(ctx, structure, frames, chains, probe_radius, n_points, sap_radius, per_frame, radii)
    n_frames, ptr, keep = _frames_arg(structure, frames, "sasa ensemble")
    with_sap = sap_radius is not None
    fp = C.POINTER(C.c_float)
    rows, used = C.c_uint64(), C.c_uint64()
    atoms = np.zeros(max(structure.n_atoms, 1), "<u4")
    args = (structure._h, int(n_frames), ptr, chains.encode(), C.c_float(probe_radius), int(n_points), int(with_sap), C.c_float(sap_radius if with_sap else 0.0),
            C.byref(rows), C.byref(used), atoms.ctypes.data_as(C.POINTER(C.c_uint32)))
    if ctx is None:
        _check(lib.arp_sasa_ensemble(None, *args, *([None] * 11)))
        return {"atoms": atoms[: rows.value].copy(), "n_frames": int(used.value)}
    # outputs sized by their bounds: m <= the topology's atoms, F = the frames given or the structure's models
    n_top = _topology_atoms(structure)
    f_cap = n_frames if frames is not None else (structure.n_atoms // n_top if n_top else 1)
    names = ["mean_sasa", "std_sasa", "min_sasa", "max_sasa"] + (["mean_sap", "std_sap", "min_sap", "max_sap"] if with_sap else [])
    cols = {k: np.zeros(max(n_top, 1), "<f4") for k in names}
    total = np.zeros(max(f_cap, 1), "<f4")
    count = np.zeros(max(f_cap * n_top, 1), "<i4") if per_frame else None
    sap = np.zeros(max(f_cap * n_top, 1), "<f4") if per_frame and with_sap else None
    p = lambda k: cols[k].ctypes.data_as(fp) if k in cols else None  # noqa: E731
    _check(lib.arp_sasa_ensemble(ctx._h, *args, p("mean_sasa"), p("std_sasa"), p("min_sasa"), p("max_sasa"), p("mean_sap"), p("std_sap"), p("min_sap"),
                                 p("max_sap"), total.ctypes.data_as(fp), None if count is None else count.ctypes.data_as(C.POINTER(C.c_int32)),
                                 None if sap is None else sap.ctypes.data_as(fp)))
    del keep
    m, F = int(rows.value), int(used.value)
    out = {"atoms": atoms[:m].copy(), "n_frames": F}
    out.update({k: v[:m].copy() for k, v in cols.items()})
    out["total_sasa"] = total[:F].copy()
    if count is not None:
        out["count"] = count[: F * m].reshape(F, m)
    if sap is not None:
        out["sap"] = sap[: F * m].reshape(F, m)
    return out


def _sasa_ensemble_radii(ctx: "Context | None", structure: Structure, frames, chains: str, probe_radius: float, n_points: int, sap_radius, per_frame: bool,
                         radii) -> dict:
    table = _radii_table(radii)
    if sap_radius is not None:
        raise ValueError("the SAP statistics use the van der Waals radii: radii must be None with sap_radius")
    n_frames, ptr, keep = _frames_arg(structure, frames, "sasa ensemble")
    fp = C.POINTER(C.c_float)
    rows, used = C.c_uint64(), C.c_uint64()
    atoms = np.zeros(max(structure.n_atoms, 1), "<u4")
    args = (structure._h, int(n_frames), ptr, chains.encode(), C.c_float(probe_radius), int(n_points), table, C.byref(rows), C.byref(used),
            atoms.ctypes.data_as(C.POINTER(C.c_uint32)))
    if ctx is None:
        _check(lib.arp_sasa_ensemble_radii(None, *args, *([None] * 6)))
        return {"atoms": atoms[: rows.value].copy(), "n_frames": int(used.value)}
    n_top = _topology_atoms(structure)
    f_cap = n_frames if frames is not None else (structure.n_atoms // n_top if n_top else 1)
    cols = {k: np.zeros(max(n_top, 1), "<f4") for k in ("mean_sasa", "std_sasa", "min_sasa", "max_sasa")}
    total = np.zeros(max(f_cap, 1), "<f4")
    count = np.zeros(max(f_cap * n_top, 1), "<i4") if per_frame else None
    _check(lib.arp_sasa_ensemble_radii(ctx._h, *args, *(cols[k].ctypes.data_as(fp) for k in cols), total.ctypes.data_as(fp),
                                       None if count is None else count.ctypes.data_as(C.POINTER(C.c_int32))))
    del keep
    m, F = int(rows.value), int(used.value)
    out = {"atoms": atoms[:m].copy(), "n_frames": F}
    out.update({k: v[:m].copy() for k, v in cols.items()})
    out["total_sasa"] = total[:F].copy()
    if count is not None:
        out["count"] = count[: F * m].reshape(F, m)
    return out


def _residue_sasa_ensemble(ctx: "Context | None", structure: Structure, frames, chains: str, probe_radius: float, n_points: int, radii, per_frame: bool) -> dict:
    """arp_sasa_ensemble_residues.  ctx None: the inputs are only checked (raises their error); the result then holds res_atoms, chain_atoms
    and n_frames only."""
    table = _radii_table(radii)
    n_frames, ptr, keep = _frames_arg(structure, frames, "sasa ensemble")
    fp, bp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)
    rows, n_chains, used = C.c_uint64(), C.c_uint64(), C.c_uint64()
    n = max(structure.n_atoms, 1)
    res_atoms, chain_atoms = np.zeros(n, "<u4"), np.zeros(n, "<u4")
    head = (structure._h, int(n_frames), ptr, chains.encode(), C.c_float(probe_radius), int(n_points), table, C.byref(rows), C.byref(n_chains), C.byref(used),
            res_atoms.ctypes.data_as(up))
    # the checks alone: they size the outputs (residues, chains, frames)
    _check(lib.arp_sasa_ensemble_residues(None, *head, *([None] * 7), chain_atoms.ctypes.data_as(up), None, None))
    nr, nc, F = int(rows.value), int(n_chains.value), int(used.value)
    if ctx is None:
        return {"res_atoms": res_atoms[:nr].copy(), "chain_atoms": chain_atoms[:nc].copy(), "n_frames": F}
    cols = {k: np.zeros(max(nr, 1), "<f4") for k in ("mean_sasa", "std_sasa", "min_sasa", "max_sasa", "mean_relative_sasa")}
    polar, valid = np.zeros(max(nr, 1), np.uint8), np.zeros(max(nr, 1), np.uint8)
    chain_sasa = np.zeros(max(F * nc, 1), "<f4")
    per = np.zeros(max(F * nr, 1), "<f4") if per_frame else None
    _check(lib.arp_sasa_ensemble_residues(ctx._h, *head, polar.ctypes.data_as(bp), *(cols[k].ctypes.data_as(fp) for k in cols), valid.ctypes.data_as(bp),
                                          chain_atoms.ctypes.data_as(up), chain_sasa.ctypes.data_as(fp), None if per is None else per.ctypes.data_as(fp)))
    del keep
    nr, nc, F = int(rows.value), int(n_chains.value), int(used.value)
    out = {"res_atoms": res_atoms[:nr].copy(), "chain_atoms": chain_atoms[:nc].copy(), "n_frames": F, "is_polar": polar[:nr].astype(bool),
           "relative_valid": valid[:nr].astype(bool), "chain_sasa": chain_sasa[: F * nc].reshape(F, nc)}
    out.update({k: v[:nr].copy() for k, v in cols.items()})
    if per is not None:
        out["residue_sasa"] = per[: F * nr].reshape(F, nr)
    return out


def sasa_ensemble_stats(n_frames: int, radius_plus_probe, n_points: int, s1, s2, cmin, cmax, t1=None, t2=None) -> dict:
    """arp_sasa_ensemble_stats: the host-side finishing of arp_sasa_ensemble from its per-atom accumulators (no device)."""
    R = np.ascontiguousarray(radius_plus_probe, dtype="<f4")
    m = len(R)
    s1, s2 = (np.ascontiguousarray(v, dtype="<u8") for v in (s1, s2))
    cmin, cmax = (np.ascontiguousarray(v, dtype="<i4") for v in (cmin, cmax))
    with_sap = t1 is not None
    if with_sap:
        t1, t2 = (np.ascontiguousarray(v, dtype="<f8") for v in (t1, t2))
    names = ["mean_sasa", "std_sasa", "min_sasa", "max_sasa"] + (["mean_sap", "std_sap"] if with_sap else [])
    out = {k: np.zeros(m, "<f4") for k in names}
    fp, dp, u64, i32 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int32)
    p = lambda k: out[k].ctypes.data_as(fp) if k in out else None  # noqa: E731
    _check(lib.arp_sasa_ensemble_stats(int(n_frames), m, R.ctypes.data_as(fp), int(n_points), s1.ctypes.data_as(u64), s2.ctypes.data_as(u64),
                                       cmin.ctypes.data_as(i32), cmax.ctypes.data_as(i32), t1.ctypes.data_as(dp) if with_sap else None,
                                       t2.ctypes.data_as(dp) if with_sap else None, p("mean_sasa"), p("std_sasa"), p("min_sasa"), p("max_sasa"),
                                       p("mean_sap"), p("std_sap")))
    return out


def sap_weight(resn: str, sasa: float) -> float:
    """hydrophobicity(resn) * clamp(sasa / max side-chain SASA(resn), 0, 1) as src/sap.rs:41-101,198-209 forms it (f32)."""
    return float(lib.arp_sap_weight(str(resn).encode(), C.c_float(sasa)))


def sap_neighbor_sum(ctx: "Context", x, y, z, sidechain, weight, sap_radius: float = 5.0) -> np.ndarray:
    """The radius sum of the SAP score (src/sap.rs:155-204) on the contact engine's cell list: for every side-chain atom the f32 sum of
    `weight` over the side-chain atoms within `sap_radius` (itself included).  The per-atom SASA behind the weights is the caller's."""
    x, y, z = (np.ascontiguousarray(v, dtype="<f8") for v in (x, y, z))
    m = np.ascontiguousarray(sidechain, dtype=np.uint8)
    w = np.ascontiguousarray(weight, dtype="<f4")
    out = np.zeros(len(x), dtype="<f4")
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    _check(lib.arp_sap_neighbor_sum(ctx._h, len(x), x.ctypes.data_as(dp), y.ctypes.data_as(dp), z.ctypes.data_as(dp), m.ctypes.data_as(C.POINTER(C.c_uint8)),
                                    w.ctypes.data_as(fp), C.c_float(sap_radius), out.ctypes.data_as(fp)))
    return out


def atomic_contacts_batch(contexts, atoms_list, params: _lib.arp_params | None = None) -> list:
    """Independent structures over one or more device contexts (arp_contacts_atomic_batch): longest-first deal over the
    contexts, small structures packed into shared launches.  Returns one pair array per structure, in input order."""
    contexts = list(contexts)
    keep = []
    views = [atoms_from_arrays(a, keep=keep) if isinstance(a, dict) else a for a in atoms_list]
    params = params or default_params()
    arr = (C.POINTER(_lib.arp_atoms) * max(len(views), 1))(*[C.pointer(v) for v in views])
    outs = (_lib.arp_pairs * max(len(views), 1))()
    handles = (C.c_void_p * len(contexts))(*[c._h for c in contexts])
    st = lib.arp_contacts_atomic_batch(handles, len(contexts), arr, len(views), C.byref(params), outs)
    if st != _lib.ARP_OK:
        for k in range(len(views)):
            lib.arp_pairs_free(C.byref(outs[k]))
        _check(st)
    result = []
    for k in range(len(views)):  # every list becomes a zero-copy numpy view that frees it with its last reference
        one = _lib.arp_pairs()
        one.n, one.data, one.location = outs[k].n, outs[k].data, outs[k].location
        result.append(_adopt_pairs(one))
    return result


_default_ctx: dict = {}


def _context(device: int = 0) -> Context:
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]


def load_model(input_file, ignore_zero_occupancy: bool = False) -> Structure:
    """utils.rs:51-63."""
    return Structure.load(input_file, ignore_zero_occupancy)


def get_contacts(structure: Structure, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, device: int = 0,
                 num_threads: int = -1):
    """`arpeggia::get_contacts(&pdb, groups, vdw_comp, dist_cutoff) -> DataFrame` (mod.rs:61).

    The table crosses into Python as one Arrow record batch (arp_table_export_arrow): no per-row Python work.
    `num_threads`: host workers of THIS call (0 = all cores, < 0 = the process-wide default of arp_set_num_threads)."""
    return _table(_context(device), structure, groups, vdw_comp, dist_cutoff, num_threads)


def _table(ctx: "Context", structure: Structure, groups: str, vdw_comp: float, dist_cutoff: float, num_threads: int = -1):
    t = C.c_void_p()
    _check(lib.arp_get_contacts_mt(ctx._h, structure._h, groups.encode(), vdw_comp, dist_cutoff, int(num_threads), C.byref(t)))
    try:
        table = _arrow_of(t)
    finally:
        lib.arp_table_free(t)
    return _frame_of(table)


def contacts(input_file: str, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5,
             ignore_zero_occupancy: bool = False, num_threads: int = 1):
    """Drop-in for `arpeggia.contacts` (src/python.rs:31-56): same keywords and defaults, 20-column table.

    Returns a polars.DataFrame when polars is importable, else the identical pyarrow.Table.  `num_threads` sizes the host
    workers of this call only (the reference builds a scoped rayon pool per call, utils.rs:8-30; 0 = all cores); no
    process-wide state is touched, and the search and classification run on the GPU regardless.
    """
    s = Structure.load(input_file, ignore_zero_occupancy)
    return get_contacts(s, groups, vdw_comp, dist_cutoff, num_threads=int(num_threads))


def get_contact_frequencies(structure: Structure, frames=None, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, device: int = 0,
                            rings: bool = False, waters: bool = False, level: str = "atom"):
    """How often every atom-atom contact occurs across the frames of an ensemble (arp_contact_frequencies_ex): one row per distinct
    (from atom, to atom, interaction) with n_frames, frequency, min_distance and max_distance (FREQ_COLUMNS).  frames: [F, N, 3] f64
    coordinates of the N atoms of the topology (model 0 of `structure`); None: the structure's models are the frames.  rings=True adds the
    ring rows (CationPi, Pi* stackings; atomn "Ring", atomi 0) of every frame regarded as a single-model structure, behind the atom rows;
    ring-ring rows do not depend on dist_cutoff.  level="residue" (arp_residue_contact_frequencies): one row per distinct (residue of from,
    residue of to, interaction) instead -- n_frames counts the distinct frames in which ANY item of the residue pair has the interaction (what
    the atom-level table cannot give), min_distance / max_distance are the extremes over those frames of the frame's closest approach
    (RESIDUE_FREQ_COLUMNS).  waters=True (level="residue" only; ValueError otherwise, before any device work) adds the water-bridge rows,
    interaction "WaterBridge": residue pair (A, B) is bridged in a frame when a water atom (residue HOH, not hydrogen) lies within 3.5 A of a polar
    heavy atom (donor or acceptor) of A and of one of B, A in the ligand and B in the receptor set, under the residue rule of the contact table
    (one orientation per pair, residues at least two apart on one chain); the water's own chain plays no part, nor do vdw_comp and dist_cutoff.
    The row's distance is the longer leg of the frame's tightest bridge.  Returns a polars.DataFrame when polars is importable, else a
    pyarrow.Table, like get_contacts."""
    _check_level(level)
    _check_waters(waters, level)
    ctx = _with_context(device, lambda: _freq_table(None, structure, frames, groups, vdw_comp, dist_cutoff, rings, level, waters))
    t = _freq_table(ctx, structure, frames, groups, vdw_comp, dist_cutoff, rings, level, waters)
    try:
        table = _arrow_of(t)
    finally:
        lib.arp_table_free(t)
    return _frame_of(table)


def contact_frequencies(input_file: str, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, ignore_zero_occupancy: bool = False,
                        rings: bool = False, waters: bool = False, level: str = "atom"):
    """Contact frequencies across the models of a multi-model file (NMR models, MODEL-record snapshots): see get_contact_frequencies.  With
    rings=True the rings are those of model 0 regarded as a single-model structure, not what get_contacts files for the multi-model file.
    level="residue": the residue-level table; waters=True: with the water-bridge rows."""
    _check_level(level)
    _check_waters(waters, level)
    return get_contact_frequencies(Structure.load(input_file, ignore_zero_occupancy), None, groups, vdw_comp, dist_cutoff, rings=rings, level=level, waters=waters)


def get_contact_timelines(structure: Structure, frames=None, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, device: int = 0,
                          rings: bool = False, level: str = "atom", bitmap: bool = True, waters: bool = False) -> dict:
    """When every contact of an ensemble exists (arp_contact_timelines): the rows of get_contact_frequencies for the same arguments, as a dict of
    numpy columns -- the frequency columns of the level (FREQ_COLUMNS + from_atom / to_atom, with rings from_ring / to_ring; RESIDUE_FREQ_COLUMNS +
    from_residue / to_residue), identical bytes -- plus TIMELINE_COLUMNS per row: first_frame, last_frame, n_events (maximal runs of consecutive
    frames with the contact), longest_run (frames) and mean_run = n_frames / n_events.  bitmap=True adds timeline_words [rows, ceil(F / 32)] <u4
    (frame f = bit f & 31 of word f >> 5; unpack_timeline) and n_total_frames.  frames, groups, rings, level and waters as get_contact_frequencies
    (bit_gram, bit_autocorrelation and bit_cluster on timeline_words give similarity, lifetimes and clusters of tables with water-bridge rows)."""
    _check_level(level)
    _check_waters(waters, level)
    ctx = _with_context(device, lambda: _timeline_table(None, structure, frames, groups, vdw_comp, dist_cutoff, rings, level, bitmap, waters))
    return ctx.contact_timelines(structure, frames, groups, vdw_comp, dist_cutoff, rings, level, bitmap, waters)


def contact_timelines(input_file: str, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, ignore_zero_occupancy: bool = False,
                      rings: bool = False, level: str = "atom", bitmap: bool = True, waters: bool = False) -> dict:
    """Contact timelines across the models of a multi-model file (the models are the frames): see get_contact_timelines."""
    _check_level(level)
    _check_waters(waters, level)
    return get_contact_timelines(Structure.load(input_file, ignore_zero_occupancy), None, groups, vdw_comp, dist_cutoff, rings=rings, level=level, bitmap=bitmap, waters=waters)


def get_water_bridges(structure: Structure, frames=None, groups: str = "/", device: int = 0):
    """Every water bridge of every frame (arp_water_bridges): one row per (frame, from atom, to atom, water atom) with the identity of the three atoms,
    the two legs (from_distance, to_distance) and the longer of them (distance) -- WATER_BRIDGE_COLUMNS.  The rule is get_contact_frequencies'
    waters=True; grouping the rows by the residues of from and to gives that table's WaterBridge rows.  frames and groups as get_contact_frequencies.
    Returns a polars.DataFrame when polars is importable, else a pyarrow.Table."""
    ctx = _with_context(device, lambda: _water_bridge_table(None, structure, frames, groups))
    t = _water_bridge_table(ctx, structure, frames, groups)
    try:
        table = _arrow_of(t)
    finally:
        lib.arp_table_free(t)
    return _frame_of(table)


def water_bridges(input_file: str, groups: str = "/", ignore_zero_occupancy: bool = False):
    """Water bridges of every model of a file (the models are the frames): see get_water_bridges."""
    return get_water_bridges(Structure.load(input_file, ignore_zero_occupancy), None, groups)


def get_contact_similarity(structure: Structure, frames=None, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, device: int = 0,
                           rings: bool = False, level: str = "atom", axis: str = "frames", metric: str = "tanimoto") -> dict:
    """Which frames of an ensemble look alike, which contacts come and go together (arp_contact_similarity): the rows of get_contact_frequencies for
    the same arguments as a dict of numpy columns, identical bytes, plus the [M, M] matrix of the per-frame contact fingerprints (axis "frames", M =
    F) or of the rows' frame sets (axis "rows", M = rows): `similarity` <f4 (metric "tanimoto") or `intersection` <u4 (metric "count"), with `sizes`
    [M] <u4, `axis` and `n_total_frames`.  frames, groups, rings and level as get_contact_frequencies."""
    _check_level(level)
    _similarity_flags(axis, metric)
    ctx = _with_context(device, lambda: _similarity_table(None, structure, frames, groups, vdw_comp, dist_cutoff, rings, level, axis, metric))
    return ctx.contact_similarity(structure, frames, groups, vdw_comp, dist_cutoff, rings, level, axis, metric)


def contact_similarity(input_file: str, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, ignore_zero_occupancy: bool = False,
                       rings: bool = False, level: str = "atom", axis: str = "frames", metric: str = "tanimoto") -> dict:
    """Contact similarity across the models of a multi-model file (the models are the frames): see get_contact_similarity."""
    _check_level(level)
    _similarity_flags(axis, metric)
    return get_contact_similarity(Structure.load(input_file, ignore_zero_occupancy), None, groups, vdw_comp, dist_cutoff, rings=rings, level=level, axis=axis, metric=metric)


def get_contact_autocorrelation(structure: Structure, frames=None, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, device: int = 0,
                                rings: bool = False, level: str = "atom", mode: str = "intermittent", max_lag: int | None = None, matrix: bool = True) -> dict:
    """How long every contact of an ensemble lives and how fast it decays (arp_contact_autocorrelation): the rows of get_contact_frequencies for the same
    arguments as a dict of numpy columns, identical bytes, plus `half_life` <f4 per row (NaN: none), `autocorrelation` <u4 [rows, L + 1] (absent with
    matrix=False), `lags`, `by_interaction` {interaction name: {"counts": <u8 [L + 1], "curve": <f8 [L + 1]}}, `mode` and `n_total_frames`.  mode
    "intermittent": the contact exists now and `lag` frames on; "continuous": and in every frame between.  max_lag None: F - 1.  frames, groups, rings and
    level as get_contact_frequencies."""
    _check_level(level)
    _autocorr_flags(mode, matrix)
    ctx = _with_context(device, lambda: _autocorr_table(None, structure, frames, groups, vdw_comp, dist_cutoff, rings, level, mode, max_lag, matrix))
    return ctx.contact_autocorrelation(structure, frames, groups, vdw_comp, dist_cutoff, rings, level, mode, max_lag, matrix)


def contact_autocorrelation(input_file: str, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, ignore_zero_occupancy: bool = False,
                            rings: bool = False, level: str = "atom", mode: str = "intermittent", max_lag: int | None = None, matrix: bool = True) -> dict:
    """Contact autocorrelation across the models of a multi-model file (the models are the frames): see get_contact_autocorrelation."""
    _check_level(level)
    _autocorr_flags(mode, matrix)
    return get_contact_autocorrelation(Structure.load(input_file, ignore_zero_occupancy), None, groups, vdw_comp, dist_cutoff, rings=rings, level=level, mode=mode,
                                       max_lag=max_lag, matrix=matrix)


def get_contact_clusters(structure: Structure, frames=None, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, device: int = 0, rings: bool = False,
                         level: str = "atom", *, min_similarity: float, max_clusters: int | None = None, counts: bool = True) -> dict:
    """Which conformational states an ensemble has, which frame stands for each and which contacts tell them apart (arp_contact_clusters): the rows of
    get_contact_frequencies for the same arguments as a dict of numpy columns, identical bytes, plus the gromos clusters (Daura et al. 1999) of the frames'
    contact fingerprints on the neighbour relation tanimoto >= min_similarity: `cluster`, `similarity_to_centre`, `n_neighbours`, `sizes` per frame, `centre`
    and `cluster_size` per cluster, `cluster_counts` [rows, n_clusters] (absent with counts=False), `n_clusters` and `n_total_frames`.  min_similarity has no
    default: there is no meaningful one.  max_clusters None: no limit.  frames, groups, rings and level as get_contact_frequencies."""
    _check_level(level)
    ctx = _with_context(device, lambda: _cluster_table(None, structure, frames, groups, vdw_comp, dist_cutoff, rings, level, min_similarity, max_clusters, counts))
    return ctx.contact_clusters(structure, frames, groups, vdw_comp, dist_cutoff, rings, level, min_similarity=min_similarity, max_clusters=max_clusters, counts=counts)


def contact_clusters(input_file: str, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, ignore_zero_occupancy: bool = False, rings: bool = False,
                     level: str = "atom", *, min_similarity: float, max_clusters: int | None = None, counts: bool = True) -> dict:
    """Contact clusters across the models of a multi-model file (the models are the frames): see get_contact_clusters."""
    _check_level(level)
    return get_contact_clusters(Structure.load(input_file, ignore_zero_occupancy), None, groups, vdw_comp, dist_cutoff, rings=rings, level=level,
                                min_similarity=min_similarity, max_clusters=max_clusters, counts=counts)


# ---- RMSD between frames after optimal superposition (arp_rmsd_matrix / arp_rmsd_reference / arp_rmsd_clusters) ----
RMSD_ATOMS = ("ca", "backbone", "heavy", "all")


def rmsd_select(structure: Structure, atoms="ca", chains: str = "") -> np.ndarray:
    """The <u4 topology atom indices (model 0, strictly increasing) an rmsd call superposes on.  atoms: "ca" (atom name CA), "backbone" (N, CA, C, O),
    "heavy" (not hydrogen) or "all" -- residue HOH is left out of every keyword, every altloc that matches is kept -- or an explicit integer array, which
    is passed through sorted (a duplicate is an error).  chains: a comma list of chain ids ("" = every chain) that the keywords are restricted to."""
    n = _topology_atoms(structure)
    if not isinstance(atoms, str):
        a = np.asarray(atoms)
        if a.ndim != 1 or a.dtype.kind not in "iu":
            raise ValueError(f"atoms must be one of {RMSD_ATOMS} or a 1-D integer array, got {atoms!r}")
        if len(a) and (int(a.min()) < 0 or int(a.max()) >= 1 << 32):
            raise ValueError("atoms: an index is negative or does not fit 32 bits")
        a = np.sort(a.astype("<u4"))
        if len(a) > 1 and (np.diff(a.astype(np.int64)) == 0).any():
            raise ValueError("atoms: duplicate indices")
        return a
    if atoms not in RMSD_ATOMS:
        raise ValueError(f"atoms must be one of {RMSD_ATOMS} or an integer array, got {atoms!r}")
    name, resn, elem, chain = (structure.strings(k)[:n] for k in ("atomn", "resn", "element", "chain"))
    keep = resn != b"HOH"
    if atoms == "ca":
        keep &= name == b"CA"
    elif atoms == "backbone":
        keep &= np.isin(name, [b"N", b"CA", b"C", b"O"])
    elif atoms == "heavy":
        keep &= ~np.isin(elem, [b"H", b"D"])
    wanted = [c.strip().encode() for c in chains.split(",") if c.strip()]
    if wanted:
        keep &= np.isin(chain, wanted)
    return np.flatnonzero(keep).astype("<u4")


def _rmsd_args(structure: Structure, frames, atoms, chains: str, what: str):
    """(the leading arguments of the arp_rmsd_* calls behind ctx, F or None when the models are the frames, keep-alive arrays)."""
    sel = rmsd_select(structure, atoms, chains)
    n_frames, ptr, keep = _frames_arg(structure, frames, what)
    sel_keep = sel if len(sel) else np.zeros(1, "<u4")
    return (structure._h, int(n_frames), ptr, sel_keep.ctypes.data_as(C.POINTER(C.c_uint32)), len(sel)), (keep, sel_keep)


def _rmsd_frames(structure: Structure, frames) -> int:
    n = _topology_atoms(structure)
    return int(np.asarray(frames).shape[0]) if frames is not None else (structure.n_atoms // n if n else 0)


def _rmsd_matrix(ctx: "Context | None", structure: Structure, frames, atoms, chains: str):
    """arp_rmsd_matrix.  ctx None: the inputs are only checked (raises their error, else returns None)."""
    args, keep = _rmsd_args(structure, frames, atoms, chains, "rmsd matrix")
    if ctx is None:
        _check(lib.arp_rmsd_matrix(None, *args, None))
        return None
    F = _rmsd_frames(structure, frames)
    out = np.zeros((F, F), "<f4")
    _check(lib.arp_rmsd_matrix(ctx._h, *args, (out if out.size else np.zeros(1, "<f4")).ctypes.data_as(C.POINTER(C.c_float))))
    return out


def _rmsd_reference(ctx: "Context | None", structure: Structure, frames, reference, atoms, chains: str):
    """arp_rmsd_reference.  ctx None: the inputs are only checked."""
    args, keep = _rmsd_args(structure, frames, atoms, chains, "rmsd")
    ref_keep, ref_ptr, ref_frame = None, None, 0
    if isinstance(reference, (int, np.integer)):
        if int(reference) < 0:
            raise ValueError(f"reference must be a frame index or an [N, 3] array, got {reference!r}")
        ref_frame = int(reference)
    else:
        n = _topology_atoms(structure)
        ref_keep = np.ascontiguousarray(reference, dtype="<f8")
        if ref_keep.shape != (n, 3):
            raise ArpeggiaError(_lib.ARP_ERR_BAD_INPUT, f"rmsd: reference must be a frame index or have shape [{n}, 3] (the topology's atoms), got {list(ref_keep.shape)}")
        ref_ptr = (ref_keep if ref_keep.size else np.zeros(1, "<f8")).ctypes.data_as(C.POINTER(C.c_double))
    if ctx is None:
        _check(lib.arp_rmsd_reference(None, *args, ref_ptr, ref_frame, None))
        return None
    out = np.zeros(_rmsd_frames(structure, frames), "<f4")
    _check(lib.arp_rmsd_reference(ctx._h, *args, ref_ptr, ref_frame, (out if out.size else np.zeros(1, "<f4")).ctypes.data_as(C.POINTER(C.c_float))))
    return out


def _rmsd_clusters(ctx: "Context | None", structure: Structure, frames, atoms, chains: str, cutoff: float, max_clusters):
    """arp_rmsd_clusters.  ctx None: the inputs are only checked."""
    args, keep = _rmsd_args(structure, frames, atoms, chains, "rmsd clusters")
    cap_arg = _max_clusters_arg(max_clusters)
    if ctx is None:
        _check(lib.arp_rmsd_clusters(None, *args, C.c_float(cutoff), cap_arg, *([None] * 6)))
        return None
    F = _rmsd_frames(structure, frames)
    cap = min(F, cap_arg)
    out = {"cluster": np.zeros(F, "<u4"), "rmsd_to_centre": np.zeros(F, "<f4"), "n_neighbours": np.zeros(F, "<u4"), "centre": np.zeros(cap, "<u4"),
           "cluster_size": np.zeros(cap, "<u4")}
    n = np.zeros(1, "<u4")
    u32p = C.POINTER(C.c_uint32)
    ptr = lambda a, t=u32p: (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(t)
    _check(lib.arp_rmsd_clusters(ctx._h, *args, C.c_float(cutoff), cap_arg, ptr(out["cluster"]), ptr(out["rmsd_to_centre"], C.POINTER(C.c_float)), ptr(out["n_neighbours"]),
                                 ptr(out["centre"]), ptr(out["cluster_size"]), ptr(n)))
    K = int(n[0])
    out["centre"] = out["centre"][:K].copy()
    out["cluster_size"] = out["cluster_size"][:K].copy()
    out["n_clusters"] = K
    return out


def rmsd_host(xyz_sel) -> np.ndarray:
    """arp_rmsd_host: the <f4 [F, F] rmsd matrix of [F, n, 3] f64 coordinates (the selected atoms only) by the definition in plain sequential C++ on the
    CPU -- the yardstick of the device calls."""
    x = np.ascontiguousarray(xyz_sel, dtype="<f8")
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"xyz_sel must have shape [F, n, 3], got {list(x.shape)}")
    F, n = x.shape[:2]
    out = np.zeros((F, F), "<f4")
    _check(lib.arp_rmsd_host(F, n, (x if x.size else np.zeros(1, "<f8")).ctypes.data_as(C.POINTER(C.c_double)), (out if out.size else np.zeros(1, "<f4")).ctypes.data_as(C.POINTER(C.c_float))))
    return out


def get_rmsd(structure: Structure, frames=None, reference=0, atoms="ca", chains: str = "", device: int = 0) -> np.ndarray:
    """How far every frame of an ensemble is from a reference: <f4 [F], the rmsd after optimal superposition (proper rotations only: a mirror image does
    not superpose) on the atoms of rmsd_select(structure, atoms, chains).  reference: a frame index (default: the first frame) or an [N, 3] array of the
    topology's atoms.  frames: [F, N, 3] f64 coordinates of the atoms of model 0; None: the structure's models."""
    ctx = _with_context(device, lambda: _rmsd_reference(None, structure, frames, reference, atoms, chains))
    return ctx.rmsd(structure, frames, reference, atoms, chains)


def get_rmsd_matrix(structure: Structure, frames=None, atoms="ca", chains: str = "", device: int = 0) -> np.ndarray:
    """The rmsd between every two frames of an ensemble, <f4 [F, F]: exactly symmetric, the diagonal exactly 0.  Arguments as get_rmsd."""
    ctx = _with_context(device, lambda: _rmsd_matrix(None, structure, frames, atoms, chains))
    return ctx.rmsd_matrix(structure, frames, atoms, chains)


def get_rmsd_clusters(structure: Structure, frames=None, atoms="ca", chains: str = "", device: int = 0, *, cutoff: float, max_clusters: int | None = None) -> dict:
    """Which frames of an ensemble are the same conformation: the gromos clusters (Daura et al. 1999) on the neighbour relation rmsd <= cutoff, the loop
    of get_contact_clusters on coordinates.  Keys: cluster, rmsd_to_centre, n_neighbours [F]; centre, cluster_size [n_clusters]; n_clusters.  The F x F
    matrix never exists: the call also takes the ensembles get_rmsd_matrix refuses.  cutoff has no default.  max_clusters None: no limit."""
    ctx = _with_context(device, lambda: _rmsd_clusters(None, structure, frames, atoms, chains, cutoff, max_clusters))
    return ctx.rmsd_clusters(structure, frames, atoms, chains, cutoff=cutoff, max_clusters=max_clusters)


def rmsd(input_file: str, reference=0, atoms="ca", chains: str = "", ignore_zero_occupancy: bool = False) -> np.ndarray:
    """RMSD of every model of a multi-model file to a reference (the models are the frames): see get_rmsd."""
    return get_rmsd(Structure.load(input_file, ignore_zero_occupancy), None, reference, atoms, chains)


def rmsd_matrix(input_file: str, atoms="ca", chains: str = "", ignore_zero_occupancy: bool = False) -> np.ndarray:
    """RMSD between the models of a multi-model file: see get_rmsd_matrix."""
    return get_rmsd_matrix(Structure.load(input_file, ignore_zero_occupancy), None, atoms, chains)


def rmsd_clusters(input_file: str, atoms="ca", chains: str = "", ignore_zero_occupancy: bool = False, *, cutoff: float, max_clusters: int | None = None) -> dict:
    """RMSD clusters of the models of a multi-model file: see get_rmsd_clusters."""
    return get_rmsd_clusters(Structure.load(input_file, ignore_zero_occupancy), None, atoms, chains, cutoff=cutoff, max_clusters=max_clusters)


# ---- RMSF and the mean structure: the frames superposed on a reference or on their iterated mean (arp_rmsf) ----
RMSF_COLUMNS = ["chain", "resn", "resi", "insertion", "altloc", "atomn", "atomi", "mean_x", "mean_y", "mean_z", "rmsf", "bfactor"]
RMSF_RESIDUE_COLUMNS = ["chain", "resn", "resi", "insertion", "n_atoms", "rmsf", "bfactor"]
_BFACTOR = 8.0 * np.pi ** 2 / 3.0


def _bfactor(rmsf_values: np.ndarray) -> np.ndarray:
    """B = 8 pi^2 / 3 rmsf^2, formed in f64 from the f32 rmsf and rounded to f32 once."""
    r = np.asarray(rmsf_values, np.float64)
    return (_BFACTOR * r * r).astype("<f4")


def rmsf_residues(chain, resi, insertion, rmsf_values) -> dict:
    """Residue rows from atom rows: the atoms sharing (chain, resi, insertion) -- the residue identity of the residue SASA table --, sorted stably by
    (chain as a byte string, resi, insertion).  Per row `first` (the index of its first atom, whose names are the row's), `n_atoms`, `rmsf` = the square
    root of the unweighted mean of rmsf^2 over its atoms, formed in f64 in the order of the atoms and rounded to f32 once, and `bfactor` of that."""
    groups: dict = {}
    for k, key in enumerate(zip(chain, (int(r) for r in resi), insertion)):
        groups.setdefault(key, []).append(k)
    as_bytes = lambda v: v.encode() if isinstance(v, str) else bytes(v)
    keys = sorted(groups, key=lambda g: (as_bytes(g[0]), g[1], as_bytes(g[2])))
    r = np.asarray(rmsf_values, np.float64)
    out = np.zeros(len(keys), np.float64)
    for row, g in enumerate(keys):
        total = 0.0
        for k in groups[g]:
            total += float(r[k]) * float(r[k])
        out[row] = np.sqrt(total / len(groups[g]))
    value = out.astype("<f4")
    return {"first": np.array([groups[g][0] for g in keys], "<u4"), "n_atoms": np.array([len(groups[g]) for g in keys], "<u4"), "rmsf": value, "bfactor": _bfactor(value)}


def _rmsf_reference(structure: Structure, reference, max_rounds):
    """(ref_ptr, ref_frame, max_rounds, keep-alive) of the `reference` argument: "mean" iterates from frame 0; a frame index or an [N, 3] array is one round
    on that reference."""
    if isinstance(reference, str):
        if reference != "mean":
            raise ValueError(f"reference must be 'mean', a frame index or an [N, 3] array, got {reference!r}")
        if not isinstance(max_rounds, (int, np.integer)) or int(max_rounds) < 0 or int(max_rounds) >= 1 << 32:
            raise ValueError(f"max_rounds must be a positive integer, got {max_rounds!r}")
        return None, 0, int(max_rounds), None
    if isinstance(reference, (int, np.integer)):
        if int(reference) < 0:
            raise ValueError(f"reference must be 'mean', a frame index or an [N, 3] array, got {reference!r}")
        return None, int(reference), 1, None
    n = _topology_atoms(structure)
    keep = np.ascontiguousarray(reference, dtype="<f8")
    if keep.shape != (n, 3):
        raise ArpeggiaError(_lib.ARP_ERR_BAD_INPUT, f"rmsf: reference must be 'mean', a frame index or have shape [{n}, 3] (the topology's atoms), got {list(keep.shape)}")
    return (keep if keep.size else np.zeros(1, "<f8")).ctypes.data_as(C.POINTER(C.c_double)), 0, 1, keep


def _rmsf(ctx: "Context | None", structure: Structure, frames, fit, atoms, chains: str, reference, max_rounds, tol, level: str, aligned: bool, transforms: bool):
    """arp_rmsf.  ctx None: the inputs are only checked (raises their error, else returns None)."""
    _check_level(level)
    args, keep = _rmsd_args(structure, frames, fit, chains, "rmsf")
    msel = None if atoms is None else rmsd_select(structure, atoms, chains)
    msel_keep = None if msel is None else (msel if len(msel) else np.zeros(1, "<u4"))
    msel_ptr = None if msel is None else msel_keep.ctypes.data_as(C.POINTER(C.c_uint32))
    ref_ptr, ref_frame, rounds, ref_keep = _rmsf_reference(structure, reference, max_rounds)
    head = (*args, msel_ptr, 0 if msel is None else len(msel), ref_ptr, ref_frame, rounds, C.c_double(tol))
    if ctx is None:
        _check(lib.arp_rmsf(None, *head, *([None] * 7)))
        return None
    F = _rmsd_frames(structure, frames)
    idx = rmsd_select(structure, fit, chains) if msel is None else msel
    m = len(idx)
    out = {"atom": idx.copy(), "mean": np.zeros((m, 3), "<f8"), "rmsf": np.zeros(m, "<f4"), "frame_rmsd": np.zeros(F, "<f4")}
    if transforms:
        out["transforms"] = np.zeros((F, 12), "<f8")
    if aligned:
        out["aligned"] = np.zeros((F, m, 3), "<f8")
    n_rounds, last = C.c_uint32(), C.c_double()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    ptr = lambda key, t: (out[key] if out[key].size else np.zeros(1, out[key].dtype)).ctypes.data_as(t) if key in out else None
    _check(lib.arp_rmsf(ctx._h, *head, ptr("mean", dp), ptr("rmsf", fp), ptr("frame_rmsd", fp), ptr("transforms", dp), ptr("aligned", dp), C.byref(n_rounds), C.byref(last)))
    out["bfactor"] = _bfactor(out["rmsf"])
    out["n_rounds"], out["last_change"] = int(n_rounds.value), float(last.value)
    out["converged"] = bool(out["last_change"] <= tol)
    if level == "residue":
        n = _topology_atoms(structure)
        chain, ins = structure.strings("chain")[:n][idx], structure.strings("insertion")[:n][idx]
        out["residue"] = rmsf_residues(chain, structure.ints("resi")[:n][idx], ins, out["rmsf"])
        out["residue"]["atom"] = idx[out["residue"].pop("first")]
    return out


def rmsf_host(xyz_sel, xyz_msel=None, reference=0, max_rounds: int = 1, tol: float = 0.0, aligned: bool = True, transforms: bool = True) -> dict:
    """arp_rmsf_host: the definition of arp_rmsf in plain sequential C++ on the CPU, on already-selected coordinates -- xyz_sel [F, n, 3] the fit atoms,
    xyz_msel [F, m, 3] the measured atoms (None: the fit atoms), reference a frame index or the reference's fit atoms [n, 3].  The yardstick of the device
    call.  Keys: mean, rmsf, frame_rmsd, n_rounds, last_change and, on request, aligned and transforms."""
    x = np.ascontiguousarray(xyz_sel, dtype="<f8")
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"xyz_sel must have shape [F, n, 3], got {list(x.shape)}")
    F, n = x.shape[:2]
    xm = None if xyz_msel is None else np.ascontiguousarray(xyz_msel, dtype="<f8")
    if xm is not None and (xm.ndim != 3 or xm.shape[0] != F or xm.shape[2] != 3):
        raise ValueError(f"xyz_msel must have shape [{F}, m, 3], got {list(xm.shape)}")
    m = n if xm is None else xm.shape[1]
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    arr = lambda a, t=dp: (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(t)
    ref, ref_frame = None, 0
    if isinstance(reference, (int, np.integer)):
        if int(reference) < 0:
            raise ValueError(f"reference must be a frame index or an [n, 3] array, got {reference!r}")
        ref_frame = int(reference)
    else:
        ref = np.ascontiguousarray(reference, dtype="<f8")
        if ref.shape != (n, 3):
            raise ValueError(f"reference must be a frame index or have shape [{n}, 3], got {list(ref.shape)}")
    out = {"mean": np.zeros((m, 3), "<f8"), "rmsf": np.zeros(m, "<f4"), "frame_rmsd": np.zeros(F, "<f4")}
    if transforms:
        out["transforms"] = np.zeros((F, 12), "<f8")
    if aligned:
        out["aligned"] = np.zeros((F, m, 3), "<f8")
    n_rounds, last = C.c_uint32(), C.c_double()
    _check(lib.arp_rmsf_host(F, n, m, arr(x), None if xm is None else arr(xm), None if ref is None else arr(ref), ref_frame, int(max_rounds), C.c_double(tol), arr(out["mean"]),
                             arr(out["rmsf"], fp), arr(out["frame_rmsd"], fp), arr(out["transforms"]) if transforms else None, arr(out["aligned"]) if aligned else None,
                             C.byref(n_rounds), C.byref(last)))
    out["n_rounds"], out["last_change"] = int(n_rounds.value), float(last.value)
    return out


def get_rmsf(structure: Structure, frames=None, fit="ca", atoms=None, chains: str = "", reference="mean", max_rounds: int = 50, tol: float = 1e-4, level: str = "atom",
             aligned: bool = False, transforms: bool = False, device: int = 0) -> dict:
    """How much each atom moves across the frames of an ensemble.  Every frame is superposed (proper rotations only) on the atoms of rmsd_select(structure, fit,
    chains) onto the reference -- "mean": the iterated mean structure, started from frame 0 and repeated until the mean moves by at most `tol` A (rms over the
    fit atoms) or `max_rounds` rounds are done; a frame index or an [N, 3] array: one fit to that fixed reference -- and the superposed frames are averaged.
    atoms: the measured atoms (as rmsd_select takes them; None: the fit atoms).  Returns a dict: `atom` <u4 [m] (topology indices), `mean` <f8 [m, 3] (in the
    reference's frame), `rmsf` <f4 [m], `bfactor` <f4 [m] (8 pi^2 / 3 rmsf^2), `frame_rmsd` <f4 [F] (each superposed frame against the mean, over the fit
    atoms), `n_rounds`, `last_change`, `converged` (last_change <= tol); with aligned / transforms also `aligned` <f8 [F, m, 3] and `transforms` <f8 [F, 12]
    (R row-major, then t: y = R x + t).  level="residue" adds `residue`: per residue of the measured atoms `atom` (its first), `n_atoms`, `rmsf` (the square
    root of the mean of rmsf^2 over its atoms) and `bfactor`.  frames: [F, N, 3] f64; None: the structure's models."""
    ctx = _with_context(device, lambda: _rmsf(None, structure, frames, fit, atoms, chains, reference, max_rounds, tol, level, aligned, transforms))
    return ctx.rmsf(structure, frames, fit, atoms, chains, reference, max_rounds, tol, level, aligned, transforms)


def rmsf(input_file: str, fit="ca", atoms=None, chains: str = "", reference="mean", max_rounds: int = 50, tol: float = 1e-4, level: str = "atom", aligned: bool = False,
         transforms: bool = False, ignore_zero_occupancy: bool = False) -> dict:
    """RMSF and the mean structure of the models of a multi-model file (the models are the frames): see get_rmsf."""
    return get_rmsf(Structure.load(input_file, ignore_zero_occupancy), None, fit, atoms, chains, reference, max_rounds, tol, level, aligned, transforms)


def rmsf_table(structure: Structure, result: dict, level: str = "atom"):
    """The result of an rmsf call as a table of the contact table's type: RMSF_COLUMNS per measured atom, RMSF_RESIDUE_COLUMNS per residue."""
    import pyarrow as pa

    _check_level(level)
    if level == "atom":
        cols = _identity(structure, result["atom"])
        for k, name in enumerate(("mean_x", "mean_y", "mean_z")):
            cols[name] = pa.array(result["mean"][:, k], pa.float64())
        cols["rmsf"], cols["bfactor"] = pa.array(result["rmsf"], pa.float32()), pa.array(result["bfactor"], pa.float32())
        return _frame({k: cols[k] for k in RMSF_COLUMNS})
    res = result["residue"]
    cols = _identity(structure, res["atom"])
    cols["n_atoms"] = pa.array(res["n_atoms"], pa.uint32())
    cols["rmsf"], cols["bfactor"] = pa.array(res["rmsf"], pa.float32()), pa.array(res["bfactor"], pa.float32())
    return _frame({k: cols[k] for k in RMSF_RESIDUE_COLUMNS})


# ---- Covariance, DCCM and principal components of the superposed coordinates (arp_covariance, arp_project) ----
_ID_COLUMNS = ["chain", "resn", "resi", "insertion", "altloc", "atomn", "atomi"]
DCCM_COLUMNS = [f"from_{k}" for k in _ID_COLUMNS] + [f"to_{k}" for k in _ID_COLUMNS] + ["correlation"]


def _covariance(ctx: "Context | None", structure: Structure, frames, fit, atoms, chains: str, reference, max_rounds, tol, cov: bool, dccm: bool, transforms: bool):
    """arp_covariance.  ctx None: the inputs are only checked (raises their error, else returns None)."""
    if not cov and not dccm:
        raise ValueError("covariance: at least one of cov and dccm must be asked for")
    args, keep = _rmsd_args(structure, frames, fit, chains, "covariance")
    msel = None if atoms is None else rmsd_select(structure, atoms, chains)
    msel_keep = None if msel is None else (msel if len(msel) else np.zeros(1, "<u4"))
    msel_ptr = None if msel is None else msel_keep.ctypes.data_as(C.POINTER(C.c_uint32))
    ref_ptr, ref_frame, rounds, ref_keep = _rmsf_reference(structure, reference, max_rounds)
    head = (*args, msel_ptr, 0 if msel is None else len(msel), ref_ptr, ref_frame, rounds, C.c_double(tol))
    if ctx is None:
        _check(lib.arp_covariance(None, *head, *([None] * 8)))
        return None
    F = _rmsd_frames(structure, frames)
    idx = rmsd_select(structure, fit, chains) if msel is None else msel
    m = len(idx)
    out = {"atom": idx.copy(), "mean": np.zeros((m, 3), "<f8"), "rmsf": np.zeros(m, "<f4"), "frame_rmsd": np.zeros(F, "<f4")}
    if cov:
        out["covariance"] = np.zeros((3 * m, 3 * m), "<f8")
    if dccm:
        out["dccm"] = np.zeros((m, m), "<f4")
    if transforms:
        out["transforms"] = np.zeros((F, 12), "<f8")
    n_rounds, last = C.c_uint32(), C.c_double()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    ptr = lambda key, t: (out[key] if out[key].size else np.zeros(1, out[key].dtype)).ctypes.data_as(t) if key in out else None
    _check(lib.arp_covariance(ctx._h, *head, ptr("covariance", dp), ptr("dccm", fp), ptr("mean", dp), ptr("rmsf", fp), ptr("frame_rmsd", fp), ptr("transforms", dp),
                              C.byref(n_rounds), C.byref(last)))
    out["bfactor"] = _bfactor(out["rmsf"])
    out["n_rounds"], out["last_change"] = int(n_rounds.value), float(last.value)
    out["converged"] = bool(out["last_change"] <= tol)
    return out


def _project_arrays(m: int, F, mean, modes, transforms):
    """(mean [m, 3], modes [k, 3m], transforms [F, 12] or None) as contiguous <f8, their shapes checked (F None: any number of frames)."""
    mean = np.ascontiguousarray(mean, dtype="<f8")
    if mean.shape != (m, 3):
        raise ValueError(f"mean must have shape [{m}, 3] (the measured atoms), got {list(mean.shape)}")
    modes = np.ascontiguousarray(modes, dtype="<f8")
    if modes.ndim != 2 or modes.shape[1] != 3 * m:
        raise ValueError(f"modes must have shape [k, {3 * m}] (atom-major rows over the measured atoms), got {list(modes.shape)}")
    if transforms is not None:
        transforms = np.ascontiguousarray(transforms, dtype="<f8")
        if transforms.ndim != 2 or transforms.shape[1] != 12 or (F is not None and transforms.shape[0] != F):
            raise ValueError(f"transforms must have shape [{'F' if F is None else F}, 12] (R row-major, then t), got {list(transforms.shape)}")
    return mean, modes, transforms


def _project(ctx: "Context | None", structure: Structure, frames, atoms, mean, modes, transforms):
    """arp_project.  ctx None: the inputs are only checked."""
    msel = rmsd_select(structure, atoms)
    F = _rmsd_frames(structure, frames)
    mean, modes, transforms = _project_arrays(len(msel), F, mean, modes, transforms)
    n_frames, fptr, keep = _frames_arg(structure, frames, "project")
    dp = C.POINTER(C.c_double)
    arr = lambda a, t=dp: None if a is None else (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(t)
    k = modes.shape[0]
    head = (structure._h, int(n_frames), fptr, arr(msel, C.POINTER(C.c_uint32)), len(msel), arr(transforms), arr(mean), arr(modes), k)
    if ctx is None:
        _check(lib.arp_project(None, *head, None))
        return None
    out = np.zeros((F, k), "<f8")
    _check(lib.arp_project(ctx._h, *head, arr(out)))
    return out


def pca_modes(covariance, n_modes: int = 10) -> dict:
    """The host half of pca(): numpy.linalg.eigh of a symmetric [3m, 3m] matrix.  `eigenvalues` <f8 [3m], descending, raw (rounding may leave a small negative
    one); `modes` <f8 [k, 3m], k = min(n_modes, 3m), unit rows, each with the sign that makes its largest-magnitude component positive (the lowest index
    on ties); `explained` [k] = eigenvalue / trace and `cumulative` [k] its running sum (zeros when the trace is 0)."""
    c = np.asarray(covariance, np.float64)
    if c.ndim != 2 or c.shape[0] != c.shape[1] or c.shape[0] == 0:
        raise ValueError(f"covariance must be a square matrix, got {list(c.shape)}")
    if not isinstance(n_modes, (int, np.integer)) or int(n_modes) < 1:
        raise ValueError(f"n_modes must be a positive integer, got {n_modes!r}")
    k = min(int(n_modes), c.shape[0])
    w, v = np.linalg.eigh(c)
    w, v = w[::-1].copy(), v[:, ::-1]
    modes = np.ascontiguousarray(v[:, :k].T, dtype="<f8")
    top = np.argmax(np.abs(modes), axis=1)  # (the first of equal magnitudes)
    modes[modes[np.arange(k), top] < 0.0] *= -1.0
    total = float(np.trace(c))
    explained = w[:k] / total if total > 0.0 else np.zeros(k)
    return {"eigenvalues": w.astype("<f8"), "modes": modes, "explained": explained, "cumulative": np.cumsum(explained)}


def _pca(ctx: "Context | None", structure: Structure, frames, fit, atoms, chains: str, reference, max_rounds, tol, n_modes):
    if not isinstance(n_modes, (int, np.integer)) or int(n_modes) < 1:
        raise ValueError(f"n_modes must be a positive integer, got {n_modes!r}")
    out = _covariance(ctx, structure, frames, fit, atoms, chains, reference, max_rounds, tol, True, False, True)
    if ctx is None:
        return None
    out.update(pca_modes(out["covariance"], n_modes))
    out["projections"] = _project(ctx, structure, frames, out["atom"], out["mean"], out["modes"], out["transforms"])
    return out


def covariance_host(aligned, mean, cov: bool = True, dccm: bool = False) -> dict:
    """arp_covariance_host: the definition of arp_covariance's `covariance` and `dccm` in plain sequential C++ on the CPU, from superposed coordinates
    aligned [F, m, 3] and their mean [m, 3] (rmsf's `aligned` and `mean`).  The yardstick of the device call."""
    a = np.ascontiguousarray(aligned, dtype="<f8")
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"aligned must have shape [F, m, 3], got {list(a.shape)}")
    F, m = a.shape[:2]
    mu = np.ascontiguousarray(mean, dtype="<f8")
    if mu.shape != (m, 3):
        raise ValueError(f"mean must have shape [{m}, 3], got {list(mu.shape)}")
    out = {}
    if cov:
        out["covariance"] = np.zeros((3 * m, 3 * m), "<f8")
    if dccm:
        out["dccm"] = np.zeros((m, m), "<f4")
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    arr = lambda x, t=dp: (x if x.size else np.zeros(1, x.dtype)).ctypes.data_as(t)
    _check(lib.arp_covariance_host(F, m, arr(a), arr(mu), arr(out["covariance"]) if cov else None, arr(out["dccm"], fp) if dccm else None))
    return out


def project_host(xyz_msel, mean, modes, transforms=None) -> np.ndarray:
    """arp_project_host: the definition of arp_project in plain sequential C++ on the CPU, on the measured atoms' absolute coordinates xyz_msel [F, m, 3]."""
    x = np.ascontiguousarray(xyz_msel, dtype="<f8")
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"xyz_msel must have shape [F, m, 3], got {list(x.shape)}")
    F, m = x.shape[:2]
    mean, modes, transforms = _project_arrays(m, F, mean, modes, transforms)
    k = modes.shape[0]
    out = np.zeros((F, k), "<f8")
    dp = C.POINTER(C.c_double)
    arr = lambda a: None if a is None else (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(dp)
    _check(lib.arp_project_host(F, m, arr(x), arr(transforms), arr(mean), arr(modes), k, arr(out)))
    return out


def get_covariance(structure: Structure, frames=None, fit="ca", atoms=None, chains: str = "", reference="mean", max_rounds: int = 50, tol: float = 1e-4, cov: bool = True,
                   dccm: bool = False, transforms: bool = False, device: int = 0) -> dict:
    """Which coordinates of an ensemble move together.  The frames are superposed exactly as get_rmsf superposes them (same arguments, same bytes) and, under
    the last rotations, d = the measured atoms' superposed coordinates minus their mean.  Returns get_rmsf's keys (`atom`, `mean`, `rmsf`, `bfactor`,
    `frame_rmsd`, `n_rounds`, `last_change`, `converged`, on request `transforms`) plus `covariance` <f8 [3m, 3m] (cov=True): (1 / F) sum_f d_a d_b with
    the coordinate index a = 3 i + k, exactly symmetric, the trace of atom i's block = rmsf_i^2; and / or `dccm` <f4 [m, m] (dccm=True): see get_dccm."""
    ctx = _with_context(device, lambda: _covariance(None, structure, frames, fit, atoms, chains, reference, max_rounds, tol, cov, dccm, transforms))
    return ctx.covariance(structure, frames, fit, atoms, chains, reference, max_rounds, tol, cov, dccm, transforms)


def get_dccm(structure: Structure, frames=None, fit="ca", atoms=None, chains: str = "", reference="mean", max_rounds: int = 50, tol: float = 1e-4, transforms: bool = False,
             device: int = 0) -> dict:
    """Which atoms of an ensemble move together: the dynamic cross-correlation map `dccm` <f4 [m, m], <d_i . d_j> / sqrt(<d_i^2> <d_j^2>) of the measured
    atoms' deviations from their mean after get_rmsf's superposition: +1 the same direction, -1 opposite, 0 unrelated (or an atom that does not move); the
    diagonal is exactly 1, the matrix exactly symmetric.  Residue-level maps: measure atoms="ca".  The other keys are get_rmsf's."""
    ctx = _with_context(device, lambda: _covariance(None, structure, frames, fit, atoms, chains, reference, max_rounds, tol, False, True, transforms))
    return ctx.dccm(structure, frames, fit, atoms, chains, reference, max_rounds, tol, transforms)


def get_projection(structure: Structure, frames, atoms, mean, modes, transforms=None, device: int = 0) -> np.ndarray:
    """Frames along given collective directions: <f8 [F, k], sum_a d_a modes[j, a] with d = R p + t - mean of the measured atoms (rmsd_select(structure,
    atoms)).  transforms [F, 12] as get_rmsf(transforms=True) returns them; None: the frames are already superposed.  New frames, fitted to an old mean
    structure with get_rmsf(reference=...), project onto old modes: no fit is repeated here."""
    ctx = _with_context(device, lambda: _project(None, structure, frames, atoms, mean, modes, transforms))
    return ctx.project(structure, frames, atoms, mean, modes, transforms)


def get_pca(structure: Structure, frames=None, fit="ca", atoms=None, chains: str = "", reference="mean", max_rounds: int = 50, tol: float = 1e-4, n_modes: int = 10,
            device: int = 0) -> dict:
    """Along which few collective directions an ensemble moves (principal components, "essential dynamics").  The covariance is formed on the device
    (get_covariance), its eigen-decomposition is numpy.linalg.eigh on the HOST -- O((3m)^3) on the CPU; its measured share of the call: 12 % at 76 atoms
    x 10^4 frames, 81 - 88 % at 602 atoms x 10^4, 93 % at 1055 atoms x 10^3 --, and the frames are projected on the device (get_projection).  Keys: get_covariance's (with `covariance` and
    `transforms`), `eigenvalues` <f8 [3m] descending, raw; `modes` <f8 [k, 3m], k = min(n_modes, 3m), unit rows, the sign fixed so that each mode's
    largest-magnitude component is positive (lowest index on ties); `explained` and `cumulative` [k] (shares of the trace); `projections` <f8 [F, k]."""
    ctx = _with_context(device, lambda: _pca(None, structure, frames, fit, atoms, chains, reference, max_rounds, tol, n_modes))
    return ctx.pca(structure, frames, fit, atoms, chains, reference, max_rounds, tol, n_modes)


def covariance(input_file: str, fit="ca", atoms=None, chains: str = "", reference="mean", max_rounds: int = 50, tol: float = 1e-4, cov: bool = True, dccm: bool = False,
               transforms: bool = False, ignore_zero_occupancy: bool = False) -> dict:
    """Covariance of the models of a multi-model file (the models are the frames): see get_covariance."""
    return get_covariance(Structure.load(input_file, ignore_zero_occupancy), None, fit, atoms, chains, reference, max_rounds, tol, cov, dccm, transforms)


def dccm(input_file: str, fit="ca", atoms=None, chains: str = "", reference="mean", max_rounds: int = 50, tol: float = 1e-4, transforms: bool = False,
         ignore_zero_occupancy: bool = False) -> dict:
    """DCCM of the models of a multi-model file: see get_dccm."""
    return get_dccm(Structure.load(input_file, ignore_zero_occupancy), None, fit, atoms, chains, reference, max_rounds, tol, transforms)


def pca(input_file: str, fit="ca", atoms=None, chains: str = "", reference="mean", max_rounds: int = 50, tol: float = 1e-4, n_modes: int = 10,
        ignore_zero_occupancy: bool = False) -> dict:
    """Principal components of the models of a multi-model file: see get_pca."""
    return get_pca(Structure.load(input_file, ignore_zero_occupancy), None, fit, atoms, chains, reference, max_rounds, tol, n_modes)


def dccm_table(structure: Structure, result: dict):
    """The `dccm` of a result in long form, as a table of the contact table's type: one row per pair i < j of measured atoms, DCCM_COLUMNS -- the identity
    columns of both atoms, then `correlation`."""
    import pyarrow as pa

    idx = np.asarray(result["atom"])
    i, j = np.triu_indices(len(idx), 1)
    cols = {f"from_{k}": v for k, v in _identity(structure, idx[i]).items()}
    cols.update({f"to_{k}": v for k, v in _identity(structure, idx[j]).items()})
    cols["correlation"] = pa.array(np.asarray(result["dccm"])[i, j], pa.float32())
    return _frame({k: cols[k] for k in DCCM_COLUMNS})


# ---- Secondary structure (DSSP, Kabsch & Sander 1983) per frame and across the frames of an ensemble (arp_dssp) ----
SS_CODES = "-HBEGITS"   # code k of every output is SS_CODES[k]: loop, alpha helix, isolated bridge, strand, 3-10 helix, pi helix, turn, bend
DSSP_CHAIN_START, DSSP_NO_H = 1, 2
SS_COLUMNS = ["chain", "resn", "resi", "insertion"] + [f"frac_{c}" for c in ("loop", "H", "B", "E", "G", "I", "T", "S")] + ["consensus"]


def backbone_select(structure: Structure, chains: str = "") -> dict:
    """The residues arp_dssp works on: the residues of model 0 in file order (a residue: a maximal run of atoms with the same chain, resi and insertion code),
    HOH left out, restricted to the comma list `chains` ("" = every chain), and only those with all of N, CA, C, O -- the first atom of each name, so an
    altloc after the first is ignored; a residue without one of the four is dropped (the gap it leaves is a chain break by geometry).  Returns `atom` <u4 [R]
    (each residue's first atom), `bb` <u4 [R, 4] (the topology indices of N, CA, C, O) and `flags` u1 [R] (bit 0 DSSP_CHAIN_START: the first residue, or another
    chain than the residue before; bit 1 DSSP_NO_H: residue name PRO)."""
    n = _topology_atoms(structure)
    name, resn, chain, ins = (structure.strings(k)[:n] for k in ("atomn", "resn", "chain", "insertion"))
    resi = structure.ints("resi")[:n]
    if n == 0:
        return {"atom": np.zeros(0, "<u4"), "bb": np.zeros((0, 4), "<u4"), "flags": np.zeros(0, "u1")}
    new = np.ones(n, bool)
    new[1:] = (chain[1:] != chain[:-1]) | (resi[1:] != resi[:-1]) | (ins[1:] != ins[:-1])
    run = np.cumsum(new) - 1
    first = np.flatnonzero(new)
    keep = resn[first] != b"HOH"
    wanted = [c.strip().encode() for c in chains.split(",") if c.strip()]
    if wanted:
        keep &= np.isin(chain[first], wanted)
    bb = np.zeros((len(first), 4), np.int64)
    for k, atom_name in enumerate((b"N", b"CA", b"C", b"O")):
        idx = np.flatnonzero(name == atom_name)
        runs, at = np.unique(run[idx], return_index=True)   # the first atom of that name in every run that has one
        has = np.zeros(len(first), bool)
        has[runs] = True
        bb[runs, k] = idx[at]
        keep &= has
    rows = np.flatnonzero(keep)
    atom, ch = first[rows], chain[first[rows]]
    flags = np.where(resn[atom] == b"PRO", DSSP_NO_H, 0).astype("u1")
    if len(rows):
        flags[0] |= DSSP_CHAIN_START
        flags[1:][ch[1:] != ch[:-1]] |= DSSP_CHAIN_START
    return {"atom": atom.astype("<u4"), "bb": np.ascontiguousarray(bb[rows], "<u4"), "flags": flags}


def _secondary_structure(ctx: "Context | None", structure: Structure, frames, chains: str, codes: bool, hbonds: bool):
    """arp_dssp.  ctx None: the inputs are only checked (raises their error, else returns None)."""
    sel = backbone_select(structure, chains)
    R = len(sel["atom"])
    n_frames, ptr, keep = _frames_arg(structure, frames, "dssp")
    u8p, u32p, fp = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    arr = lambda a, t: (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(t)
    head = (structure._h, int(n_frames), ptr, arr(sel["bb"], u32p), arr(sel["flags"], u8p), R)
    if ctx is None:
        _check(lib.arp_dssp(None, *head, *([None] * 5)))
        return None
    F = _rmsd_frames(structure, frames)
    out = {"residue": sel["atom"], "counts": np.zeros((R, 8), "<u4"), "frame_counts": np.zeros((F, 8), "<u4")}
    if codes:
        out["codes"] = np.zeros((F, R), "u1")
    if hbonds:
        out["hb_acceptor"], out["hb_energy"] = np.zeros((F, R, 2), "<u4"), np.zeros((F, R, 2), "<f4")
    ptr_of = lambda key, t: arr(out[key], t) if key in out else None
    _check(lib.arp_dssp(ctx._h, *head, ptr_of("codes", u8p), ptr_of("counts", u32p), ptr_of("frame_counts", u32p), ptr_of("hb_acceptor", u32p), ptr_of("hb_energy", fp)))
    out["fraction"] = (out["counts"].astype(np.float64) / F).astype("<f4")
    return out


def secondary_structure_host(bb_xyz, flags, codes: bool = True, hbonds: bool = True) -> dict:
    """arp_dssp_host: the definition of arp_dssp in plain sequential C++ on the CPU, on already-gathered coordinates bb_xyz [F, R, 4, 3] (N, CA, C, O of every
    residue) and flags [R].  The yardstick of the device call.  Keys: counts, frame_counts and, on request, codes, hb_acceptor and hb_energy."""
    x = np.ascontiguousarray(bb_xyz, dtype="<f8")
    if x.ndim != 4 or x.shape[2:] != (4, 3):
        raise ValueError(f"bb_xyz must have shape [F, R, 4, 3], got {list(x.shape)}")
    F, R = x.shape[:2]
    fl = np.ascontiguousarray(flags, dtype="u1")
    if fl.shape != (R,):
        raise ValueError(f"flags must have shape [{R}], got {list(fl.shape)}")
    u8p, u32p, fp, dp = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    arr = lambda a, t: (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(t)
    out = {"counts": np.zeros((R, 8), "<u4"), "frame_counts": np.zeros((F, 8), "<u4")}
    if codes:
        out["codes"] = np.zeros((F, R), "u1")
    if hbonds:
        out["hb_acceptor"], out["hb_energy"] = np.zeros((F, R, 2), "<u4"), np.zeros((F, R, 2), "<f4")
    ptr_of = lambda key, t: arr(out[key], t) if key in out else None
    _check(lib.arp_dssp_host(F, R, arr(x, dp), arr(fl, u8p), ptr_of("codes", u8p), arr(out["counts"], u32p), arr(out["frame_counts"], u32p), ptr_of("hb_acceptor", u32p),
                             ptr_of("hb_energy", fp)))
    return out


def ss_string(codes_row) -> str:
    """One row of `codes` as a string over SS_CODES ("-HBEGITS")."""
    return "".join(SS_CODES[int(c)] for c in np.asarray(codes_row).ravel())


def get_secondary_structure(structure: Structure, frames=None, chains: str = "", codes: bool = True, hbonds: bool = False, device: int = 0) -> dict:
    """Where the helices and strands are, and in what share of the frames: DSSP (Kabsch & Sander 1983) on the residues of backbone_select(structure, chains),
    for every frame of an ensemble.  Returns a dict: `residue` <u4 [R] (the first atom of every residue), `counts` <u4 [R, 8] (in how many frames the residue
    has each code of SS_CODES), `fraction` <f4 [R, 8] = counts / F, `frame_counts` <u4 [F, 8]; codes=True: `codes` u1 [F, R]; hbonds=True: `hb_acceptor` <u4
    [F, R, 2] (row indices of each donor's two best acceptors, 0xFFFFFFFF: none) and `hb_energy` <f4 [F, R, 2] (kcal/mol).  Departures from mkdssp: energies are
    not rounded to three decimals, ladders are not linked across beta bulges, and G is assigned before I.  frames: [F, N, 3] f64; None: the structure's models."""
    ctx = _with_context(device, lambda: _secondary_structure(None, structure, frames, chains, codes, hbonds))
    return ctx.secondary_structure(structure, frames, chains, codes, hbonds)


def secondary_structure(input_file: str, chains: str = "", codes: bool = True, hbonds: bool = False, ignore_zero_occupancy: bool = False) -> dict:
    """Secondary structure of the models of a file (the models are the frames; one model: one frame): see get_secondary_structure."""
    return get_secondary_structure(Structure.load(input_file, ignore_zero_occupancy), None, chains, codes, hbonds)


def ss_consensus(counts) -> np.ndarray:
    """u1 [R]: the most frequent code of every residue, the lower code on ties."""
    return np.argmax(np.asarray(counts), axis=1).astype("u1")


def secondary_structure_table(structure: Structure, result: dict):
    """The result of a secondary-structure call as a table of the contact table's type, one row per residue: SS_COLUMNS -- chain, resn, resi, insertion, the
    eight fractions and `consensus`, the most frequent code as a character (the lower code on ties)."""
    import pyarrow as pa

    ident = _identity(structure, np.asarray(result["residue"]))
    cols = {k: ident[k] for k in ("chain", "resn", "resi", "insertion")}
    for k, name in enumerate(SS_COLUMNS[4:12]):
        cols[name] = pa.array(np.asarray(result["fraction"])[:, k], pa.float32())
    cols["consensus"] = pa.array([SS_CODES[int(c)] for c in ss_consensus(result["counts"])], pa.string())
    return _frame({k: cols[k] for k in SS_COLUMNS})


# ---- Torsion angles, rotamer states and Ramachandran maps across the frames of an ensemble (arp_torsions) ----
TORSION_KINDS = ["phi", "psi", "omega", "chi1", "chi2", "chi3", "chi4", "chi5"]   # `kind` of every torsion indexes this
TORSION_STATES = "-+t-"   # state k of every output: 0 undefined, 1 g+, 2 t, 3 g-
RAMA_CLASSES = ["general", "GLY", "PRO", "pre-PRO"]   # `rama_class` of every (phi, psi) pair, tested GLY, PRO, pre-PRO, general
TORSION_COLUMNS = ["chain", "resn", "resi", "insertion", "torsion", "n_defined", "mean", "resultant", "circ_std", "frac_gplus", "frac_trans", "frac_gminus", "n_transitions"]
LINK_MAX = 2.5   # A: |C[r-1] - N[r]| of model 0 above it, and r-1 and r are not linked (the chain break of arp_dssp)


def _chi_atoms() -> dict:
    """resn -> [(p0, p1, p2, p3)] of chi1 .. (IUPAC; the first of two equivalent branches: CG1, OD1, ND1, CD1, OE1, NH1)."""
    chi = {}
    fourth = {1: {"CG": "ARG ASN ASP GLN GLU HIS LEU LYS MET PHE PRO TRP TYR", "CG1": "ILE VAL", "OG": "SER", "OG1": "THR", "SG": "CYS"},
              2: {"CD": "ARG GLN GLU LYS PRO", "OD1": "ASN ASP", "ND1": "HIS", "CD1": "LEU PHE TRP TYR", "SD": "MET"},
              3: {"NE": "ARG", "OE1": "GLN GLU", "CE": "LYS"}}
    head = {1: ("N", "CA", "CB"), 2: ("CA", "CB", "CG"), 3: ("CB", "CG", "CD")}
    for n in (1, 2, 3):
        for atom, names in fourth[n].items():
            for resn in names.split():
                chi.setdefault(resn, []).append(head[n] + (atom,))
    chi["ILE"].append(("CA", "CB", "CG1", "CD1"))
    chi["MET"].append(("CB", "CG", "SD", "CE"))
    chi["ARG"] += [("CG", "CD", "NE", "CZ"), ("CD", "NE", "CZ", "NH1")]
    chi["LYS"].append(("CG", "CD", "CE", "NZ"))
    return chi


CHI_ATOMS = _chi_atoms()


def _torsion_kinds(kinds) -> set:
    """The indices into TORSION_KINDS a `kinds` argument names: a comma list or a sequence of phi, psi, omega, chi (all five) and chi1 .. chi5."""
    names = [k.strip() for k in kinds.split(",")] if isinstance(kinds, str) else list(kinds)
    want = set()
    for k in names:
        if k == "chi":
            want |= {3, 4, 5, 6, 7}
        elif k in TORSION_KINDS:
            want.add(TORSION_KINDS.index(k))
        elif k:
            raise ValueError(f"Invalid torsion kind '{k}'. Must be one of: {', '.join(TORSION_KINDS[:3] + ['chi'] + TORSION_KINDS[3:])}")
    return want


def torsion_select(structure: Structure, chains: str = "", kinds=("phi", "psi", "omega", "chi")) -> dict:
    """The torsions arp_torsions works on.  Residues are those of model 0 as in backbone_select -- file order, HOH out, `chains`, the first atom of each name --
    but a residue is NOT dropped for a missing atom: only the torsions that lack an atom are.  Rows r-1 and r are linked iff they have the same chain, follow each
    other in the selection and |C[r-1] - N[r]| <= 2.5 A in model 0.  phi(r) = C[r-1]-N-CA-C where r-1 is linked; psi(r) = N-CA-C-N[r+1] and omega(r) =
    CA-C-N[r+1]-CA[r+1] where r+1 is linked; chi1 .. chi5 by CHI_ATOMS.  Order: residues in selection order, within one phi, psi, omega, chi1 ..
    Returns `quads` <u4 [D, 4] (topology atom indices), `kind` u1 [D] (index into TORSION_KINDS), `residue` <u4 [D] (the first atom of the owning residue), `row`
    <u4 [D] (the residue's index in the selection), `n_rows`, `pairs` <u4 [P, 3] (phi, psi of one residue, and its rama_class as the group) and `rama_class` u1 [P]
    (1 GLY, 2 PRO, 3 the residue before a PRO, 0 general -- tested in this order)."""
    want = _torsion_kinds(kinds)
    n = _topology_atoms(structure)
    empty = {"quads": np.zeros((0, 4), "<u4"), "kind": np.zeros(0, "u1"), "residue": np.zeros(0, "<u4"), "row": np.zeros(0, "<u4"), "n_rows": 0,
             "pairs": np.zeros((0, 3), "<u4"), "rama_class": np.zeros(0, "u1")}
    if n == 0:
        return empty
    name, resn, chain, ins = (structure.strings(k)[:n] for k in ("atomn", "resn", "chain", "insertion"))
    resi = structure.ints("resi")[:n]
    new = np.ones(n, bool)
    new[1:] = (chain[1:] != chain[:-1]) | (resi[1:] != resi[:-1]) | (ins[1:] != ins[:-1])
    run = np.cumsum(new) - 1
    first = np.flatnonzero(new)
    keep = resn[first] != b"HOH"
    wanted = [c.strip().encode() for c in chains.split(",") if c.strip()]
    if wanted:
        keep &= np.isin(chain[first], wanted)
    rows = np.flatnonzero(keep)
    R = len(rows)
    if R == 0:
        return empty
    atom_names = sorted({"N", "CA", "C"} | {a for quads in CHI_ATOMS.values() for q in quads for a in q})
    at = {}   # atom name -> [R] topology index of the first atom of that name in every selected residue, -1: none
    for a in atom_names:
        idx = np.flatnonzero(name == a.encode())
        runs, pos = np.unique(run[idx], return_index=True)
        col = np.full(len(first), -1, np.int64)
        col[runs] = idx[pos]
        at[a] = col[rows]
    soa = structure.soa()
    xyz = np.stack([np.asarray(soa[k][:n], np.float64) for k in ("x", "y", "z")], 1)
    names_r = [b.decode() for b in resn[first[rows]]]
    ch = chain[first[rows]]
    link = np.zeros(R + 1, bool)   # link[r]: rows r - 1 and r are linked (link[0] and link[R]: no neighbour)
    ok = (ch[1:] == ch[:-1]) & (at["C"][:-1] >= 0) & (at["N"][1:] >= 0)
    dist = np.sqrt(((xyz[at["C"][:-1]] - xyz[at["N"][1:]]) ** 2).sum(1))
    link[1:R] = ok & (dist <= LINK_MAX)
    link = link.tolist()
    at = {a: col.tolist() for a, col in at.items()}   # (plain lists: the loop below indexes them a few times per residue)
    quads, kind, row, pairs, rama = [], [], [], [], []
    for r in range(R):
        here = {}
        cand = []
        if link[r]:
            cand.append((0, (at["C"][r - 1], at["N"][r], at["CA"][r], at["C"][r])))
        if link[r + 1]:
            cand.append((1, (at["N"][r], at["CA"][r], at["C"][r], at["N"][r + 1])))
            cand.append((2, (at["CA"][r], at["C"][r], at["N"][r + 1], at["CA"][r + 1])))
        for k, q in enumerate(CHI_ATOMS.get(names_r[r], ())):
            cand.append((3 + k, tuple(at[a][r] for a in q)))
        for k, q in cand:
            if k in want and min(q) >= 0:
                here[k] = len(quads)
                quads.append(q); kind.append(k); row.append(r)
        if 0 in here and 1 in here:
            cls = 1 if names_r[r] == "GLY" else 2 if names_r[r] == "PRO" else 3 if names_r[r + 1] == "PRO" else 0   # (psi exists: r + 1 is linked)
            pairs.append((here[0], here[1], cls)); rama.append(cls)
    row = np.asarray(row, "<u4")
    return {"quads": np.asarray(quads, "<u4").reshape(-1, 4), "kind": np.asarray(kind, "u1"), "residue": first[rows][row].astype("<u4"), "row": row, "n_rows": R,
            "pairs": np.asarray(pairs, "<u4").reshape(-1, 3), "rama_class": np.asarray(rama, "u1")}


def _torsion_outputs(F: int, D: int, bins: int, G: int, angles: bool, cossin: bool, states: bool) -> dict:
    out = {"sums": np.zeros((D, 2), "<f8"), "n_defined": np.zeros(D, "<u4"), "state_counts": np.zeros((D, 4), "<u4"), "n_transitions": np.zeros(D, "<u4")}
    if angles:
        out["angles"] = np.zeros((F, D), "<f4")
    if cossin:
        out["cossin"] = np.zeros((F, D, 2), "<f8")
    if states:
        out["states"] = np.zeros((F, D), "u1")
    if bins:
        out["hist"] = np.zeros((D, bins), "<u4")
        if G:
            out["hist2"] = np.zeros((G, bins, bins), "<u4")
    return out


def _torsion_pointers(out: dict) -> tuple:
    u8p, u32p, fp, dp = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_double)
    arr = lambda a, t: (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(t)
    ptr_of = lambda key, t: arr(out[key], t) if key in out else None
    return (ptr_of("angles", fp), ptr_of("cossin", dp), ptr_of("states", u8p), arr(out["sums"], dp), arr(out["n_defined"], u32p), arr(out["state_counts"], u32p),
            arr(out["n_transitions"], u32p), ptr_of("hist", u32p), ptr_of("hist2", u32p))


def _torsion_statistics(out: dict) -> dict:
    """The circular statistics of a result, on the host in f64: mean = degrees(atan2(sum s, sum c)), resultant = hypot(sum c, sum s) / n_defined, circ_std =
    degrees(sqrt(-2 ln resultant)) (a resultant that rounding lifts above 1 counts as 1), NaN where the torsion is never defined; state_fraction f4 [D, 3]."""
    nd = out["n_defined"].astype(np.float64)
    sc, ss = out["sums"][:, 0], out["sums"][:, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        out["mean"] = np.where(nd > 0, np.degrees(np.arctan2(ss, sc)), np.nan)
        out["resultant"] = np.where(nd > 0, np.hypot(sc, ss) / nd, np.nan)
        out["circ_std"] = np.degrees(np.sqrt(np.abs(2.0 * np.log(np.minimum(out["resultant"], 1.0)))))
        out["state_fraction"] = (out["state_counts"][:, 1:].astype(np.float64) / nd[:, None]).astype("<f4")
    return out


def _torsions(ctx: "Context | None", structure: Structure, frames, chains: str, kinds, bins: int, rama, angles: bool, cossin: bool, states: bool):
    """arp_torsions.  ctx None: the inputs are only checked (raises their error, else returns None)."""
    if rama not in ("class", "residue", None):
        raise ValueError(f"Invalid rama '{rama}'. Must be one of: 'class', 'residue', None")
    sel = torsion_select(structure, chains, kinds)
    D, P = len(sel["quads"]), len(sel["pairs"])
    n_frames, ptr, keep = _frames_arg(structure, frames, "torsions")
    pairs = sel["pairs"].copy()
    if rama == "residue":
        pairs[:, 2] = sel["row"][pairs[:, 0]]
    G = 0 if rama is None or P == 0 or int(bins) <= 0 else len(RAMA_CLASSES) if rama == "class" else int(sel["n_rows"])
    u32p = C.POINTER(C.c_uint32)
    arr = lambda a, t: (a if a.size else np.zeros(4, a.dtype)).ctypes.data_as(t)
    head = (structure._h, int(n_frames), ptr, arr(sel["quads"], u32p), D, max(int(bins), 0), arr(pairs, u32p), P if G else 0, G)
    if ctx is None:
        _check(lib.arp_torsions(None, *head, *([None] * 9)))
        return None
    F = _rmsd_frames(structure, frames)
    out = _torsion_outputs(F, D, max(int(bins), 0), G, angles, cossin, states)
    _check(lib.arp_torsions(ctx._h, *head, *_torsion_pointers(out)))
    out.update({k: v for k, v in sel.items() if k != "pairs"})
    out["pairs"], out["n_groups"] = pairs, G
    return _torsion_statistics(out)


def torsions_host(quad_xyz, pairs=None, n_groups: int = 0, bins: int = 36, angles: bool = True, cossin: bool = True, states: bool = True) -> dict:
    """arp_torsions_host: the definition of arp_torsions in plain sequential C++ on the CPU, on already-gathered coordinates quad_xyz [F, D, 4, 3].  pairs [P, 3]
    with n_groups > 0 ask for `hist2`.  The yardstick of the device call.  Keys: sums, n_defined, state_counts, n_transitions, the statistics derived from them
    and, on request, angles, cossin, states, hist (bins > 0), hist2."""
    x = np.ascontiguousarray(quad_xyz, dtype="<f8")
    if x.ndim != 4 or x.shape[2:] != (4, 3):
        raise ValueError(f"quad_xyz must have shape [F, D, 4, 3], got {list(x.shape)}")
    F, D = x.shape[:2]
    pr = np.zeros((0, 3), "<u4") if pairs is None else np.ascontiguousarray(pairs, dtype="<u4").reshape(-1, 3)
    G = int(n_groups) if len(pr) else 0
    out = _torsion_outputs(F, D, max(int(bins), 0), G, angles, cossin, states)
    arr = lambda a, t: (a if a.size else np.zeros(4, a.dtype)).ctypes.data_as(t)
    _check(lib.arp_torsions_host(F, D, arr(x, C.POINTER(C.c_double)), max(int(bins), 0), arr(pr, C.POINTER(C.c_uint32)), len(pr) if G else 0, G, *_torsion_pointers(out)))
    return _torsion_statistics(out)


def get_torsions(structure: Structure, frames=None, chains: str = "", kinds=("phi", "psi", "omega", "chi"), bins: int = 36, rama="class", angles: bool = True,
                 cossin: bool = False, states: bool = False, device: int = 0) -> dict:
    """What phi, psi, omega and the side-chain chi angles are in every frame, which well each sits in, how often it jumps, and the Ramachandran map of the
    ensemble.  The torsions are those of torsion_select(structure, chains, kinds).  Returns the selection's arrays and, per torsion: `n_defined`, `state_counts`
    [D, 4] (undefined, g+, t, g-), `state_fraction` f4 [D, 3], `n_transitions`, `sums` [D, 2] (sum cos, sum sin), `mean` (degrees), `resultant`, `circ_std`
    (degrees); with bins > 0 `hist` [D, bins]; with rama="class" `hist2` [4, bins, bins] (RAMA_CLASSES; rows phi, columns psi, bin k = [-180 + k w, -180 + (k + 1)
    w)), with rama="residue" `hist2` [n_rows, bins, bins], one map per residue of the selection; angles=True: `angles` f4 [F, D] in degrees, NaN where undefined;
    cossin=True: `cossin` f8 [F, D, 2] (what a dihedral PCA takes); states=True: `states` u1 [F, D].  frames: [F, N, 3] f64; None: the structure's models."""
    ctx = _with_context(device, lambda: _torsions(None, structure, frames, chains, kinds, bins, rama, angles, cossin, states))
    return ctx.torsions(structure, frames, chains, kinds, bins, rama, angles, cossin, states)


def torsions(input_file: str, chains: str = "", kinds=("phi", "psi", "omega", "chi"), bins: int = 36, rama="class", angles: bool = True, cossin: bool = False,
             states: bool = False, ignore_zero_occupancy: bool = False) -> dict:
    """Torsions of the models of a file (the models are the frames; one model: one frame): see get_torsions."""
    return get_torsions(Structure.load(input_file, ignore_zero_occupancy), None, chains, kinds, bins, rama, angles, cossin, states)


def torsion_table(structure: Structure, result: dict):
    """The result of a torsion call as a table of the contact table's type, one row per torsion: TORSION_COLUMNS -- chain, resn, resi, insertion, `torsion` (a
    name of TORSION_KINDS), n_defined, mean, resultant, circ_std, the three state fractions and n_transitions."""
    import pyarrow as pa

    ident = _identity(structure, np.asarray(result["residue"]))
    cols = {k: ident[k] for k in ("chain", "resn", "resi", "insertion")}
    cols["torsion"] = pa.array([TORSION_KINDS[int(k)] for k in result["kind"]], pa.string())
    cols["n_defined"] = pa.array(np.asarray(result["n_defined"], "<u4"), pa.uint32())
    for k in ("mean", "resultant", "circ_std"):
        cols[k] = pa.array(np.asarray(result[k], np.float64), pa.float64())
    for k, name in enumerate(("frac_gplus", "frac_trans", "frac_gminus")):
        cols[name] = pa.array(np.asarray(result["state_fraction"])[:, k], pa.float32())
    cols["n_transitions"] = pa.array(np.asarray(result["n_transitions"], "<u4"), pa.uint32())
    return _frame({k: cols[k] for k in TORSION_COLUMNS})


def _contact_clusters_arrow(input_file: str, groups: str, vdw_comp: float, dist_cutoff: float, ignore_zero_occupancy: bool, rings: bool, level: str, min_similarity: float,
                            max_clusters, counts: bool):
    """The command line's form of contact_clusters: (Arrow table of the frequency columns, the dict of _cluster_arrays)."""
    structure = Structure.load(input_file, ignore_zero_occupancy)
    ctx = _with_context(0, lambda: _cluster_table(None, structure, None, groups, vdw_comp, dist_cutoff, rings, level, min_similarity, max_clusters, counts))
    owner = _TableOwner(_cluster_table(ctx, structure, None, groups, vdw_comp, dist_cutoff, rings, level, min_similarity, max_clusters, counts))
    return _arrow_of(owner.t), _cluster_arrays(owner)


def _contact_autocorrelation_arrow(input_file: str, groups: str, vdw_comp: float, dist_cutoff: float, ignore_zero_occupancy: bool, rings: bool, level: str, mode: str,
                                   max_lag, matrix: bool):
    """The command line's form of contact_autocorrelation: (Arrow table of the frequency columns + half_life, the dict of _autocorr_columns)."""
    structure = Structure.load(input_file, ignore_zero_occupancy)
    ctx = _with_context(0, lambda: _autocorr_table(None, structure, None, groups, vdw_comp, dist_cutoff, rings, level, mode, max_lag, matrix))
    owner = _TableOwner(_autocorr_table(ctx, structure, None, groups, vdw_comp, dist_cutoff, rings, level, mode, max_lag, matrix))
    return _arrow_of(owner.t), _autocorr_columns(owner, rings, level, structure, None)


def _contact_similarity_arrow(input_file: str, groups: str, vdw_comp: float, dist_cutoff: float, ignore_zero_occupancy: bool, rings: bool, level: str, axis: str,
                              metric: str):
    """The command line's form of contact_similarity: (Arrow table of the frequency columns, the matrix)."""
    structure = Structure.load(input_file, ignore_zero_occupancy)
    ctx = _with_context(0, lambda: _similarity_table(None, structure, None, groups, vdw_comp, dist_cutoff, rings, level, axis, metric))
    owner = _TableOwner(_similarity_table(ctx, structure, None, groups, vdw_comp, dist_cutoff, rings, level, axis, metric))
    return _arrow_of(owner.t), _similarity_matrix(owner)["intersection" if metric == "count" else "similarity"]


def _contact_timelines_arrow(input_file: str, groups: str, vdw_comp: float, dist_cutoff: float, ignore_zero_occupancy: bool, rings: bool, level: str, bitmap: bool,
                             waters: bool = False):
    """The command line's form of contact_timelines: (Arrow table of the frequency + timeline columns, timeline_words or None)."""
    structure = Structure.load(input_file, ignore_zero_occupancy)
    ctx = _with_context(0, lambda: _timeline_table(None, structure, None, groups, vdw_comp, dist_cutoff, rings, level, bitmap, waters))
    t = _timeline_table(ctx, structure, None, groups, vdw_comp, dist_cutoff, rings, level, bitmap, waters)
    try:
        return _arrow_of(t), _timeline_columns(t, rings, level).get("timeline_words")
    finally:
        lib.arp_table_free(t)


def contacts_batch(input_files, groups: str = "/", vdw_comp: float = 0.1, dist_cutoff: float = 6.5, ignore_zero_occupancy: bool = False,
                   num_workers: int = 8, devices=None) -> list:
    """`contacts()` over many files: parsing, GPU pairs and table assembly of different files overlap on `num_workers` host threads
    (the C library releases the GIL), each with its own context; files are dealt round-robin over `devices` (default: all visible
    gfx950 devices).  Results come back in input order.  This is the file-level form of BASELINE config 5 (a batch of independent
    structures): on real files the parse and the host table, not the GPU, set the pace, and they scale with the workers."""
    import threading
    from concurrent.futures import ThreadPoolExecutor

    files = [str(f) for f in input_files]
    devs = list(devices) if devices is not None else list(range(max(device_count(), 1)))
    local = threading.local()

    def one(job):
        k, path = job
        dev = devs[k % len(devs)]
        ctxs = getattr(local, "ctxs", None)
        if ctxs is None:
            ctxs = local.ctxs = {}
        if dev not in ctxs:
            ctxs[dev] = Context(dev)
        s = Structure.load(path, ignore_zero_occupancy)
        return _table(ctxs[dev], s, groups, vdw_comp, dist_cutoff)

    if not files:
        return []
    with ThreadPoolExecutor(max_workers=max(1, min(int(num_workers), len(files)))) as pool:
        return list(pool.map(one, enumerate(files)))


# ---------------------------------------------------------------------------------------------- atom SASA, SAP score, dSASA
# Atom-level SASA (reference src/sasa.rs:174-249) and everything built on it: per-atom / per-residue SAP (src/sap.rs:137-340) and dSASA
# (src/sasa.rs:400-451, python.rs:161-191).  The Shrake-Rupley kernel, the SAP weights and the neighbour sum run on the device
# (include/arpeggia_amd.h "atom SASA").  Residue- and chain-level SASA and relative_sasa (src/sasa.rs:284-382, 520-561) sum the per-atom values
# on the device (arp_segment_sum) with the radii of a NAMED table: the reference computes them through rust-sasa, whose table is not part of its
# tree; "protor" is the table that reproduces the reference's chain-level pin, "vdw" the element radii of the atom level.
# On the older entry points (sasa, get_atom_sasa, get_dsasa, get_sasa_ensemble) radii=None keeps their behaviour: van der Waals radii at the
# atom level, the other levels refused.  dSASA is built from atom-level SASA here, where the reference sums chain-level SASA.
SASA_LEVELS = ("atom", "residue", "chain")
RADII_TABLES = {"vdw": _lib.ARP_RADII_VDW, "protor": _lib.ARP_RADII_PROTOR}
RESIDUE_SASA_COLUMNS = ["chain", "resn", "resi", "insertion", "sasa", "is_polar"]
CHAIN_SASA_COLUMNS = ["chain", "sasa"]
RELATIVE_SASA_COLUMNS = RESIDUE_SASA_COLUMNS + ["relative_sasa"]
SAP_LEVELS = ("atom", "residue")
# src/sap.rs:77-101 get_sc_max_asa (the table of arp_sap_weight; tests/test_sasa_host.py checks the two agree)
SAP_MAX_SC_ASA = {
    "ALA": 15.395, "ARG": 124.338, "ASN": 90.303, "ASP": 87.601, "CYS": 46.456, "GLU": 95.534, "GLN": 99.186, "GLY": 3.229, "HIS": 96.532,
    "ILE": 31.448, "LEU": 30.271, "LYS": 61.962, "MET": 65.233, "PHE": 67.945, "PRO": 17.812, "SER": 39.355, "THR": 42.648, "TRP": 101.491,
    "TYR": 94.478, "VAL": 26.702,
}
ATOM_SASA_COLUMNS = ["atomi", "sasa", "chain", "resn", "resi", "insertion", "altloc", "atomn"]
ATOM_SAP_COLUMNS = ["chain", "resn", "resi", "insertion", "atomn", "atomi", "sasa", "sap_score"]
RESIDUE_SAP_COLUMNS = ["chain", "resn", "resi", "insertion", "sc_sasa", "sap_score", "max_sc_asa", "relative_sc_sasa"]


def sasa_sphere_points(n_points: int) -> np.ndarray:
    """The n_points x 3 f32 unit vectors of the SASA contract (arp_sasa_sphere_points: golden spiral in f64, rounded to f32)."""
    out = np.zeros((int(n_points), 3), dtype="<f4")
    _check(lib.arp_sasa_sphere_points(int(n_points), out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def atom_sasa(ctx: "Context", x, y, z, radius, include=None, probe: float = 1.4, n_points: int = 100):
    """arp_atom_sasa on host arrays: (sasa f32, count i32) per atom; atoms outside `include` get 0 and neither bury nor are buried."""
    x, y, z = (np.ascontiguousarray(v, dtype="<f8") for v in (x, y, z))
    r = np.ascontiguousarray(radius, dtype="<f4")
    n = len(x)
    inc = None if include is None else np.ascontiguousarray(include, dtype=np.uint8)
    sasa = np.zeros(n, dtype="<f4")
    count = np.zeros(n, dtype="<i4")
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    _check(lib.arp_atom_sasa(ctx._h, n, x.ctypes.data_as(dp), y.ctypes.data_as(dp), z.ctypes.data_as(dp), r.ctypes.data_as(fp),
                             None if inc is None else inc.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_float(probe), int(n_points),
                             sasa.ctypes.data_as(fp), count.ctypes.data_as(C.POINTER(C.c_int32))))
    return sasa, count


def atom_sasa_groups(ctx: "Context | None", x, y, z, radius, group, probe: float = 1.4, n_points: int = 100):
    """arp_atom_sasa_groups on host arrays: group is a u8 mask per atom (0: out, 1: group 1, 2: group 2, 3: both).  Returns (count [3, n] i32,
    sasa [3, n] f32, buried [n] i32): the planes are complex, group 1, group 2 (0 where the atom is not in the group); buried = own group
    counts - complex count, in points.  ctx None: the arguments are only checked (raises their error, else the missing context's)."""
    x, y, z = (np.ascontiguousarray(v, dtype="<f8") for v in (x, y, z))
    r = np.ascontiguousarray(radius, dtype="<f4")
    g = np.ascontiguousarray(group, dtype=np.uint8)
    n = len(x)
    count, sasa_, buried = np.zeros((3, n), "<i4"), np.zeros((3, n), "<f4"), np.zeros(n, "<i4")
    dp, fp, ip = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_int32)
    _check(lib.arp_atom_sasa_groups(ctx._h if ctx is not None else None, n, x.ctypes.data_as(dp), y.ctypes.data_as(dp), z.ctypes.data_as(dp),
                                    r.ctypes.data_as(fp), g.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_float(probe), int(n_points),
                                    count.ctypes.data_as(ip), sasa_.ctypes.data_as(fp), buried.ctypes.data_as(ip)))
    return count, sasa_, buried


def sasa_tests(ctx: "Context") -> int:
    """f32 distance tests the kernel of the context's most recent SASA call made (diagnostics)."""
    return int(lib.arp_sasa_tests(ctx._h))


def sasa_select(structure: Structure, chains: str = "", model_num: int = 0, remove_hydrogens: bool = True) -> np.ndarray:
    """Structure atom indices get_atom_sasa works on (prepare_pdb_for_sasa + filter_pdb_by_model, sasa.rs:27-135,183-195; the steps and
    the model quirk are in include/arpeggia_amd.h arp_structure_sasa_select)."""
    out = np.zeros(max(structure.n_atoms, 1), dtype="<u4")
    n = C.c_uint64()
    _check(lib.arp_structure_sasa_select(structure._h, chains.encode(), int(model_num), int(bool(remove_hydrogens)), C.byref(n),
                                         out.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out[: n.value].copy()


def _frame(cols: dict):
    """A table of the contact table's type: polars.DataFrame when polars is importable, else pyarrow.Table."""
    import pyarrow as pa

    return _frame_of(pa.table(cols))


def _strings(structure: Structure, column: str, idx: np.ndarray) -> list:
    return [b.decode() for b in structure.strings(column)[idx]]


def _identity(structure: Structure, idx: np.ndarray) -> dict:
    """Entity columns of the given atoms with the contact table's conventions (utf8, "" for a blank insertion code / altloc)."""
    import pyarrow as pa

    return {
        "chain": pa.array(_strings(structure, "chain", idx), pa.string()), "resn": pa.array(_strings(structure, "resn", idx), pa.string()),
        "resi": pa.array(structure.ints("resi")[idx].astype("<i4"), pa.int32()),
        "insertion": pa.array(_strings(structure, "insertion", idx), pa.string()),
        "altloc": pa.array(_strings(structure, "altloc", idx), pa.string()), "atomn": pa.array(_strings(structure, "atomn", idx), pa.string()),
        "atomi": pa.array(structure.ints("atomi")[idx].astype("<i4"), pa.int32()),
    }


def _radii_table(radii) -> int:
    """The table code of a radii name ("vdw" / "protor", case-insensitive); an unknown name is a ValueError."""
    key = str(radii).lower()
    if key not in RADII_TABLES:
        raise ValueError(f"Invalid radii '{radii}'. Must be one of: 'vdw', 'protor'")
    return RADII_TABLES[key]


def sasa_radius(resn: str, atomn: str, element: str = "", radii: str = "protor") -> float:
    """arp_sasa_radius: the f32 radius of (residue, atom name) in the named table, with its van der Waals fallback by element."""
    out = C.c_float()
    _check(lib.arp_sasa_radius(resn.encode(), atomn.encode(), element.encode(), _radii_table(radii), C.byref(out)))
    return float(out.value)


def max_asa(resn: str):
    """arp_max_asa: MaxASA of Tien et al. 2013 (the reference's get_max_asa), None for a residue without one."""
    v = float(lib.arp_max_asa(resn.encode()))
    return v if v > 0.0 else None


def segment_sum(ctx: "Context | None", values, seg_start, seg_item) -> np.ndarray:
    """arp_segment_sum: values [rows, m] f32, a CSR of segments over the m items -> [rows, n_seg] f32, every sum the sequential f64 chain in
    list order rounded to f32 once.  ctx None: the inputs are only checked."""
    v = np.ascontiguousarray(values, dtype="<f4")
    if v.ndim == 1:
        v = v[None]
    start = np.ascontiguousarray(seg_start, dtype="<u4")
    item = np.ascontiguousarray(seg_item, dtype="<u4")
    rows, m = v.shape
    n_seg = len(start) - 1
    out = np.zeros((rows, max(n_seg, 0)), dtype="<f4")
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    pad = lambda a, ty: (a if a.size else np.zeros(1, a.dtype)).ctypes.data_as(ty)  # noqa: E731  (a valid pointer for an empty array)
    _check(lib.arp_segment_sum(ctx._h if ctx is not None else None, rows, m, pad(v, fp), max(n_seg, 0), pad(start, up), pad(item, up), pad(out, fp)))
    return out


def atom_sasa_rows(structure: Structure, probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, remove_hydrogens: bool = True,
                   chains: str = "", device: int = 0, radii=None):
    """arp_structure_atom_sasa as numpy arrays: (structure atom index u32, sasa f32, count i32), rows sorted by serial number.  radii: None (van
    der Waals, as ever) or a table name."""
    table = None if radii is None else _radii_table(radii)
    n = max(structure.n_atoms, 1)
    atoms, sasa, count = np.zeros(n, "<u4"), np.zeros(n, "<f4"), np.zeros(n, "<i4")
    rows = C.c_uint64()
    tail = (C.byref(rows), atoms.ctypes.data_as(C.POINTER(C.c_uint32)), sasa.ctypes.data_as(C.POINTER(C.c_float)), count.ctypes.data_as(C.POINTER(C.c_int32)))
    head = (structure._h, chains.encode(), int(model_num), int(bool(remove_hydrogens)), C.c_float(probe_radius), int(n_points))
    if table is None:
        _check(lib.arp_structure_atom_sasa(_context(device)._h, *head, *tail))
    else:
        _check(lib.arp_structure_atom_sasa_radii(_context(device)._h, *head, table, *tail))
    k = rows.value
    return atoms[:k].copy(), sasa[:k].copy(), count[:k].copy()


def get_atom_sasa(structure: Structure, probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, remove_hydrogens: bool = True,
                  chains: str = "", device: int = 0, radii=None):
    """`arpeggia::get_atom_sasa` (sasa.rs:174): columns atomi i32, sasa f32, chain, resn, resi i32, insertion, altloc, atomn; sorted by atomi."""
    import pyarrow as pa

    idx, sasa, _ = atom_sasa_rows(structure, probe_radius, n_points, model_num, remove_hydrogens, chains, device, radii)
    ident = _identity(structure, idx)
    cols = {"atomi": ident["atomi"], "sasa": pa.array(sasa, pa.float32())}
    cols.update({k: ident[k] for k in ATOM_SASA_COLUMNS[2:]})
    return _frame(cols)


def level_sasa_rows(structure: Structure, level: str, probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, chains: str = "",
                    radii: str = "protor", device: int = 0) -> dict:
    """arp_structure_residue_sasa / _chain_sasa / _relative_sasa as numpy arrays: atoms (the first selected atom of every row: its identity),
    sasa f32, and for the residue levels is_polar (bool); level "relative" adds relative_sasa f32 (NaN where null) and valid (bool)."""
    table = _radii_table(radii)
    n = max(structure.n_atoms, 1)
    atoms, sasa_ = np.zeros(n, "<u4"), np.zeros(n, "<f4")
    polar, valid, rel = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, "<f4")
    rows = C.c_uint64()
    fp, bp = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
    args = (_context(device)._h, structure._h, chains.encode(), int(model_num), C.c_float(probe_radius), int(n_points), table, C.byref(rows),
            atoms.ctypes.data_as(C.POINTER(C.c_uint32)), sasa_.ctypes.data_as(fp))
    if level == "chain":
        _check(lib.arp_structure_chain_sasa(*args))
    elif level == "residue":
        _check(lib.arp_structure_residue_sasa(*args, polar.ctypes.data_as(bp)))
    elif level == "relative":
        _check(lib.arp_structure_relative_sasa(*args, polar.ctypes.data_as(bp), rel.ctypes.data_as(fp), valid.ctypes.data_as(bp)))
    else:
        raise ValueError(f"Invalid level '{level}'")
    k = rows.value
    out = {"atoms": atoms[:k].copy(), "sasa": sasa_[:k].copy()}
    if level != "chain":
        out["is_polar"] = polar[:k].astype(bool)
    if level == "relative":
        out["relative_sasa"], out["valid"] = rel[:k].copy(), valid[:k].astype(bool)
    return out


def _residue_identity(structure: Structure, idx: np.ndarray) -> dict:
    ident = _identity(structure, idx)
    return {k: ident[k] for k in RESIDUE_SASA_COLUMNS[:4]}


def _nullable_f32(values: np.ndarray, valid: np.ndarray):
    import pyarrow as pa

    return pa.array(values, pa.float32(), mask=~np.asarray(valid, bool))


def get_residue_sasa(structure: Structure, probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, chains: str = "",
                     radii: str = "protor", device: int = 0):
    """`arpeggia::get_residue_sasa` (sasa.rs:284): chain, resn, resi i32, insertion, sasa f32, is_polar; sorted by chain, resi, insertion."""
    import pyarrow as pa

    r = level_sasa_rows(structure, "residue", probe_radius, n_points, model_num, chains, radii, device)
    cols = _residue_identity(structure, r["atoms"])
    cols["sasa"] = pa.array(r["sasa"], pa.float32())
    cols["is_polar"] = pa.array(r["is_polar"], pa.bool_())
    return _frame(cols)


def get_chain_sasa(structure: Structure, probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, chains: str = "",
                   radii: str = "protor", device: int = 0):
    """`arpeggia::get_chain_sasa` (sasa.rs:352): chain, sasa f32; sorted by chain."""
    import pyarrow as pa

    r = level_sasa_rows(structure, "chain", probe_radius, n_points, model_num, chains, radii, device)
    return _frame({"chain": pa.array(_strings(structure, "chain", r["atoms"]), pa.string()), "sasa": pa.array(r["sasa"], pa.float32())})


def get_relative_sasa(structure: Structure, probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, chains: str = "",
                      radii: str = "protor", device: int = 0):
    """`arpeggia::get_relative_sasa` (sasa.rs:520, its code): the residue rows plus relative_sasa = sasa / MaxASA (Tien et al. 2013), null for
    a residue without a MaxASA."""
    import pyarrow as pa

    r = level_sasa_rows(structure, "relative", probe_radius, n_points, model_num, chains, radii, device)
    cols = _residue_identity(structure, r["atoms"])
    cols["sasa"] = pa.array(r["sasa"], pa.float32())
    cols["is_polar"] = pa.array(r["is_polar"], pa.bool_())
    cols["relative_sasa"] = _nullable_f32(r["relative_sasa"], r["valid"])
    return _frame(cols)


def relative_sasa(input_file: str, probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, chains: str = "", num_threads: int = 1):
    """Drop-in for `arpeggia.relative_sasa` (python.rs:242), with the "protor" radii."""
    del num_threads  # (the computation runs on the GPU; accepted for signature compatibility)
    return get_relative_sasa(Structure.load(input_file), probe_radius, n_points, model_num, chains)


def sasa(input_file: str, level: str = "atom", probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, chains: str = "",
         num_threads: int = 1, radii=None):
    """Drop-in for `arpeggia.sasa` (python.rs:93).  radii None: level "atom" with van der Waals radii, the other levels refused (they need a
    named radius table: see the section comment above); radii "protor" / "vdw": every level, with that table."""
    lv = str(level).lower()
    if lv not in ("atom", "residue", "chain"):
        raise ValueError(f"Invalid level '{level}'. Must be one of: 'atom', 'residue', 'chain'")
    if radii is not None:
        _radii_table(radii)
    elif lv != "atom":
        raise NotImplementedError(f"sasa level '{lv}' needs a named radius table: the reference computes it with rust-sasa's own table, which is "
                                  "not part of its source tree; pass radii='protor' (the table that reproduces its chain-level pin) or radii='vdw'")
    del num_threads  # (the computation runs on the GPU; accepted for signature compatibility)
    s = Structure.load(input_file)
    if lv == "atom":
        return get_atom_sasa(s, probe_radius, n_points, model_num, True, chains, radii=radii)
    return (get_residue_sasa if lv == "residue" else get_chain_sasa)(s, probe_radius, n_points, model_num, chains, radii)


def atom_sap_rows(structure: Structure, probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, sap_radius: float = 5.0,
                  chains: str = "", device: int = 0):
    """arp_structure_sap_score as numpy arrays: (structure atom index, sasa f32, sap_score f32), rows sorted by serial number."""
    n = max(structure.n_atoms, 1)
    atoms, sasa_, sap = np.zeros(n, "<u4"), np.zeros(n, "<f4"), np.zeros(n, "<f4")
    rows = C.c_uint64()
    fp = C.POINTER(C.c_float)
    _check(lib.arp_structure_sap_score(_context(device)._h, structure._h, chains.encode(), int(model_num), C.c_float(probe_radius), int(n_points),
                                       C.c_float(sap_radius), C.byref(rows), atoms.ctypes.data_as(C.POINTER(C.c_uint32)), sasa_.ctypes.data_as(fp),
                                       sap.ctypes.data_as(fp)))
    k = rows.value
    return atoms[:k].copy(), sasa_[:k].copy(), sap[:k].copy()


def get_per_atom_sap_score(structure: Structure, probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, sap_radius: float = 5.0,
                           chains: str = "", device: int = 0):
    """`arpeggia::get_per_atom_sap_score` (sap.rs:137-259): chain, resn, resi, insertion, atomn, atomi, sasa, sap_score; sorted by atomi."""
    import pyarrow as pa

    idx, sasa_, sap = atom_sap_rows(structure, probe_radius, n_points, model_num, sap_radius, chains, device)
    ident = _identity(structure, idx)
    cols = {k: ident[k] for k in ATOM_SAP_COLUMNS[:6]}
    cols["sasa"] = pa.array(sasa_, pa.float32())
    cols["sap_score"] = pa.array(sap, pa.float32())
    return _frame(cols)


def residue_sap_from_atoms(chain, resn, resi, insertion, sasa_, sap) -> dict:
    """sap.rs:295-340 on per-atom columns: rows with sap_score > 0, grouped by (chain, resn, resi, insertion), sc_sasa and sap_score summed
    (in f64, rounded to f32 once), sorted by chain, resi, insertion (stable), then max_sc_asa and relative_sc_sasa = clip(sc_sasa / max_sc_asa,
    0, 1) in f32.  Returns numpy / list columns in RESIDUE_SAP_COLUMNS order."""
    groups: dict = {}
    for c, rn, ri, ic, a, s in zip(chain, resn, resi, insertion, sasa_, sap):
        if not s > 0.0:
            continue
        g = groups.setdefault((c, rn, int(ri), ic), [0.0, 0.0])
        g[0] += float(a)
        g[1] += float(s)
    keys = sorted(groups, key=lambda k: (k[0], k[2], k[3]))
    sc = np.array([groups[k][0] for k in keys], dtype=np.float64).astype(np.float32)
    sp = np.array([groups[k][1] for k in keys], dtype=np.float64).astype(np.float32)
    mx = np.array([SAP_MAX_SC_ASA[k[1]] for k in keys], dtype=np.float32)  # (sap.rs:326 unwraps: every residue with a score has a value)
    rel = np.clip(sc / mx, np.float32(0.0), np.float32(1.0)).astype(np.float32) if keys else np.zeros(0, np.float32)
    return {"chain": [k[0] for k in keys], "resn": [k[1] for k in keys], "resi": np.array([k[2] for k in keys], dtype="<i4"),
            "insertion": [k[3] for k in keys], "sc_sasa": sc, "sap_score": sp, "max_sc_asa": mx, "relative_sc_sasa": rel}


def get_per_residue_sap_score(structure: Structure, probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, sap_radius: float = 5.0,
                              chains: str = "", device: int = 0):
    """`arpeggia::get_per_residue_sap_score` (sap.rs:295-340): chain, resn, resi, insertion, sc_sasa, sap_score, max_sc_asa, relative_sc_sasa."""
    import pyarrow as pa

    idx, sasa_, sap = atom_sap_rows(structure, probe_radius, n_points, model_num, sap_radius, chains, device)
    cols = residue_sap_from_atoms(_strings(structure, "chain", idx), _strings(structure, "resn", idx), structure.ints("resi")[idx],
                                  _strings(structure, "insertion", idx), sasa_, sap)
    types = {"chain": pa.string(), "resn": pa.string(), "resi": pa.int32(), "insertion": pa.string()}
    return _frame({k: pa.array(v, types.get(k, pa.float32())) for k, v in cols.items()})


def sap_score(input_file: str, level: str = "residue", probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0,
              sap_radius: float = 5.0, chains: str = "", num_threads: int = 1):
    """Drop-in for `arpeggia.sap_score` (python.rs:286-325)."""
    lv = str(level).lower()
    if lv not in SAP_LEVELS:
        raise ValueError(f"Invalid level '{level}'. Must be one of: 'atom', 'residue'")
    del num_threads
    s = Structure.load(input_file)
    f = get_per_atom_sap_score if lv == "atom" else get_per_residue_sap_score
    return f(s, probe_radius, n_points, model_num, sap_radius, chains)


def get_dsasa(structure: Structure, groups: str, probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, device: int = 0, radii=None) -> float:
    """`arpeggia::get_dsasa` (sasa.rs:400-451) from atom-level SASA: SASA(group 1) + SASA(group 2) - SASA(complex), not halved.
    A negative value raises (python.rs:177-188); group errors are those of the contact path's parse_groups.  radii: None (van der Waals) or a table name."""
    out = C.c_float()
    if radii is None:
        _check(lib.arp_structure_dsasa(_context(device)._h, structure._h, groups.encode(), C.c_float(probe_radius), int(n_points), int(model_num),
                                       C.byref(out)))
    else:
        table = _radii_table(radii)
        _check(lib.arp_structure_dsasa_radii(_context(device)._h, structure._h, groups.encode(), C.c_float(probe_radius), int(n_points), int(model_num),
                                             table, C.byref(out)))
    return float(out.value)


def dsasa(input_file: str, groups: str, probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, num_threads: int = 1, radii=None) -> float:
    """Drop-in for `arpeggia.dsasa` (python.rs:161-191)."""
    del num_threads
    return get_dsasa(Structure.load(input_file), groups, probe_radius, n_points, model_num, radii=radii)


# ---- buried surface per atom and residue; dSASA across frames (include/arpeggia_amd.h arp_structure_buried_sasa; no counterpart in the reference) ----
BURIED_SASA_VALUE_COLUMNS = ["sasa_complex", "sasa_group1", "sasa_group2", "buried"]
BURIED_ATOM_COLUMNS = ATOM_SASA_COLUMNS[:1] + ATOM_SASA_COLUMNS[2:] + ["group"] + BURIED_SASA_VALUE_COLUMNS
BURIED_RESIDUE_COLUMNS = ["chain", "resn", "resi", "insertion", "group"] + BURIED_SASA_VALUE_COLUMNS + ["n_buried_atoms"]
DSASA_FRAME_COLUMNS = ["frame", "total_complex", "total_group1", "total_group2", "dsasa"]
DSASA_ENSEMBLE_COLUMNS = ["chain", "resn", "resi", "insertion", "altloc", "atomn", "atomi", "group", "n_frames", "buried_mean", "buried_std", "buried_min",
                          "buried_max", "occupancy"]


def _buried_sasa(ctx: "Context | None", structure: Structure, groups: str, probe_radius: float, n_points: int, model_num: int, radii) -> dict:
    """arp_structure_buried_sasa.  ctx None: the checks that need no device run (raises their error, else the missing context's)."""
    table = RADII_TABLES["vdw"] if radii is None else _radii_table(radii)
    n = max(structure.n_atoms, 1)
    atoms, grp, sasa_, count, buried = np.zeros(n, "<u4"), np.zeros(n, np.uint8), np.zeros(3 * n, "<f4"), np.zeros(3 * n, "<i4"), np.zeros(n, "<i4")
    res_atoms, res_sasa, res_nb, totals = np.zeros(n, "<u4"), np.zeros(3 * n, "<f4"), np.zeros(n, "<u4"), np.zeros(4, "<f4")
    rows, res_rows = C.c_uint64(), C.c_uint64()
    fp, ip, up = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32)
    _check(lib.arp_structure_buried_sasa(ctx._h if ctx is not None else None, structure._h, groups.encode(), C.c_float(probe_radius), int(n_points),
                                         int(model_num), table, C.byref(rows), atoms.ctypes.data_as(up), grp.ctypes.data_as(C.POINTER(C.c_uint8)),
                                         sasa_.ctypes.data_as(fp), count.ctypes.data_as(ip), buried.ctypes.data_as(ip), C.byref(res_rows),
                                         res_atoms.ctypes.data_as(up), res_sasa.ctypes.data_as(fp), res_nb.ctypes.data_as(up), totals.ctypes.data_as(fp)))
    m, nr = int(rows.value), int(res_rows.value)
    return {"atoms": atoms[:m].copy(), "group": grp[:m].copy(), "sasa": sasa_[: 3 * m].reshape(3, m).copy(), "count": count[: 3 * m].reshape(3, m).copy(),
            "buried": buried[:m].copy(), "res_atoms": res_atoms[:nr].copy(), "res_sasa": res_sasa[: 3 * nr].reshape(3, nr).copy(),
            "res_buried_atoms": res_nb[:nr].copy(), "totals": totals.copy(), "dsasa": float(totals[3])}


def dsasa_total(total_complex: float, total_group1: float, total_group2: float) -> float:
    """arp_dsasa_total: group 1 + group 2 - complex in f32, as get_dsasa forms its scalar; a negative value raises as there."""
    out = C.c_float()
    _check(lib.arp_dsasa_total(C.c_float(total_complex), C.c_float(total_group1), C.c_float(total_group2), C.byref(out)))
    return float(out.value)


def _buried_value_columns(group: np.ndarray, planes: np.ndarray) -> dict:
    """group, sasa_complex, sasa_group1 / sasa_group2 (null where the row is not in the group) and buried = the non-null group values - complex, in f32."""
    import pyarrow as pa

    in1, in2 = (group & 1) != 0, (group & 2) != 0
    own = np.where(in1, planes[1], np.float32(0.0)).astype(np.float32) + np.where(in2, planes[2], np.float32(0.0)).astype(np.float32)
    return {"group": pa.array(group, pa.uint8()), "sasa_complex": pa.array(planes[0], pa.float32()), "sasa_group1": _nullable_f32(planes[1], in1),
            "sasa_group2": _nullable_f32(planes[2], in2), "buried": pa.array((own - planes[0]).astype(np.float32), pa.float32())}


def get_buried_sasa(structure: Structure, groups: str, level: str = "atom", probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0,
                    radii=None, device: int = 0):
    """The interface between two chain groups, row by row: returns (table, dsasa).  level "atom": one row per atom of the two groups (the rows
    and order of get_atom_sasa on their chains) with the identity columns of get_atom_sasa, group (1, 2, 3 = in both), sasa_complex, sasa_group1,
    sasa_group2 (null where the atom is not in the group) and buried (A^2, f32: the non-null group values - sasa_complex) -- BURIED_ATOM_COLUMNS.
    level "residue": one row per residue (the rows and order of get_residue_sasa) with the same value columns from segment sums on the device and
    n_buried_atoms (atoms with buried points) -- BURIED_RESIDUE_COLUMNS.  dsasa: the scalar of get_dsasa on the same arguments, bit for bit (a
    negative value raises, as there).  radii: None (van der Waals) or a table name."""
    import pyarrow as pa

    lv = str(level).lower()
    if lv not in ("atom", "residue"):
        raise ValueError(f"Invalid level '{level}'. Must be one of: 'atom', 'residue'")
    if radii is not None:
        _radii_table(radii)
    ctx = _with_context(device, lambda: _buried_sasa(None, structure, groups, probe_radius, n_points, model_num, radii))
    r = ctx.buried_sasa(structure, groups, probe_radius, n_points, model_num, radii)
    if lv == "atom":
        ident = _identity(structure, r["atoms"])
        cols = {"atomi": ident["atomi"]}
        cols.update({k: ident[k] for k in ATOM_SASA_COLUMNS[2:]})
        cols.update(_buried_value_columns(r["group"], r["sasa"]))
        return _frame(cols), r["dsasa"]
    cols = _residue_identity(structure, r["res_atoms"])
    by_atom = dict(zip(r["atoms"].tolist(), r["group"].tolist()))
    cols.update(_buried_value_columns(np.array([by_atom[a] for a in r["res_atoms"].tolist()], np.uint8), r["res_sasa"]))
    cols["n_buried_atoms"] = pa.array(r["res_buried_atoms"], pa.uint32())
    return _frame(cols), r["dsasa"]


def buried_sasa(input_file: str, groups: str, level: str = "atom", probe_radius: float = 1.4, n_points: int = 100, model_num: int = 0, radii=None):
    """get_buried_sasa on a file: (table, dsasa)."""
    return get_buried_sasa(Structure.load(input_file), groups, level, probe_radius, n_points, model_num, radii)


def _dsasa_ensemble(ctx: "Context | None", structure: Structure, frames, groups: str, probe_radius: float, n_points: int, radii, per_frame: bool) -> dict:
    """arp_dsasa_ensemble.  ctx None: the inputs are only checked (raises their error); the result then holds atoms, group, R and n_frames only."""
    table = RADII_TABLES["vdw"] if radii is None else _radii_table(radii)
    n_frames, ptr, keep = _frames_arg(structure, frames, "dsasa ensemble")
    fp, ip, up, qp = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    rows, used = C.c_uint64(), C.c_uint64()
    n = max(structure.n_atoms, 1)
    atoms, grp, R = np.zeros(n, "<u4"), np.zeros(n, np.uint8), np.zeros(n, "<f4")
    head = (structure._h, int(n_frames), ptr, groups.encode(), C.c_float(probe_radius), int(n_points), table, C.byref(rows), C.byref(used),
            atoms.ctypes.data_as(up), grp.ctypes.data_as(C.POINTER(C.c_uint8)), R.ctypes.data_as(fp))
    if ctx is None:
        _check(lib.arp_dsasa_ensemble(None, *head, *([None] * 10)))
        m = int(rows.value)
        return {"atoms": atoms[:m].copy(), "group": grp[:m].copy(), "R": R[:m].copy(), "n_frames": int(used.value)}
    n_top = _topology_atoms(structure)
    f_cap = n_frames if frames is not None else (structure.n_atoms // n_top if n_top else 1)
    s1, s2 = np.zeros(max(n_top, 1), "<u8"), np.zeros(max(n_top, 1), "<u8")
    bmin, bmax, fb = np.zeros(max(n_top, 1), "<i4"), np.zeros(max(n_top, 1), "<i4"), np.zeros(max(n_top, 1), "<u4")
    tot = {k: np.zeros(max(f_cap, 1), "<f4") for k in ("total_complex", "total_g1", "total_g2", "dsasa")}
    per = np.zeros(max(f_cap * n_top, 1), "<i4") if per_frame else None
    _check(lib.arp_dsasa_ensemble(ctx._h, *head, s1.ctypes.data_as(qp), s2.ctypes.data_as(qp), bmin.ctypes.data_as(ip), bmax.ctypes.data_as(ip),
                                  fb.ctypes.data_as(up), *(tot[k].ctypes.data_as(fp) for k in tot), None if per is None else per.ctypes.data_as(ip)))
    del keep
    m, F = int(rows.value), int(used.value)
    out = {"atoms": atoms[:m].copy(), "group": grp[:m].copy(), "R": R[:m].copy(), "n_frames": F, "sum_buried": s1[:m].copy(), "sum_buried_sq": s2[:m].copy(),
           "min_buried": bmin[:m].copy(), "max_buried": bmax[:m].copy(), "frames_buried": fb[:m].copy()}
    out.update({k: v[:F].copy() for k, v in tot.items()})
    if per is not None:
        out["buried"] = per[: F * m].reshape(F, m)
    return out


def dsasa_ensemble_stats(n_frames: int, radius_plus_probe, n_points: int, sum_buried, sum_buried_sq, min_buried, max_buried, frames_buried) -> dict:
    """The per-atom columns of get_dsasa_ensemble from the integer accumulators of arp_dsasa_ensemble, on the host: buried_mean, buried_std
    (population), buried_min, buried_max in A^2 -- sasa_ensemble_stats on the buried points, a point being 4 pi R^2 / n_points -- and
    occupancy = frames_buried / n_frames (f64)."""
    r = sasa_ensemble_stats(n_frames, radius_plus_probe, n_points, sum_buried, sum_buried_sq, min_buried, max_buried)
    out = {"buried_mean": r["mean_sasa"], "buried_std": r["std_sasa"], "buried_min": r["min_sasa"], "buried_max": r["max_sasa"]}
    out["occupancy"] = np.asarray(frames_buried, np.float64) / float(n_frames)
    return out


def get_dsasa_ensemble(structure: Structure, frames=None, groups: str = "/", probe_radius: float = 1.4, n_points: int = 100, radii=None,
                       per_frame: bool = False, device: int = 0):
    """dSASA across the frames of an ensemble, frames packed on the device in one call: returns (frame_table, atom_table).  frame_table: frame,
    total_complex, total_group1, total_group2, dsasa (DSASA_FRAME_COLUMNS; a negative frame value is returned as it is).  atom_table: one row per
    atom of the two groups with the identity columns, group, n_frames, buried_mean, buried_std, buried_min, buried_max (A^2) and occupancy = the
    share of frames in which the atom has buried points (DSASA_ENSEMBLE_COLUMNS).  frames: [F, N, 3] f64 coordinates of the N atoms of model 0;
    None: the structure's models are the frames.  per_frame=True adds a third value {"buried": [F, m] i32 points}."""
    import pyarrow as pa

    ctx = _with_context(device, lambda: _dsasa_ensemble(None, structure, frames, groups, probe_radius, n_points, radii, False))
    r = ctx.dsasa_ensemble(structure, frames, groups, probe_radius, n_points, radii, per_frame)
    F = r["n_frames"]
    ft = _frame({"frame": pa.array(np.arange(F, dtype="<u4"), pa.uint32()), "total_complex": pa.array(r["total_complex"], pa.float32()),
                 "total_group1": pa.array(r["total_g1"], pa.float32()), "total_group2": pa.array(r["total_g2"], pa.float32()),
                 "dsasa": pa.array(r["dsasa"], pa.float32())})
    st = dsasa_ensemble_stats(F, r["R"], n_points, r["sum_buried"], r["sum_buried_sq"], r["min_buried"], r["max_buried"], r["frames_buried"])
    ident = _identity(structure, r["atoms"])
    cols = {k: ident[k] for k in DSASA_ENSEMBLE_COLUMNS[:7]}
    cols["group"] = pa.array(r["group"], pa.uint8())
    cols["n_frames"] = pa.array(np.full(len(r["atoms"]), F, "<u4"), pa.uint32())
    for k in ("buried_mean", "buried_std", "buried_min", "buried_max"):
        cols[k] = pa.array(st[k], pa.float32())
    cols["occupancy"] = pa.array(st["occupancy"], pa.float64())
    at = _frame(cols)
    return (ft, at, {"buried": r["buried"]}) if per_frame else (ft, at)


def dsasa_ensemble(input_file: str, groups: str, probe_radius: float = 1.4, n_points: int = 100, radii=None):
    """dSASA across the models of a multi-model file: see get_dsasa_ensemble."""
    return get_dsasa_ensemble(Structure.load(input_file), None, groups, probe_radius, n_points, radii)


# ---- shape complementarity (reference src/sc/, python.rs:369-381; include/arpeggia_amd.h "shape complementarity")
# ---- SASA / SAP statistics over the frames of an ensemble (include/arpeggia_amd.h arp_sasa_ensemble; no counterpart in the reference) ----
ENSEMBLE_SASA_COLUMNS = ["chain", "resn", "resi", "insertion", "altloc", "atomn", "atomi", "n_frames", "mean_sasa", "std_sasa", "min_sasa", "max_sasa"]
ENSEMBLE_SAP_COLUMNS = ENSEMBLE_SASA_COLUMNS + ["mean_sap", "std_sap", "min_sap", "max_sap"]
RESIDUE_ENSEMBLE_SAP_COLUMNS = RESIDUE_SAP_COLUMNS + ["n_frames"]


def _ensemble_table(structure: Structure, r: dict, names: list):
    import pyarrow as pa

    ident = _identity(structure, r["atoms"])
    cols = {k: ident[k] for k in ENSEMBLE_SASA_COLUMNS[:7]}
    cols["n_frames"] = pa.array(np.full(len(r["atoms"]), r["n_frames"], "<u4"), pa.uint32())
    for k in names[8:]:
        cols[k] = pa.array(r[k], pa.float32())
    return _frame(cols)


def _ensemble_run(structure: Structure, frames, chains: str, probe_radius: float, n_points: int, sap_radius, per_frame: bool, device: int, radii=None) -> dict:
    ctx = _with_context(device, lambda: _sasa_ensemble(None, structure, frames, chains, probe_radius, n_points, sap_radius, False, radii))
    return ctx.sasa_ensemble(structure, frames, chains, probe_radius, n_points, sap_radius, per_frame, radii)


RESIDUE_ENSEMBLE_SASA_COLUMNS = ["chain", "resn", "resi", "insertion", "is_polar", "mean_sasa", "std_sasa", "min_sasa", "max_sasa", "mean_relative_sasa", "n_frames"]


def get_residue_sasa_ensemble(structure: Structure, frames=None, chains: str = "", probe_radius: float = 1.4, n_points: int = 100, radii: str = "protor",
                              per_frame: bool = False, device: int = 0):
    """Residue-level SASA statistics over the frames of an ensemble, the per-atom values summed per residue and per chain on the device: one row
    per residue of the selection (the rows and order of get_residue_sasa) with is_polar, mean_sasa, std_sasa (population), min_sasa, max_sasa,
    mean_relative_sasa (mean_sasa / MaxASA, null without one) and n_frames (RESIDUE_ENSEMBLE_SASA_COLUMNS).  Returns (table, extras) with
    extras = {"chains": the chain ids in get_chain_sasa's order, "chain_sasa": [F, n_chains] f32}; per_frame=True adds "residue_sasa": [F, n_res] f32."""
    import pyarrow as pa

    ctx = _with_context(device, lambda: _residue_sasa_ensemble(None, structure, frames, chains, probe_radius, n_points, radii, False))
    r = ctx.residue_sasa_ensemble(structure, frames, chains, probe_radius, n_points, radii, per_frame)
    cols = _residue_identity(structure, r["res_atoms"])
    cols["is_polar"] = pa.array(r["is_polar"], pa.bool_())
    for k in ("mean_sasa", "std_sasa", "min_sasa", "max_sasa"):
        cols[k] = pa.array(r[k], pa.float32())
    cols["mean_relative_sasa"] = _nullable_f32(r["mean_relative_sasa"], r["relative_valid"])
    cols["n_frames"] = pa.array(np.full(len(r["res_atoms"]), r["n_frames"], "<u4"), pa.uint32())
    extras = {"chains": _strings(structure, "chain", r["chain_atoms"]), "chain_sasa": r["chain_sasa"]}
    if per_frame:
        extras["residue_sasa"] = r["residue_sasa"]
    return _frame(cols), extras


def get_sasa_ensemble(structure: Structure, frames=None, chains: str = "", probe_radius: float = 1.4, n_points: int = 100, per_frame: bool = False,
                      device: int = 0, radii=None):
    """Per-atom SASA statistics over the frames of an ensemble, frames packed on the device in one call: one row per selected heavy atom with
    the identity columns of get_atom_sasa, n_frames, mean_sasa, std_sasa (population), min_sasa, max_sasa (ENSEMBLE_SASA_COLUMNS).  frames:
    [F, N, 3] f64 coordinates of the N atoms of model 0; None: the structure's models are the frames.  per_frame=True returns (table, extras)
    with extras = {"total_sasa": [F] f32, "count": [F, m] i32 unburied points}."""
    r = _ensemble_run(structure, frames, chains, probe_radius, n_points, None, per_frame, device, radii)
    t = _ensemble_table(structure, r, ENSEMBLE_SASA_COLUMNS)
    return (t, {k: r[k] for k in ("total_sasa", "count")}) if per_frame else t


def get_sap_ensemble(structure: Structure, frames=None, chains: str = "", probe_radius: float = 1.4, n_points: int = 100, sap_radius: float = 5.0,
                     per_frame: bool = False, device: int = 0):
    """get_sasa_ensemble plus the SAP score of every frame averaged over the frames -- SAP as Chennamsetty et al. define it: mean_sap, std_sap,
    min_sap, max_sap (ENSEMBLE_SAP_COLUMNS; 0 for backbone atoms).  per_frame=True also returns "sap": [F, m] f32 among the extras."""
    r = _ensemble_run(structure, frames, chains, probe_radius, n_points, float(sap_radius), per_frame, device)
    t = _ensemble_table(structure, r, ENSEMBLE_SAP_COLUMNS)
    return (t, {k: r[k] for k in ("total_sasa", "count", "sap")}) if per_frame else t


def get_residue_sap_ensemble(structure: Structure, frames=None, chains: str = "", probe_radius: float = 1.4, n_points: int = 100,
                             sap_radius: float = 5.0, device: int = 0):
    """Residue-level time-averaged SAP: residue_sap_from_atoms on the per-atom means (mean_sasa, mean_sap) of get_sap_ensemble, plus n_frames."""
    import pyarrow as pa

    r = _ensemble_run(structure, frames, chains, probe_radius, n_points, float(sap_radius), False, device)
    idx = r["atoms"]
    cols = residue_sap_from_atoms(_strings(structure, "chain", idx), _strings(structure, "resn", idx), structure.ints("resi")[idx],
                                  _strings(structure, "insertion", idx), r["mean_sasa"], r["mean_sap"])
    types = {"chain": pa.string(), "resn": pa.string(), "resi": pa.int32(), "insertion": pa.string()}
    out = {k: pa.array(v, types.get(k, pa.float32())) for k, v in cols.items()}
    out["n_frames"] = pa.array(np.full(len(cols["resi"]), r["n_frames"], "<u4"), pa.uint32())
    return _frame(out)


def sasa_ensemble(input_file: str, probe_radius: float = 1.4, n_points: int = 100, chains: str = "", level: str = "atom", radii=None):
    """SASA statistics across the models of a multi-model file (NMR models, MODEL-record snapshots): see get_sasa_ensemble.  With a named radius
    table (radii "protor" / "vdw") level "residue" gives get_residue_sasa_ensemble's table and level "chain" one row per chain with the mean,
    spread and extremes of its per-frame sums; without one only level "atom" is offered, as in sasa()."""
    lv = str(level).lower()
    if lv not in SASA_LEVELS:
        raise ValueError(f"Invalid level '{level}'. Must be one of: 'atom', 'residue', 'chain'")
    if radii is not None:
        _radii_table(radii)
    elif lv != "atom":
        raise NotImplementedError(f"sasa level '{lv}' needs a named radius table: pass radii='protor' or radii='vdw'")
    s = Structure.load(input_file)
    if lv == "atom":
        return get_sasa_ensemble(s, None, chains, probe_radius, n_points, radii=radii)
    table, extras = get_residue_sasa_ensemble(s, None, chains, probe_radius, n_points, radii)
    return table if lv == "residue" else _chain_ensemble_table(extras, len(extras["chain_sasa"]))


def _chain_ensemble_table(extras: dict, n_frames: int):
    """One row per chain from the per-frame chain sums: f64 statistics over the frames, rounded to f32 once."""
    import pyarrow as pa

    v = np.asarray(extras["chain_sasa"], np.float64).reshape(n_frames, len(extras["chains"]))
    f32 = lambda a: pa.array(np.asarray(a, np.float64).astype(np.float32), pa.float32())  # noqa: E731
    return _frame({"chain": pa.array(extras["chains"], pa.string()), "mean_sasa": f32(v.mean(0)), "std_sasa": f32(v.std(0)), "min_sasa": f32(v.min(0)),
                   "max_sasa": f32(v.max(0)), "n_frames": pa.array(np.full(v.shape[1], n_frames, "<u4"), pa.uint32())})


def sap_ensemble(input_file: str, level: str = "residue", probe_radius: float = 1.4, n_points: int = 100, sap_radius: float = 5.0, chains: str = ""):
    """SAP averaged across the models of a multi-model file, per atom or per residue: see get_sap_ensemble / get_residue_sap_ensemble."""
    lv = str(level).lower()
    if lv not in SAP_LEVELS:
        raise ValueError(f"Invalid level '{level}'. Must be one of: 'atom', 'residue'")
    f = get_sap_ensemble if lv == "atom" else get_residue_sap_ensemble
    return f(Structure.load(input_file), None, chains, probe_radius, n_points, sap_radius)


def _sc_dict(r: _lib.arp_sc_results) -> dict:
    surf = lambda s: {k: (int(getattr(s, k)) if k.startswith("n_") else float(getattr(s, k))) for k, _ in _lib.arp_sc_surface._fields_}
    out = {"surfaces": [surf(r.surface[0]), surf(r.surface[1])], "combined": surf(r.combined)}
    out.update({k: int(getattr(r, k)) for k in ("n_convex", "n_toroidal", "n_concave", "n_probes")})
    out.update({k: float(getattr(r, k)) for k in ("sc", "distance", "area")})
    return out


def sc_radius(resn: str, atomn: str, element: str = "") -> float:
    """Lawrence & Colman radius of (residue, atom) from the reference's table, else the element's van der Waals radius; 0 if none."""
    return float(lib.arp_sc_radius(resn.encode(), atomn.encode(), element.encode()))


def sc_select(structure: Structure, groups: str, model_num: int = 0):
    """(structure atom indices, molecule 0/1) that get_sc works on (mod.rs:51-80; arp_structure_sc_select)."""
    m = max(structure.n_atoms, 1)
    atoms, mol, n = np.zeros(m, dtype="<u4"), np.zeros(m, dtype=np.uint8), C.c_uint64()
    _check(lib.arp_structure_sc_select(structure._h, groups.encode(), int(model_num), C.byref(n), atoms.ctypes.data_as(C.POINTER(C.c_uint32)),
                                       mol.ctypes.data_as(C.POINTER(C.c_uint8))))
    return atoms[: n.value].copy(), mol[: n.value].copy()


def sc_arrays(ctx: Context, x, y, z, radius, molecule, serial=None, settings: dict | None = None) -> dict:
    """arp_sc on raw arrays: molecule 0/1 per atom, serial None = the index.  Returns the results dict of get_sc_results."""
    x, y, z, r = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, z, radius))
    mol = np.ascontiguousarray(molecule, dtype=np.uint8)
    ser = None if serial is None else np.ascontiguousarray(serial, dtype=np.int64)
    st = _lib.arp_sc_settings()
    lib.arp_sc_default_settings(C.byref(st))
    for k, v in (settings or {}).items():
        setattr(st, k, float(v))
    res = _lib.arp_sc_results()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    _check(lib.arp_sc(ctx._h, len(x), dp(x), dp(y), dp(z), dp(r), mol.ctypes.data_as(C.POINTER(C.c_uint8)),
                      None if ser is None else ser.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(st), C.byref(res)))
    return _sc_dict(res)


def sc_dots(ctx: Context, surface: int) -> dict:
    """The dots of one surface of ctx's last SC call (arp_sc_dots): xyz, normal, area, flags, nn_dist, score."""
    n = C.c_uint64()
    _check(lib.arp_sc_dots(ctx._h, int(surface), 0, C.byref(n), None, None, None, None, None, None))
    m = n.value
    d = {"xyz": np.zeros((m, 3)), "normal": np.zeros((m, 3)), "area": np.zeros(m), "flags": np.zeros(m, dtype="<u4"), "nn_dist": np.zeros(m),
         "score": np.zeros(m)}
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    _check(lib.arp_sc_dots(ctx._h, int(surface), m, C.byref(n), dp(d["xyz"]), dp(d["normal"]), dp(d["area"]),
                           d["flags"].ctypes.data_as(C.POINTER(C.c_uint32)), dp(d["nn_dist"]), dp(d["score"])))
    return d


def get_sc_results(structure: Structure, groups: str, model_num: int = 0, device: int = 0) -> dict:
    """Every result of `get_sc` (mod.rs:51-80): per surface, combined, dot and probe counts, sc, distance, area."""
    res = _lib.arp_sc_results()
    _check(lib.arp_structure_sc(_context(device)._h, structure._h, groups.encode(), int(model_num), C.byref(res)))
    return _sc_dict(res)


def get_sc(structure: Structure, groups: str, model_num: int = 0, device: int = 0) -> float:
    """`arpeggia::get_sc`: the shape complementarity of the two chain groups."""
    return get_sc_results(structure, groups, model_num, device)["sc"]


def sc(input_file: str, groups: str, model_num: int = 0, num_threads: int = 0) -> float:
    """Drop-in for `arpeggia.sc` (python.rs:369-381): raises RuntimeError("SC calculation failed: ...") on failure."""
    del num_threads
    try:
        return get_sc(Structure.load(input_file), groups, model_num)
    except ArpeggiaError as e:
        raise RuntimeError(f"SC calculation failed: {e}") from e


# ---- shape complementarity across the frames of an ensemble (include/arpeggia_amd.h arp_sc_ensemble; no counterpart in the reference) ----
SC_FRAME_STATUS = ["ok", "no_dots", "coincident", "sampling_limit"]  # ARP_SC_FRAME_*
_SC_SURFACE_STATS = ["n_all_dots", "n_trimmed_dots", "trimmed_area", "d_median", "s_median", "d_mean", "s_mean"]
SC_FRAME_COLUMNS = ["frame", "status", "sc", "distance", "area"] + [f"{k}_{m}" for k in _SC_SURFACE_STATS for m in (1, 2)] + \
                   ["n_probes", "n_convex", "n_toroidal", "n_concave"]
SC_ENSEMBLE_COLUMNS = ["chain", "resn", "resi", "insertion", "altloc", "atomn", "atomi", "molecule", "n_frames", "occupancy", "mean_trimmed_dots"]
_SC_SURFACE_DT = np.dtype([(k, "<u8" if t is C.c_uint64 else "<f8") for k, t in _lib.arp_sc_surface._fields_])
SC_RESULTS_DTYPE = np.dtype([("surface", _SC_SURFACE_DT, (2,)), ("combined", _SC_SURFACE_DT)] +
                            [(k, "<u8") for k in ("n_convex", "n_toroidal", "n_concave", "n_probes")] + [(k, "<f8") for k in ("sc", "distance", "area")])
assert SC_RESULTS_DTYPE.itemsize == C.sizeof(_lib.arp_sc_results)


def _sc_ens_out(F: int, n: int):
    res = np.zeros(max(F, 1), SC_RESULTS_DTYPE)
    status, err = np.zeros(max(F, 1), "<u4"), np.zeros((max(F, 1), 2), "<u4")
    fi, td = np.zeros(max(n, 1), "<u4"), np.zeros(max(n, 1), "<u8")
    up = C.POINTER(C.c_uint32)
    ptrs = (res.ctypes.data_as(C.POINTER(_lib.arp_sc_results)), status.ctypes.data_as(up), err.ctypes.data_as(up), fi.ctypes.data_as(up),
            td.ctypes.data_as(C.POINTER(C.c_uint64)))
    return res, status, err, fi, td, ptrs


def sc_arrays_ensemble(ctx: "Context | None", xyz, radius, molecule, serial=None, settings: dict | None = None) -> dict:
    """arp_sc_ensemble on raw arrays: xyz [F, n, 3], radius / molecule / serial [n] as sc_arrays takes them.  Returns results (a structured
    array of F arp_sc_results, SC_RESULTS_DTYPE), status [F] (indices into SC_FRAME_STATUS), err_atoms [F, 2] (the coincident pair, ~0 elsewhere),
    frames_in_interface [n] u32 and trimmed_dots [n] u64 (over the frames with status ok).  ctx None: the inputs are only checked."""
    xyz = np.ascontiguousarray(xyz, dtype="<f8")
    r = np.ascontiguousarray(radius, dtype=np.float64)
    mol = np.ascontiguousarray(molecule, dtype=np.uint8)
    if xyz.ndim != 3 or xyz.shape[1:] != (len(r), 3) or len(mol) != len(r):
        raise ArpeggiaError(_lib.ARP_ERR_BAD_INPUT, f"sc ensemble: xyz must have shape [F, {len(r)}, 3] (one row per radius), got {list(xyz.shape)}")
    ser = None if serial is None else np.ascontiguousarray(serial, dtype=np.int64)
    st = _lib.arp_sc_settings()
    lib.arp_sc_default_settings(C.byref(st))
    for k, v in (settings or {}).items():
        setattr(st, k, float(v))
    F, n = xyz.shape[0], len(r)
    res, status, err, fi, td, ptrs = _sc_ens_out(F, n)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    src = xyz if xyz.size else np.zeros(1)
    _check(lib.arp_sc_ensemble(None if ctx is None else ctx._h, n, F, dp(src), dp(r), mol.ctypes.data_as(C.POINTER(C.c_uint8)),
                               None if ser is None else ser.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(st), *ptrs))
    return {"n_frames": F, "results": res[:F], "status": status[:F], "err_atoms": err[:F], "frames_in_interface": fi[:n], "trimmed_dots": td[:n]}


def _sc_ensemble(ctx: "Context | None", structure: Structure, frames, groups: str) -> dict:
    """arp_structure_sc_ensemble.  ctx None: the inputs are only checked (raises their error); the result then holds atoms, molecule and n_frames."""
    n_frames, ptr, keep = _frames_arg(structure, frames, "sc ensemble")
    rows, used = C.c_uint64(), C.c_uint64()
    n = max(structure.n_atoms, 1)
    atoms, mol = np.zeros(n, "<u4"), np.zeros(n, np.uint8)
    head = (structure._h, int(n_frames), ptr, groups.encode(), C.byref(rows), C.byref(used), atoms.ctypes.data_as(C.POINTER(C.c_uint32)),
            mol.ctypes.data_as(C.POINTER(C.c_uint8)))
    if ctx is None:
        _check(lib.arp_structure_sc_ensemble(None, *head, *([None] * 5)))
        m = int(rows.value)
        return {"atoms": atoms[:m].copy(), "molecule": mol[:m].copy(), "n_frames": int(used.value)}
    n_top = _topology_atoms(structure)
    f_cap = n_frames if frames is not None else (structure.n_atoms // n_top if n_top else 1)
    res, status, err, fi, td, ptrs = _sc_ens_out(f_cap, n_top)
    _check(lib.arp_structure_sc_ensemble(ctx._h, *head, *ptrs))
    del keep
    m, F = int(rows.value), int(used.value)
    return {"atoms": atoms[:m].copy(), "molecule": mol[:m].copy(), "n_frames": F, "results": res[:F], "status": status[:F], "err_atoms": err[:F],
            "frames_in_interface": fi[:m].copy(), "trimmed_dots": td[:m].copy()}


def sc_frame_table(results, status):
    """The per-frame table of get_sc_ensemble (SC_FRAME_COLUMNS) from the results and status arrays of an ensemble call."""
    import pyarrow as pa

    res, status = np.asarray(results), np.asarray(status)
    bad = status != 0
    f64 = lambda a: pa.array(np.ascontiguousarray(a, np.float64), pa.float64(), mask=bad)
    cols = {"frame": pa.array(np.arange(len(res), dtype="<u4"), pa.uint32()), "status": pa.array([SC_FRAME_STATUS[int(k)] for k in status], pa.utf8())}
    for k in ("sc", "distance", "area"):
        cols[k] = f64(res[k])
    for k in _SC_SURFACE_STATS:
        for m in (0, 1):
            v = res["surface"][k][:, m]
            cols[f"{k}_{m + 1}"] = pa.array(np.ascontiguousarray(v), pa.uint64()) if k.startswith("n_") else f64(v)
    for k in ("n_probes", "n_convex", "n_toroidal", "n_concave"):
        cols[k] = pa.array(np.ascontiguousarray(res[k]), pa.uint64())
    return _frame(cols)


def get_sc_ensemble(structure: Structure, frames=None, groups: str = "/", device: int = 0):
    """Shape complementarity across the frames of an ensemble, every frame of a pass in one set of launches: returns (frame_table, atom_table).
    frame_table (SC_FRAME_COLUMNS): frame, status (SC_FRAME_STATUS), sc, distance, area, the statistics of the two surfaces (_1, _2) and the
    probe and dot counts; a frame whose SC fails is a row with its status and nulls in the float columns.  atom_table (SC_ENSEMBLE_COLUMNS): one
    row per selected atom with the identity columns, molecule (0 / 1), n_frames (the frames that succeeded), occupancy = the share of those in
    which the atom owns a trimmed dot (f64) and mean_trimmed_dots; both null when no frame succeeded.  frames: [F, N, 3] f64 coordinates of the N
    atoms of model 0; None: the structure's models are the frames."""
    import pyarrow as pa

    ctx = _with_context(device, lambda: _sc_ensemble(None, structure, frames, groups))
    r = ctx.sc_ensemble(structure, frames, groups)
    ft = sc_frame_table(r["results"], r["status"])
    n_ok = int(np.count_nonzero(r["status"] == 0))
    m = len(r["atoms"])
    ident = _identity(structure, r["atoms"])
    cols = {k: ident[k] for k in SC_ENSEMBLE_COLUMNS[:7]}
    cols["molecule"] = pa.array(r["molecule"], pa.uint8())
    cols["n_frames"] = pa.array(np.full(m, n_ok, "<u4"), pa.uint32())
    none = np.full(m, n_ok == 0)
    cols["occupancy"] = pa.array(r["frames_in_interface"].astype(np.float64) / float(max(n_ok, 1)), pa.float64(), mask=none)
    cols["mean_trimmed_dots"] = pa.array(r["trimmed_dots"].astype(np.float64) / float(max(n_ok, 1)), pa.float64(), mask=none)
    return ft, _frame(cols)


def sc_ensemble(input_file: str, groups: str):
    """Shape complementarity across the models of a multi-model file: see get_sc_ensemble."""
    return get_sc_ensemble(Structure.load(input_file), None, groups)


def sc_dot_atoms(ctx: Context, surface: int) -> np.ndarray:
    """The owner atom (index into the call's atoms) of every dot of one surface of ctx's last SC call, in sc_dots' order (arp_sc_dot_atoms)."""
    n = C.c_uint64()
    _check(lib.arp_sc_dot_atoms(ctx._h, int(surface), 0, C.byref(n), None))
    a = np.zeros(max(n.value, 1), "<u4")
    _check(lib.arp_sc_dot_atoms(ctx._h, int(surface), n.value, C.byref(n), a.ctypes.data_as(C.POINTER(C.c_uint32))))
    return a[: n.value]


def sc_dot_stats(seg_start, flags, area, nn_dist, score, other, device: int | None = None) -> np.ndarray:
    """The statistics of dot segments as the ensemble call forms them: segment s = dots [seg_start[s], seg_start[s + 1]); a dot counts when its
    flags have ARP_SC_DOT_TRIMMED (8); other[s] = the segment whose trimmed dots must exist for the means and medians of s.  Returns a structured
    array, one arp_sc_surface per segment (n_all_dots, n_trimmed_dots, trimmed_area, d_mean, d_median, s_mean, s_median; the atom counts zero).
    device None: arp_sc_dot_stats_host, the restatement on the CPU; a device number: arp_sc_dot_stats, the kernel.  The twins are bit-identical."""
    start = np.ascontiguousarray(seg_start, dtype="<u8")
    fl = np.ascontiguousarray(flags, dtype="<u4")
    cols = [np.ascontiguousarray(a, dtype="<f8") for a in (area, nn_dist, score)]
    oth = np.ascontiguousarray(other, dtype="<u4")
    n_seg = len(oth)
    if len(start) != n_seg + 1 or any(len(a) != len(fl) for a in cols) or (n_seg and int(start[-1]) != len(fl)):
        raise ArpeggiaError(_lib.ARP_ERR_BAD_INPUT, "sc_dot_stats: seg_start needs one more entry than other, its last entry the length of the dot columns")
    out = np.zeros(max(n_seg, 1), _SC_SURFACE_DT)
    pad = lambda a: a if a.size else np.zeros(1, a.dtype)
    dp = lambda a: pad(a).ctypes.data_as(C.POINTER(C.c_double))
    args = (n_seg, start.ctypes.data_as(C.POINTER(C.c_uint64)), pad(fl).ctypes.data_as(C.POINTER(C.c_uint32)), *(dp(a) for a in cols),
            pad(oth).ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(C.POINTER(_lib.arp_sc_surface)))
    if device is None:
        _check(lib.arp_sc_dot_stats_host(*args))
    else:
        _check(lib.arp_sc_dot_stats(_context(int(device))._h, *args))
    return out[:n_seg]
