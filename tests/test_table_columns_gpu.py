"""What every kind of table serves by name (arp_table_column) and shows as an Arrow batch (arp_table_export_arrow), kind by kind on 1ubq: the
contact table, the frequency tables of both levels with and without ring rows, the timeline tables with and without their bitmap, the similarity
tables.  The vocabulary is probed in full -- every name any kind serves is asked of every kind, and is served with its width or refused -- and
every Arrow column is compared with the accessor's values.  Generalises test_gpu_parity.py::test_arrow_export_equals_the_column_accessors."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import arpeggia_amd as aa
from arpeggia_amd import _lib
from arpeggia_amd import api
from arpeggia_amd._lib import lib

pytestmark = pytest.mark.gpu

SIDE_WIDTHS = {"chain": 8, "resn": 8, "atomn": 8, "insertion": 4, "altloc": 4, "resi": 4, "atomi": 4, "atom": 4, "ring": 4, "residue": 4}
STATS = ["n_frames", "frequency", "min_distance", "max_distance"]
TIMELINE = [c for c, _ in aa.TIMELINE_COLUMNS]


def _sides(fields):
    return {f"{side}_{f}": SIDE_WIDTHS[f] for side in ("from", "to") for f in fields}


CONTACT = {"model": 4, "interaction": 4, "distance": 4, **_sides(["chain", "resn", "atomn", "insertion", "altloc", "resi", "atomi", "atom"]),
           "sc_centroid_dist": 4, "sc_dihedral": 4, "sc_centroid_angle": 4, "sc_valid": 1}
ATOM_FREQ = {"interaction": 4, **_sides(["chain", "resn", "atomn", "insertion", "altloc", "resi", "atomi", "atom", "ring"]), **{c: 4 for c in STATS}}
RESIDUE_FREQ = {"interaction": 4, **_sides(["chain", "resn", "insertion", "resi", "residue"]), **{c: 4 for c in STATS}}
VOCABULARY = sorted(set(CONTACT) | set(ATOM_FREQ) | set(RESIDUE_FREQ) | set(TIMELINE))

# kind -> (how the table is made, the names it serves with their widths, the columns of its batch)
KINDS = {
    "contacts": ("contacts", {}, CONTACT, aa.TABLE_COLUMNS),
    "freq-atom": ("freq", dict(level="atom", rings=False), ATOM_FREQ, aa.FREQ_COLUMNS),
    "freq-atom-rings": ("freq", dict(level="atom", rings=True), ATOM_FREQ, aa.FREQ_COLUMNS),
    "freq-residue": ("freq", dict(level="residue", rings=False), RESIDUE_FREQ, aa.RESIDUE_FREQ_COLUMNS),
    "freq-residue-rings": ("freq", dict(level="residue", rings=True), RESIDUE_FREQ, aa.RESIDUE_FREQ_COLUMNS),
    "timeline-atom-bitmap": ("timeline", dict(level="atom", rings=True, bitmap=True), {**ATOM_FREQ, **{c: 4 for c in TIMELINE}}, aa.FREQ_COLUMNS + aa.TIMELINE_COLUMNS),
    "timeline-residue-no-bitmap": ("timeline", dict(level="residue", rings=False, bitmap=False), {**RESIDUE_FREQ, **{c: 4 for c in TIMELINE}},
                                   aa.RESIDUE_FREQ_COLUMNS + aa.TIMELINE_COLUMNS),
    "timeline-atom-no-bitmap": ("timeline", dict(level="atom", rings=False, bitmap=False), {**ATOM_FREQ, **{c: 4 for c in TIMELINE}}, aa.FREQ_COLUMNS + aa.TIMELINE_COLUMNS),
    "timeline-residue-bitmap": ("timeline", dict(level="residue", rings=True, bitmap=True), {**RESIDUE_FREQ, **{c: 4 for c in TIMELINE}},
                                aa.RESIDUE_FREQ_COLUMNS + aa.TIMELINE_COLUMNS),
    "similarity-atom": ("similarity", dict(level="atom", rings=True, axis="frames", metric="tanimoto"), ATOM_FREQ, aa.FREQ_COLUMNS),
    "similarity-residue": ("similarity", dict(level="residue", rings=False, axis="rows", metric="count"), RESIDUE_FREQ, aa.RESIDUE_FREQ_COLUMNS),
}


@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.load_model(ubq_path)


@pytest.fixture(scope="module")
def frames(ubq):
    """three jittered copies of 1ubq, as the ensemble tests build them"""
    soa = ubq.soa("/")
    base = np.stack([soa["x"], soa["y"], soa["z"]], 1)
    return base[None] + np.random.default_rng(7).normal(scale=0.3, size=(3, len(base), 3))


def _make(ctx, s, frames, how, kw):
    if how == "contacts":
        t = C.c_void_p()
        api._check(lib.arp_get_contacts(ctx._h, s._h, b"/", 0.1, 6.5, C.byref(t)))
        return t
    if how == "freq":
        return api._freq_table(ctx, s, frames, "/", 0.1, 6.5, kw["rings"], kw["level"])
    if how == "timeline":
        return api._timeline_table(ctx, s, frames, "/", 0.1, 6.5, kw["rings"], kw["level"], kw["bitmap"])
    return api._similarity_table(ctx, s, frames, "/", 0.1, 6.5, kw["rings"], kw["level"], kw["axis"], kw["metric"])


def _column(t, name, n, kind):
    w = C.c_int32(-1)
    p = lib.arp_table_column(t, name.encode(), C.byref(w))
    assert p, name
    dtype = "<i4" if name == "interaction" else f"S{w.value}" if kind == "str" else "u1" if name == "sc_valid" else "<" + kind
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n * w.value,)).view(dtype).copy()


def _arrow(t):
    import pyarrow as pa

    arr, sch = _lib.ArrowArray(), _lib.ArrowSchema()
    api._check(lib.arp_table_export_arrow(t, C.byref(arr), C.byref(sch)))
    return pa.RecordBatch._import_from_c(C.addressof(arr), C.addressof(sch))


def _check_batch_layout(batch, columns):
    import pyarrow as pa

    types = {"str": pa.string(), "u4": pa.uint32(), "i4": pa.int32(), "f4": pa.float32()}
    assert batch.schema.names == [c for c, _ in columns]
    for name, kind in columns:
        field = batch.schema.field(name)
        assert field.type == types[kind], name
        assert field.nullable == name.startswith("sc_"), name


@pytest.mark.parametrize("kind", list(KINDS))
def test_columns_and_arrow_batch(ctx, ubq, frames, kind):
    how, kw, served, columns = KINDS[kind]
    t = _make(ctx, ubq, frames, how, kw)
    try:
        n = int(lib.arp_table_rows(t))
        assert n > 0
        # the vocabulary: served with its width, or refused
        for name in VOCABULARY + ["nonsense", "from_", "sc_"]:
            w = C.c_int32(-1)
            p = lib.arp_table_column(t, name.encode(), C.byref(w))
            if name in served:
                assert p and w.value == served[name], (name, w.value)
            else:
                assert not p, name
        # the batch: names, order, types; every column equal to the accessor's values
        batch = _arrow(t)
        assert batch.num_rows == n
        _check_batch_layout(batch, columns)
        sc_valid = _column(t, "sc_valid", n, "u1").astype(bool) if how == "contacts" else None
        for name, ckind in columns:
            got = batch.column(name)
            col = _column(t, name, n, ckind)
            if name == "interaction":
                want = [_lib.INTERACTIONS[k] for k in col]
            elif ckind == "str":
                want = [v.decode() for v in col]
            elif name.startswith("sc_"):
                want = [float(v) if ok else None for v, ok in zip(col, sc_valid)]
                assert got.null_count == int((~sc_valid).sum()) and got.null_count > 0
            else:
                want = col.tolist()
            if not name.startswith("sc_"):
                assert got.null_count == 0, name
            assert got.to_pylist() == want, name
        if "from_ring" in served:  # a side is a ring entity (atomn "Ring", atomi 0, no atom index) exactly where its ring index says so
            for side in ("from", "to"):
                ring = _column(t, f"{side}_ring", n, "i4") >= 0
                assert np.array_equal(ring, _column(t, f"{side}_atomn", n, "str") == b"Ring") and np.array_equal(ring, _column(t, f"{side}_atom", n, "i4") < 0)
                assert not ring.any() or kw["rings"]
        batch.validate(full=True)
        # what rides along with the kinds that have it
        wpr, nf = C.c_uint64(), C.c_uint64()
        assert bool(lib.arp_table_timeline(t, C.byref(wpr), C.byref(nf))) == bool(kw.get("bitmap"))
        if kw.get("bitmap"):
            assert (wpr.value, nf.value) == (1, 3)
        m, flags, sizes = C.c_uint64(), C.c_uint32(), C.POINTER(C.c_uint32)()
        assert bool(lib.arp_table_similarity(t, C.byref(m), C.byref(flags), C.byref(sizes))) == (how == "similarity")
        if how == "similarity":
            assert m.value == (n if kw["axis"] == "rows" else 3)
    finally:
        lib.arp_table_free(t)


def test_table_without_rows(ctx, ubq):
    """a frequency table with no rows (the frames blown up tenfold, as test_freq_gpu.py builds its empty one): names and order hold"""
    soa = ubq.soa("/")
    far = (np.stack([soa["x"], soa["y"], soa["z"]], 1) * 10.0)[None].repeat(3, 0)
    for level, columns in (("atom", aa.FREQ_COLUMNS), ("residue", aa.RESIDUE_FREQ_COLUMNS)):
        t = api._freq_table(ctx, ubq, far, "/", 0.1, 6.5, False, level)
        try:
            assert int(lib.arp_table_rows(t)) == 0
            batch = _arrow(t)
            assert batch.num_rows == 0
            _check_batch_layout(batch, columns)
            batch.validate(full=True)
        finally:
            lib.arp_table_free(t)
