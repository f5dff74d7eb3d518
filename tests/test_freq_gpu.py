"""Contact frequencies across frames (arp_contact_frequencies) on the device, against per-frame atomic_contacts aggregated in numpy.

The per-frame pair lists come from Context.atomic_contacts on the topology with that frame's coordinates -- the path the oracle pins -- so
every column is checked for exact equality, row order included.
"""
from __future__ import annotations

import numpy as np
import pytest

import arpeggia_amd as aa
import synth
from arpeggia_amd import _lib
from freq_common import RING_CODES, assert_table_equal, expected, to_bytes  # noqa: F401

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def ctx():
    return aa.Context(0)


@pytest.fixture(autouse=True)
def _reset_chunk():
    yield
    aa.debug_set("freq_chunk_atoms", 0)


def topology_xyz(s: aa.Structure, n: int) -> np.ndarray:
    soa = s.soa("/")
    return np.stack([soa["x"][:n], soa["y"][:n], soa["z"][:n]], 1)


def jittered(s: aa.Structure, n_frames: int, seed: int, sigma: float = 0.3) -> np.ndarray:
    n = aa.api._topology_atoms(s)
    base = topology_xyz(s, n)
    rng = np.random.default_rng(seed)
    return base[None] + rng.normal(scale=sigma, size=(n_frames, n, 3))


@pytest.fixture(scope="module")
def ubq(ubq_path):
    return aa.load_model(ubq_path)


@pytest.fixture(scope="module")
def bft(bft_path):
    return aa.load_model(bft_path)


@pytest.fixture(scope="module")
def stress():
    return aa.Structure.from_records(synth.gen_stress(n_res=120, seed=11, hydrogens=True, altlocs=True))


@pytest.mark.parametrize("which,groups", [("ubq", "/"), ("bft", "/"), ("bft", "H,L/C")])
def test_single_frame(ctx, request, which, groups):
    s = request.getfixturevalue(which)
    frames = topology_xyz(s, s.n_atoms)[None]
    got = ctx.contact_frequencies(s, frames, groups)
    want = expected(ctx, s, frames, groups)
    assert_table_equal(got, want)
    assert len(got["n_frames"]) > 0
    assert (got["n_frames"] == 1).all() and (got["frequency"] == 1.0).all() and np.array_equal(got["min_distance"], got["max_distance"])


CASES = [("ubq", 64, "/", 25), ("bft", 16, "/", 5), ("bft", 16, "H,L/C", 5), ("bft", 16, "A,B,C/G,H,L", 5), ("stress", 32, "/", 10)]


@pytest.mark.parametrize("which,F,groups,per", CASES)
def test_jittered_frames_and_chunks(ctx, request, which, F, groups, per):
    s = request.getfixturevalue(which)
    frames = jittered(s, F, seed=F + len(groups))
    want = expected(ctx, s, frames, groups)
    got = ctx.contact_frequencies(s, frames, groups)
    assert_table_equal(got, want)
    f = got["frequency"]
    assert ((f > 0) & (f < 1)).any() and (f == 1).any()
    # several passes with a partial last one: per frames each, F % per != 0
    assert F % per and -(-F // per) >= 3
    aa.debug_set("freq_chunk_atoms", per * frames.shape[1])
    chunked = ctx.contact_frequencies(s, frames, groups)
    assert to_bytes(chunked) == to_bytes(got)


def test_two_thousand_frames(ctx, ubq):
    frames = jittered(ubq, 2000, seed=2000)
    got = ctx.contact_frequencies(ubq, frames, "/")
    assert_table_equal(got, expected(ctx, ubq, frames, "/"))


def test_model_file_matches_arrays_and_get_contacts(ctx, tmp_path, ubq_path):
    rec = synth.read_pdb_records(ubq_path)
    F = 8
    rng = np.random.default_rng(8)
    parts = []
    for m in range(F):
        r = {k: v.copy() for k, v in rec.items()}
        for ax in ("x", "y", "z"):
            r[ax] = np.round(r[ax] + rng.normal(scale=0.3, size=len(r[ax])), 3)
        r["model_serial"][:] = m + 1
        parts.append(r)
    multi = {k: np.concatenate([p[k] for p in parts]) for k in rec}
    path = tmp_path / "ubq_models.pdb"
    synth.write_pdb(multi, path)
    s = aa.load_model(str(path))
    n = aa.api._topology_atoms(s)
    assert s.n_atoms == F * n
    soa = s.soa("/")
    frames = np.stack([soa["x"], soa["y"], soa["z"]], 1).reshape(F, n, 3)
    from_models = ctx.contact_frequencies(s, None, "/")
    from_arrays = ctx.contact_frequencies(s, frames, "/")
    assert to_bytes(from_models) == to_bytes(from_arrays)
    assert_table_equal(from_models, expected(ctx, s, frames, "/"))
    # the reference-pinned table on the same file: its atom-atom rows grouped by (atom i, atom j, interaction)
    t = ctx.get_contacts(s, "/", 0.1, 6.5)
    atom_rows = (t["from_atom"] >= 0) & (t["to_atom"] >= 0)
    key = ((t["from_atom"][atom_rows] % n).astype(np.uint64) << np.uint64(34)) | ((t["to_atom"][atom_rows] % n).astype(np.uint64) << np.uint64(5)) \
        | t["interaction"][atom_rows].astype(np.uint64)
    d = t["distance"][atom_rows]
    uk, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    mn = np.full(len(uk), np.inf, np.float32); np.minimum.at(mn, inv, d)
    mx = np.full(len(uk), -np.inf, np.float32); np.maximum.at(mx, inv, d)
    got_key = (from_models["from_atom"].astype(np.uint64) << np.uint64(34)) | (from_models["to_atom"].astype(np.uint64) << np.uint64(5)) \
        | from_models["interaction"].astype(np.uint64)
    assert np.array_equal(got_key, uk)
    assert np.array_equal(from_models["n_frames"], cnt.astype(np.uint32))
    assert np.array_equal(from_models["min_distance"], mn) and np.array_equal(from_models["max_distance"], mx)
    assert np.array_equal(from_models["from_chain"], t["from_chain"][atom_rows][np.unique(key, return_index=True)[1]])


def test_determinism(ctx, bft):
    frames = jittered(bft, 16, seed=3)
    a = ctx.contact_frequencies(bft, frames, "/")
    b = ctx.contact_frequencies(bft, frames, "/")
    assert to_bytes(a) == to_bytes(b)
    ta, tb = aa.get_contact_frequencies(bft, frames, "/"), aa.get_contact_frequencies(bft, frames, "/")
    assert ta.equals(tb)


def test_no_contacts(ctx, ubq):
    frames = (topology_xyz(ubq, ubq.n_atoms) * 10.0)[None].repeat(3, 0)
    got = ctx.contact_frequencies(ubq, frames, "/")
    assert set(got) == {c for c, _ in aa.FREQ_COLUMNS} | {"from_atom", "to_atom"}
    assert all(len(v) == 0 for v in got.values())
    t = aa.get_contact_frequencies(ubq, frames, "/")
    assert len(t) == 0 and list(t.column_names if hasattr(t, "column_names") else t.columns) == [c for c, _ in aa.FREQ_COLUMNS]


def test_table_types_and_arrow(ctx, bft):
    frames = jittered(bft, 4, seed=5)
    t = aa.get_contact_frequencies(bft, frames, "H,L/C")
    cols = ctx.contact_frequencies(bft, frames, "H,L/C")
    import pyarrow as pa

    arrow = t if isinstance(t, pa.Table) else t.to_arrow()
    assert arrow.column_names == [c for c, _ in aa.FREQ_COLUMNS]
    assert arrow.schema.field("n_frames").type == pa.uint32() and arrow.schema.field("frequency").type == pa.float32()
    assert arrow.column("interaction").to_pylist() == [_lib.INTERACTIONS[c] for c in cols["interaction"]]
    assert arrow.column("from_chain").to_pylist() == [v.decode() for v in cols["from_chain"]]
    assert np.array_equal(arrow.column("min_distance").to_numpy(), cols["min_distance"])


def test_cli_end_to_end(tmp_path, ubq_path):
    from arpeggia_amd.__main__ import main

    rec = synth.read_pdb_records(ubq_path)
    rng = np.random.default_rng(4)
    parts = []
    for m in range(3):
        r = {k: v.copy() for k, v in rec.items()}
        r["x"] = np.round(r["x"] + rng.normal(scale=0.3, size=len(r["x"])), 3)
        r["model_serial"][:] = m + 1
        parts.append(r)
    path = tmp_path / "m3.pdb"
    synth.write_pdb({k: np.concatenate([p[k] for p in parts]) for k in rec}, path)
    out = tmp_path / "out"
    assert main(["contact-frequency", "-i", str(path), "-o", str(out)]) == 0
    import pyarrow.csv as pacsv

    csv = pacsv.read_csv(str(out / "contact_frequency.csv"))
    want = aa.contact_frequencies(str(path))
    assert csv.num_rows == len(want) > 0
    assert csv.column_names == [c for c, _ in aa.FREQ_COLUMNS]
