"""Helpers of the residue-level contact-frequency tests on the device (tests/test_freq_residue_gpu.py, tests/freq_residue_timing.py): the expected
table from one Context.atomic_contacts call per frame (as freq_common.expected, but keeping the frame) and, with rings, one Context.get_contacts
call per frame on the single-model structure that holds the frame's coordinates (as freq_common.device_reference), both grouped by residue in
numpy.  Expected values never come from the residue call itself."""
from __future__ import annotations

import numpy as np

import arpeggia_amd as aa
from arpeggia_amd import _lib

COLUMNS = [c for c, _ in aa.RESIDUE_FREQ_COLUMNS] + ["from_residue", "to_residue"]
RING_CODES = set(range(11, 18))


def topology_residues(s: aa.Structure, n: int):
    """(res [n]: the ingest's residue ordinal of every topology atom, first [n_res]: the first atom of every residue)."""
    res = s.soa("/")["res_id"][:n].astype(np.int64)
    order = np.argsort(res, kind="stable")
    first = order[np.concatenate([[True], np.diff(res[order]) != 0])]
    assert np.array_equal(res[first], np.arange(len(first)))
    return res, first


def atom_items(ctx, s: aa.Structure, frames: np.ndarray, groups: str, dist_cutoff: float = 6.5):
    """(i, j, code, frame, f32 distance) of every atom-atom item: one atomic_contacts call per frame on the topology with the frame's coordinates."""
    soa = s.soa(groups)
    F, n = frames.shape[0], frames.shape[1]
    nr = int(soa["res_id"][:n].max()) + 1 if n and len(soa["res_cb"]) else 0
    top = {k: soa[k][:n] for k in ("attr", "res_ord", "chain_rank", "model", "res_id")}
    top.update(res_h_ptr=soa["res_h_ptr"][: nr + 1] if nr else soa["res_h_ptr"][:0], res_cb=soa["res_cb"][:nr], res_sg=soa["res_sg"][:nr])
    nh = int(top["res_h_ptr"][-1]) if nr else 0
    top["res_h_idx"] = soa["res_h_idx"][:nh]
    out = [[], [], [], [], []]
    for f in range(F):
        d = dict(top, x=frames[f, :, 0].copy(), y=frames[f, :, 1].copy(), z=frames[f, :, 2].copy())
        p = ctx.atomic_contacts(d, aa.default_params(0.1, dist_cutoff))
        p = p[p["kind"] != 0]
        for code in range(len(_lib.INTERACTIONS)):
            q = p[(p["kind"] >> np.uint32(code)) & np.uint32(1) == 1]
            if len(q):
                assert code not in RING_CODES
                for k, v in enumerate((q["i"].astype(np.int64), q["j"].astype(np.int64), np.full(len(q), code, np.int64), np.full(len(q), f, np.int64), q["dist"])):
                    out[k].append(v)
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
    return cat(out[0], np.int64), cat(out[1], np.int64), cat(out[2], np.int64), cat(out[3], np.int64), cat(out[4], np.float32)


def ring_items(ctx, s: aa.Structure, rec: dict, frames: np.ndarray, groups: str, dist_cutoff: float = 6.5):
    """(A, B, code, frame, f32 distance) of every ring item, by residue: the rows with a Ring entity of Context.get_contacts on S_f, the residues
    looked up by (chain, resi, insertion) among the topology's atoms."""
    F, n = frames.shape[0], frames.shape[1]
    res, _ = topology_residues(s, n)
    chain, resi, ins = s.strings("chain")[:n], s.ints("resi")[:n], s.strings("insertion")[:n]
    of = {(bytes(chain[k]), int(resi[k]), bytes(ins[k])): int(res[k]) for k in range(n)}
    out = [[], [], [], [], []]
    for f in range(F):
        sf = aa.Structure.from_records(dict(rec, x=frames[f, :, 0].copy(), y=frames[f, :, 1].copy(), z=frames[f, :, 2].copy()))
        assert sf.n_atoms == n
        t = ctx.get_contacts(sf, groups, 0.1, dist_cutoff)
        for k in np.flatnonzero((t["from_atom"] < 0) | (t["to_atom"] < 0)):
            assert t["from_atomn"][k] == b"Ring" and int(t["interaction"][k]) in RING_CODES
            vals = (of[(bytes(t["from_chain"][k]), int(t["from_resi"][k]), bytes(t["from_insertion"][k]))],
                    of[(bytes(t["to_chain"][k]), int(t["to_resi"][k]), bytes(t["to_insertion"][k]))], int(t["interaction"][k]), f, t["distance"][k])
            for c, v in enumerate(vals):
                out[c].append(v)
    return (np.array(out[0], np.int64), np.array(out[1], np.int64), np.array(out[2], np.int64), np.array(out[3], np.int64), np.array(out[4], np.float32))


def group_by_residue(s: aa.Structure, F: int, n: int, A, B, code, frame, dist, rb: int = 29) -> dict:
    """Items by residue -> the residue frequency table: per (A, B, code, frame) the smallest distance, then per (A, B, code) the number of frames
    and the smallest and largest of those."""
    _, first = topology_residues(s, n)
    key = (A.astype(np.uint64) << np.uint64(rb + 5)) | (B.astype(np.uint64) << np.uint64(5)) | code.astype(np.uint64)
    order = np.lexsort((frame, key))
    key, frame, dist = key[order], frame[order], dist[order]
    new_sub = np.concatenate([[True], (key[1:] != key[:-1]) | (frame[1:] != frame[:-1])]) if len(key) else np.zeros(0, bool)
    sub = np.cumsum(new_sub) - 1
    cf = np.full(int(new_sub.sum()), np.inf, np.float32)
    np.minimum.at(cf, sub, dist)
    sub_key = key[new_sub]
    uk, inv, cnt = np.unique(sub_key, return_inverse=True, return_counts=True)
    mn, mx = np.full(len(uk), np.inf, np.float32), np.full(len(uk), -np.inf, np.float32)
    np.minimum.at(mn, inv, cf)
    np.maximum.at(mx, inv, cf)
    a = (uk >> np.uint64(rb + 5)).astype(np.int64)
    b = ((uk >> np.uint64(5)) & np.uint64((1 << rb) - 1)).astype(np.int64)
    out = {"interaction": (uk & np.uint64(31)).astype(np.int32), "from_residue": a.astype(np.int32), "to_residue": b.astype(np.int32),
           "n_frames": cnt.astype(np.uint32), "frequency": (cnt.astype(np.float64) / F).astype(np.float32), "min_distance": mn, "max_distance": mx}
    for side, idx in (("from", first[a]), ("to", first[b])):
        out[f"{side}_chain"] = s.strings("chain")[idx]
        out[f"{side}_resn"] = s.strings("resn")[idx]
        out[f"{side}_resi"] = s.ints("resi")[idx]
        out[f"{side}_insertion"] = s.strings("insertion")[idx]
    return out


def expected(ctx, s: aa.Structure, frames: np.ndarray, groups: str, rec: dict | None = None, dist_cutoff: float = 6.5) -> dict:
    """The residue frequency table by definition; rec (the topology's records) given: with the ring items."""
    F, n = frames.shape[0], frames.shape[1]
    res, _ = topology_residues(s, n)
    i, j, code, frame, dist = atom_items(ctx, s, frames, groups, dist_cutoff)
    A, B = res[i], res[j]
    if rec is not None:
        rA, rB, rcode, rframe, rdist = ring_items(ctx, s, rec, frames, groups, dist_cutoff)
        A, B, code, frame, dist = (np.concatenate(v) for v in ((A, rA), (B, rB), (code, rcode), (frame, rframe), (dist, rdist)))
    return group_by_residue(s, F, n, A, B, code, frame, dist)


def assert_same_table(got: dict, want: dict):
    """Every column, row order included, for equality (floats by their bits)."""
    assert set(got) == set(COLUMNS) and set(want) == set(COLUMNS), (sorted(got), sorted(want))
    for c in COLUMNS:
        assert len(got[c]) == len(want[c]), (c, len(got[c]), len(want[c]))
        if got[c].dtype.kind == "S":
            assert np.array_equal(got[c], want[c].astype(got[c].dtype)), c
        elif got[c].dtype.kind == "f":
            assert got[c].dtype == np.float32 and np.array_equal(got[c].view(np.uint32), want[c].astype(np.float32).view(np.uint32)), c
        else:
            assert np.array_equal(got[c], want[c].astype(got[c].dtype)), c


def to_bytes(t: dict) -> bytes:
    return b"".join(np.ascontiguousarray(t[c]).tobytes() for c in sorted(t))


def assert_consistent_with_atom_table(res_t: dict, atom_t: dict, res: np.ndarray, F: int, ring_res: np.ndarray | None = None):
    """The cross-checks against the atom-level call on the same input.  For every residue row: min_distance is the minimum of the atom table's
    min_distance over its group, and max(atom n_frames) <= n_frames <= min(F, sum of atom n_frames); the groups are exactly the residue rows.
    At F == 1 the whole table is the group-by of the atom table.  ring_res: the residue of every ring entity (tables with ring rows)."""
    ent = lambda atom, ring: np.where(atom >= 0, res[np.maximum(atom, 0)], ring_res[np.maximum(ring, 0)] if ring_res is not None else -1)
    none = np.full(len(atom_t["from_atom"]), -1)
    A = ent(atom_t["from_atom"], atom_t.get("from_ring", none))
    B = ent(atom_t["to_atom"], atom_t.get("to_ring", none))
    key = (A.astype(np.uint64) << np.uint64(34)) | (B.astype(np.uint64) << np.uint64(5)) | atom_t["interaction"].astype(np.uint64)
    uk, inv = np.unique(key, return_inverse=True)
    rkey = (res_t["from_residue"].astype(np.uint64) << np.uint64(34)) | (res_t["to_residue"].astype(np.uint64) << np.uint64(5)) | res_t["interaction"].astype(np.uint64)
    assert np.array_equal(uk, rkey)  # the same rows in the same order
    mn = np.full(len(uk), np.inf, np.float32)
    np.minimum.at(mn, inv, atom_t["min_distance"])
    assert np.array_equal(mn, res_t["min_distance"])
    most = np.zeros(len(uk), np.int64)
    np.maximum.at(most, inv, atom_t["n_frames"].astype(np.int64))
    total = np.zeros(len(uk), np.int64)
    np.add.at(total, inv, atom_t["n_frames"].astype(np.int64))
    nf = res_t["n_frames"].astype(np.int64)
    assert (most <= nf).all() and (nf <= np.minimum(F, total)).all()
    assert (res_t["max_distance"] >= res_t["min_distance"]).all()
    mx = np.full(len(uk), -np.inf, np.float32)
    np.maximum.at(mx, inv, atom_t["max_distance"])
    assert (res_t["max_distance"] <= mx).all()
    if F == 1:
        assert (nf == 1).all() and np.array_equal(res_t["max_distance"], mn) and (res_t["frequency"] == 1.0).all()
