"""Helpers of the contact-frequency tests on the device (tests/test_freq_gpu.py, tests/test_freq_rings_gpu.py, tests/test_ens_shapes_gpu.py): the
expected table from one Context.atomic_contacts call per frame aggregated in numpy, the ring rows from one Context.get_contacts call per frame
on the single-model structure that holds the frame's coordinates, and the comparisons.  Expected values never come from contact_frequencies."""
from __future__ import annotations

import numpy as np

import arpeggia_amd as aa
from arpeggia_amd import _lib

RING_CODES = set(range(11, 18))  # Pi* stackings and CationPi: ring rows, not part of the frequency table


def expected(ctx, s: aa.Structure, frames: np.ndarray, groups: str) -> dict:
    """One atomic_contacts call per frame on the topology (model 0) with the frame's coordinates; rows aggregated by (i, j, code)."""
    soa = s.soa(groups)
    F, n = frames.shape[0], frames.shape[1]
    # model 0's residues are the residues of its atoms: ids 0 .. max + 1 (the hierarchy is built model by model)
    nr = int(soa["res_id"][:n].max()) + 1 if n and len(soa["res_cb"]) else 0
    top = {k: soa[k][:n] for k in ("attr", "res_ord", "chain_rank", "model", "res_id")}
    top.update(res_h_ptr=soa["res_h_ptr"][: nr + 1] if nr else soa["res_h_ptr"][:0], res_cb=soa["res_cb"][:nr], res_sg=soa["res_sg"][:nr])
    nh = int(top["res_h_ptr"][-1]) if nr else 0
    top["res_h_idx"] = soa["res_h_idx"][:nh]
    keys, dists = [], []
    for f in range(F):
        d = dict(top, x=frames[f, :, 0].copy(), y=frames[f, :, 1].copy(), z=frames[f, :, 2].copy())
        p = ctx.atomic_contacts(d)
        p = p[p["kind"] != 0]
        for code in range(len(_lib.INTERACTIONS)):
            sel = (p["kind"] >> np.uint32(code)) & np.uint32(1) == 1
            if sel.any():
                q = p[sel]
                keys.append((q["i"].astype(np.uint64) << np.uint64(34)) | (q["j"].astype(np.uint64) << np.uint64(5)) | np.uint64(code))
                dists.append(q["dist"])
    keys = np.concatenate(keys) if keys else np.zeros(0, np.uint64)
    dists = np.concatenate(dists) if dists else np.zeros(0, np.float32)
    uk, inv, cnt = np.unique(keys, return_inverse=True, return_counts=True)
    mn = np.full(len(uk), np.inf, np.float32)
    mx = np.full(len(uk), -np.inf, np.float32)
    np.minimum.at(mn, inv, dists)
    np.maximum.at(mx, inv, dists)
    i = (uk >> np.uint64(34)).astype(np.int64)
    j = ((uk >> np.uint64(5)) & np.uint64((1 << 29) - 1)).astype(np.int64)
    code = (uk & np.uint64(31)).astype(np.int32)
    assert not (set(np.unique(code).tolist()) & RING_CODES)
    out = {"interaction": code, "from_atom": i.astype(np.int32), "to_atom": j.astype(np.int32), "n_frames": cnt.astype(np.uint32),
           "frequency": (cnt.astype(np.float64) / F).astype(np.float32), "min_distance": mn, "max_distance": mx}
    for side, idx in (("from", i), ("to", j)):
        out[f"{side}_chain"] = s.strings("chain")[idx]
        out[f"{side}_resn"] = s.strings("resn")[idx]
        out[f"{side}_resi"] = s.ints("resi")[idx]
        out[f"{side}_insertion"] = s.strings("insertion")[idx]
        out[f"{side}_altloc"] = s.strings("altloc")[idx]
        out[f"{side}_atomn"] = s.strings("atomn")[idx]
        out[f"{side}_atomi"] = s.ints("atomi")[idx]
    return out


def assert_table_equal(got: dict, want: dict):
    names = [c for c, _ in aa.FREQ_COLUMNS] + ["from_atom", "to_atom"]
    assert set(got) == set(names)
    for c in names:
        assert len(got[c]) == len(want[c]), c
        if got[c].dtype.kind == "S":
            assert np.array_equal(got[c].astype(want[c].dtype), want[c]), c
        else:
            kind = dict(aa.FREQ_COLUMNS + [("from_atom", "i4"), ("to_atom", "i4")])[c]
            assert got[c].dtype == np.dtype("<" + (kind if kind != "str" else "i4")), c
            assert np.array_equal(got[c], want[c].astype(got[c].dtype)), c


def to_bytes(t: dict) -> bytes:
    return b"".join(np.ascontiguousarray(t[c]).tobytes() for c in sorted(t))


BASE = [c for c, _ in aa.FREQ_COLUMNS] + ["from_atom", "to_atom"]


RING_ATOMS = {b"HIS": {b"CG", b"ND1", b"CE1", b"NE2", b"CD2"}, b"PHE": {b"CG", b"CD1", b"CD2", b"CE1", b"CE2", b"CZ"},
              b"TYR": {b"CG", b"CD1", b"CD2", b"CE1", b"CE2", b"CZ"}, b"TRP": {b"CG", b"CD1", b"CD2", b"NE1", b"CE2", b"CE3", b"CZ2", b"CZ3", b"CH2"}}


def ring_entities(rec: dict) -> dict:
    """(chain, resi, insertion, altloc) -> ring entity index: one entity per altloc of every residue with at least 3 ring-plane atoms, in residue
    order (records whose chains are contiguous: file order is hierarchy order)."""
    residues, atoms_of = [], {}
    for k in range(len(rec["x"])):
        key = (bytes(rec["chain"][k]), int(rec["resi"][k]), bytes(rec["icode"][k]))
        if key not in atoms_of:
            residues.append(key)
            atoms_of[key] = []
        atoms_of[key].append(k)
    out = {}
    for key in residues:
        ks = atoms_of[key]
        names = RING_ATOMS.get(bytes(rec["resn"][ks[0]]))
        if not names or sum(bytes(rec["name"][k]) in names for k in ks) < 3:
            continue
        for alt in dict.fromkeys(bytes(rec["altloc"][k]) for k in ks):
            out[(key[0], key[1], key[2], alt)] = len(out)
    return out


def device_reference(ctx, rec: dict, frames: np.ndarray, groups: str, dist_cutoff: float = 6.5) -> dict:
    """The ring rows of the frequency table by definition: Context.get_contacts on S_f for every frame, aggregated."""
    ents = ring_entities(rec)
    F, n = frames.shape[0], frames.shape[1]
    first, dists = {}, {}
    for f in range(F):
        s = aa.Structure.from_records(dict(rec, x=frames[f, :, 0].copy(), y=frames[f, :, 1].copy(), z=frames[f, :, 2].copy()))
        assert s.n_atoms == n
        t = ctx.get_contacts(s, groups, 0.1, dist_cutoff)
        for k in np.flatnonzero((t["from_atom"] < 0) | (t["to_atom"] < 0)):
            assert t["from_atom"][k] < 0 and t["from_atomn"][k] == b"Ring"
            e1 = ents[(bytes(t["from_chain"][k]), int(t["from_resi"][k]), bytes(t["from_insertion"][k]), bytes(t["from_altloc"][k]))]
            if t["to_atom"][k] >= 0:
                to_ent, e2 = int(t["to_atom"][k]), -1
            else:
                e2 = ents[(bytes(t["to_chain"][k]), int(t["to_resi"][k]), bytes(t["to_insertion"][k]), bytes(t["to_altloc"][k]))]
                to_ent = n + e2
            key = (n + e1, to_ent, int(t["interaction"][k]))
            if key not in first:
                row = {c: t[c][k] for c in BASE if c in t and c != "interaction"}
                row.update(interaction=key[2], from_ring=e1, to_ring=e2)
                first[key] = row
            dists.setdefault(key, []).append(t["distance"][k])
    keys = sorted(first)
    out = {}
    for c in BASE + ["from_ring", "to_ring"]:
        if c == "n_frames":
            out[c] = np.array([len(dists[k]) for k in keys], np.uint32)
        elif c == "frequency":
            out[c] = np.array([np.float32(len(dists[k]) / F) for k in keys], np.float32)
        elif c == "min_distance":
            out[c] = np.array([min(dists[k]) for k in keys], np.float32)
        elif c == "max_distance":
            out[c] = np.array([max(dists[k]) for k in keys], np.float32)
        else:
            out[c] = np.array([first[k][c] for k in keys]) if keys else np.zeros(0, "S8" if c.endswith(("chain", "resn", "atomn", "insertion", "altloc")) else np.int32)
    return out


def ring_part(t: dict) -> dict:
    sel = t["from_ring"] >= 0
    assert not sel.any() or sel[int(np.argmax(sel)):].all()  # every ring row follows every atom row
    assert (t["to_ring"][~sel] == -1).all()
    return {c: v[sel] for c, v in t.items()}


def atom_part(t: dict) -> dict:
    sel = t["from_ring"] < 0
    return {c: t[c][sel] for c in BASE}


def assert_same_rows(got: dict, want: dict):
    for c in BASE + ["from_ring", "to_ring"]:
        assert len(got[c]) == len(want[c]), c
        assert np.array_equal(got[c], want[c].astype(got[c].dtype)), c
