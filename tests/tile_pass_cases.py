"""Inputs of tests/test_gpu_tile_passes.py and tests/golden/make_dense_terms_guard.py: the smallest committed case of each
dense-term mode, a move of several molecules whose 64-atom blocks arrive at the engine in DESCENDING order, and the
sequence of evaluations both files record.

Why descending.  A step of the existing incremental tests moves one molecule: one dirty block, or two in ascending order.
The rule "the tile of two dirty blocks belongs to the earlier entry of the list" (kernels_tile.h, owned_tile) decides
something only when a later entry has a lower block index than an earlier one: then the mutual tile must be computed
once, by the earlier entry, although the later one holds its row.
"""
import numpy as np

import at_cases as ac
import phahst_cases as pc
import rdc_cases as rc
from mpmc_amd import synth

MAX_MOVED = 32  # kMaxMoves: the moves ride in the MoveList of the pair kernel's launch
RDC_ORDER = 2


def _at_phahst(s):
    """tests/test_gpu_at.py's "phahst" variant: epsilon / sigma become the exponent b and the range rho"""
    on = s["epsilon"] != 0.0
    return dict(s, epsilon=np.where(on, 3.2, 0.0), sigma=np.where(on, 2.9, 0.0), c8=20.0 * s["c6"], c10=500.0 * s["c6"])


# name -> (system, flags, mode)
CASES = {
    "phahst-c320-polarizable": lambda: (pc.system("c320"), pc.VARIANTS["polarizable"], "phahst"),
    "phahst-c320-damp_extrapolate": lambda: (pc.system("c320"), pc.VARIANTS["damp_extrapolate"], "phahst"),
    "rdc-t150-fh4": lambda: (rc.system("t150"), rc.flags("fh4", RDC_ORDER), "rdc"),
    "rdc-t150-lrc": lambda: (rc.system("t150"), rc.flags("lrc", RDC_ORDER), "rdc"),
    "at-n320-lj": lambda: (ac.case("n320"), dict(synth.FLAGS_AT), "at"),
    "at-n320-phahst": lambda: (_at_phahst(ac.case("n320")), dict(synth.FLAGS_PHAHST, axilrod_teller=1), "at"),
}
# the three the multi-block test runs on (the guard records all six)
TEST_CASES = ("phahst-c320-polarizable", "rdc-t150-fh4", "at-n320-lj")
EDIT_CASE = "lj-s_pol320"  # plain Lennard-Jones + Ewald + rd_lrc: remove_molecule / insert_molecule (lj_lrc_kernel's pass)


def moves(s, seed=23):
    """[(first atom, new coordinates)], one non-frozen molecule per 64-atom block that has one, highest block first; where
    non-frozen molecules lie across a block border, the first of them stands for the block its first atom is in."""
    mol, frozen = np.asarray(s["molecule"]), np.asarray(s["frozen"])
    rng = np.random.default_rng(seed)
    mols = [np.flatnonzero(mol == m) for m in np.unique(mol[frozen == 0])]
    for idx in mols:
        assert np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx))) and not frozen[idx].any()
    if "active" in s:  # axilrod_teller cases: molecules with a site that carries the term first
        mols.sort(key=lambda idx: not np.isin(idx, s["active"]).any())
    straddlers = [idx for idx in mols if idx[0] // 64 != idx[-1] // 64]
    pick = {}  # block of the first atom -> atom indices of the molecule
    for idx in straddlers[:1] + mols:
        pick.setdefault(idx[0] // 64, idx)
    out = []
    for b in sorted(pick, reverse=True):
        idx = pick[b]
        c = s["pos"][idx].mean(axis=0)
        th = rng.uniform(-0.2, 0.2)
        rot = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
        out.append((int(idx[0]), (s["pos"][idx] - c) @ rot.T + c + rng.uniform(-0.15, 0.15, 3)))
    assert sum(len(new) for _, new in out) <= MAX_MOVED
    return out


def moved(s, mv):
    pos = s["pos"].copy()
    for first, new in mv:
        pos[first:first + len(new)] = new
    return dict(s, pos=pos)


def _record(e, mode):
    r = dict(e.energy())
    if mode == "at":
        r["three_body"] = e.three_body_energy()
    return r


def run_case(engine, name, **options):
    """(first evaluation, evaluation after the multi-block move) of a new context; each a dict of the Result fields, plus
    three_body in the axilrod_teller cases"""
    s, flags, mode = CASES[name]()
    e = engine.Engine(len(s["charge"]))
    for k, v in options.items():
        e.set_option(k, v)
    e.load_system(s, flags)
    first = _record(e, mode)
    for at, new in moves(s):
        e.update_atoms(at, new)
    after = _record(e, mode)
    e.close()
    return first, after


def run_edit_case(engine):
    """(first evaluation, after remove_molecule of molecule 26 -- which lies across the border of blocks 1 and 2 --, after
    insert_molecule puts it back) on synth.s_pol(320) without polarization"""
    s, flags = synth.s_pol(320), dict(synth.FLAGS_ES)
    assert flags.get("rd_lrc", 1) and not flags.get("polarization")
    idx = np.flatnonzero(np.asarray(s["molecule"]) == 26)
    assert idx[0] // 64 != idx[-1] // 64
    e = engine.Engine(320)
    e.load_system(s, flags)
    out = [dict(e.energy())]
    assert e.remove_molecule(int(idx[0]), len(idx)) is True
    out.append(dict(e.energy()))
    assert e.insert_molecule(s["pos"][idx], s["charge"][idx], s["alpha"][idx], s["epsilon"][idx], s["sigma"][idx],
                             s["mass"][idx]) == int(idx[0])
    out.append(dict(e.energy()))
    e.close()
    return out


def guard_entries(engine):
    """{key: value} of everything tests/golden/dense_terms_guard.npz holds"""
    d = {}
    for name in CASES:
        for tag, r in zip(("first", "moved"), run_case(engine, name)):
            for k, v in r.items():
                d["%s:%s:%s" % (name, tag, k)] = v
    for tag, r in zip(("first", "removed", "inserted"), run_edit_case(engine)):
        for k, v in r.items():
            d["%s:%s:%s" % (EDIT_CASE, tag, k)] = v
    return d
