"""GPU tests of the tile-pass scheme the dense terms share (mpmc_amd/csrc/kernels_tile.h; tile_pass() in engine.hip):
disp_tile_kernel, rdc_tile_kernel and at_triple_kernel after ONE evaluation's worth of moves that dirty several 64-atom
blocks in descending order (tests/tile_pass_cases.py says why that order), and every dense kernel against the bits of the
commit before the scheme was shared (tests/golden/dense_terms_guard.npz); and the host half's table of what drops which
cached sum (positions_unknown() and its three siblings in engine.hip, and the mode setters): every
mode through every event, against a fresh context.

No tolerance is introduced here: the bit comparisons have none, and the comparisons with the CPU references use
phahst_cases.RD_TOL, rdc_cases.RD_TOL and at_cases.TOLERANCE (1e-12 of sum |terms| each) as the tests of those terms do.
"""
import os

import numpy as np
import pytest

import at_cases as ac
import at_reference
import phahst_cases as pc
import phahst_reference
import rdc_cases as rc
import rdc_reference
import tile_pass_cases as tp
from mpmc_amd import engine

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_terms_guard.npz")


def _fresh(s, flags, mode):
    e = engine.Engine(len(s["charge"]))
    e.load_system(s, flags)
    r = tp._record(e, mode)
    e.close()
    return r


@pytest.mark.parametrize("name", tp.TEST_CASES)
def test_several_dirty_blocks_in_descending_order(name):
    s, flags, mode = tp.CASES[name]()
    mv = tp.moves(s)
    blocks = [first // 64 for first, _ in mv]
    straddling = [first for first, new in mv if first // 64 != (first + len(new) - 1) // 64]
    print(name, "blocks of the calls", blocks, "atoms moved", sum(len(new) for _, new in mv), "straddling", straddling)
    assert len(set(blocks)) >= 3 and blocks != sorted(blocks)
    assert blocks == sorted(blocks, reverse=True)
    mol, frozen = np.asarray(s["molecule"]), np.asarray(s["frozen"])
    has_straddler = any(mol[b - 1] == mol[b] and not frozen[b] for b in range(64, len(mol), 64))
    assert bool(straddling) == has_straddler
    assert sum(len(new) for _, new in mv) <= tp.MAX_MOVED
    for first, new in mv:
        assert not frozen[first:first + len(new)].any()

    first_live, live = tp.run_case(engine, name)
    first_full, full = tp.run_case(engine, name, incremental_pairs=0)
    cur = tp.moved(s, mv)
    fresh = _fresh(cur, flags, mode)
    assert first_live == first_full and first_live != live
    for f in fresh:  # every Result field, and three_body in the axilrod_teller case
        assert live[f] == fresh[f], ("incremental vs fresh", f, live[f], fresh[f])
        assert full[f] == fresh[f], ("incremental_pairs = 0 vs fresh", f, full[f], fresh[f])
    assert live["status"] == 0
    if mode == "at":
        assert all(np.isin(np.arange(first, first + len(new)), s["active"]).any() for first, new in mv)
        assert live["three_body"] != first_live["three_body"]

    if mode == "phahst":
        ref = phahst_reference.rd_terms(cur, flags)
        got, want, tol = live["rd_energy"], float(ref["total"]), pc.RD_TOL * float(ref["abs_sum"])
    elif mode == "rdc":
        ref = rdc_reference.rd_terms(cur, flags, tp.RDC_ORDER)
        got, want, tol = live["rd_energy"], float(ref["total"]), rc.RD_TOL * float(ref["abs_sum"])
    else:
        u = at_reference.unordered(cur)
        got, want, tol = live["three_body"], u.total, ac.TOLERANCE * u.sum_abs
    print("%s: %.15g reference %.15g |diff| %.3g tol %.3g" % (name, got, want, abs(got - want), tol))
    assert abs(got - want) <= tol, (name, got, want, tol)


def _fresh_snapshot(s, flags):
    e = engine.Engine(len(s["charge"]))
    e.load_system(s, flags)
    r = tp.snapshot(e)
    e.close()
    return r


@pytest.mark.parametrize("mode,event", tp.EVENT_CELLS)
def test_an_event_leaves_the_bits_of_a_fresh_context(mode, event):
    """The table of what drops which cached sum, from outside: a live context that went through the
    event gives, field for field with ==, what a fresh context gives on the final state -- and again after one more
    single-molecule move, whose incremental passes start from the sums the event left valid.  A sum the event should have
    dropped and did not shows as the stale value; the event itself must show in the fields it is about, so that no cell
    passes by doing nothing."""
    m = tp.EVENT_MODES[mode]()
    s, f = m["system"], m["flags"]
    e = engine.Engine(len(s["charge"]))
    e.load_system(s, f)
    before = tp.snapshot(e)
    assert before["status"] == 0 and before[m["term"]] != 0.0
    assert (before["close_contacts"] > 0) == (mode in tp.AUTOREJECT_MODES)  # the count is on in those, and not trivially 0
    s, f, probe, fields = tp.EVENTS[event](e, m, s, f, before)
    got = tp.snapshot(e)
    kept = tp.E_ISO_FIELDS if mode == "polarvdw" and event in tp.E_ISO_KEPT_BY else ()

    def same(live, fresh, what):
        diff = {k: (live[k], fresh[k]) for k in fresh if live[k] != fresh[k] and k not in kept}
        print(mode, event, what, "fields compared", len(fresh) - len(kept), "differing", diff)
        assert sorted(live) == sorted(fresh) and not diff, (what, diff)
        if kept:  # the kept e_iso, and the two sums made with it
            assert live["e_iso"] == before["e_iso"]
            assert live["vdw_energy"] == (live["e_total"] - live["e_iso"]) + live["lr_corr"]
            assert live["energy"] == ((live["rd_energy"] + live["coulombic_energy"]) + live["polarization_energy"]) + live["vdw_energy"]

    same(got, _fresh_snapshot(s, f), "behind the event")
    probe = got if probe is None else probe
    for k in fields:
        assert probe[k] != before[k], (k, probe[k])
    if not fields:  # (rd_lrc under the sg form: no term reads it)
        assert got == before

    mv = tp.moves(s, seed=37)[-1:]
    e.update_atoms(*mv[0])
    after = tp.snapshot(e)
    e.close()
    same(after, _fresh_snapshot(tp.moved(s, mv), f), "behind the move")
    assert after["energy"] != got["energy"] and after["status"] == 0


def test_dense_terms_give_the_bits_of_the_parent_commit():
    """Every dense kernel (disp_tile / disp_lrc, rdc_tile / rdc_self / lj_lrc at the crystal cutoff, at_triple, lj_lrc's
    incremental pass after remove_molecule / insert_molecule): first evaluation and the one after the move, bit for bit
    what the build of the commit before kernels_tile.h gave on the same kind of device
    (tests/golden/make_dense_terms_guard.py)."""
    gold = np.load(GOLD)
    got = tp.guard_entries(engine)
    assert sorted(got) == sorted(gold.files)
    bad = [(k, got[k], gold[k][()]) for k in sorted(got) if got[k] != gold[k][()]]
    assert not bad, bad
