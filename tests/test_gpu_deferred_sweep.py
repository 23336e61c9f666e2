"""GPU tests of the deferred last Jacobi sweep (engine_polar.inc defer_last_sweep(),
complete_pending_sweep(); kernels_coef.h pair_finish_kernel).

The comparison engine is always the same call sequence under polar_rrms = 1, which runs all n sweeps and takes U_pol from
the last one's dipoles, as every solve did before.  Tolerances: U_pol is a re-associated sum of the same terms, 1e-12
relative (the bound tests/test_gpu_parity.py holds the half-tile sweep to); everything else is compared bit for bit, and
against the oracle with that file's own bounds.
"""
import os

import numpy as np
import pytest

import deferred_sweep_cases as dc
from mpmc_amd import engine, host
from oracle import oracle

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deferred_sweep_guard.npz")
SAME = ("energy", "rd_energy", "coulombic_energy", "polarization_energy")
_systems = {}


def system(n):
    if n not in _systems:
        _systems[n] = dc.system(n)
    return _systems[n]


def make(s, flags, timing=None, **opts):
    e = engine.Engine(len(s["charge"]))
    e.load_system(s, flags)
    for k, v in opts.items():
        e.set_option(k, v)
    if timing is not None:
        e.set_option("timing", timing)
    return e


def pair_of(s, **flag_overrides):
    """(engine under test, comparison engine)"""
    return make(s, dict(dc.FLAGS, **flag_overrides)), make(s, dict(dc.FLAGS_ALL_SWEEPS, **flag_overrides))


def same_energies(got, want, what):
    print(what, "U_pol %.17g comparison %.17g rel %.3g" % (
        got["polarization_energy"], want["polarization_energy"],
        abs(got["polarization_energy"] - want["polarization_energy"]) / abs(want["polarization_energy"])))
    assert abs(got["polarization_energy"] - want["polarization_energy"]) <= 1e-12 * abs(want["polarization_energy"]), what
    for k in ("rd_energy", "coulombic_energy", "polar_iterations"):
        assert got[k] == want[k], (what, k)
    # energy = (rd + coulombic) + U_pol carries U_pol's last bits: it is exactly that sum of the equal terms and its own
    # U_pol, and within U_pol's bound of the comparison's
    assert got["energy"] == want["rd_energy"] + want["coulombic_energy"] + got["polarization_energy"], what
    assert abs(got["energy"] - want["energy"]) <= 1e-12 * abs(want["polarization_energy"]), what
    assert got["energy"] == want["energy"], what  # (|energy| >> |U_pol|: the last-bit difference does not survive the sum here)


def same_vectors(got, want, what):
    for k in ("mu", "ef_induced", "ef_static"):
        assert np.array_equal(got[k], want[k]), (what, k, np.abs(got[k] - want[k]).max())
    assert np.abs(got["mu"]).max() > 0 and np.abs(got["ef_induced"]).max() > 0


# ---------------------------------------------------------------------------------------------
# 1. energy and solution
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("niter", [2, 4, 5])
@pytest.mark.parametrize("n", dc.SIZES)
def test_energy_and_solution(n, niter):
    s = system(n)
    assert dc.blocks(s) == {2300: 22, 2560: 24}[n]
    a, b = pair_of(s, polar_max_iter=niter)
    first, new = dc.molecule_move(s, 100)
    for tag in ("first", "moved"):
        if tag == "moved":
            a.update_atoms(first, new)
            b.update_atoms(first, new)
        ra, rb = a.energy(), b.energy()
        same_energies(ra, rb, (n, niter, tag))
        assert ra["polar_iterations"] == niter
        da, db = a.dipoles(), b.dipoles()
        same_vectors(da, db, (n, niter, tag))
        if niter == 4:  # the headline count: the dipoles the commit before the deferral gave
            gold = np.load(GOLD)
            assert np.array_equal(da["mu"], gold["headline_%d:%s:mu" % (n, tag)]), (n, tag)
            for k in ("rd_energy", "coulombic_energy", "polar_iterations"):
                assert ra[k] == gold["headline_%d:%s:%s" % (n, tag, k)][()], (n, tag, k)
            want = gold["headline_%d:%s:polarization_energy" % (n, tag)][()]
            assert abs(ra["polarization_energy"] - want) <= 1e-12 * abs(want)
    a.close()
    b.close()


def test_against_the_oracle():
    from test_gpu_parity import check_energies

    s = system(2560)
    a = make(s, dc.FLAGS)
    got = a.energy()
    got.update(a.dipoles())
    a.close()
    want = oracle.energy(s, dc.FLAGS, want_vectors=True)
    check_energies(got, want)
    assert np.abs(got["mu"] - want["mu"]).max() <= 1e-10 * np.abs(want["mu"]).max()


def test_one_iteration_takes_the_old_path():
    s = system(2300)
    a = make(s, dict(dc.FLAGS, polar_max_iter=1), timing=2)
    b = make(s, dict(dc.FLAGS_ALL_SWEEPS, polar_max_iter=1))
    ra, rb = a.energy(), b.energy()
    assert a.timings()["sweep_count"] == 1
    for k in SAME:
        assert ra[k] == rb[k], k
    same_vectors(a.dipoles(), b.dipoles(), "one iteration")
    assert a.timings()["sweep_count"] == 1
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------
# 2. launch counts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("niter", [2, 4])
def test_launch_counts(niter):
    s = system(2300)
    a = make(s, dict(dc.FLAGS, polar_max_iter=niter), timing=2)
    b = make(s, dict(dc.FLAGS_ALL_SWEEPS, polar_max_iter=niter), timing=2)
    a.energy()
    b.energy()
    assert a.timings()["sweep_count"] == niter - 1 and b.timings()["sweep_count"] == niter
    d1 = a.dipoles()
    assert a.timings()["sweep_count"] == niter  # the first reader pays the last sweep ...
    d2 = a.dipoles()
    assert a.timings()["sweep_count"] == niter  # ... once
    same_vectors(d1, d2, "second download")
    same_vectors(d1, b.dipoles(), "first download")
    # two evaluations with nothing moved in between: the first one's pending sweep is dropped, the second one's is run
    a.energy()
    ra = a.energy()
    rb = b.energy()
    assert a.timings()["sweep_count"] == niter - 1
    same_energies(ra, rb, "repeated")
    same_vectors(a.dipoles(), b.dipoles(), "repeated")
    assert a.timings()["sweep_count"] == niter
    a.close()
    b.close()


# ---------------------------------------------------------------------------------------------
# 3. the pending sweep against state changes
# ---------------------------------------------------------------------------------------------
def _act_noted_move(e, s):
    first, new = dc.molecule_move(s, 77)
    e.update_atoms(first, new)
    return dc.moved(s, first, new), True


def _act_big_move(e, s):
    first, new = dc.big_move(s)
    assert len(new) > 32
    e.update_atoms(first, new)
    return dc.moved(s, first, new), True


def _act_remove_insert(e, s):
    # the molecule leaves and comes back displaced: it takes the hole it left, so the slots are those of an upload
    first, new = dc.molecule_move(s, 77, shift=(0.4, 0.3, -0.2))
    assert e.remove_molecule(first, 5)
    sl = slice(first, first + 5)
    got = e.insert_molecule(new, s["charge"][sl], s["alpha"][sl], s["epsilon"][sl], s["sigma"][sl], s["mass"][sl])
    assert got == first
    return dc.moved(s, first, new), False  # (an edit discards the result: nobody can ask for its dipoles)


def _act_box(e, s):
    out = dict(s)
    out["basis"] = np.asarray(s["basis"]) * 1.01
    e.set_box(out["basis"])
    return out, True


ACTIONS = {"noted_move": _act_noted_move, "big_move": _act_big_move, "remove_insert": _act_remove_insert,
           "box": _act_box}


@pytest.mark.parametrize("action", sorted(ACTIONS))
@pytest.mark.parametrize("n", dc.SIZES)
def test_pending_sweep_against_state_changes(n, action):
    s = system(n)
    a, b = pair_of(s)
    got = []
    for e in (a, b):
        e.energy()
        after, readable = ACTIONS[action](e, s)
        if readable:
            d = e.dipoles()  # the result of the evaluation BEFORE the change
        else:
            with pytest.raises(engine.EngineError):
                e.dipoles()
            d = None
        r = e.energy()
        got.append((d, r, e.dipoles()))
    (da, ra, da2), (db, rb, db2) = got
    if da is not None:
        same_vectors(da, db, (n, action, "before"))
    same_energies(ra, rb, (n, action))
    same_vectors(da2, db2, (n, action, "after"))
    fresh = make(after, dc.FLAGS)
    rf = fresh.energy()
    for k in SAME:
        assert ra[k] == rf[k], (n, action, "fresh context", k, ra[k], rf[k])
    same_vectors(da2, fresh.dipoles(), (n, action, "fresh context"))
    for e in (a, b, fresh):
        e.close()


# ---------------------------------------------------------------------------------------------
# 4. not applied where excluded
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(dc.EXCLUDED))
def test_excluded_modes_run_every_sweep_and_keep_their_bits(name):
    flags, opts = dc.EXCLUDED[name]
    s = system(2560)
    gold = np.load(GOLD)
    e = make(s, flags, timing=2, **opts)
    first, new = dc.molecule_move(s, 100)
    for tag in ("first", "moved"):
        if tag == "moved":
            e.update_atoms(first, new)
        r = e.energy()
        t = e.timings()
        print(name, tag, "iterations", r["polar_iterations"], "sweep launches", t["sweep_count"], "palmo ms", t["palmo_ms"])
        assert r["polar_iterations"] >= 2
        assert t["sweep_count"] == r["polar_iterations"]
        assert (t["palmo_ms"] > 0) == (name == "palmo")  # (its contraction is one more pass, timed in a class of its own)
        for f in dc.ENERGY_KEYS:
            assert r[f] == gold["%s:%s:%s" % (name, tag, f)][()], (name, tag, f)
        e.dipoles()
        assert e.timings()["sweep_count"] == r["polar_iterations"]
    e.close()


# ---------------------------------------------------------------------------------------------
# 5. options stay bit-neutral
# ---------------------------------------------------------------------------------------------
def _chain(engs, s, nsteps, seed, dipoles_at=()):
    rng = np.random.default_rng(seed)
    pos = np.array(s["pos"], copy=True)
    hist = [[] for _ in engs]
    for step in range(nsteps):
        first = 5 * int(rng.integers(0, len(pos) // 5))
        new = pos[first:first + 5] + rng.normal(scale=0.2, size=3)
        accept = step % 3 != 2
        for k, e in enumerate(engs):
            e.update_atoms(first, new)
            hist[k].append(e.energy())
            if step in dipoles_at:
                hist[k][-1]["mu"] = e.dipoles()["mu"]
            if not accept:
                e.update_atoms(first, pos[first:first + 5])
        if accept:
            pos[first:first + 5] = new
    return hist


def test_step_graph_replay_carries_the_pending_sweep():
    s = system(2560)
    engs = [make(s, dc.FLAGS, timing=0, step_graph=g) for g in (1, 0)]
    hist = _chain(engs, s, 12, seed=5, dipoles_at=(7, 11))
    assert engs[0].timings()["graph_steps"] >= 8 and engs[1].timings()["graph_steps"] == 0
    for a, b in zip(*hist):
        for k in SAME:
            assert a[k] == b[k], k
        if "mu" in a:
            assert np.array_equal(a["mu"], b["mu"]) and np.abs(a["mu"]).max() > 0
    for e in engs:
        e.close()


def test_sweep_split_agrees():
    s = system(2560)
    out = []
    for split in (1, 0):
        e = make(s, dc.FLAGS, sweep_split=split)
        r = e.energy()
        out.append((r, e.dipoles()["mu"]))
        e.close()
    (ra, ma), (rb, mb) = out
    assert abs(ra["polarization_energy"] - rb["polarization_energy"]) <= 1e-12 * abs(rb["polarization_energy"])
    assert np.abs(ma - mb).max() <= 1e-13 * np.abs(mb).max()


def test_incremental_maintenance_is_bit_neutral():
    s = system(2560)
    engs = [make(s, dc.FLAGS, incremental_amatrix=v, incremental_pairs=v) for v in (1, 0)]
    hist = _chain(engs, s, 4, seed=9, dipoles_at=(1, 3))
    for a, b in zip(*hist):
        for k in SAME:
            assert a[k] == b[k], k
        if "mu" in a:
            assert np.array_equal(a["mu"], b["mu"])
    for e in engs:
        e.close()


# ---------------------------------------------------------------------------------------------
# 6. the host's chain
# ---------------------------------------------------------------------------------------------
def test_host_chain_is_the_same_chain():
    s = system(2560)
    out = []
    for flags in (dc.FLAGS, dc.FLAGS_ALL_SWEEPS):  # one after the other: one random-number stream per process
        h = host.HostSystem(s, flags, seed=11, move_factor=0.05, rot_factor=0.05)
        h.mc_steps(60)
        o = h.observables()
        out.append((h.positions(), o["accept"], o["reject"], h.dipoles()["mu"], o["polarization_energy"]))
        h.close()
    a, b = out
    assert 0 < a[1] < 60 and a[1] + a[2] == 60
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]
    assert np.array_equal(a[3], b[3]) and np.abs(a[3]).max() > 0
    assert abs(a[4] - b[4]) <= 1e-12 * abs(b[4])
