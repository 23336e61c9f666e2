"""Sweeps m + 1 .. n of a fixed-count plain Jacobi solve (m = ceil(n / 2)) run only when somebody asks for the dipoles
(engine_polar.inc run_polarization(), complete_pending_sweep(); engine.hip PendingSweep).

U_pol is complete behind the finish of sweep m and the record goes out there (tests/test_gpu_early_publish.py).  Where
it HAS gone out there, the call launches nothing behind it: sweeps m + 1 .. n wait, in order, for the first reader of the
dipoles, and the next evaluation drops them.  A call timed with events, a captured or replayed step and a call that could
not publish early keep n - 1 launched sweeps and one pending, as before.

The comparison engine is the same call sequence under polar_rrms = 1, which launches all n sweeps inside the call.
Shapes, helpers and bounds are those of tests/test_gpu_deferred_sweep.py: U_pol is a re-associated sum of the same terms,
1e-12 relative; everything else is compared bit for bit.  `pending_sweeps` (mpmc_hip_timings) is state and is filled on
every call; `sweep_count` exists only on calls timed with events, which keep the old placement, so a timing-2 engine
counts launches and must agree with the timing-0 engine to the bit.
"""
import numpy as np
import pytest

import deferred_sweep_cases as dc
import test_gpu_deferred_sweep as ds
from mpmc_amd import engine, host

pytestmark = pytest.mark.gpu
ALL = ds.SAME + ("polar_iterations",)
NITER = [2, 3, 4, 5, 6, 7]


def tail(niter):
    """sweeps a call leaves unlaunched once its record has gone out behind sweep ceil(n / 2)"""
    return niter - (niter + 1) // 2


def pending(e):
    return e.timings()["pending_sweeps"]


def same_energies(got, want, what):
    """U_pol within 1e-12 relative of the comparison's; the other terms, and the sum taken with the own U_pol, to the bit"""
    up, uq = got["polarization_energy"], want["polarization_energy"]
    print(what, "U_pol %.17g comparison %.17g rel %.3g" % (up, uq, abs(up - uq) / abs(uq)))
    assert abs(up - uq) <= 1e-12 * abs(uq), what
    for k in ("rd_energy", "coulombic_energy", "polar_iterations"):
        assert got[k] == want[k], (what, k)
    assert got["energy"] == want["rd_energy"] + want["coulombic_energy"] + up, what
    assert abs(got["energy"] - want["energy"]) <= 1e-12 * abs(uq), what


def same_bits(ra, rb, what):
    for k in ALL:
        assert ra[k] == rb[k], (what, k, ra[k], rb[k])


def trio(s, niter):
    """(untimed engine under test, timed engine, all-sweeps comparison)"""
    flags = dict(dc.FLAGS, polar_max_iter=niter)
    return (ds.make(s, flags, timing=0), ds.make(s, flags, timing=2),
            ds.make(s, dict(dc.FLAGS_ALL_SWEEPS, polar_max_iter=niter), timing=0))


# ---------------------------------------------------------------------------------------------
# 1. counts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("niter", NITER)
@pytest.mark.parametrize("n", dc.SIZES)
def test_counts(n, niter):
    s = ds.system(n)
    flags = dict(dc.FLAGS, polar_max_iter=niter)
    a = ds.make(s, flags, timing=0)
    t = ds.make(s, flags, timing=2)
    assert pending(a) == 0
    a.energy()
    t.energy()
    assert pending(a) == tail(niter)
    ta = t.timings()
    assert ta["pending_sweeps"] == 1 and ta["sweep_count"] == niter - 1
    a.dipoles()
    t.dipoles()
    assert pending(a) == 0
    ta = t.timings()
    assert ta["pending_sweeps"] == 0 and ta["sweep_count"] == niter
    a.dipoles()
    t.dipoles()
    assert pending(a) == 0
    ta = t.timings()
    assert ta["pending_sweeps"] == 0 and ta["sweep_count"] == niter
    a.close()
    t.close()


def test_all_sweeps_engine_leaves_nothing_pending():
    s = ds.system(2300)
    b = ds.make(s, dc.FLAGS_ALL_SWEEPS, timing=0)
    b.energy()
    assert pending(b) == 0
    b.close()


# ---------------------------------------------------------------------------------------------
# 2. bits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("niter", NITER)
@pytest.mark.parametrize("n", dc.SIZES)
def test_bits(n, niter):
    s = ds.system(n)
    a, t, b = trio(s, niter)
    first, new = dc.molecule_move(s, 100)
    for tag in ("first", "moved"):
        if tag == "moved":
            for e in (a, t, b):
                e.update_atoms(first, new)
        ra, rt, rb = a.energy(), t.energy(), b.energy()
        assert pending(a) == tail(niter)
        assert ra["polar_iterations"] == niter
        same_energies(ra, rb, (n, niter, tag))
        same_bits(ra, rt, (n, niter, tag, "timed call"))
        da, dt, db = a.dipoles(), t.dipoles(), b.dipoles()
        ds.same_vectors(da, dt, (n, niter, tag, "timed call"))
        ds.same_vectors(da, db, (n, niter, tag))
        if niter == 4:
            gold = np.load(ds.GOLD)
            assert np.array_equal(da["mu"], gold["headline_%d:%s:mu" % (n, tag)]), (n, tag)
    for e in (a, t, b):
        e.close()


# ---------------------------------------------------------------------------------------------
# 3. state changes against several pending sweeps
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("action", sorted(ds.ACTIONS))
@pytest.mark.parametrize("niter", [6, 7])
@pytest.mark.parametrize("n", dc.SIZES)
def test_state_changes_against_pending_sweeps(n, niter, action):
    s = ds.system(n)
    flags = dict(dc.FLAGS, polar_max_iter=niter)
    a = ds.make(s, flags, timing=0)
    b = ds.make(s, dict(dc.FLAGS_ALL_SWEEPS, polar_max_iter=niter), timing=0)
    got = []
    for e in (a, b):
        e.energy()
        if e is a:
            assert pending(e) == tail(niter) >= 3
        after, readable = ds.ACTIONS[action](e, s)
        if readable:
            d = e.dipoles()  # the result of the evaluation BEFORE the change
        else:
            with pytest.raises(engine.EngineError):
                e.dipoles()
            d = None
        assert pending(e) == 0
        r = e.energy()
        got.append((d, r, e.dipoles()))
    (da, ra, da2), (db, rb, db2) = got
    if da is not None:
        ds.same_vectors(da, db, (n, niter, action, "before"))
    same_energies(ra, rb, (n, niter, action))
    ds.same_vectors(da2, db2, (n, niter, action, "after"))
    fresh = ds.make(after, flags, timing=0)
    rf = fresh.energy()
    same_bits(ra, rf, (n, niter, action, "fresh context"))
    ds.same_vectors(da2, fresh.dipoles(), (n, niter, action, "fresh context"))
    for e in (a, b, fresh):
        e.close()


@pytest.mark.parametrize("niter", [6, 7])
def test_set_option_between_energy_and_dipoles(niter):
    """The pending sweeps run under the options of the call they belong to: the half-tile sweep re-associates the row
    sums (tests/test_gpu_deferred_sweep.py::test_sweep_split_agrees holds it to a tolerance, not to the bit)."""
    s = ds.system(2560)
    a, _t, b = trio(s, niter)
    _t.close()
    ra, rb = a.energy(), b.energy()
    assert pending(a) == tail(niter)
    a.set_option("sweep_split", 1)
    assert pending(a) == 0
    same_energies(ra, rb, (niter, "before the option"))
    ds.same_vectors(a.dipoles(), b.dipoles(), (niter, "sweeps of the call before the option"))
    # ... and the next evaluation is one under the new option
    fresh = ds.make(s, dict(dc.FLAGS, polar_max_iter=niter), timing=0, sweep_split=1)
    ra, rf = a.energy(), fresh.energy()
    same_bits(ra, rf, (niter, "after the option"))
    ds.same_vectors(a.dipoles(), fresh.dipoles(), (niter, "after the option"))
    for e in (a, b, fresh):
        e.close()


# ---------------------------------------------------------------------------------------------
# 4. evaluations that nobody reads
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("niter", [4, 7])
@pytest.mark.parametrize("n", dc.SIZES)
def test_evaluations_nobody_reads(n, niter):
    s = ds.system(n)
    a, t, b = trio(s, niter)
    first, new = dc.molecule_move(s, 100)
    old = np.asarray(s["pos"])[first:first + 5]
    engs = (a, t, b)

    def step(what):
        ra, rt, rb = [e.energy() for e in engs]
        assert pending(a) == tail(niter) and pending(b) == 0
        same_energies(ra, rb, (n, niter, what))
        same_bits(ra, rt, (n, niter, what, "timed call"))
        return ra

    # twice with nothing moved: the first call's sweeps are dropped, never launched
    r1 = step("first")
    r2 = step("again")
    same_bits(r1, r2, (n, niter, "repeated"))
    # a rejected move: there and back, then somebody asks
    for e in engs:
        e.update_atoms(first, new)
    r3 = step("trial")
    assert r3["energy"] != r1["energy"]
    for e in engs:
        e.update_atoms(first, old)
    step("back")
    da, dt, db = [e.dipoles() for e in engs]
    assert pending(a) == 0
    ds.same_vectors(da, db, (n, niter, "back"))
    ds.same_vectors(da, dt, (n, niter, "back", "timed call"))
    for e in engs:
        e.close()


# ---------------------------------------------------------------------------------------------
# 5. step graph: a context that captures and replays its steps keeps n - 1 launched sweeps, one of direct steps does not
# ---------------------------------------------------------------------------------------------
class Watched:
    """an engine whose energy() also notes what the call left pending and whether it was replayed as a graph"""

    def __init__(self, e):
        self.e = e
        self.graph_steps = 0

    def __getattr__(self, name):
        return getattr(self.e, name)

    def energy(self):
        r = self.e.energy()
        t = self.e.timings()
        r["pending_sweeps"] = t["pending_sweeps"]
        r["graph_step"] = t["graph_steps"] > self.graph_steps
        self.graph_steps = t["graph_steps"]
        return r


@pytest.mark.parametrize("niter", [4, 6])
def test_step_graph(niter):
    s = ds.system(2560)
    flags = dict(dc.FLAGS, polar_max_iter=niter)
    engs = [Watched(ds.make(s, flags, timing=0, step_graph=g)) for g in (1, 0)]
    hist = ds._chain(engs, s, 12, seed=5, dipoles_at=(7, 11))
    assert engs[0].graph_steps >= 8 and engs[1].graph_steps == 0
    for a, b in zip(*hist):
        same_bits(a, b, "graph against direct")
        # (a context with the option on joins its two streams into one record in every call, also in those it enqueues
        #  launch by launch before the capture and after a reader: none of them publishes early)
        assert a["pending_sweeps"] == 1
        assert b["pending_sweeps"] == tail(niter) and not b["graph_step"]
        if "mu" in a:
            assert np.array_equal(a["mu"], b["mu"]) and np.abs(a["mu"]).max() > 0
    assert sum("mu" in a for a in hist[0]) == 2
    for e in engs:
        e.close()


# ---------------------------------------------------------------------------------------------
# 6. the host's chain
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("niter", [4, 6])
def test_host_chain_is_the_same_chain(niter):
    s = ds.system(2560)
    out = []
    for flags in (dc.FLAGS, dc.FLAGS_ALL_SWEEPS):  # one after the other: one random-number stream per process
        h = host.HostSystem(s, dict(flags, polar_max_iter=niter), seed=11, move_factor=0.05, rot_factor=0.05)
        h.energy()  # (the device context exists now)
        h.set_option("timing", 0)  # every step of the chain publishes early and leaves its tail unlaunched
        h.mc_steps(60)
        o = h.observables()
        out.append((h.positions(), o["accept"], o["reject"], h.dipoles()["mu"], o["polarization_energy"]))
        h.close()
    a, b = out
    print("accept / reject", a[1], a[2], "U_pol %.17g comparison %.17g" % (a[4], b[4]))
    assert 0 < a[1] < 60 and a[1] + a[2] == 60
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2]
    assert np.array_equal(a[3], b[3]) and np.abs(a[3]).max() > 0
    assert abs(a[4] - b[4]) <= 1e-12 * abs(b[4])
