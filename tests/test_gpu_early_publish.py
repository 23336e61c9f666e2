"""U_pol from the finish of sweep m = ceil(n / 2) of a fixed-count plain Jacobi solve, and the result record published
behind that finish (engine_polar.inc run_polarization(); engine.hip enqueue_direct();
kernels_coef.h pair_finish_kernel).

With mu_0 = alpha E, s_k = T mu_{k-1}, mu_k = alpha (E - s_k) and T symmetric,

    sum_i mu_n.E = sum_i [ mu_m.E - (mu_m - mu_{m-1}).s_{n-m} ]

so the energy of n sweeps is known after m of them.  The comparison engine is the same call sequence under polar_rrms = 1,
which runs all n sweeps and sums mu_n.E, as in tests/test_gpu_deferred_sweep.py, whose shapes, helpers and bounds these
tests use: U_pol is a re-associated sum of the same terms, 1e-12 relative; everything else bit for bit.

A call that is timed with events keeps the publication at the end of the chain, and the sweep counter exists only on
timed calls; so the engine under test runs with timing 0 (early publication on every call) and a third engine with
timing 2 counts the launches and must agree with it to the bit.  The engine has no option for the placement (its option
table is fixed by tests/test_gpu_parity.py), so "timing" is also the switch of the placement test: 0 publishes early in
every call, 2 at the end of the chain in every call.
"""
import numpy as np
import pytest

import deferred_sweep_cases as dc
import test_gpu_deferred_sweep as ds
from mpmc_amd import host

gpu = pytest.mark.gpu
ALL = ds.SAME + ("polar_iterations",)


def same_energies(got, want, what):
    """U_pol within 1e-12 relative of the comparison's; the other terms, and the sum taken with the own U_pol, to the bit"""
    up, uq = got["polarization_energy"], want["polarization_energy"]
    print(what, "U_pol %.17g comparison %.17g rel %.3g" % (up, uq, abs(up - uq) / abs(uq)))
    assert abs(up - uq) <= 1e-12 * abs(uq), what
    for k in ("rd_energy", "coulombic_energy", "polar_iterations"):
        assert got[k] == want[k], (what, k)
    assert got["energy"] == want["rd_energy"] + want["coulombic_energy"] + up, what
    assert abs(got["energy"] - want["energy"]) <= 1e-12 * abs(uq), what


def same_bits(ra, rb, da, db, what):
    for k in ALL:
        assert ra[k] == rb[k], (what, k, ra[k], rb[k])
    ds.same_vectors(da, db, what)


# ---------------------------------------------------------------------------------------------
# 1. energy and dipoles against the old path
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("niter", [2, 3, 4, 5, 6, 7])
@pytest.mark.parametrize("n", dc.SIZES)
def test_energy_and_dipoles_against_all_sweeps(n, niter):
    s = ds.system(n)
    a = ds.make(s, dict(dc.FLAGS, polar_max_iter=niter), timing=0)
    t = ds.make(s, dict(dc.FLAGS, polar_max_iter=niter), timing=2)
    b = ds.make(s, dict(dc.FLAGS_ALL_SWEEPS, polar_max_iter=niter))
    first, new = dc.molecule_move(s, 100)
    for tag in ("first", "moved"):
        if tag == "moved":
            for e in (a, t, b):
                e.update_atoms(first, new)
        ra, rt, rb = a.energy(), t.energy(), b.energy()
        same_energies(ra, rb, (n, niter, tag))
        assert ra["polar_iterations"] == niter
        assert t.timings()["sweep_count"] == niter - 1
        da, dt, db = a.dipoles(), t.dipoles(), b.dipoles()
        assert t.timings()["sweep_count"] == niter
        ds.same_vectors(da, db, (n, niter, tag))
        same_bits(ra, rt, da, dt, (n, niter, tag, "timed call"))
    for e in (a, t, b):
        e.close()


# ---------------------------------------------------------------------------------------------
# 2. the placement changes no bit
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("niter", [4, 5])
@pytest.mark.parametrize("n", dc.SIZES)
def test_placement_changes_no_bit(n, niter):
    s = ds.system(n)
    # (timing 0: behind the finish of sweep ceil(n / 2); timing 2: behind sweep n - 1, as before)
    engs = [ds.make(s, dict(dc.FLAGS, polar_max_iter=niter), timing=v) for v in (0, 2)]
    first, new = dc.molecule_move(s, 100)
    for tag in ("first", "moved", "again"):
        if tag == "moved":
            for e in engs:
                e.update_atoms(first, new)
        (ra, da), (rb, db) = [(e.energy(), e.dipoles()) for e in engs]
        same_bits(ra, rb, da, db, (n, niter, tag))
    for e in engs:
        e.close()


# ---------------------------------------------------------------------------------------------
# 3. work still in flight: n = 6 leaves sweeps 4 and 5 queued behind the record when energy() returns
# ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("action", ["noted_move", "remove_insert", "box"])
@pytest.mark.parametrize("n", dc.SIZES)
def test_state_changes_against_sweeps_in_flight(n, action):
    s = ds.system(n)
    flags = dict(dc.FLAGS, polar_max_iter=6)
    a = ds.make(s, flags, timing=0)
    a.energy()
    after, _ = ds.ACTIONS[action](a, s)  # at once: nothing waits for the device in between
    ra = a.energy()
    da = a.dipoles()
    fresh = ds.make(after, flags, timing=0)
    rf = fresh.energy()
    same_bits(ra, rf, da, fresh.dipoles(), (n, action, "fresh context"))
    # ... and the dipoles of an evaluation whose record went out early, asked for at once
    b = ds.make(after, dict(flags, polar_rrms=1))
    rb = b.energy()
    same_energies(rf, rb, (n, action, "all sweeps"))
    rf2 = fresh.energy()
    ds.same_vectors(fresh.dipoles(), b.dipoles(), (n, action, "dipoles at once"))
    for k in ALL:
        assert rf2[k] == rf[k], k
    for e in (a, b, fresh):
        e.close()


# ---------------------------------------------------------------------------------------------
# 4. a short chain through the host layer
# ---------------------------------------------------------------------------------------------
@gpu
def test_host_chain_is_the_same_chain():
    s = ds.system(2560)
    out = []
    for flags in (dc.FLAGS, dc.FLAGS_ALL_SWEEPS):  # one after the other: one random-number stream per process
        h = host.HostSystem(s, flags, seed=23, move_factor=0.05, rot_factor=0.05)
        h.energy()  # (the device context exists now)
        h.set_option("timing", 0)  # every step of the chain publishes early
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


# ---------------------------------------------------------------------------------------------
# 5. the identity, on the CPU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("niter", [2, 3, 4, 5, 6, 7])
def test_identity_in_numpy(niter):
    rng = np.random.default_rng(niter)
    nsite = 40
    T = rng.normal(size=(3 * nsite, 3 * nsite))
    T = 0.02 * (T + T.T)  # symmetric; small enough that the iteration contracts
    alpha = np.repeat(rng.uniform(0.5, 2.0, size=nsite), 3)
    alpha[np.repeat(rng.random(nsite) < 0.25, 3)] = 0.0
    assert np.count_nonzero(alpha == 0.0) > 0
    E = rng.normal(size=3 * nsite)
    mu = [alpha * E]
    sums = [None]
    for k in range(1, niter + 1):
        sums.append(T @ mu[k - 1])
        mu.append(alpha * (E - sums[k]))
    want = -0.5 * np.dot(mu[niter], E)
    m = (niter + 1) // 2
    got = -0.5 * (np.dot(mu[m], E) - np.dot(mu[m] - mu[m - 1], sums[niter - m]))
    print(niter, m, got, want, abs(got - want) / abs(want))
    assert abs(got - want) <= 1e-13 * abs(want)
