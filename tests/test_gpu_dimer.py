"""The dimer scans on the device (mpmc_hip_dimer_energies / mpmc_hip_dimer_grid_means, kernels_dimer.h) against the
longdouble reference of tests/dimer_reference.py:

* list form: es and rd within 1e-12 * sum |terms|; U_pol, every dipole and the sweep count within that module's DERIVED
  forward-error bound, at the smallest shapes at which the kernel can go wrong (1+1 .. 16+16 sites; no polarizable site on
  one molecule, on both; zero-charge and zero-epsilon sites mixed in), on every solver path, tensor model, mixing rule and
  PHAHST switch;
* a placement's numbers are those of that placement alone: `==` at every position of a batch, at the batch sizes around the
  wave and the kernel's chunk, and through the grid form;
* the grid form's means are, with `==`, the fixed-order sum the documentation states, recomputed on the host from the list
  form's outputs;
* the resident configuration is untouched (`==` on every field of energy() before and after), and a call between
  energy_begin() and energy_end() is refused by name;
* the periodic engine on the same dimer in a 10^6 A cubic cell agrees on rd_energy and polarization_energy.

Every comparison prints a `DIMER` line with max(diff / bound); profiles/dimer_scan/README.md keeps the largest."""
import functools
import itertools

import numpy as np
import pytest

import dimer_cases as dc
import dimer_reference as dr
from mpmc_amd import engine, synth

pytestmark = pytest.mark.gpu
CHUNK = engine.DIMER_CHUNK


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(384, device=0)
    yield e
    e.close()


def check_against_reference(eng, a, b, conf, flags, what):
    got = eng.dimer_energies(a, b, conf, mu=True, **flags)
    n = len(a["charge"]) + len(b["charge"])
    worst = dict(es=0.0, rd=0.0, polar=0.0, mu=0.0)
    for k, c in enumerate(conf):
        want = dr.energies(a, b, c, flags)
        assert want["decisive"], "%s: placement %d: a stopping decision lies within the bound of its threshold" % (what, k)
        for key in ("es", "rd"):
            diff, bound = abs(float(dr.LD(got[key][k]) - want[key])), 1e-12 * float(want[key + "_abs"])
            assert diff <= bound, (what, k, key, got[key][k], float(want[key]), diff, bound)
            worst[key] = max(worst[key], diff / bound if bound else 0.0)
        assert got["iterations"][k] == want["iterations"] and bool(got["not_converged"][k]) == want["not_converged"], (
            what, k, got["iterations"][k], want["iterations"])
        diff = abs(float(dr.LD(got["polar"][k]) - want["polar"]))
        assert diff <= want["polar_err"], (what, k, "polar", got["polar"][k], float(want["polar"]), diff, want["polar_err"])
        worst["polar"] = max(worst["polar"], diff / want["polar_err"] if want["polar_err"] else 0.0)
        dmu = np.abs((got["mu"][k, :n].astype(dr.LD) - want["mu"]).astype(np.float64))
        assert np.all(dmu <= want["mu_err"]), (what, k, "mu", float(np.max(dmu - want["mu_err"])))
        assert np.all(got["mu"][k, n:] == 0.0)
        with np.errstate(divide="ignore", invalid="ignore"):
            worst["mu"] = max(worst["mu"], float(np.nanmax(np.where(want["mu_err"] > 0, dmu / want["mu_err"], 0.0))))
    print("DIMER %s: max diff / bound es %.3g rd %.3g polar %.3g mu %.3g" % (what, worst["es"], worst["rd"], worst["polar"],
                                                                           worst["mu"]))
    return got


@pytest.mark.parametrize("solver", sorted(dc.SOLVERS))
@pytest.mark.parametrize("shape", dc.SHAPES, ids=lambda s: "%d+%d" % s)
def test_list_form_solver_paths(eng, shape, solver):
    a, b = dc.molecule(shape[0], 1), dc.molecule(shape[1], 2)
    check_against_reference(eng, a, b, dc.placements(3, seed=shape[0]), dc.SOLVERS[solver], "%d+%d %s" % (shape + (solver,)))


@pytest.mark.parametrize("which", ["a", "b", "both"])
def test_molecules_without_polarizable_sites(eng, which):
    a = dc.molecule(5, 3, polarizable=which == "b")
    b = dc.molecule(16, 4, polarizable=which == "a")
    got = check_against_reference(eng, a, b, dc.placements(3, seed=9), dc.SOLVERS["ranked_palmo5"], "no alpha on " + which)
    if which == "both":
        assert np.all(got["polar"] == 0.0) and np.all(got["iterations"] == 0)
    else:
        assert np.all(got["polar"] != 0.0)


@pytest.mark.parametrize("model", sorted(dc.MODELS))
@pytest.mark.parametrize("shape", [(5, 5), (15, 16)], ids=lambda s: "%d+%d" % s)
def test_tensor_models(eng, shape, model):
    a, b = dc.molecule(shape[0], 5), dc.molecule(shape[1], 6)
    check_against_reference(eng, a, b, dc.placements(3, seed=11), dc.MODELS[model], "%d+%d %s" % (shape + (model,)))


@pytest.mark.parametrize("rule", sorted(dc.RD))
def test_lennard_jones_mixing_rules(eng, rule):
    a, b = dc.molecule(15, 7), dc.molecule(16, 8)
    got = check_against_reference(eng, a, b, dc.placements(4, seed=13), dc.RD[rule], "15+16 " + rule)
    assert np.all(got["es"] == 0.0) and np.all(got["polar"] == 0.0) and np.all(got["rd"] != 0.0)  # rd_only


@pytest.mark.parametrize("switches", sorted(dc.PHAHST))
def test_disp_expansion(eng, switches):
    a, b = dc.molecule(5, 9, phahst=True), dc.molecule(16, 10, phahst=True)
    check_against_reference(eng, a, b, dc.placements(4, seed=15), dc.PHAHST[switches], "5+16 phahst " + switches)


def test_n2_dimer_global_axis(eng):
    """the quaternion path: radians read as degrees, third rotation about x"""
    flags = dict(dc.SOLVERS["ranked_palmo5"], surf_global_axis=1)
    check_against_reference(eng, dc.n2(), dc.n2(), dc.placements(4, seed=17, rmin=3.0, rmax=5.0), flags, "n2 global_axis")


# ---------------------------------------------------------------------------------------------- placement independence
FLAGS = dc.SOLVERS["ranked_palmo5"]
KEYS = ("es", "rd", "polar", "iterations")


@functools.lru_cache(maxsize=None)
def _batch():
    return dc.molecule(15, 21), dc.molecule(16, 22), dc.placements(CHUNK + 1, seed=23)


@pytest.fixture(scope="module")
def whole(eng):
    a, b, conf = _batch()
    return eng.dimer_energies(a, b, conf, **FLAGS)


@pytest.mark.parametrize("nconf", [1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1])
def test_batch_sizes_and_positions(eng, whole, nconf):
    """the first nconf placements, the last nconf ones, and nconf from the middle give the bits of the whole batch"""
    a, b, conf = _batch()
    n = len(conf)
    for first in sorted({0, n - nconf, (n - nconf) // 2}):
        got = eng.dimer_energies(a, b, conf[first:first + nconf], **FLAGS)
        for key in KEYS:
            assert np.array_equal(got[key], whole[key][first:first + nconf]), (nconf, first, key)
    assert np.all(whole["polar"] != 0.0) and np.all(whole["iterations"] == 5)


def test_one_placement_through_the_grid_form(eng, whole):
    a, b, conf = _batch()
    for k in (0, 100, CHUNK):
        got = eng.dimer_grid_means(a, b, conf[k, 0], [[x] for x in conf[k, 1:]], **FLAGS)
        assert got["count"] == 1 and got["not_converged"] == 0
        for key in ("es", "rd", "polar"):
            assert got[key] == whole[key][k], (k, key)


# ---------------------------------------------------------------------------------------------- the grid form's means
def _split(total):
    """three list lengths whose product is `total`"""
    return {1: (1, 1, 1), 63: (7, 3, 3), 64: (4, 4, 4), 65: (5, 1, 13)}[total]


@pytest.mark.parametrize("sides", [(1, 1), (1, 65), (64, 63), (65, 65)], ids=lambda s: "%dx%d" % s)
def test_grid_means_are_the_stated_fixed_order_sum(eng, sides):
    a, b = dc.molecule(5, 31), dc.molecule(15, 32)
    rng = np.random.default_rng(sides[0] * 100 + sides[1])
    lists = [rng.uniform(0.0, np.pi, k) for k in _split(sides[0]) + _split(sides[1])]
    r = 6.1
    conf = np.array([(r,) + t for t in itertools.product(*lists)])
    assert len(conf) == sides[0] * sides[1]
    per = eng.dimer_energies(a, b, conf, **FLAGS)
    got = eng.dimer_grid_means(a, b, r, lists, **FLAGS)
    assert got["count"] == len(conf) and got["not_converged"] == 0
    for key in ("es", "rd", "polar"):
        assert got[key] == dr.fixed_order_mean(per[key]), (sides, key)
        assert got[key] != 0.0


def test_not_converged_is_flagged_and_counted(eng):
    """a polarization catastrophe (two sites of 3 A^3 one A apart: Jacobi diverges): the 128-sweep give-up, dipoles =
    alpha E, flag and count"""
    a = dict(pos=np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), charge=np.array([0.4, -0.4]) * dc.E2REDUCED,
             alpha=np.array([3.0, 3.0]), epsilon=np.array([10.0, 10.0]), sigma=np.array([3.0, 3.0]), mass=np.array([12.0, 16.0]))
    b = a
    flags = dict(polar_damp=dc.DAMP, polar_precision=1e-4, polar_max_iter=0)
    conf = dc.placements(3, seed=43)
    got = eng.dimer_energies(a, b, conf, mu=True, **flags)
    assert np.all(got["not_converged"]) and np.all(got["iterations"] == 128)
    for k, c in enumerate(conf):
        want = dr.energies(a, b, c, flags)
        assert want["not_converged"] and abs(float(dr.LD(got["polar"][k]) - want["polar"])) <= want["polar_err"]
    lists = [[x] for x in conf[0, 1:]]
    assert eng.dimer_grid_means(a, b, conf[0, 0], lists, **flags)["not_converged"] == 1


# ---------------------------------------------------------------------------------------------- the resident state
def test_resident_configuration_is_untouched():
    sysm, flags = synth.s_pol(320), dict(synth.FLAGS_POL_JACOBI)
    e = engine.Engine(320, device=0)
    try:
        a, b, conf = _batch()
        fresh = e.dimer_energies(a, b, conf[:5], **FLAGS)  # a context that has had no upload
        e.load_system(sysm, flags)
        before = e.energy()
        mu_before = e.dipoles()
        during = e.dimer_energies(a, b, conf[:5], **FLAGS)
        lists = [[x, x + 0.1] for x in conf[0, 1:]]
        e.dimer_grid_means(a, b, 6.0, lists, **FLAGS)
        after = e.energy()
        mu_after = e.dipoles()
        for key in before:
            assert before[key] == after[key], key
        for key in mu_before:
            assert np.array_equal(mu_before[key], mu_after[key]), key
        for key in KEYS:
            assert np.array_equal(fresh[key], during[key]), key
        e.energy_begin()
        try:
            with pytest.raises(engine.EngineError, match="dimer_energies between energy_begin"):
                e.dimer_energies(a, b, conf[:5], **FLAGS)
            with pytest.raises(engine.EngineError, match="dimer_grid_means between energy_begin"):
                e.dimer_grid_means(a, b, 6.0, lists, **FLAGS)
        finally:
            end = e.energy_end()
        for key in before:
            assert before[key] == end[key], key
    finally:
        e.close()


def test_refusals_by_name(eng):
    a, b, conf = _batch()
    big = dict(a, **{k: np.concatenate([v, v[:2]]) for k, v in a.items()})
    with pytest.raises(engine.EngineError, match="17 sites"):
        eng.dimer_energies(big, b, conf[:1], **FLAGS)
    with pytest.raises(engine.EngineError, match="polar_max_iter"):
        eng.dimer_energies(a, b, conf[:1], polar_damp=dc.DAMP, polar_max_iter=0)
    with pytest.raises(engine.EngineError, match="disp_expansion reads c6"):
        eng.dimer_energies(a, b, conf[:1], disp_expansion=1, rd_only=1)
    with pytest.raises(ValueError, match="not sg"):
        eng.dimer_energies(a, b, conf[:1], sg=1)


# ---------------------------------------------------------------------------------------------- the periodic engine
@pytest.mark.parametrize("solver", ["jacobi4", "ranked_palmo5"])
def test_periodic_engine_in_a_huge_cell_agrees(eng, solver):
    """The dimer in a 10^6 A cubic cell (the helium sample's box) through the existing kernels: rd_energy and
    polarization_energy agree with the dimer path within the sum of the two paths' bounds -- each path's own bound being
    the reference's for this placement (the cell adds no lattice translation: every image index is 0).  es is left out:
    Ewald is not the bare sum."""
    a, b = dc.molecule(15, 51), dc.molecule(16, 52)
    flags = dc.SOLVERS[solver]
    conf = dc.placements(2, seed=53)
    got = eng.dimer_energies(a, b, conf, **flags)
    n1, n2 = len(a["charge"]), len(b["charge"])
    e = engine.Engine(64, device=0)
    try:
        for k, c in enumerate(conf):
            want = dr.energies(a, b, c, flags)
            cols = {key: np.concatenate([a[key], b[key]]) for key in ("charge", "alpha", "epsilon", "sigma", "mass")}
            sysm = dict(cols, pos=want["pos"], molecule=np.array([0] * n1 + [1] * n2, dtype=np.int32),
                        frozen=np.zeros(n1 + n2, dtype=np.int32), basis=np.diag([1.0e6] * 3))
            e.load_system(sysm, dict(flags, temperature=77.0, polarization=1, rd_lrc=0))
            res = e.energy()
            assert abs(res["rd_energy"] - got["rd"][k]) <= 2e-12 * float(want["rd_abs"]), (k, res["rd_energy"], got["rd"][k])
            assert abs(res["polarization_energy"] - got["polar"][k]) <= 2.0 * want["polar_err"], (
                k, res["polarization_energy"], got["polar"][k], want["polar_err"])
            assert res["polar_iterations"] == got["iterations"][k]
            print("DIMER periodic %s: rd %.3g polar %.3g of the bound" % (
                solver, abs(res["rd_energy"] - got["rd"][k]) / (2e-12 * float(want["rd_abs"])),
                abs(res["polarization_energy"] - got["polar"][k]) / (2.0 * want["polar_err"])))
    finally:
        e.close()
