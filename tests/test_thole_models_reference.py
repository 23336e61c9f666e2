"""CPU: the longdouble reference of the linear / undamped / polar_wolf_full dipole tensors (tests/thole_models_reference.py)
against closed forms, the reference's exclusion rule, and the digits the reference program printed for the inputs of
tests/golden/thole_models/."""
import json
import os

import numpy as np
import pytest

import exact_reference as xref
import pair_reference as pr
import polar_reference as pref
import thole_models_reference as tm
from mpmc_amd import synth

LD = np.longdouble
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "thole_models")
ALPHA, DAMP = 0.6938, 2.1304


def blocks(t):
    """(T_xx, T_zz, dT_xx, dT_zz) of the pair (0, 1) of a two-site tensor"""
    return t.T[0, 3], t.T[2, 5], t.dT[0, 3], t.dT[2, 5]


def read_fixture(name):
    """(system, flags) of tests/golden/thole_models/<name>.in, from the files the reference program read"""
    kw = {}
    for line in open(os.path.join(GOLD, name + ".in")).read().splitlines():
        t = line.split()
        kw[t[0]] = t[1:]
    rows = [l.split() for l in open(os.path.join(GOLD, kw["pqr_input"][0])).read().splitlines() if l.startswith("ATOM")]
    col = lambda k: np.array([float(r[k]) for r in rows])
    s = dict(pos=np.stack([col(6), col(7), col(8)], axis=1), mass=col(9), charge=col(10) * synth.E2REDUCED, alpha=col(11),
             epsilon=col(12), sigma=col(13), molecule=np.array([int(r[5]) for r in rows], dtype=np.int32),
             frozen=np.array([r[4] == "F" for r in rows], dtype=np.int32),
             basis=np.array([[float(v) for v in kw["basis%d" % k]] for k in (1, 2, 3)]))
    onoff = lambda k: int(kw.get(k, ["off"])[0] == "on")
    flags = dict(temperature=float(kw["temperature"][0]), polarization=1, polar_damp=float(kw.get("polar_damp", ["0"])[0]),
                 polar_damp_type=kw["polar_damp_type"][0], polar_wolf_full=onoff("polar_wolf_full"), polar_wolf=onoff("polar_wolf"),
                 polar_iterative=onoff("polar_iterative"), polar_max_iter=int(kw.get("polar_max_iter", ["0"])[0]))
    return s, flags


def fixture_names():
    return sorted(json.load(open(os.path.join(GOLD, "reference_energies.json"))))


@pytest.mark.parametrize("r", [1.9, 3.7, 11.0])
def test_off_closed_forms(r):
    t = tm.ModelTensor(tm.two_site(r, ALPHA, DAMP), DAMP, "off")
    txx, tzz, dxx, dzz = blocks(t)
    assert abs(txx - 1 / LD(r) ** 3) <= dxx and abs(tzz + 2 / LD(r) ** 3) <= dzz
    assert dxx < 1e-14 / r ** 3 and dzz < 1e-13 / r ** 3  # the bound is no wider than a few dozen roundings
    assert t.T[0, 4] == 0 and t.T[0, 5] == 0 and np.array_equal(t.T, t.T.T)


def test_off_exclusions():
    """es_excluded (pairs.c:61-77): one molecule, or either charge exactly 0.0 -- no coupling at all"""
    for kw in (dict(molecule=(3, 3)), dict(charge=(0.0, -1.0)), dict(charge=(1.0, 0.0))):
        t = tm.ModelTensor(tm.two_site(2.5, ALPHA, DAMP, **kw), DAMP, "none")
        assert not t.T.any() and not t.dT.any(), kw
    t = tm.ModelTensor(tm.two_site(2.5, ALPHA, DAMP, charge=(1e-300, -1e-300)), DAMP, "off")
    assert t.T[0, 3] != 0  # a tiny charge is not 0.0
    # the other models do not look at charges or molecules
    for damping in ("linear", "exponential"):
        a = tm.ModelTensor(tm.two_site(2.5, ALPHA, DAMP, molecule=(3, 3), charge=(0.0, 0.0)), DAMP, damping)
        b = tm.ModelTensor(tm.two_site(2.5, ALPHA, DAMP), DAMP, damping)
        assert np.array_equal(a.T, b.T) and a.T[0, 3] != 0


def test_linear_closed_forms():
    s = DAMP * (ALPHA * ALPHA) ** (1.0 / 6.0)
    # v = 1/2: damp1 = (4 - 3/2) / 8 = 5/16, damp2 = 1/16: T_xx = (5/16) / r^3, T_zz = (5/16 - 3/16) / r^3
    r = 0.5 * s
    t = tm.ModelTensor(tm.two_site(r, ALPHA, DAMP), DAMP, "linear")
    txx, tzz, dxx, dzz = blocks(t)
    assert abs(txx - LD(5) / 16 / LD(r) ** 3) <= dxx and abs(tzz - LD(2) / 16 / LD(r) ** 3) <= dzz
    assert dxx < 1e-13 * abs(float(txx)) and not t.near_tie.any()
    cxx, czz = tm.closed_forms(r, ALPHA, DAMP, "linear")
    assert abs(txx - cxx) <= dxx and abs(tzz - czz) <= dzz
    # just outside and just inside r = s: undamped exactly / damped, and continuous (damp1 flat, damp2 slope 4 at v = 1)
    for sign in (+1, -1):
        r = s * (1.0 + sign * 2.0 ** -40)
        t = tm.ModelTensor(tm.two_site(r, ALPHA, DAMP), DAMP, "linear")
        txx, tzz, dxx, dzz = blocks(t)
        assert not t.near_tie.any()  # 2^-40 is far outside the few-ulp uncertainty of s
        if sign > 0:
            assert abs(txx - 1 / LD(r) ** 3) <= dxx and abs(tzz + 2 / LD(r) ** 3) <= dzz
        else:
            v = LD(r) / (LD(DAMP) * np.power(LD(ALPHA) * LD(ALPHA), LD(1.0 / 6.0)))
            assert abs(txx - (4 - 3 * v) * v ** 3 / LD(r) ** 3) <= dxx
            assert abs(tzz - ((4 - 3 * v) * v ** 3 - 3 * v ** 4) / LD(r) ** 3) <= dzz
            assert abs(float(txx * LD(r) ** 3 - 1)) < 2.0 ** -60  # 6 (2^-40)^2 and longdouble's own roundings
            assert abs(float((txx - tzz) / 3 * LD(r) ** 3 - 1) + 4 * 2.0 ** -40) < 1e-14  # (v is 1 - 2^-40 to the rounding of the fp64 s)
    # ON the branch point (to a rounding): whichever way r < s is decided, the other branch is inside the bound
    t = tm.ModelTensor(tm.two_site(s, ALPHA, DAMP), DAMP, "linear")
    txx, tzz, dxx, dzz = blocks(t)
    assert t.near_tie[0, 1] and t.near_tie[1, 0]
    assert abs(txx - 1 / LD(s) ** 3) <= dxx and abs(tzz + 2 / LD(s) ** 3) <= dzz
    v = LD(1) - LD(2.0) ** -52
    assert abs(txx - (4 - 3 * v) * v ** 3 / LD(s) ** 3) <= dxx and abs(tzz - ((4 - 3 * v) * v ** 3 - 3 * v ** 4) / LD(s) ** 3) <= dzz
    assert dzz < 1e-13 / s ** 3


def test_linear_alpha_zero_is_undamped():
    """s = 0 for a site without polarizability: no damping (download_amatrix() covers such sites)"""
    s = tm.two_site(0.8, ALPHA, DAMP)
    s["alpha"] = np.array([ALPHA, 0.0])
    t = tm.ModelTensor(s, DAMP, "linear", all_sites=True)
    txx, tzz, dxx, dzz = blocks(t)
    assert abs(txx - 1 / LD(0.8) ** 3) <= dxx and abs(tzz + 2 / LD(0.8) ** 3) <= dzz
    A, dA = pref.amatrix(t, s)
    assert A[0, 0] == 1 / LD(ALPHA) and A[3, 3] == LD(pref.MAXVALUE) and A[0, 3] == txx


def test_wolf_full_closed_forms():
    L = 24.0
    rc = L / 2
    # r = rc exactly (a half-box tie): c3 = damp1 / r^3 - wdamp1 / rc^3 is EXACTLY 0; the bound is that of the parts
    t = tm.ModelTensor(tm.two_site(rc, ALPHA, DAMP, L=L), DAMP, "exponential", wolf_full=True)
    assert t.cutoff == rc and t.rimg[0, 1] == rc
    txx, tzz, dxx, dzz = blocks(t)
    assert txx == 0 and t.c3[0, 1] == 0.0
    w1, w2, _, _ = tm.wolf_constants(DAMP, rc)
    assert dxx >= 2 * float(pref.U * w1 / LD(rc) ** 3) and dxx < 1e-13 / rc ** 3  # |A| + |B|, not |A - B| = 0
    assert tzz == 0  # c5 = damp2 / r^5 - wdamp2 / (r^2 rc^3) vanishes there as well
    assert dzz >= 3 * rc * rc * 2 * float(pref.U * w2 / LD(rc) ** 5)
    # inside: the closed form; the plain exponential tensor differs by exactly the Wolf part
    for r in (2.0, 7.5, 11.999):
        t = tm.ModelTensor(tm.two_site(r, ALPHA, DAMP, L=L), DAMP, "exponential", wolf_full=True)
        e = tm.ModelTensor(tm.two_site(r, ALPHA, DAMP, L=L), DAMP, "exponential")
        p = pref.Tensor(tm.two_site(r, ALPHA, DAMP, L=L), DAMP)
        txx, tzz, dxx, dzz = blocks(t)
        cxx, czz = tm.closed_forms(r, ALPHA, DAMP, "exponential", True, rc)
        assert abs(txx - cxx) <= dxx and abs(tzz - czz) <= dzz
        assert np.array_equal(e.T, p.T) and np.array_equal(e.dT, p.dT)  # the module's exponential model IS polar_reference's
        assert abs((e.T[0, 3] - txx) - w1 / LD(rc) ** 3) < 1e-18
    # beyond the cutoff (a pair along the box diagonal): the subtraction still applies (no r < rc test)
    s = tm.two_site(1.0, ALPHA, DAMP, L=L)
    s["pos"][1] = [11.0, 11.0, 11.0]
    t = tm.ModelTensor(s, DAMP, "exponential", wolf_full=True)
    e = tm.ModelTensor(s, DAMP, "exponential")
    assert t.rimg[0, 1] > rc
    assert abs((e.T[0, 0 + 3] - t.T[0, 3]) - (w1 / LD(rc) ** 3 - 3 * 121 * w2 / (LD(363) * LD(rc) ** 3))) < 1e-18


def test_wolf_full_coincident_sites():
    """rimg == 0: the dyad is 0 and damp1 MAXVALUE = 0, what stays is -wdamp1 / rc^3 on the block's diagonal"""
    s = tm.two_site(0.0, ALPHA, DAMP, L=24.0)
    t = tm.ModelTensor(s, DAMP, "exponential", wolf_full=True)
    w1, _, _, _ = tm.wolf_constants(DAMP, 12.0)
    assert t.T[0, 3] == t.T[1, 4] == t.T[2, 5] == -w1 / LD(12.0) ** 3 and t.T[0, 4] == 0
    assert not tm.ModelTensor(s, DAMP, "linear").T.any()  # v = 0: damp = 0


def test_model_tensor_runs_the_solver_machinery():
    """solve / check / check_energy / amatrix / without of polar_reference take a ModelTensor as they are"""
    s = synth.s_pol(40)
    E = np.random.default_rng(3).normal(size=(40, 3))
    for damping, wf in (("linear", False), ("off", False), ("exponential", True)):
        t = tm.ModelTensor(s, DAMP, damping, wolf_full=wf)
        res = pref.solve(t, s, dict(polar_max_iter=4, polar_gs_ranked=1, polar_palmo=1, polar_gamma=1.03), E)
        got = {k: res[k].astype(np.float64) for k in ("mu", "ef_induced", "ef_induced_change")}
        pref.check(t, s, res, got, keys=("mu", "ef_induced", "ef_induced_change"))
        pref.check_energy(res, float(res["upol"]))
        A, dA = pref.amatrix(t, s)
        assert np.array_equal(A, A.T) and (dA >= 0).all()
        atom = int(t.view[5])
        w = t.without(atom)
        assert isinstance(w, tm.ModelTensor) and w.nv == t.nv - 1 and atom not in w.view and w.damping == t.damping
    with pytest.raises(AssertionError):
        pref.solve(t, s, dict(polar_max_iter=4, polar_wolf_full=1), E)  # the setting belongs to the tensor, not to params


def test_bound_is_tight_on_regular_geometry():
    """a loose bound cannot hide a failure: on S-POL(320) every model's dT stays below 1e-13 of the largest |T| entry"""
    s = synth.s_pol(320)
    for damping, wf in (("linear", False), ("off", False), ("exponential", True)):
        t = tm.ModelTensor(s, DAMP, damping, wolf_full=wf)
        assert t.dT.max() < 1e-13 * float(np.abs(t.T).max()), damping


@pytest.mark.parametrize("name", fixture_names())
def test_reference_program_digits(name):
    """every polarization digit the reference program printed for the golden inputs (OUTPUT line: 5 decimals; energy file:
    6), from this module: field from pair_reference, dipoles from polar_reference.solve (ten Jacobi sweeps) or from a
    longdouble Cholesky solve (polar_iterative off)"""
    want = json.load(open(os.path.join(GOLD, "reference_energies.json")))[name]
    s, f = read_fixture(name)
    fparams = dict(temperature=f["temperature"], polarization=1, polar_damp=f["polar_damp"],
                   polar_wolf=int(f["polar_wolf"] or f["polar_wolf_full"]))  # thole_field.c:32
    E = pr.sums(pr.pair_table(s, fparams), s, fparams)["ef_static"]
    t = tm.ModelTensor(s, f["polar_damp"], f["polar_damp_type"], wolf_full=bool(f["polar_wolf_full"]))
    if f["polar_iterative"]:
        upol = pref.solve(t, s, dict(polar_max_iter=f["polar_max_iter"]), E)["upol"]
    else:
        Ev = E[t.view].reshape(-1).astype(LD)
        upol = LD(-0.5) * (xref.solve(tm.view_matrix(t), Ev) @ Ev)
    assert "%.5f" % float(upol) == want["printed"]["polarization energy"]
    assert "%.6f" % float(upol) == want["energy_dat"]["polar"]
