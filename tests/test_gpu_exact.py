"""The exact Thole dipoles (polar_iterative off: mpmc_hip_set_exact_polar, mpmc_amd/csrc/kernels_exact.h) on the device.

The reference of every accuracy check is longdouble (tests/exact_reference.py), on the engine's OWN matrix -- amatrix()
restricted to the polarizable rows -- and its own ef_static, as tests/test_gpu_pinning.py does: that isolates the solver.

Bounds.  With n rows and u = 2^-53:
  backward  |A mu - E| <= n u (|A||mu| + |E|) componentwise: the textbook bound for Cholesky and two substitutions with
            constant 1 (LAPACK's fp64 Cholesky sits at 0.005 .. 0.09 of it on these matrices);
  forward   max |mu - mu_ref| <= ||A^-1||_inf max(n u (|A||mu| + |E|)), which follows from the first;
  energy    |U_pol - U_ref| <= 1e-12 sum |1/2 mu_i E_i|, the project's convention (LAPACK: <= 1.2e-16 of that sum).  Every
            iterative path is 1.6e-6 away.
Cases: S-POL boxes of 18, 63, 72, 189, 198, 387 and 1152 rows (both sides of the 64-row panel, both sides of the 64-site
block, three site blocks, 18 panels) and the triclinic framework boxes of tests/vdw_cases.py (192 and 354 rows, a frozen
framework, alpha = 0 sites interleaved).  All are positive definite, which the tests assert on the downloaded matrix.
"""
import numpy as np
import pytest

import exact_reference as xr
import vdw_cases as vc
from mpmc_amd import engine, synth
from pair_reference import _molecule_index

pytestmark = pytest.mark.gpu

FLAGS = dict(temperature=77.0, polarization=1, polar_damp=2.1304, polar_iterative=0)
SPOL = (10, 35, 40, 105, 110, 215, 640)
CASES = ["spol%d" % n for n in SPOL] + ["box70", "box130"]
U = 2.0 ** -53


def _system(case):
    return synth.s_pol(int(case[4:])) if case.startswith("spol") else vc.system(case)


def _engine(s, flags=FLAGS):
    e = engine.Engine(len(s["alpha"]))
    e.load_system(s, flags)
    return e


def _all(e, r=None):
    """every result field and the four per-atom vectors of one evaluation, as comparable python objects"""
    out = dict(e.energy() if r is None else r)
    for k, v in e.dipoles().items():
        out[k] = v.tobytes()
    return out


def _fresh(s, flags=FLAGS):
    e = _engine(s, flags)
    try:
        return _all(e)
    finally:
        e.close()


def _block(e, s):
    """(mask, A restricted to the polarizable rows, as downloaded)"""
    pol = np.repeat(np.asarray(s["alpha"]) != 0.0, 3)
    return pol, e.amatrix()[np.ix_(pol, pol)]


_solved = {}


def solved(case):
    """one evaluation of a case and its longdouble reference, made once and shared (never modified)"""
    if case not in _solved:
        s = _system(case)
        e = _engine(s)
        try:
            r = e.energy()
            d = e.dipoles()
            pol, A = _block(e, s)
        finally:
            e.close()
        E = d["ef_static"].reshape(-1)[pol]
        mu = d["mu"].reshape(-1)
        ref = xr.solve(A, E)
        _solved[case] = dict(s=s, r=r, d=d, pol=pol, A=A, E=E, mu=mu[pol], mu_all=mu, ref=ref,
                             bound=xr.backward_bound(A, mu[pol], E))
    return _solved[case]


def _assert_backward(A, mu, E, what):
    res = np.abs(np.array(A, dtype=xr.LD) @ np.array(mu, dtype=xr.LD) - np.array(E, dtype=xr.LD))
    bound = xr.backward_bound(A, mu, E)
    worst = float((res / bound).max())
    print("%s: %d rows, backward error %.3g of the bound" % (what, len(E), worst))
    assert np.all(res <= bound), (what, worst)


@pytest.mark.parametrize("case", CASES)
def test_matrix_is_positive_definite_and_rows_are_as_stated(case):
    c = solved(case)
    rows = {"spol10": 18, "spol35": 63, "spol40": 72, "spol105": 189, "spol110": 198, "spol215": 387, "spol640": 1152,
            "box70": 192, "box130": 354}[case]
    assert c["A"].shape == (rows, rows)
    assert np.linalg.eigvalsh(c["A"]).min() > 0.0
    assert np.abs(c["E"]).max() > 0.0


@pytest.mark.parametrize("case", CASES)
def test_backward_error(case):
    c = solved(case)
    _assert_backward(c["A"], c["mu"], c["E"], case)


@pytest.mark.parametrize("case", CASES)
def test_forward_error(case):
    c = solved(case)
    ninv = np.abs(np.linalg.inv(c["A"])).sum(axis=1).max()
    err = float(np.abs(np.array(c["mu"], dtype=xr.LD) - c["ref"]).max())
    allowed = float(ninv * c["bound"].max())
    print("%s: forward error %.3g, allowed %.3g" % (case, err, allowed))
    assert err <= allowed, (case, err, allowed)


@pytest.mark.parametrize("case", CASES)
def test_energy(case):
    c = solved(case)
    E = np.array(c["E"], dtype=xr.LD)
    uref = float(-0.5 * (c["ref"] @ E))
    scale = float(np.abs(0.5 * c["ref"] * E).sum())
    got = c["r"]["polarization_energy"]
    print("%s: U_pol %.17g, reference %.17g, |diff| / sum|terms| = %.3g" % (case, got, uref, abs(got - uref) / scale))
    assert abs(got - uref) <= 1e-12 * scale, (case, got, uref, scale)


@pytest.mark.parametrize("case", CASES)
def test_other_sites_and_result_fields(case):
    c = solved(case)
    assert np.all(c["mu_all"][~c["pol"]] == 0.0)
    assert c["r"]["polar_iterations"] == 0 and c["r"]["iter_success"] == 0 and c["r"]["dipole_rrms"] == 0.0
    assert c["r"]["status"] == 0
    # the reference leaves both untouched on this path
    assert not c["d"]["ef_induced"].any() and not c["d"]["ef_induced_change"].any()


@pytest.mark.parametrize("case", CASES)
def test_end_to_end_against_the_converged_iteration(case):
    """tests/test_gpu_pinning.py:63's number: the same engine, iterating to 1e-10 Debye"""
    c = solved(case)
    it = _fresh(c["s"], dict(temperature=77.0, polarization=1, polar_damp=2.1304, polar_max_iter=0, polar_precision=1e-10))
    assert it["iter_success"] == 0 and it["polar_iterations"] > 3
    uit = it["polarization_energy"]
    assert abs(c["r"]["polarization_energy"] - uit) <= 1e-7 * abs(uit), (case, c["r"]["polarization_energy"], uit)


# ---- bits ----------------------------------------------------------------------------------------------------------------

def _solved_all(case):
    c = solved(case)
    out = dict(c["r"])
    for k, v in c["d"].items():
        out[k] = v.tobytes()
    return out


def test_two_contexts_and_begin_end_agree_bit_for_bit():
    s = _system("spol110")
    want = _solved_all("spol110")
    assert _fresh(s) == want
    e = _engine(s)
    try:
        e.energy_begin()
        assert _all(e, e.energy_end()) == want
        assert _all(e) == want  # nothing moved: the same record again
    finally:
        e.close()


def _later_molecule(s, sites):
    """a movable molecule of `sites` atoms with a polarizable site, past the first 64 atoms when there is one"""
    mol = _molecule_index(s["molecule"])
    best = None
    for m in range(mol.max() + 1):
        at = np.flatnonzero(mol == m)
        if len(at) == sites and not np.asarray(s["frozen"])[at].any() and (np.asarray(s["alpha"])[at] != 0.0).any():
            best = m
            if at[0] >= 64:
                break
    assert best is not None
    return best


@pytest.mark.parametrize("case", ["box70", "spol110"])
def test_update_atoms_leaves_the_bits_of_a_fresh_context(case):
    s = _system(case)
    e = _engine(s)
    try:
        before = _all(e)
        assert before == _solved_all(case)
        for step, (shift, rot) in enumerate([((0.21, -0.13, 0.08), 11), ((-0.3, 0.2, 0.1), None)]):
            s, first, pos = vc.moved(s, _later_molecule(s, 5), shift, rot)
            e.update_atoms(first, pos)
            got, want = _all(e), _fresh(s)
            assert got == want, (case, step, [k for k in got if got[k] != want[k]])
            assert got["polarization_energy"] != before["polarization_energy"]
            if step == 0:
                pol, A = _block(e, s)
                d = e.dipoles()
                _assert_backward(A, d["mu"].reshape(-1)[pol], d["ef_static"].reshape(-1)[pol], case + " moved")
    finally:
        e.close()


def test_scale_box_and_second_upload_leave_the_bits_of_a_fresh_context():
    s = _system("box70")
    e = engine.Engine(300)  # (room for the second system; more padding rows than the fresh contexts have)
    e.load_system(s, FLAGS)
    try:
        before = _all(e)
        mol = _molecule_index(s["molecule"])
        first = np.array([np.flatnonzero(mol == m)[0] for m in range(mol.max() + 1)])
        basis = np.asarray(s["basis"]) * 1.01
        delta = 0.01 * s["pos"][first]
        assert e.scale_box(basis, delta)
        t = dict(s, basis=basis, pos=s["pos"] + delta[mol])
        got, want = _all(e), _fresh(t)
        assert got == want, [k for k in got if got[k] != want[k]]
        assert got["polarization_energy"] != before["polarization_energy"]
        # a second upload, of another system: the setting persists, nothing of the first configuration does
        s2 = _system("spol110")
        e.load_system(s2, FLAGS)
        assert _all(e) == _solved_all("spol110")
    finally:
        e.close()


def test_mode_off_again_is_a_context_that_never_had_it_on():
    s = _system("spol110")
    flags = dict(synth.FLAGS_POL_JACOBI)
    want = _fresh(s, flags)
    e = _engine(s, dict(flags, polar_iterative=0))
    try:
        on = _all(e)
        e.load_system(s, flags)  # (no polar_iterative among them: load_system switches the mode off)
        assert _all(e) == want
        assert on["polarization_energy"] != want["polarization_energy"]
        e.set_exact_polar(True)  # the switch alone, on a live configuration
        assert _all(e) == on
        e.set_exact_polar(False)
        assert _all(e) == want
    finally:
        e.close()


# ---- not positive definite --------------------------------------------------------------------------------------------------

def test_not_positive_definite_is_reported_and_falls_back():
    s = dict(vc.system("clip"))
    s["charge"] = np.array([0.3, -0.3, 0.3, -0.3, 0.3, -0.3]) * synth.E2REDUCED
    flags = dict(FLAGS, polar_damp=10.0)
    e = _engine(s, flags)
    try:
        r = e.energy()
        d = e.dipoles()
        pol, A = _block(e, s)
        assert np.linalg.eigvalsh(A).min() < 0.0
        assert np.abs(d["ef_static"]).max() > 0.0
        assert r["iter_success"] == 1 and r["polar_iterations"] == 0
        assert np.array_equal(d["mu"], np.asarray(s["alpha"])[:, None] * d["ef_static"])
        assert np.isfinite(r["polarization_energy"]) and r["polarization_energy"] != 0.0
        with pytest.raises(engine.EngineError, match="not positive definite"):
            e.polarizability_tensor()
        # the flag is that call's alone: the close pair moved 4 A apart
        pos = s["pos"][1:2] + np.array([4.0 - 1.2, 0.0, 0.0])
        e.update_atoms(1, pos)
        r = e.energy()
        assert r["iter_success"] == 0
        t = dict(s, pos=np.vstack([s["pos"][:1], pos, s["pos"][2:]]))
        d = e.dipoles()
        pol, A = _block(e, t)
        assert np.linalg.eigvalsh(A).min() > 0.0
        _assert_backward(A, d["mu"].reshape(-1)[pol], d["ef_static"].reshape(-1)[pol], "clip, moved apart")
    finally:
        e.close()


# ---- the polarizability tensor ----------------------------------------------------------------------------------------------

def _sites(pos, alpha, L=60.0):
    n = len(pos)
    z = np.zeros(n)
    return synth._finish(np.array(pos, dtype=float), z, np.full(n, alpha), z, z, np.full(n, 16.0), np.ones(n), z, L)


def test_tensor_of_one_site_is_alpha():
    e = _engine(_sites([[1.0, 2.0, 3.0]], 1.1))
    try:
        e.energy()
        C = e.polarizability_tensor()
    finally:
        e.close()
    print("one site: C_pp / alpha - 1 =", np.diag(C) / 1.1 - 1.0)
    assert np.all(C[~np.eye(3, dtype=bool)] == 0.0)
    assert np.all(np.abs(np.diag(C) - 1.1) <= 2.0 * np.spacing(1.1))


def test_tensor_of_two_sites_is_the_closed_form():
    alpha, r, damp = 1.1, 2.3, 2.1304
    e = _engine(_sites([[0.5, -1.0, 0.0], [0.5, -1.0, r]], alpha))
    try:
        e.energy()
        C = e.polarizability_tensor()
    finally:
        e.close()
    cxx, czz = (float(v) for v in xr.two_site_tensor(alpha, r, damp))
    print("two sites: C_xx %.15g (closed form %.15g), C_zz %.15g (%.15g)" % (C[0, 0], cxx, C[2, 2], czz))
    assert abs(cxx - 2.040147173883) < 1e-11 and abs(czz - 2.491797607119) < 1e-11  # the recomputation reads as the issue does
    for got, want in ((C[0, 0], cxx), (C[1, 1], cxx), (C[2, 2], czz)):
        assert abs(got - want) <= 1e-13 * abs(want), (got, want)
    assert np.all(np.abs(C[~np.eye(3, dtype=bool)]) <= 1e-13 * cxx)


def test_tensor_of_box21_matches_the_block_sums():
    s = vc.system("box21")
    e = _engine(s)
    try:
        e.energy()
        C = e.polarizability_tensor()
        pol, A = _block(e, s)
    finally:
        e.close()
    assert np.linalg.eigvalsh(A).min() > 0.0
    ref, scale = xr.tensor(A)
    tol = 1e-12 * float(scale)
    print("box21: max |C - C_ref| = %.3g, allowed %.3g" % (float(np.abs(C - ref).max()), tol))
    assert np.all(np.abs(C - ref) <= tol)
    assert np.all(np.abs(C - C.T) <= tol)


def test_tensor_entry_refuses_by_name():
    s = _system("spol10")
    e = _engine(s, dict(synth.FLAGS_POL_JACOBI))
    try:
        e.energy()
        with pytest.raises(engine.EngineError, match="exact dipoles are off"):
            e.polarizability_tensor()
        e.load_system(s, FLAGS)
        with pytest.raises(engine.EngineError, match="no energy\\(\\)"):
            e.polarizability_tensor()
        e.energy()
        assert np.all(np.isfinite(e.polarizability_tensor()))
    finally:
        e.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flag", ["polar_palmo", "polar_zodid"])
def test_energy_refuses_solver_variants_by_name(flag):
    e = _engine(_system("spol10"), dict(FLAGS, **{flag: 1}))
    try:
        with pytest.raises(engine.EngineError, match=flag):
            e.energy()
    finally:
        e.close()


def test_energy_refuses_polarvdw_by_name():
    s = vc.system("box21")
    e = _engine(s, dict(vc.FLAGS, polar_iterative=0))
    try:
        with pytest.raises(engine.EngineError, match="polarvdw"):
            e.energy()
    finally:
        e.close()


def test_insert_molecule_asks_for_an_upload():
    s = _system("spol10")
    e = engine.Engine(64)
    try:
        e.load_system(s, FLAGS)
        e.energy()
        k = slice(0, 5)
        assert e.insert_molecule(s["pos"][k] + 0.7, s["charge"][k], s["alpha"][k], s["epsilon"][k], s["sigma"][k],
                                 s["mass"][k]) is None
        assert e.remove_molecule(0, 5) is False
    finally:
        e.close()


def test_a_parameter_set_without_iteration_count_needs_the_mode():
    s = _system("spol10")
    e = _engine(s, dict(FLAGS, polar_max_iter=0))  # accepted: neither polar_max_iter nor polar_precision
    try:
        e.energy()
        e.set_exact_polar(False)
        with pytest.raises(engine.EngineError, match="polar_max_iter"):
            e.energy()
    finally:
        e.close()
