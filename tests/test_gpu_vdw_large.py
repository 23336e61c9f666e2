"""GPU tests of the coupled-dipole eigenvalue sum where the small cases of tests/test_gpu_vdw.py do not reach.

* Matrices above 1024 rows: vdw_reflect_kernel and vdw_sum_kernel are single workgroups of 1024 threads with strided loops,
  and only from n = 1025 (the sum) and n = 1027 (the reflector's norm) does any thread take a second trip.  The references
  are recorded (tests/golden/vdw_large.npz, made by tests/golden/make_vdw_large.py with the certified
  vdw_reference.prerotated_eigen_energy); tests/test_vdw_reference.py checks the record on the CPU.  Tolerance of a term:
  TOL * sum |terms| + the reference's own certified error (zero for the terms without eigenvalues).
* Spectra with exact structure (vdw_cases.EXACT): degenerate eigenvalues, a tridiagonal matrix that splits exactly.
* A zero crossing (vdw_cases.crossing): the flat tolerance cannot hold where sqrt meets an eigenvalue at 0; the bound is
  vdw_cases.crossing_bound, derived in DESIGN.md section 12 and checked against the numpy model of the solver in
  tests/test_vdw_model.py.
"""
import numpy as np
import pytest

import vdw_cases as vc
from test_gpu_vdw import _all, _engine, _fresh, _later_molecule

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", vc.LARGE)
def test_large_terms_against_the_record(name):
    ref = vc.large_reference(name)
    s = vc.system(name)
    assert ref["rows"] == vc.LARGE_ROWS[name] == vc.active_rows(s)
    assert ref["b_min"] >= vc.COND * ref["b_max"]  # the condition the tolerance rests on
    got = _fresh(s, vc.FLAGS)
    worst = 0.0
    for t in vc.LARGE_TERMS:
        want, tol = float(ref[t]), vc.TOL * float(ref["abs_" + t]) + ref.get("err_" + t, 0.0)
        err = abs(got[t] - want)
        print("%s (matrix %d): %-13s %.8f record %.8f |diff| %.3g tol %.3g |diff| / tolerance %.3g" % (
            name, ref["rows"], t, got[t], want, err, tol, err / tol))
        worst = max(worst, err / tol)
    assert got["vdw_energy"] == (got["e_total"] - got["e_iso"]) + got["lr_corr"]
    assert got["status"] == 0
    assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize("name", ["big1", "frame"])
def test_large_two_fresh_contexts_agree_to_the_bit(name):
    assert _fresh(vc.system(name), vc.FLAGS) == _fresh(vc.system(name), vc.FLAGS)


@pytest.mark.parametrize("name", ["big1", "frame"])
def test_large_update_atoms_leaves_the_bits_of_a_fresh_context(name):
    s = vc.system(name)
    e = _engine(s, vc.FLAGS)
    before = _all(e)
    for step, (kind, shift, rot) in enumerate([(vc.TYPE_FIVE, (0.21, -0.13, 0.08), 11), (vc.TYPE_ONE, (-0.3, 0.2, 0.1), None)]):
        s, first, pos = vc.moved(s, _later_molecule(s, kind), shift, rot)
        e.update_atoms(first, pos)
        got = _all(e)
        want = _fresh(s, vc.FLAGS)
        assert got == want, (name, step, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
        assert got["e_total"] != before["e_total"] and got["repulsion"] != before["repulsion"]
        assert got["e_iso"] == before["e_iso"] and got["lr_corr"] == before["lr_corr"]
    assert _all(e) == got
    e.close()


@pytest.mark.parametrize("name", vc.EXACT)
def test_exact_structure(name):
    ref = vc.reference(name)
    lam = ref["lam"]
    assert lam.min() >= vc.COND * lam.max()
    s = vc.system(name)
    got = _fresh(s, vc.FLAGS)
    for t in ("e_total", "e_iso"):
        want, tol = float(ref[t]), vc.TOL * float(ref["abs_" + t])
        err = abs(got[t] - want)
        print("%s (matrix %d): %-8s %.10f reference %.10f |diff| / tolerance %.3g" % (name, len(lam), t, got[t], want, err / tol))
        assert err <= tol, (name, t, got[t], want)
    assert got["status"] == 0
    assert got == _fresh(s, vc.FLAGS)


@pytest.mark.parametrize("step", vc.CROSS_STEPS)
def test_zero_crossing(step):
    name = vc.cross_name(step)
    ref = vc.reference(name)
    lam = ref["lam"]
    assert (lam.min() < 0) == (step < 0)
    bound = vc.crossing_bound(lam)
    got = _fresh(vc.system(name), vc.CLIP_FLAGS)
    err = abs(got["e_total"] - float(ref["e_total"]))
    print("%s: r* %+.0e A lambda_min / lambda_max %.3g e_total %.10f reference %.10f |diff| %.3g bound %.3g |diff| / bound %.3g"
          % (name, step, float(lam.min() / lam.max()), got["e_total"], float(ref["e_total"]), err, bound, err / bound))
    assert got["status"] == 0 and np.isfinite(got["e_total"]) and np.isfinite(got["energy"])
    assert err <= bound, (name, got["e_total"], float(ref["e_total"]), err, bound)
    # the other eigenvalue sums of the case are far from zero: e_iso (one-site molecules) keeps the flat tolerance
    assert abs(got["e_iso"] - float(ref["e_iso"])) <= vc.TOL * float(ref["abs_e_iso"])
