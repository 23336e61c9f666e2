"""CPU tests of tests/vdw_model.py, the fp64 numpy restatement of the eigenvalue solver of mpmc_amd/csrc/kernels_vdw.h, and
through it of the spectrum-edge cases of tests/vdw_cases.py: that the exact-structure cases take the branches they are meant
to take, that the zero crossing changes sign where the GPU test says it does, and that the solver's algorithm in honest fp64
stays inside the derived error bound which tests/test_gpu_vdw_large.py applies to the device."""
from itertools import combinations

import numpy as np
import pytest

import vdw_cases as vc
import vdw_model as vm
import vdw_reference as vr

U = 2.0 ** -53


def _model(name):
    Cm, _ = vr.c_matrix(vc.system(name), vc.flags_of(name))
    return vm.energy(Cm.astype(np.float64))


@pytest.mark.parametrize("name", ["box1", "box2", "box22", "box43", "clip"])
def test_model_against_the_reference(name):
    ref = vc.reference(name)
    lam = ref["lam"]
    en, got, _, _, _ = _model(name)
    assert abs(en - float(ref["e_total"])) <= vc.TOL * float(ref["abs_e_total"])
    # every eigenvalue inside the solver's part of the bound (the model starts from the reference's matrix rounded to fp64:
    # one rounding per element, inside BUILD_ULPS)
    delta = vc.delta_factor(len(lam)) * U * float(np.abs(lam).max())
    assert np.abs(got - lam.astype(np.float64)).max() <= delta


def test_model_one_site_matrix_takes_the_zero_branch():
    """a diagonal 3 x 3 (every one-site molecule's e_iso): column 0 has an exactly zero tail and a trailing block"""
    _, lam, tau, xn2, e = _model("box1")
    assert xn2[0] == 0.0 and tau[0] == 0.0 and e[0] == 0.0 and lam[0] == lam[1] == lam[2]


def test_axis2_splits_exactly():
    """x, y and z decouple with exact zeros.  Column 0 (site 0's x row) has ONE non-zero entry below x_0 = 0, so its
    reflector is an exact signed permutation (v = (1, 0, +-1, 0, 0), tau = 1), the zeros stay exact, and the reduction
    reaches a column with an exactly zero tail in front of a non-empty trailing block."""
    name = "axis2"
    Cm, _ = vr.c_matrix(vc.system(name), vc.FLAGS)
    C = Cm.astype(np.float64)
    n = C.shape[0]
    assert n == 6 and (C[1::3, 1::3] == C[2::3, 2::3]).all()          # the y and the z block: the same bits
    assert not C[0::3, 1::3].any() and not C[0::3, 2::3].any() and not C[1::3, 2::3].any()
    _, lam, tau, xn2, e = _model(name)
    split = [j for j in range(n - 2) if xn2[j] == 0.0]
    assert split and all(tau[j] == 0.0 for j in split), xn2
    assert any(e[j] == 0.0 for j in split), e                          # an exact e_j = 0 inside the bisection
    ref = vc.reference(name)["lam"]
    tiny = 1e-18 * ref.max()                                           # doubly degenerate to the longdouble rounding
    assert ref[2] - ref[1] <= tiny and ref[4] - ref[3] <= tiny and ref[0] < ref[1] < ref[3] < ref[5]
    assert np.abs(lam - ref.astype(np.float64)).max() <= vc.delta_factor(n) * U * float(ref.max())


def test_axis3_splits_to_rounding():
    """Three collinear sites cannot take the exact branch, whatever the spacing: site 0's x row has TWO non-zero entries
    a, b below x_0 = 0 (the xx couplings to both other sites; no cutoff), so the first reflector holds a / sqrt(a^2 + b^2),
    which rounds, and it mixes site 0's y slot (the position of x_0) into the x subspace.  What the case does give, and
    what is asserted: an input whose y and z blocks are the same bits (exactly doubly degenerate eigenvalues), and a
    tridiagonal matrix that splits to rounding -- off-diagonals of 1e-14 of the largest, not 0 -- which the Sturm recurrence
    has to take in its stride.  The exact split is axis2's and the one-site matrix's."""
    name = "axis3"
    Cm, _ = vr.c_matrix(vc.system(name), vc.FLAGS)
    C = Cm.astype(np.float64)
    assert C.shape[0] == 9 and (C[1::3, 1::3] == C[2::3, 2::3]).all()
    assert not C[0::3, 1::3].any() and not C[0::3, 2::3].any() and not C[1::3, 2::3].any()
    assert np.count_nonzero(C[0, 1:]) == 2
    _, lam, tau, xn2, e = _model(name)
    assert (xn2[:-1] != 0.0).all()
    small = np.sort(np.abs(e))[:2]
    assert (small > 0).all() and (small <= 1e-12 * np.abs(e).max()).all(), e
    ref = vc.reference(name)["lam"]
    pairs = np.flatnonzero(np.diff(ref) <= 1e-18 * ref.max())
    assert len(pairs) == 3                                             # the three y = z pairs
    assert np.abs(lam - ref.astype(np.float64)).max() <= vc.delta_factor(9) * U * float(ref.max())


def test_lattice27_is_highly_degenerate():
    ref = vc.reference("lattice27")["lam"]
    assert len(ref) == 81
    groups = np.split(ref, np.flatnonzero(np.diff(ref) > 1e-15 * ref.max()) + 1)
    sizes = sorted(len(g) for g in groups)
    assert len(groups) <= 9 and sizes[-1] >= 12, sizes
    en, lam, _, _, _ = _model("lattice27")
    assert abs(en - float(vc.reference("lattice27")["e_total"])) <= vc.TOL * float(vc.reference("lattice27")["abs_e_total"])


def test_delta_factor_is_the_counted_bound():
    # n = 18: 16 columns with trailing blocks of 17 .. 2 rows, every depth at its smallest: 9 * 23 + 8 * 7 + 4 * 11 + 130
    assert vc.delta_factor(18) == np.sqrt(18.0) * (vc.BUILD_ULPS + 16 * 437) + vc.BISECT_ULPS
    assert vc.delta_factor(18) < 100 * 18 ** 2  # a bound in n^2 with a modest constant


def test_crossing_is_where_the_sign_changes():
    r = vc.crossing()
    assert 1.2 < r < 2.0
    assert vc._lambda_min(np.nextafter(r, 0.0)) < 0 <= vc._lambda_min(r)


@pytest.mark.parametrize("step", vc.CROSS_STEPS)
def test_crossing_sign_pattern_and_model_inside_the_bound(step):
    name = vc.cross_name(step)
    s, ref = vc.system(name), vc.reference(name)
    lam = ref["lam"]
    assert len(lam) == 18
    assert (lam.min() < 0) == (step < 0) and (lam[1:] > vc.COND * lam.max()).all()  # ONE eigenvalue near zero
    assert 0.5 * abs(step) <= abs(float(lam.min())) <= abs(step)  # as near zero as the step is (d lambda / dr = 0.8 / A)
    # the build's part of the bound holds where polar_damp * r >= 10 for every pair
    pos = np.asarray(s["pos"])
    assert min(np.linalg.norm(pos[i] - pos[j]) for i, j in combinations(range(len(pos)), 2)) * vc.CLIP_FLAGS["polar_damp"] >= 10
    en, got, _, _, _ = _model(name)
    bound = vc.crossing_bound(lam)
    err = abs(en - float(ref["e_total"]))
    print("%s: lambda_min %.3g model |diff| %.3g bound %.3g |diff| / bound %.3g" % (name, float(lam.min()), err, bound,
                                                                                     err / bound))
    assert np.isfinite(en) and err <= bound
    assert np.abs(got - lam.astype(np.float64)).max() <= vc.delta_factor(18) * U * float(np.abs(lam).max())
