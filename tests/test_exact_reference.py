"""The longdouble Cholesky reference of the exact-dipole tests (tests/exact_reference.py) checked on the CPU: against
numpy.linalg.solve, against the residual it leaves in its own arithmetic, and on the closed form of the two-site tensor."""
import numpy as np
import pytest

import exact_reference as xr

LD = xr.LD


def _spd(n, seed, cond=1.0e3):
    """a random symmetric positive definite matrix with eigenvalues between 1 and cond, rounded to fp64"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    lam = np.exp(rng.uniform(0.0, np.log(cond), n))
    A = (q * lam) @ q.T
    return 0.5 * (A + A.T)


@pytest.mark.parametrize("n", [1, 3, 18, 63, 192])
def test_solve_against_lapack_and_its_own_residual(n):
    A = _spd(n, 100 + n)
    b = np.random.default_rng(n).normal(size=n)
    x = xr.solve(A, b)
    assert x.dtype == LD
    w = np.linalg.solve(A, b)
    # LAPACK in fp64 is within cond * n * 2^-53 of the solution; the longdouble solve is the more accurate of the two
    assert np.abs(x.astype(np.float64) - w).max() <= 1.0e3 * n * 2.0 ** -53 * np.abs(w).max()
    res = np.abs(A.astype(LD) @ x - b.astype(LD))
    eps = float(np.finfo(LD).eps)
    assert np.all(res <= n * eps * (np.abs(A).astype(LD) @ np.abs(x) + np.abs(b)))
    if eps < 2.0 ** -60:  # an extended longdouble: the residual sits far below the fp64 bound the device is held to
        assert np.all(res <= 1e-3 * xr.backward_bound(A, x, b))


def test_factor_and_several_right_hand_sides():
    A = _spd(40, 7)
    L = xr.cholesky(A)
    assert np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) > 0)
    assert np.abs(L @ L.T - A).max() <= 40 * float(np.finfo(LD).eps) * np.abs(A).max()
    B = np.random.default_rng(3).normal(size=(40, 4))
    X = xr.solve(A, B)
    for k in range(4):
        assert np.array_equal(X[:, k], xr.solve(A, B[:, k]))


def test_a_matrix_that_is_not_positive_definite_is_refused():
    A = _spd(12, 5)
    A[3, 3] = -A[3, 3]
    assert np.linalg.eigvalsh(A).min() < 0
    with pytest.raises(ValueError):
        xr.cholesky(A)


def _thole_pair(alpha, r, damp):
    """the 6 x 6 matrix of two sites on the z axis, written out independently of two_site_tensor (thole_matrix.c:72-137)"""
    lr = damp * r
    e = np.exp(-lr)
    d1 = 1.0 - e * (0.5 * lr * lr + lr + 1.0)
    d2 = d1 - e * lr ** 3 / 6.0
    d = np.array([0.0, 0.0, r])
    T = d1 / r ** 3 * np.eye(3) - 3.0 * d2 / r ** 5 * np.outer(d, d)
    A = np.zeros((6, 6))
    A[:3, :3] = A[3:, 3:] = np.eye(3) / alpha
    A[:3, 3:] = A[3:, :3] = T
    return A


def test_two_site_tensor_closed_form():
    alpha, r, damp = 1.1, 2.3, 2.1304
    cxx, czz = xr.two_site_tensor(alpha, r, damp)
    assert abs(float(cxx) - 2.040147173883) < 1e-11 and abs(float(czz) - 2.491797607119) < 1e-11
    C, scale = xr.tensor(_thole_pair(alpha, r, damp))
    want = np.diag([float(cxx), float(cxx), float(czz)])
    assert np.abs(C.astype(np.float64) - want).max() <= 1e-14 * float(scale)
    # one site: C = alpha I
    C1, _ = xr.tensor(np.eye(3) / alpha)
    assert np.abs(C1.astype(np.float64) - alpha * np.eye(3)).max() <= 2 * np.spacing(alpha)


def test_tensor_is_the_sum_of_unit_field_dipoles():
    """C[:, q] = sum_i mu_i^(q), mu^(q) the solution for a unit field along q at every site: what the device computes"""
    A = _spd(30, 11)
    C, _ = xr.tensor(A)
    for q in range(3):
        b = np.zeros(30)
        b[q::3] = 1.0
        mu = xr.solve(A, b)
        for p in range(3):
            assert abs(mu[p::3].sum() - C[p, q]) <= 1e-15 * float(np.abs(C).max()) * 30
