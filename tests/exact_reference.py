"""Reference for the exact Thole dipoles (a plain helper module): a longdouble Cholesky factorization and solve in numpy,
what the device solver of mpmc_amd/csrc/kernels_exact.h is held against, and the closed forms of the two-site tensor.

  cholesky(A)            lower factor of a symmetric positive definite matrix, longdouble; ValueError on a pivot <= 0
  solve(A, B)            A^-1 B through that factor (B a vector or a matrix of right-hand sides), longdouble
  tensor(A)              C[p][q] = sum_ij (A^-1)[3i+p][3j+q] (thole_polarizability.c:27-37), longdouble, with sum |B_ij|
  backward_bound(A,x,b)  n 2^-53 (|A||x| + |b|) componentwise: the textbook bound for Cholesky + two substitutions
  two_site_tensor(...)   C_xx = C_yy and C_zz of two equal sites on the z axis with the exponential Thole damping
"""
import numpy as np

LD = np.longdouble


def cholesky(A):
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            raise ValueError("pivot %d is not positive: %r" % (j, d))
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def _forward(L, B):
    Y = np.array(B, dtype=LD)
    for i in range(L.shape[0]):
        Y[i] = (Y[i] - L[i, :i] @ Y[:i]) / L[i, i]
    return Y


def _backward(L, Y):
    X = np.array(Y, dtype=LD)
    n = L.shape[0]
    for i in range(n - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def solve(A, B):
    L = cholesky(A)
    return _backward(L, _forward(L, B))


def tensor(A):
    """(C, sum_ij |B_ij|) with B = A^-1 in longdouble: the reference's block sums"""
    n = np.asarray(A).shape[0]
    B = solve(A, np.eye(n, dtype=LD))
    C = np.zeros((3, 3), dtype=LD)
    for p in range(3):
        for q in range(3):
            C[p, q] = B[p::3, q::3].sum()
    return C, np.abs(B).sum()


def backward_bound(A, x, b):
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    return LD(n) * LD(2.0) ** -53 * (np.abs(A) @ np.abs(np.array(x, dtype=LD)) + np.abs(np.array(b, dtype=LD)))


def two_site_tensor(alpha, r, damp):
    """two sites of polarizability alpha a distance r apart along z: T_xx = T_yy = d1 / r^3, T_zz = (d1 - 3 d2) / r^3"""
    lr = LD(damp) * LD(r)
    e = np.exp(-lr)
    d1 = 1 - e * (lr * lr / 2 + lr + 1)
    d2 = d1 - e * lr ** 3 / 6
    r3 = LD(r) ** 3
    cxx = 2 / (1 / LD(alpha) + d1 / r3)
    czz = 2 / (1 / LD(alpha) + (d1 - 3 * d2) / r3)
    return cxx, czz
