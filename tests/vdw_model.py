"""The eigenvalue solver of mpmc_amd/csrc/kernels_vdw.h restated in plain fp64 numpy (a helper module of the tests, no
GPU): the recurrences as the kernels write them, not their summation order.

  tridiagonalise(C)   vdw_reflect_kernel (the dlarfg form: xn2 over the column below its first entry, beta =
                      -copysign(sqrt(alpha^2 + xn2), alpha), tau = (beta - alpha) / beta, v = x / (alpha - beta), v_0 = 1;
                      tau = 0 and e_j = x_0 when xn2 == 0), vdw_symv_kernel (p = tau C22 v), vdw_rank2_kernel
                      (K = (tau / 2) p.v, w = p - K v, C22 -= (v_r w_c + w_r v_c), no contraction), column by column;
                      the last column (j = n - 2) only forms its reflector and writes d[n - 1].
  bisect(d, e)        vdw_bisect_kernel: the Gershgorin interval widened as dstebz widens it, kVdwBisectSteps halvings of
                      the Sturm count with the pivmin guard.
  eigen_sum(lam)      vdw_sum_kernel: (sum sqrt(lambda < 0 ? 0 : lambda) * au2invsec) * halfHBAR.

What the tests use it for: that a case really takes the branch it is meant to take (the device cannot be asked), and that
the algorithm in honest fp64 stays inside the error bound the GPU test applies.
"""
import math

import numpy as np

BISECT_STEPS = 64                   # kVdwBisectSteps
SAFE_MIN = 2.2250738585072014e-308  # kVdwSafeMin
AU2INVSEC = 4.13412763705e16
HALF_HBAR = 3.81911146e-12


def tridiagonalise(C):
    """(d, e, tau, xn2) of the symmetric matrix C (n >= 2): tau[j], xn2[j] for the columns j = 0 .. n - 2"""
    A = np.array(C, dtype=np.float64)
    n = A.shape[0]
    d, e = np.zeros(n), np.zeros(n - 1)
    taus, xn2s = np.zeros(n - 1), np.zeros(n - 1)
    for j in range(n - 1):
        x = A[j, j + 1:].copy()  # column j below the diagonal, read as row j
        xn2 = float(np.sum(x[1:] * x[1:]))
        alpha = float(x[0])
        beta, tau, inv = alpha, 0.0, 0.0
        if xn2 != 0.0:
            beta = -math.copysign(math.sqrt(alpha * alpha + xn2), alpha)
            tau = (beta - alpha) / beta
            inv = 1.0 / (alpha - beta)
        v = x * inv
        v[0] = 1.0
        d[j], e[j], taus[j], xn2s[j] = A[j, j], beta, tau, xn2
        if j == n - 2:
            d[n - 1] = A[n - 1, n - 1]
            break
        A22 = A[j + 1:, j + 1:]
        p = tau * (A22 * v[None, :]).sum(axis=1)
        K = 0.5 * tau * float(np.sum(p * v))
        w = p - K * v
        A22 -= np.outer(v, w) + np.outer(w, v)  # (r, c) and (c, r) add the same two products
    return d, e, taus, xn2s


def bisect(d, e):
    """the eigenvalues (ascending) of the symmetric tridiagonal (d, e)"""
    d, e = np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64)
    n = len(d)
    gl = gu = d[0]
    emax2 = eprev = 0.0
    for i in range(n):
        en = abs(e[i]) if i < n - 1 else 0.0
        gl, gu = min(gl, d[i] - eprev - en), max(gu, d[i] + eprev + en)
        emax2 = max(emax2, en * en)
        eprev = en
    pivmin = SAFE_MIN * max(emax2, 1.0)
    bnorm = max(abs(gl), abs(gu))
    widen = 2.1 * bnorm * 2.0 ** -53 * n + 2.1 * pivmin
    lo, hi = np.full(n, gl - widen), np.full(n, gu + widen)
    k = np.arange(n)

    def guard(q, cnt):
        hit = q <= pivmin
        return np.where(hit, np.minimum(q, -pivmin), q), cnt + hit

    with np.errstate(divide="ignore", invalid="ignore"):
        for _ in range(BISECT_STEPS):
            x = 0.5 * (lo + hi)
            q, cnt = guard(d[0] - x, np.zeros(n, dtype=np.int64))
            for i in range(1, n):
                q, cnt = guard(d[i] - (e[i - 1] * e[i - 1]) / q - x, cnt)
            above = cnt > k
            hi, lo = np.where(above, x, hi), np.where(above, lo, x)
    return 0.5 * (lo + hi)


def eigen_sum(lam):
    s = float(np.sqrt(np.where(lam < 0.0, 0.0, lam)).sum())
    return (s * AU2INVSEC) * HALF_HBAR


def energy(C):
    """the solver end to end: (energy, eigenvalues, tau, xn2, e)"""
    C = np.asarray(C, dtype=np.float64)
    if C.shape[0] == 1:
        lam = C[0].copy()
        return eigen_sum(lam), lam, np.zeros(0), np.zeros(0), np.zeros(0)
    d, e, tau, xn2 = tridiagonalise(C)
    lam = bisect(d, e)
    return eigen_sum(lam), lam, tau, xn2, e
