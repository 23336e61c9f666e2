"""An independent model of `quantum_rotation` (mpmc_amd/host/qrot.c; reference src/quantum_rotation/).  Helper module for
the tests (a plain import, not a conftest).

Independent means: the Gauss-Legendre grid comes from numpy (leggauss(16)), Y_lm from the fully normalised recurrence in
longdouble (not from a table, and not the un-normalised recurrence qrot.c runs), the quadrature is summed in longdouble,
and the eigen-solve is numpy.linalg.eigh.  What is DEFINED by the reference is restated as it defines it: the placements
in fp64 in the operation order of align_molecule() then rotate_spherical(), the 0.5 pi^2 factor, B l (l + 1), the symmetry
test on the real parts at 64 random points with its (theta + pi, phi + pi) "inversion", the factor 3 and the para / ortho
choice, the move-type draws and the spin-flip acceptance."""
import math

import numpy as np

from reference_chain_replay import MT19937

LD = np.longdouble
GRID = 16
SYMMETRY_POINTS = 64
PARA, ORTHO = 0, 1
_X, _W = np.polynomial.legendre.leggauss(GRID)
THETA = 0.5 * math.pi * _X + 0.5 * math.pi
PHI = math.pi * _X + math.pi
WEIGHTS = _W


def ylm(l, m, theta, phi):
    """Y_lm (complex longdouble pair re, im) at arrays theta, phi: the fully normalised recurrence
    Pbar_m^m = -sqrt((2m + 1) / 2m) s Pbar_{m-1}^{m-1}, Pbar_{m+1}^m = sqrt(2m + 3) x Pbar_m^m,
    Pbar_l^m = a_lm (x Pbar_{l-1}^m - b_lm Pbar_{l-2}^m), with s = sin(theta) signed; Y_l(-m) = (-1)^m conj(Y_lm)."""
    theta = np.asarray(theta, dtype=LD)
    phi = np.asarray(phi, dtype=LD)
    ma = abs(m)
    x, s = np.cos(theta), np.sin(theta)
    pmm = np.full(theta.shape, np.sqrt(LD(1) / (4 * LD(math.pi))), dtype=LD)
    for k in range(1, ma + 1):
        pmm = -np.sqrt(LD(2 * k + 1) / LD(2 * k)) * s * pmm
    p = pmm
    if l > ma:
        pm1, pl = pmm, np.sqrt(LD(2 * ma + 3)) * x * pmm
        for ll in range(ma + 2, l + 1):
            a = np.sqrt(LD(4 * ll * ll - 1) / LD(ll * ll - ma * ma))
            b = np.sqrt(LD((ll - 1) ** 2 - ma * ma) / LD(4 * (ll - 1) ** 2 - 1))
            pm1, pl = pl, a * (x * pl - b * pm1)
        p = pl
    re, im = p * np.cos(ma * phi), p * np.sin(ma * phi)
    if m < 0:
        sign = -1 if ma % 2 else 1
        return sign * re, -sign * im
    return re, im


def closed_form(l, m, theta, phi):
    """Y_lm for l <= 2 from the textbook closed forms (complex128)."""
    c, s = np.cos(theta), np.sin(theta)
    pi = math.pi
    t = {(0, 0): 0.5 * math.sqrt(1 / pi) + 0 * c,
         (1, 0): 0.5 * math.sqrt(3 / pi) * c,
         (1, 1): -0.5 * math.sqrt(3 / (2 * pi)) * s,
         (2, 0): 0.25 * math.sqrt(5 / pi) * (3 * c * c - 1),
         (2, 1): -0.5 * math.sqrt(15 / (2 * pi)) * s * c,
         (2, 2): 0.25 * math.sqrt(15 / (2 * pi)) * s * s}[(l, abs(m))]
    y = t * np.exp(1j * abs(m) * phi)
    return y if m >= 0 else (-1) ** abs(m) * np.conj(y)


def index_lm(l_max):
    return [(l, m) for l in range(l_max + 1) for m in range(-l, l + 1)]


def basis_on_grid(l_max):
    """[dim][p][t] complex (longdouble parts)"""
    T, P = np.meshgrid(THETA, PHI)  # [p][t]
    re, im = zip(*[ylm(l, m, T, P) for l, m in index_lm(l_max)])
    return np.array(re, dtype=LD), np.array(im, dtype=LD)


def overlap(l_max):
    """<l m | l' m'> under the 16 x 16 quadrature with the sin(theta) of the grid potential: the identity up to the
    quadrature's own error, which this returns the largest element of."""
    re, im = basis_on_grid(l_max)
    w = (WEIGHTS[:, None] * WEIGHTS[None, :] * np.sin(THETA)[None, :]).astype(LD) * LD(0.5 * math.pi ** 2)
    sre = np.einsum("ipt,jpt,pt->ij", re, re, w) + np.einsum("ipt,jpt,pt->ij", im, im, w)
    sim = np.einsum("ipt,jpt,pt->ij", re, im, w) - np.einsum("ipt,jpt,pt->ij", im, re, w)
    S = sre.astype(np.float64) + 1j * sim.astype(np.float64)
    return S, float(np.abs(S - np.eye(len(S))).max())


def hindered_grid(B, barrier):
    """V[t][p] = sin(theta) * B * barrier * sin(theta)^2"""
    s = np.sin(THETA)
    return np.repeat((s * (B * barrier * (s * s)))[:, None], GRID, axis=1)


def hamiltonian(V, l_max, B):
    """H_ij = 0.5 pi^2 sum_p sum_t w_p w_t conj(Y_i) Y_j V[t][p] + B l (l + 1) delta_ij, complex128 from longdouble sums."""
    re, im = basis_on_grid(l_max)
    w = (WEIGHTS[:, None] * WEIGHTS[None, :]).astype(LD) * np.asarray(V, dtype=LD).T * LD(0.5 * math.pi ** 2)  # [p][t]
    hre = np.einsum("ipt,jpt,pt->ij", re, re, w) + np.einsum("ipt,jpt,pt->ij", im, im, w)
    him = np.einsum("ipt,jpt,pt->ij", re, im, w) - np.einsum("ipt,jpt,pt->ij", im, re, w)
    H = hre.astype(np.float64) + 1j * him.astype(np.float64)
    H = 0.5 * (H + H.conj().T)
    for k, (l, _) in enumerate(index_lm(l_max)):
        H[k, k] += B * l * (l + 1)
    return H


def quadrature_weight_norm(l_max):
    """sum_pt 0.5 pi^2 w_p w_t sin(theta_t) max_ij |Y_i Y_j|: how an error of the grid ENERGIES bounds one of a matrix
    element (and, times dim, of the Frobenius norm and so of every eigenvalue, by Weyl)."""
    re, im = basis_on_grid(l_max)
    amp = np.sqrt((re * re + im * im).astype(np.float64)).max(axis=0)  # [p][t]: max_i |Y_i|
    w = WEIGHTS[:, None] * WEIGHTS[None, :] * np.sin(THETA)[None, :] * 0.5 * math.pi ** 2
    return float((w * amp * amp).sum())


def basis_real(l, m, theta, phi):
    return float(ylm(l, m, np.array(theta), np.array(phi))[0])


def symmetry(evec, l_max, rng):
    """determine_rotational_eigensymmetry() of one eigenvector (complex [dim]): 0 symmetric, 1 antisymmetric.  The 64
    points are drawn first, theta then phi per point as the reference draws them; the first largest square wins."""
    lm = index_lm(l_max)
    pts = [(rng.rand() * math.pi, rng.rand() * 2.0 * math.pi) for _ in range(SYMMETRY_POINTS)]
    theta, phi = np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
    wf = sum(evec[k].real * ylm(l, m, theta, phi)[0].astype(np.float64) for k, (l, m) in enumerate(lm))
    sq = wf * wf
    best = int(np.argmax(sq)) if sq.max() > 0.0 else None
    bt, bp = (theta[best], phi[best]) if best is not None else (0.0, 0.0)
    mx = sum(evec[k].real * basis_real(l, m, bt, bp) for k, (l, m) in enumerate(lm))
    inv = sum(evec[k].real * basis_real(l, m, bt + math.pi, bp + math.pi) for k, (l, m) in enumerate(lm))
    return 1 if mx * inv < 0.0 else 0


def partition_functions(levels, symmetries, nsum, temperature, spin):
    g = sum(math.exp(-levels[i] / temperature) for i in range(nsum) if symmetries[i] == 0)
    u = sum(3.0 * math.exp(-levels[i] / temperature) for i in range(nsum) if symmetries[i] == 1)
    return g, u, (g if spin == PARA else u) / (g + u)


def placements(pos, com):
    """[p * 16 + t][n][3]: align_molecule() then rotate_spherical() in fp64, every placement from the unmodified
    coordinates, about the given centre of mass."""
    pos = np.asarray(pos, dtype=np.float64)
    com = np.asarray(com, dtype=np.float64)
    al = pos - com
    axis = next(k for k in range(1, len(al)) if not (al[k] == 0.0).all())
    v = al[axis]
    theta = math.pi / 2.0 if v[2] == 0.0 else math.acos(v[2] / math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]))
    if v[0] == 0:
        phi = math.pi / 2.0 if v[1] > 1e-12 else (3.0 / 2.0 * math.pi if v[1] < -1e-12 else 0.0)
    elif v[1] == 0:
        phi = math.pi
    else:
        phi = math.atan(abs(v[1] / v[0]))
        if v[1] / v[0] < 0.0:
            phi *= -1.0
    ct, st, cp, sp = math.cos(theta), math.sin(theta), math.cos(phi), math.sin(phi)
    R = [[ct * cp, ct * sp, -st], [-sp, cp, 0.0], [st * cp, st * sp, ct]]

    def apply(R, a):
        return np.array([[(R[k][0] * x[0] + R[k][1] * x[1]) + R[k][2] * x[2] for k in range(3)] for x in a])

    aligned = apply(R, al) + com
    out = np.empty((GRID * GRID, len(pos), 3))
    for p in range(GRID):
        for t in range(GRID):
            ct, st, cp, sp = math.cos(THETA_C[t]), math.sin(THETA_C[t]), math.cos(PHI_C[p]), math.sin(PHI_C[p])
            R = [[cp * ct, -sp, cp * (-st)], [sp * ct, cp, sp * (-st)], [st, 0.0, ct]]
            out[p * GRID + t] = apply(R, aligned - com) + com
    return out


# the grid angles as the SOURCE has them (decimal roots, M_PI * root + M_PI): the placements are defined by these
_ROOTS = [-0.989400934991649932596, -0.944575023073232576078, -0.865631202387831743880, -0.755404408355003033895,
          -0.617876244402643748447, -0.458016777657227386342, -0.281603550779258913230, -0.095012509837637440185]
_ROOTS = np.array(_ROOTS + [-r for r in reversed(_ROOTS)])
THETA_C = 0.5 * math.pi * _ROOTS + 0.5 * math.pi
PHI_C = math.pi * _ROOTS + math.pi


def evaluate(V, l_max, B, level_max, nsum, temperature, spin, rng):
    """One molecule's evaluation from its grid potential: (levels, symmetries, (g, u, own), eigenvectors)."""
    H = hamiltonian(V, l_max, B)
    ev, vec = np.linalg.eigh(H)
    levels = ev[:level_max]
    sym = [symmetry(vec[:, i], l_max, rng) for i in range(level_max)]
    return levels, sym, partition_functions(levels, sym, nsum, temperature, spin), vec


def movetype_draw(rng, ensemble, spinflip_probability, insert_probability=0.0):
    """checkpoint()'s move-type draws under quantum_rotation (checkpoint.c:46-81), then the molecule's draw (returned)."""
    kind = "displace"
    if ensemble == "uvt":
        if rng.rand() < insert_probability:
            kind = "insert" if rng.rand() < 0.5 else "remove"
        elif rng.rand() < spinflip_probability:
            kind = "spinflip"
    elif rng.rand() < spinflip_probability:
        kind = "spinflip"
    return kind, rng.rand()


def new_rng(seed):
    return MT19937(seed)
