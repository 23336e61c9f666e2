"""Test-side reference for the Axilrod-Teller three-body term (axilrod_teller), in plain numpy.

Two implementations of what the reference program sums (every ordered triple of pairwise distinct atoms that are not
all three on one molecule, three independent minimum images, the sum divided by 6):

  literal(system, mk)     the ordered-triple loop in fp64, `pow` calls and operation order as the formula is written,
                          for N <= 24;
  unordered(system, mk)   every unordered triple once; the lattice translation of each pair's minimum image is decided
                          in fp64 exactly as the engine decides it (same products, same order, rint), the values are
                          then formed in longdouble.  Returns the sum, sum |terms| and the smallest non-zero |term|.

A system is the dict of mpmc_amd.synth (pos, alpha, molecule, basis, c9, c6).  Energies in K.
"""
import collections

import numpy as np

ALPHA_AU = 6.7483345             # A^3 -> Bohr^3
C9_NUM, C9_DEN = 0.0032539449, 3.166811429 * 0.000001  # H Bohr^9 -> K A^9


def reciprocal(basis):
    """Inverse of the basis by cofactors over the volume, entry by entry."""
    b = np.asarray(basis, dtype=np.float64)
    vol = b[0][0] * (b[1][1] * b[2][2] - b[1][2] * b[2][1])
    vol += b[0][1] * (b[1][2] * b[2][0] - b[1][0] * b[2][2])
    vol += b[0][2] * (b[1][0] * b[2][1] - b[1][1] * b[2][0])
    iv = 1.0 / vol
    rb = np.empty((3, 3))
    rb[0][0] = iv * (b[1][1] * b[2][2] - b[1][2] * b[2][1])
    rb[0][1] = iv * (b[0][2] * b[2][1] - b[0][1] * b[2][2])
    rb[0][2] = iv * (b[0][1] * b[1][2] - b[0][2] * b[1][1])
    rb[1][0] = iv * (b[1][2] * b[2][0] - b[1][0] * b[2][2])
    rb[1][1] = iv * (b[0][0] * b[2][2] - b[0][2] * b[2][0])
    rb[1][2] = iv * (b[0][2] * b[1][0] - b[0][0] * b[1][2])
    rb[2][0] = iv * (b[1][0] * b[2][1] - b[1][1] * b[2][0])
    rb[2][1] = iv * (b[0][1] * b[2][0] - b[0][0] * b[2][1])
    rb[2][2] = iv * (b[0][0] * b[1][1] - b[0][1] * b[1][0])
    return rb


def image_shift(basis, rb, d):
    """Integer lattice coordinates n (as floats) the minimum image subtracts from displacement(s) d [..., 3], in fp64:
    n_p = rint(sum_q rb[q][p] d_q), the sum taken left to right."""
    d = np.asarray(d, dtype=np.float64)
    n = np.empty_like(d)
    for p in range(3):
        t = rb[0][p] * d[..., 0]
        t = t + rb[1][p] * d[..., 1]
        t = t + rb[2][p] * d[..., 2]
        n[..., p] = np.rint(t)
    return n


def minimum_image(basis, rb, d):
    """fp64 minimum image of one displacement: (dimg, rimg), operation order as written above."""
    b = np.asarray(basis, dtype=np.float64)
    n = image_shift(b, rb, d)
    out = np.empty(3)
    for p in range(3):
        t = b[0][p] * n[0]
        t = t + b[1][p] * n[1]
        t = t + b[2][p] * n[2]
        out[p] = d[p] - t
    r2 = out[0] * out[0]
    r2 = r2 + out[1] * out[1]
    r2 = r2 + out[2] * out[2]
    return out, np.sqrt(r2)


def effective_c9(system, mk):
    """Per-atom c9 (fp64): as read, or the Midzuno-Kihara replacement 3/4 * alpha * 6.7483345 * c6, left to right."""
    alpha = np.asarray(system["alpha"], dtype=np.float64)
    if mk:
        c6 = np.asarray(system["c6"], dtype=np.float64)
        return np.array([3.0 / 4.0 * alpha[i] * ALPHA_AU * c6[i] for i in range(len(alpha))])
    return np.asarray(system["c9"], dtype=np.float64).copy()


def c9_literal(alpha, c, i, j, k):
    """The mixed coefficient of one triple, fp64, as the formula is written (K A^9)."""
    if alpha[i] == 0.0 or alpha[j] == 0.0 or alpha[k] == 0.0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        p = [np.float64(np.power(alpha[t] * ALPHA_AU, 3)) for t in (i, j, k)]
        cc = [np.float64(c[t]) for t in (i, j, k)]
        v = np.power(p[0] * p[1] * p[2], 1.0 / 3.0) * 3.0 / (1.0 / (cc[0] / p[0]) + 1.0 / (cc[1] / p[1]) + 1.0 / (cc[2] / p[2]))
    return float(v * (C9_NUM / C9_DEN))


def one_term(basis, rb, pos, alpha, c, i, j, k):
    """One ORDERED triple in fp64: c9 (1 + cos_part) / (r_ij r_ik r_jk)^3, and its geometry (dij, dik, djk)."""
    dij, rij = minimum_image(basis, rb, pos[i] - pos[j])
    dik, rik = minimum_image(basis, rb, pos[i] - pos[k])
    djk, rjk = minimum_image(basis, rb, pos[j] - pos[k])
    cos_part = 3.0
    cos_part *= np.dot(-dij, -dik) / (np.linalg.norm(dij) * np.linalg.norm(dik))
    cos_part *= np.dot(dij, -djk) / (np.linalg.norm(dij) * np.linalg.norm(djk))
    cos_part *= np.dot(dik, djk) / (np.linalg.norm(dik) * np.linalg.norm(djk))
    return c9_literal(alpha, c, i, j, k) * ((1.0 + cos_part) / np.power(rij * rik * rjk, 3)), (dij, dik, djk)


def literal(system, mk=False):
    """(a): all ordered triples, fp64, divided by 6.  N <= 24."""
    pos = np.asarray(system["pos"], dtype=np.float64)
    n = len(pos)
    assert n <= 24
    mol = np.asarray(system["molecule"])
    alpha = np.asarray(system["alpha"], dtype=np.float64)
    c = effective_c9(system, mk)
    basis = np.asarray(system["basis"], dtype=np.float64)
    rb = reciprocal(basis)
    potential = 0.0
    for i in range(n):
        for j in range(n):
            for k in range(n):
                if i == j or i == k or j == k:
                    continue
                if mol[i] == mol[j] and mol[j] == mol[k]:
                    continue
                potential += one_term(basis, rb, pos, alpha, c, i, j, k)[0]
    return potential / 6


Unordered = collections.namedtuple("Unordered", "total sum_abs min_nonzero n_nonzero")


def unordered(system, mk=False):
    """(b): unordered triples i < j < k; image decisions in fp64, values in longdouble."""
    ld = np.longdouble
    pos64 = np.asarray(system["pos"], dtype=np.float64)
    n = len(pos64)
    mol = np.asarray(system["molecule"])
    alpha = np.asarray(system["alpha"], dtype=np.float64)
    c = effective_c9(system, mk)
    basis = np.asarray(system["basis"], dtype=np.float64)
    rb = reciprocal(basis)
    # pair geometry: d_ab = pos_a - pos_b at its own minimum image (rint is odd: d_ba = -d_ab exactly)
    d64 = pos64[:, None, :] - pos64[None, :, :]
    shift = image_shift(basis, rb, d64).astype(ld)
    d = d64.astype(ld) - shift @ basis.astype(ld)  # (exact difference of the fp64 displacement and the lattice vector)
    r = np.sqrt((d * d).sum(axis=2))
    np.fill_diagonal(r, 1)
    e = d / r[:, :, None]
    t = 1 / (r * r * r)
    a = alpha.astype(ld) * ld(ALPHA_AU)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = a ** 3
        g = 1 / (c.astype(ld) / p)  # inf where c == 0; unused where alpha == 0
    conv = ld(C9_NUM) / ld(C9_DEN)
    active = alpha != 0.0
    total, sum_abs, min_nz, n_nz = ld(0), ld(0), ld(np.inf), 0
    ejk_dot = None
    for i in range(n - 2):
        if not active[i]:
            continue
        js, ks = np.triu_indices(n - i - 1, k=1)
        js, ks = js + i + 1, ks + i + 1
        keep = active[js] & active[ks] & ~((mol[js] == mol[i]) & (mol[ks] == mol[i]))
        js, ks = js[keep], ks[keep]
        if len(js) == 0:
            continue
        c1 = (e[i, js] * e[i, ks]).sum(axis=1)
        c2 = (e[i, js] * e[js, ks]).sum(axis=1)
        c3 = (e[i, ks] * e[js, ks]).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            c9 = np.cbrt(p[i] * p[js] * p[ks]) * 3 / (g[i] + g[js] + g[ks]) * conv
        term = c9 * (1 - 3 * c1 * c2 * c3) * (t[i, js] * t[i, ks] * t[js, ks])
        total += term.sum()
        ab = np.abs(term)
        sum_abs += ab.sum()
        nz = ab[ab != 0]
        if len(nz):
            min_nz = min(min_nz, nz.min())
            n_nz += len(nz)
    return Unordered(float(total), float(sum_abs), float(min_nz), n_nz)


def triclinic(system, shear=(0.18, -0.11, 0.07)):
    """The same atoms (same fractional coordinates) in a sheared cell: rows a, b + s0 a, c + s1 a + s2 b."""
    out = dict(system)
    b0 = np.asarray(system["basis"], dtype=np.float64)
    b1 = b0.copy()
    b1[1] = b0[1] + shear[0] * b0[0]
    b1[2] = b0[2] + shear[1] * b0[0] + shear[2] * b0[1]
    frac = np.asarray(system["pos"], dtype=np.float64) @ np.linalg.inv(b0)
    out["basis"] = b1
    out["pos"] = np.ascontiguousarray(frac @ b1)
    return out
