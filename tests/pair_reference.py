"""Brute-force per-pair reference of what the LJ / real-space electrostatics kernel (pair_rd_es_body) and the
static-field kernel (static_field_body) sum.  Helper module for the tests (a plain import, not a conftest), written
from the reference's formulas and independent of oracle/.

Two kinds of arithmetic, on purpose:

* DECISIONS -- the lattice image (rint() of the fractional displacement, energy/pairs.c:230-290, same operation
  order, no contraction: numpy evaluates one rounded operation per ufunc call), the exclusions (pairs.c:55-81) and
  the three cutoff comparisons (`rimg - 1e-12 < rc`, lj.c:189 and thole_field.c:50,96; `rimg < rc`,
  coulombic.c:291; `!(rimg > rc)`, coulombic.c:167 and polar_ewald.c:52) -- are made in fp64 exactly as the
  reference makes them, because they define the answer.
* VALUES are evaluated from the fp64 rimg / dimg in numpy.longdouble (64-bit mantissa on x86) and accumulated in
  longdouble, so the rounding of this module stays below the engine's.  numpy has no longdouble erfc / erf: those two
  are taken per pair from math.erfc / math.erf (fp64, < 1 ulp) and widened; exp is numpy's longdouble exp.

pair_table() returns one row per pair that contributes to some channel (or sits within `keep` of the cutoff), so a
failing test can name the pair that is missing instead of reporting a sum.
"""
import math

import numpy as np

LD = np.longdouble
SMALL_dR = 1.0e-12  # include/defines.h:28
HBAR2, HBAR4 = LD("1.11211999e-68"), LD("1.23681087e-136")  # include/defines.h:7-61
KB, KB2 = LD("1.3806503e-23"), LD("1.90619525e-46")
M2A2, M2A4 = LD("1.0e20"), LD("1.0e40")
AMU2KG = LD("1.66053873e-27")
ONE_OVER_SQRT_PI = LD("0.56418958354")  # polarization/thole_field.c:10 (the reference's truncated constant)
PI = LD(math.pi)  # the reference's M_PI is the fp64 constant

_erfc = np.vectorize(math.erfc, otypes=[np.float64])
_erf = np.vectorize(math.erf, otypes=[np.float64])


def erfc_ld(x):
    x = np.asarray(x, dtype=np.float64)
    return _erfc(x).astype(LD) if x.size else np.zeros(x.shape, LD)


def erf_ld(x):
    x = np.asarray(x, dtype=np.float64)
    return _erf(x).astype(LD) if x.size else np.zeros(x.shape, LD)


def pbc(basis, cutoff_in=0.0):
    """energy/pbc.c:13-83 in plain fp64 scalars: volume, inverse basis (rows as the reference stores them), cutoff =
    half the shortest lattice vector over coefficients -5..5 unless given."""
    b = [[float(basis[p][q]) for q in range(3)] for p in range(3)]
    vol = b[0][0] * (b[1][1] * b[2][2] - b[1][2] * b[2][1])
    vol += b[0][1] * (b[1][2] * b[2][0] - b[1][0] * b[2][2])
    vol += b[0][2] * (b[1][0] * b[2][1] - b[1][1] * b[2][0])
    if cutoff_in == 0.0:
        short = 1.0e40
        rng = range(-5, 6)
        for i in rng:
            for j in rng:
                for k in rng:
                    if i == 0 and j == 0 and k == 0:
                        continue
                    v = [i * b[0][q] + j * b[1][q] + k * b[2][q] for q in range(3)]
                    mag = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
                    short = min(short, mag)
        cutoff = 0.5 * short
    else:
        cutoff = float(cutoff_in)
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
    return vol, rb, cutoff


def minimum_image(basis, rb, d):
    """energy/pairs.c:230-290 on displacements d[...,3] (fp64, one rounding per operation, the reference's order).
    Returns (image[...,3] as the rint() values, r, rimg, dimg[...,3])."""
    b = np.asarray(basis, dtype=np.float64)
    d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
    img = []
    for p in range(3):
        f = rb[0][p] * d0
        f = f + rb[1][p] * d1
        f = f + rb[2][p] * d2
        img.append(np.rint(f))
    di = []
    for p in range(3):
        t = b[0][p] * img[0]
        t = t + b[1][p] * img[1]
        t = t + b[2][p] * img[2]
        di.append(d[..., p] - t)
    r2 = d0 * d0
    r2 = r2 + d1 * d1
    r2 = r2 + d2 * d2
    ri2 = di[0] * di[0]
    ri2 = ri2 + di[1] * di[1]
    ri2 = ri2 + di[2] * di[2]
    r, rimg = np.sqrt(r2), np.sqrt(ri2)
    dimg = np.stack(di, axis=-1)
    nan = np.isnan(rimg)  # pairs.c:279
    rimg = np.where(nan, r, rimg)
    dimg = np.where(nan[..., None], d, dimg)
    return np.stack(img, axis=-1), r, rimg, dimg


def _molecule_index(molecule):
    """molecules are contiguous runs of equal id (io/read_pqr.c:278-287)"""
    m = np.asarray(molecule)
    return np.concatenate([[0], np.cumsum(m[1:] != m[:-1])]).astype(np.int64)


def field_mode(params):
    """thole_field(), thole_field.c:14-36"""
    if not params.get("polarization") or params.get("rd_only"):
        return None
    if params.get("polar_ewald"):
        return "ewald"
    if params.get("polar_wolf"):
        return "wolf"
    return "bare"


def pair_table(system, params, keep=0.02):
    """One row per pair i < j (atom order) that contributes to a channel, is a same-molecule pair with charges, or has
    rimg <= rc + keep.  Columns (dict of arrays): i, j, image (n,3 int), r, rimg, dimg, rd, es, es_intra (longdouble;
    es_real of the engine is sum(es) - sum(es_intra)), field_i, field_j (n,3 longdouble: what the pair adds to
    ef_static of i and of j), in_rd / in_es / in_field (bool: the pair passed that channel's cutoff comparison and
    exclusions).  Also "rc", "ewald_alpha", "polar_alpha", "volume"."""
    pos = np.ascontiguousarray(system["pos"], dtype=np.float64)
    n = pos.shape[0]
    q = np.asarray(system["charge"], dtype=np.float64)
    eps = np.asarray(system["epsilon"], dtype=np.float64)
    sig = np.asarray(system["sigma"], dtype=np.float64)
    frozen = np.asarray(system["frozen"]).astype(bool)
    midx = _molecule_index(system["molecule"])
    molmass = np.bincount(midx, weights=np.asarray(system["mass"], dtype=np.float64))[midx]  # pairs.c:373-375
    vol, rb, rc = pbc(system["basis"], params.get("pbc_cutoff", 0.0))
    alpha = params["ewald_alpha"] if params.get("ewald_alpha_set") else 3.5 / rc  # pbc.c:73-74
    palpha = params["polar_ewald_alpha"] if params.get("polar_ewald_alpha_set") else 3.5 / rc  # pbc.c:75-76
    rd_only = bool(params.get("rd_only"))
    wolf = bool(params.get("wolf"))
    fh = int(params.get("feynman_hibbs_order", 2)) if params.get("feynman_hibbs") else 0
    T = LD(params.get("temperature", 0.0))
    fmode = field_mode(params)

    I, J = np.triu_indices(n, 1)
    image, r, rimg, dimg = minimum_image(system["basis"], rb, pos[I] - pos[J])
    same = midx[I] == midx[J]
    fz = frozen[I] & frozen[J]
    rd_excl = same | (eps[I] == 0.0) | (sig[I] == 0.0) | (eps[J] == 0.0) | (sig[J] == 0.0)  # pairs.c:55-81
    es_excl = same | (q[I] == 0.0) | (q[J] == 0.0)
    attractive = (sig[I] < 0.0) | (sig[J] < 0.0)  # pair epsilon never set: contributes 0 (pairs.c:200-203)

    in_rd = (rimg - SMALL_dR < rc) & ~rd_excl & ~fz  # lj.c:189
    if rd_only:
        in_es = np.zeros_like(in_rd)
        intra = np.zeros_like(in_rd)
    elif wolf:
        in_es = ~fz & ~es_excl & (rimg < rc)  # coulombic.c:291
        intra = np.zeros_like(in_rd)
    else:
        in_es = ~fz & ~((rimg > rc) | es_excl)  # coulombic.c:167
        intra = ~fz & same & (q[I] != 0.0) & (q[J] != 0.0)  # coulombic.c:181 (a zero charge gives exactly 0)
    if fmode in ("bare", "wolf"):
        in_field = ~fz & ~same & (rimg - SMALL_dR < rc) & (rimg != 0.0)  # thole_field.c:46-50, 92-96
    elif fmode == "ewald":
        in_field = ~fz & ~((rimg > rc) | (rimg == 0.0))  # polar_ewald.c:49-52
    else:
        in_field = np.zeros_like(in_rd)
    sel = np.flatnonzero(in_rd | in_es | intra | in_field | (rimg <= rc + keep))
    I, J, image, r, rimg, dimg = I[sel], J[sel], image[sel], r[sel], rimg[sel], dimg[sel]
    same, in_rd, in_es, intra, in_field, es_excl = same[sel], in_rd[sel], in_es[sel], intra[sel], in_field[sel], es_excl[sel]
    m = len(sel)
    R = rimg.astype(LD)
    qi, qj = q[I].astype(LD), q[J].astype(LD)

    # ---- repulsion / dispersion, lj.c:189-250 (+ lj_fh_corr, lj.c:11-54)
    rd = np.zeros(m, LD)
    k = np.flatnonzero(in_rd & ~attractive[sel])
    if k.size:
        Rk = R[k]
        s = (LD(0.5) * (sig[I[k]].astype(LD) + sig[J[k]].astype(LD)))
        e = np.sqrt(eps[I[k]].astype(LD) * eps[J[k]].astype(LD))
        s6 = (np.abs(s) / Rk) ** 6
        s12 = s6 * s6
        val = 4 * e * (s12 - s6)
        if fh:
            ir = 1 / Rk
            rm = AMU2KG * molmass[I[k]].astype(LD) * molmass[J[k]].astype(LD) / (molmass[I[k]].astype(LD) + molmass[J[k]].astype(LD))
            dE = -24 * e * (2 * s12 - s6) * ir
            d2E = 24 * e * (26 * s12 - 7 * s6) * ir ** 2
            val = val + M2A2 * (HBAR2 / (24 * KB * T * rm)) * (d2E + 2 * dE / Rk)
            if fh >= 4:
                d3E = -1344 * e * (6 * s12 - s6) * ir ** 3
                d4E = 12096 * e * (10 * s12 - s6) * ir ** 4
                val = val + M2A4 * (HBAR4 / (1152 * KB2 * T * T * rm * rm)) * (15 * dE * ir ** 3 + 4 * d3E * ir + d4E)
        rd[k] = val

    # ---- electrostatics: Wolf (coulombic.c:269-308) or the Ewald real term (coulombic.c:149-194, FH :115-146)
    es = np.zeros(m, LD)
    es_intra = np.zeros(m, LD)
    k = np.flatnonzero(in_es)
    if k.size and wolf:
        Rk = R[k]
        rcl = LD(rc)
        erfaRoverR = LD(math.erf(alpha * rc)) / rcl
        es[k] = qi[k] * qj[k] * (1 / Rk - erfaRoverR - (1 / rcl) ** 2 * (rcl - Rk))
    elif k.size:
        Rk = R[k]
        a = LD(alpha)
        erfc_t = erfc_ld(alpha * rimg[k])
        val = qi[k] * qj[k] * erfc_t / Rk
        if fh:  # added WITHOUT q_i q_j, as the reference does
            g = np.exp(-a * a * Rk * Rk)
            ir = 1 / Rk
            rm = AMU2KG * molmass[I[k]].astype(LD) * molmass[J[k]].astype(LD) / (molmass[I[k]].astype(LD) + molmass[J[k]].astype(LD))
            sp = np.sqrt(PI)
            du = -2 * a * g / (Rk * sp) - erfc_t * ir ** 2
            d2u = (4 / sp) * g * (a ** 3 + ir ** 2) + 2 * erfc_t * ir ** 3
            val = val + M2A2 * (HBAR2 / (24 * KB * T * rm)) * (d2u + 2 * du / Rk)
            if fh >= 4:
                d3u = (g / sp) * (-8 * a ** 5 * Rk - 8 * a ** 3 / Rk - 12 * a * ir ** 3) - 6 * erfc_t * ir ** 4
                d4u = (g / sp) * (8 * a ** 5 + 16 * a ** 7 * Rk * Rk + 32 * a ** 3 * ir ** 2 + 48 * ir ** 4) + 24 * erfc_t * ir ** 5
                val = val + M2A4 * (HBAR4 / (1152 * (KB * KB * T * T * rm * rm))) * (15 * du * ir ** 3 + 4 * d3u / Rk + d4u)
        es[k] = val
    k = np.flatnonzero(intra)
    if k.size:  # screening term of same-molecule pairs, on the UN-imaged r (coulombic.c:181-182)
        es_intra[k] = qi[k] * qj[k] * erf_ld(alpha * r[k]) / r[k].astype(LD)

    # ---- static field: thole_field.c:39-124 (bare, Wolf), polar_ewald.c:38-80 (Ewald real term)
    f = np.zeros(m, LD)
    k = np.flatnonzero(in_field)
    if k.size:
        Rk = R[k]
        if fmode == "bare":
            f[k] = 1 / Rk ** 3
        elif fmode == "wolf":
            a = LD(params.get("polar_wolf_alpha", 0.0))
            rcl = LD(rc)
            if a == 0:
                f[k] = (1 / Rk ** 2 - 1 / rcl ** 2) / Rk
            else:
                aw = float(params["polar_wolf_alpha"])
                cut = LD(math.erfc(aw * rc)) / rcl ** 2 + 2 * a * ONE_OVER_SQRT_PI * np.exp(-a * a * rcl * rcl) / rcl
                big = erfc_ld(aw * rimg[k]) / Rk ** 2 + 2 * a * ONE_OVER_SQRT_PI * np.exp(-a * a * Rk * Rk) / Rk
                f[k] = (big - cut) / Rk
        else:
            a = LD(palpha)
            g = 2 * a * ONE_OVER_SQRT_PI * np.exp(-a * a * Rk * Rk) * Rk
            ex = es_excl[k]
            f[k] = np.where(ex, g - erf_ld(palpha * rimg[k]), g + erfc_ld(palpha * rimg[k])) / Rk ** 3
    D = dimg.astype(LD)
    field_i = (f * qj)[:, None] * D
    field_j = -(f * qi)[:, None] * D
    return dict(i=I, j=J, image=image.astype(np.int64), r=r, rimg=rimg, dimg=dimg, rd=rd, es=es, es_intra=es_intra,
                field_i=field_i, field_j=field_j, in_rd=in_rd, in_es=in_es, in_field=in_field, same=same,
                rc=rc, ewald_alpha=alpha, polar_alpha=palpha, volume=vol, n=n)


def lj_lrc(system, params):
    """LJ long-range correction, lj.c:56-107: pair part over all non-frozen pairs with eps_ij sig_ij != 0 (same-molecule
    pairs included) + per-atom self part."""
    if not params.get("rd_lrc", 1):
        return LD(0)
    eps = np.asarray(system["epsilon"], dtype=np.float64)
    sig = np.asarray(system["sigma"], dtype=np.float64)
    frozen = np.asarray(system["frozen"]).astype(bool)
    vol, _, rc = pbc(system["basis"], params.get("pbc_cutoff", 0.0))
    n = len(eps)
    I, J = np.triu_indices(n, 1)
    neg = (sig[I] < 0) | (sig[J] < 0)
    zero = (sig[I] == 0) | (sig[J] == 0)
    s = np.where(neg, 0.5 * (np.abs(sig[I]) + np.abs(sig[J])), np.where(zero, 0.0, 0.5 * (sig[I] + sig[J]))).astype(LD)
    e = np.where(neg, 0.0, np.sqrt(eps[I].astype(LD) * eps[J].astype(LD)))

    def term(e_, s_):
        sc = np.abs(s_) / LD(rc)
        return (LD(16) / 3) * PI * e_ * np.abs(s_) ** 3 * (sc ** 9 / 3 - sc ** 3) / LD(vol)

    k = (e != 0) & (s != 0) & ~(frozen[I] & frozen[J])
    total = term(e[k], s[k]).sum()
    k = (sig != 0) & (eps != 0) & ~frozen
    return total + term(eps[k].astype(LD), sig[k].astype(LD)).sum()


def ewald_field_recip(system, params):
    """recip_term(), polar_ewald.c:85-132: not a pair sum, restated here (fp64 phases, longdouble accumulation) so that
    the Ewald static field of the table can be compared with ef_static as a whole."""
    pos = np.ascontiguousarray(system["pos"], dtype=np.float64)
    q = np.asarray(system["charge"], dtype=np.float64).astype(LD)
    vol, rb, rc = pbc(system["basis"], params.get("pbc_cutoff", 0.0))
    ea = params["polar_ewald_alpha"] if params.get("polar_ewald_alpha_set") else 3.5 / rc
    kmax = int(params.get("ewald_kmax", 7))
    kv = 2.0 * math.pi * (kvector_list(kmax).astype(np.float64) @ rb.T)  # k_p = 2 pi sum_q recip[p][q] l_q
    ef = np.zeros((len(pos), 3), LD)
    for c0 in range(0, len(kv), 256):
        k = kv[c0:c0 + 256]
        k2 = (k * k).sum(axis=1)
        w = (k / k2[:, None]).astype(LD) * np.exp(-(k2.astype(LD)) / (4 * LD(ea) * LD(ea)))[:, None]
        ph = pos @ k.T
        co, si = np.cos(ph).astype(LD), np.sin(ph).astype(LD)
        f1, f2 = (q[:, None] * co).sum(axis=0), (q[:, None] * si).sum(axis=0)
        ef += (si * f1 - co * f2) @ w
    return ef * (8 * PI / LD(vol))


def kvector_list(kmax):
    """the half sphere of coulombic.c:56-60 and polar_ewald.c:85-100, in loop order"""
    ks = []
    for l0 in range(0, kmax + 1):
        for l1 in range(0 if l0 == 0 else -kmax, kmax + 1):
            for l2 in range(1 if (l0 == 0 and l1 == 0) else -kmax, kmax + 1):
                if l0 * l0 + l1 * l1 + l2 * l2 <= kmax * kmax:
                    ks.append((l0, l1, l2))
    return np.asarray(ks, dtype=np.int64).reshape(-1, 3)


U64 = 2.0 ** -53
C_PHASE = 8  # roundings between the inputs and a phase, see ewald_recip_energy()
C_WEIGHT = 19  # roundings between k, S(k) and a term of the k sum, see ewald_recip_energy()


def ewald_recip_energy(system, params):
    """coulombic_reciprocal(), coulombic.c:42-95: U = (4 pi / V) sum_k exp(-k^2 / 4 a^2) / k^2 |S(k)|^2 over the half
    sphere, S(k) = sum q_a e^{i k.x_a} over the atoms that are not frozen and carry a charge.  Returns (U, dU): the value
    in longdouble and the bound of an fp64 evaluation's distance from it.

    The phases are fp64 as the reference forms them (k_p = sum_q 2 pi recip[p][q] l_q accumulated in q, k.x accumulated in
    p): they are arguments of cos / sin, so their rounding is part of the answer's definition only up to the bound below.
    cos / sin of the fp64 phase, the products, S(k), the weights and the k sum are longdouble.

    dS_k = sum_a |q_a| (C_PHASE u Phi_ak + 2u) + N u sum_a |q_a|,   Phi_ak = sum_p |k_p x_ap|
    dU   = (4 pi / V) sum_k w_k (2 |S_k| dS_k + dS_k^2) + (C_WEIGHT + nk + max k^2/4a^2) u U
    C_PHASE: k_p is three products of two factors and two additions (4, relative to sum_q |2 pi recip[p][q] l_q|), k.x a
    product and two additions (3), one to spare for another association (2 pi (recip l)): 8.  2u: cos / sin to 1 ulp
    (at most u absolute) and the product with q.  N u: the sum of N terms in any order.  C_WEIGHT: k^2 (3), 4 a^2 (2), the
    quotient (1), exp (1 ulp = 2u, and u of its argument), / k^2 (1 + 3), |S|^2 (3), the product (1), 4 pi / V (3): 19;
    nk u for the k sum."""
    pos = np.ascontiguousarray(system["pos"], dtype=np.float64)
    q = np.asarray(system["charge"], dtype=np.float64)
    frozen = np.asarray(system["frozen"]).astype(bool)
    vol, rb, rc = pbc(system["basis"], params.get("pbc_cutoff", 0.0))
    ea = params["ewald_alpha"] if params.get("ewald_alpha_set") else 3.5 / rc
    ls = kvector_list(int(params.get("ewald_kmax", 7))).astype(np.float64)
    sel = ~frozen & (q != 0.0)
    x, qs = pos[sel], q[sel]
    N = len(qs)
    kv = np.zeros((len(ls), 3))
    kabs = np.zeros((len(ls), 3))
    for p in range(3):
        for c in range(3):
            t = 2.0 * math.pi * rb[p][c] * ls[:, c]
            kv[:, p] = kv[:, p] + t
            kabs[:, p] = kabs[:, p] + np.abs(t)
    total, dtotal, argmax = LD(0), LD(0), 0.0
    qa = np.abs(qs).astype(LD)
    for c0 in range(0, len(kv), 256):
        k = kv[c0:c0 + 256]
        ph = x[:, 0:1] * k[None, :, 0]
        ph = ph + x[:, 1:2] * k[None, :, 1]
        ph = ph + x[:, 2:3] * k[None, :, 2]
        phl = ph.astype(LD)
        re = (qs.astype(LD)[:, None] * np.cos(phl)).sum(axis=0)
        im = (qs.astype(LD)[:, None] * np.sin(phl)).sum(axis=0)
        Phi = np.abs(x).astype(LD) @ kabs[c0:c0 + 256].T.astype(LD)
        dS = (qa[:, None] * (C_PHASE * U64 * Phi + 2 * U64)).sum(axis=0) + N * U64 * qa.sum()
        k2 = (k.astype(LD) ** 2).sum(axis=1)
        arg = k2 / (4 * LD(ea) * LD(ea))
        argmax = max(argmax, float(arg.max()))
        w = np.exp(-arg) / k2
        S = np.sqrt(re * re + im * im)
        total += (w * (re * re + im * im)).sum()
        dtotal += (w * (2 * S * dS + dS * dS)).sum()
    f = 4 * PI / LD(vol)
    U = f * total
    return U, float(f * dtotal + (C_WEIGHT + len(kv) + argmax) * U64 * abs(U))


def ewald_self_energy(system, params):
    """coulombic_self(), coulombic.c:97-112: -sum alpha q^2 / sqrt(pi) over the atoms that are not frozen (pi is the
    reference's fp64 M_PI).  Returns (U_self in longdouble, the number of terms)."""
    q = np.asarray(system["charge"], dtype=np.float64)
    frozen = np.asarray(system["frozen"]).astype(bool)
    _, _, rc = pbc(system["basis"], params.get("pbc_cutoff", 0.0))
    ea = params["ewald_alpha"] if params.get("ewald_alpha_set") else 3.5 / rc
    qs = q[~frozen].astype(LD)
    return -(LD(ea) * qs * qs / np.sqrt(PI)).sum(), int(len(qs))


def sums(table, system, params):
    """What the engine and the oracle report, from the table: rd_energy (LRC included), es_real (real term minus the
    intra-molecular screening term; the Wolf sum under wolf=1) and, with polarization, ef_static[n,3]."""
    out = dict(rd_energy=float(table["rd"].sum() + lj_lrc(system, params)),
               es_real=float(table["es"].sum() - table["es_intra"].sum()))
    if field_mode(params):
        ef = np.zeros((table["n"], 3), LD)
        np.add.at(ef, table["i"], table["field_i"])
        np.add.at(ef, table["j"], table["field_j"])
        if field_mode(params) == "ewald":
            ef += ewald_field_recip(system, params)
        out["ef_static"] = ef.astype(np.float64)
    return out


def describe(table, k, note=""):
    """One line for pair row k: 'pair (i, j), image (0,1,0), rimg 11.12 < rc 11.35, ...'"""
    rimg, rc = table["rimg"][k], table["rc"]
    return "pair (%d, %d), image (%d,%d,%d), rimg %.15g %s rc %.15g (rimg - rc = %.3e)%s" % (
        table["i"][k], table["j"][k], *table["image"][k], rimg, "<" if rimg < rc else (">" if rimg > rc else "=="), rc,
        rimg - rc, (", " + note) if note else "")


def explain_energy(table, channel, diff, rows=None, top=5):
    """Rows whose removal (diff ~ -value: 'missing') or addition (diff ~ +value: 'extra') explains got - want = diff
    on an energy channel best.  `rows`: candidate row indices (default: all)."""
    rows = np.arange(len(table["i"])) if rows is None else np.asarray(rows)
    v = np.asarray(table[channel][rows], dtype=np.float64)
    if channel == "es":
        v = v - np.asarray(table["es_intra"][rows], dtype=np.float64)
    cand = [(abs(diff + x), r, "missing") for x, r in zip(v, rows) if x != 0.0]
    cand += [(abs(diff - x), r, "extra") for x, r in zip(v, rows) if x != 0.0]
    cand.sort(key=lambda t: t[0])
    head = []
    if cand and cand[0][0] > 0.05 * abs(diff):
        med = float(np.median(np.abs(v[v != 0.0])))
        head = ["no single pair explains it; the difference is about %.1f median probe terms (%.3e each) -- several pairs "
                "missing or extra; the closest single ones:" % (abs(diff) / med, med)]
    return head + [describe(table, r, "%s would leave a residual of %.3e (its %s term is %.6e)" % (
        what, res, channel, float(table[channel][r]))) for res, r, what in cand[:top]]


def explain_field(table, got, want, top=5):
    """For the atoms with the largest ef_static error: the partner whose pair term, removed or added, explains it best."""
    err = got - want
    out = []
    for a in np.argsort(-np.abs(err).max(axis=1))[:top]:
        rows_i, rows_j = np.flatnonzero(table["i"] == a), np.flatnonzero(table["j"] == a)
        best = None
        for rows, key in ((rows_i, "field_i"), (rows_j, "field_j")):
            for r in rows:
                v = np.asarray(table[key][r], dtype=np.float64)
                if not v.any():
                    continue
                for sgn, what in ((1.0, "missing"), (-1.0, "extra")):
                    res = np.abs(err[a] + sgn * v).max()
                    if best is None or res < best[0]:
                        best = (res, r, what)
        if best is not None:
            out.append("atom %d: field error %.3e; %s" % (a, np.abs(err[a]).max(), describe(
                table, best[1], "%s would leave %.3e" % (best[2], best[0]))))
    return out
