"""Per-pair longdouble reference of the pair potentials of mpmc_hip_set_rd_form (mpmc_amd/csrc/kernels_rdforms.h):
Silvera-Goldman, DREIDING, the buffered 14-7 and Lennard-Jones, under the four mixing rules.  Helper module for the tests
(a plain import, not a conftest), written from the reference's formulas (energy/sg.c:13-91, dreiding.c:13-108,
lj_buffered_14_7.c:6-35, lj.c:11-107, :165-276, mixing and exclusions energy/pairs.c:56-211, minimum image :230-290,
constants include/defines.h:8-50).  It shares nothing with oracle/ or with the kernels.

* DECISIONS are made in fp64 in the reference's operation order, which is what numpy's elementwise arithmetic does: the
  minimum image and rimg; `rimg < cutoff` (sg), `!(rimg > cutoff)` (dreiding, lj_buffered_14_7), `rimg - 1e-12 < cutoff`
  (lj); x = rimg / 0.529177249 and `x < RM`; the sign / zero branches of the mixing; `rimg < 0.4 * sigma_ij` with the fp64
  sigma_ij; rd_excluded; frozen-frozen.
* VALUES are evaluated in numpy.longdouble from the fp64 inputs (parameters, rimg, cutoff, volume) and summed in
  longdouble.

Tolerance of a comparison with the engine: RD_TOL * abs_sum with RD_TOL = 1e-12 (the project's bound for its dense sums),
abs_sum = the sum of |every term|: each piece of every pair (the repulsion and each multipole piece of sg, the exponential
and the r^-6 piece of dreiding, the two factors' product of the 14-7 as one piece, the r^-12 and r^-6 pieces of
Lennard-Jones), every addend of a Feynman-Hibbs term and every long-range-correction term separately.  An fp64 evaluation
is off by a few ulp (2^-53 = 1.1e-16) per piece plus a sum of depth log2(#pairs) <= 16: ~1e-14 * abs_sum, two orders
inside the bound.
    The one place where an input error is amplified is sg's exponential.  Its argument a = ALPHA - BETA x - GAMMA x^2 is
formed in fp64 from x = rimg / 0.529177249 (one rounding) with three more roundings, each relative to a partial result of
magnitude <= max(ALPHA, BETA x + GAMMA x^2).  With x < cutoff / 0.529 <= ~30 Bohr for a cutoff up to 16 A the partial
results stay below 1.5671 * 30 + 0.00993 * 900 = 56, and |a| itself <= ~55; inside the range where exp(a) matters at all
(exp(a) >= 1e-12 of the multipole term, |a| <= ~30) the absolute error of a is <= 5 * 2^-53 * 30 = 1.7e-14, so exp(a) is
off by 1.7e-14 relative: 60 times inside RD_TOL.  The damping exponent -(RM / x - 1)^2 lies in [-(RM/x)^2, 0] and is O(1)
for every x a real configuration reaches (x > 2 Bohr: |.| < 10): error < 1e-15.
"""
import numpy as np

LD = np.longdouble
RD_TOL = 1e-12

FORMS = ("lj", "sg", "dreiding", "lj_buffered_14_7")
MIXINGS = ("lb", "waldmanhagler", "halgren_mixing", "c6_mixing")

# include/defines.h (the fp64 constants, widened exactly)
HBAR, HBAR2, HBAR4 = LD(1.054571e-34), LD(1.11211999e-68), LD(1.23681087e-136)
KB, KB2 = LD(1.3806503e-23), LD(1.90619525e-46)
AMU2KG = LD(1.66053873e-27)
M2A2, M2A4, METER2ANGSTROM = LD(1.0e20), LD(1.0e40), LD(1.0e10)
PI = LD(np.pi)
SG_ALPHA, SG_BETA, SG_GAMMA = 1.713, 1.5671, 0.00993
SG_C6, SG_C8, SG_C10, SG_C9, SG_RM = 12.14, 215.2, 4813.9, 143.1, 8.321
AU2ANGSTROM = 0.529177249
HARTREE2KELVIN = LD(3.15774655e5)
DREIDING_GAMMA = 12.0
MAXVALUE = LD(1.0e40)
SMALL_dR = 1.0e-12


def box(basis, cutoff_in=0.0):
    """energy/pbc.c:13-83 in fp64 scalars: (volume, reciprocal basis, cutoff); cutoff 0 = half the shortest lattice
    vector over coefficients -5 .. 5."""
    b = [[float(basis[p][q]) for q in range(3)] for p in range(3)]
    vol = b[0][0] * (b[1][1] * b[2][2] - b[1][2] * b[2][1])
    vol += b[0][1] * (b[1][2] * b[2][0] - b[1][0] * b[2][2])
    vol += b[0][2] * (b[1][0] * b[2][1] - b[1][1] * b[2][0])
    cutoff = float(cutoff_in)
    if cutoff == 0.0:
        short = 1.0e40
        for i in range(-5, 6):
            for j in range(-5, 6):
                for k in range(-5, 6):
                    if i or j or k:
                        v = [i * b[0][q] + j * b[1][q] + k * b[2][q] for q in range(3)]
                        short = min(short, float(np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])))
        cutoff = 0.5 * short
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


def rimg_of(basis, rb, d):
    """pairs.c:230-290: the minimum-image distance of displacements d[:, 3], fp64, one rounding per operation"""
    b = np.asarray(basis, dtype=np.float64)
    d0, d1, d2 = d[:, 0], d[:, 1], d[:, 2]
    img = []
    for p in range(3):
        f = rb[0][p] * d0
        f = f + rb[1][p] * d1
        f = f + rb[2][p] * d2
        img.append(np.rint(f))
    ri2 = 0.0
    for p in range(3):
        t = b[0][p] * img[0]
        t = t + b[1][p] * img[1]
        t = t + b[2][p] * img[2]
        e = d[:, p] - t
        ri2 = e * e if p == 0 else ri2 + e * e
    r2 = d0 * d0
    r2 = r2 + d1 * d1
    r2 = r2 + d2 * d2
    rimg = np.sqrt(ri2)
    return np.where(np.isnan(rimg), np.sqrt(r2), rimg)


def mix(mixing, ei, si, ej, sj):
    """pairs.c:84-211 for arrays of per-atom values: (sigma_ij fp64 -- for the decisions --, sigma_ij longdouble,
    eps_ij longdouble, attractive_only).  The epsilon of an attractive-only pair is never assigned in the reference: 0."""
    ei, si, ej, sj = (np.asarray(a, dtype=np.float64) for a in (ei, si, ej, sj))
    Ei, Si, Ej, Sj = (a.astype(LD) for a in (ei, si, ej, sj))
    attractive = np.zeros(ei.shape, bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        if mixing == "waldmanhagler":
            neg = (si < 0) | (sj < 0)
            zero = ~neg & ((si == 0) | (sj == 0))
            s64 = np.where(zero, 0.0, (0.5 * (si ** 6 + sj ** 6)) ** (1.0 / 6.0))
            S = np.where(zero, LD(0), ((Si ** 6 + Sj ** 6) / 2) ** (LD(1) / 6))
            E = np.where(neg, LD(0), np.where(zero, np.sqrt(Ei * Ej),
                                               np.sqrt(Ei * Ej) * 2 * Si ** 3 * Sj ** 3 / (Si ** 6 + Sj ** 6)))
            attractive = neg
        elif mixing == "halgren_mixing":
            ps = (si > 0) & (sj > 0)
            pe = (ei > 0) & (ej > 0)
            s64 = np.where(ps, (si * si * si + sj * sj * sj) / (si * si + sj * sj), 0.0)
            S = np.where(ps, (Si ** 3 + Sj ** 3) / (Si ** 2 + Sj ** 2), LD(0))
            E = np.where(pe, 4 * Ei * Ej / (np.sqrt(np.abs(Ei)) + np.sqrt(np.abs(Ej))) ** 2, LD(0))
        elif mixing == "c6_mixing":
            s64 = 0.5 * (si + sj)
            S = (Si + Sj) / 2
            E = np.where(s64 != 0.0, 64 * np.sqrt(Ei * Ej) * Si ** 3 * Sj ** 3 / (Si + Sj) ** 6, LD(0))
        elif mixing == "lb":
            neg = (si < 0) | (sj < 0)
            zero = ~neg & ((si == 0) | (sj == 0))
            s64 = np.where(neg, 0.5 * (np.abs(si) + np.abs(sj)), np.where(zero, 0.0, 0.5 * (si + sj)))
            S = np.where(neg, (np.abs(Si) + np.abs(Sj)) / 2, np.where(zero, LD(0), (Si + Sj) / 2))
            E = np.where(neg, LD(0), np.sqrt(Ei * Ej))
            attractive = neg
        else:
            raise KeyError(mixing)
    return s64, S, E, attractive


def sg_pieces(rimg, fh=False, temperature=None, mass=None):
    """sg.c:34-77 for fp64 rimg (A, inside the cutoff): (term in K, sum |pieces| in K), longdouble.  mass: the molecular mass
    (amu) of the pair's first atom."""
    rimg = np.asarray(rimg, dtype=np.float64)
    x64 = rimg / AU2ANGSTROM
    x = rimg.astype(LD) / LD(AU2ANGSTROM)
    rep = np.exp(LD(SG_ALPHA) - LD(SG_BETA) * x - LD(SG_GAMMA) * x * x)
    m6, m8, m10, m9 = LD(SG_C6) / x ** 6, LD(SG_C8) / x ** 8, LD(SG_C10) / x ** 10, LD(SG_C9) / x ** 9
    mult = m6 + m8 + m10 - m9
    r_rm = LD(SG_RM) / x
    damp = np.where(x64 < SG_RM, np.exp(-(r_rm - 1) ** 2), LD(1))
    term = rep - mult * damp
    pieces = np.abs(rep) + (np.abs(m6) + np.abs(m8) + np.abs(m10) + np.abs(m9)) * damp
    if fh:
        bg = LD(SG_BETA) + 2 * LD(SG_GAMMA) * x
        rd1 = (r_rm * r_rm - r_rm) / x
        rd2 = (3 * r_rm * r_rm - 2 * r_rm) / (x * x)
        d1 = [-bg * rep,
              (6 * LD(SG_C6) / x ** 7 + 8 * LD(SG_C8) / x ** 9 - 9 * LD(SG_C9) / x ** 10 + 10 * LD(SG_C10) / x ** 11) * damp,
              -2 * mult * damp * rd1]
        d2 = [(bg ** 2 - 2 * LD(SG_GAMMA)) * rep,
              -damp * (42 * LD(SG_C6) / x ** 8 + 72 * LD(SG_C8) / x ** 10 - 90 * LD(SG_C9) / x ** 11
                       + 110 * LD(SG_C10) / x ** 10),  # x^10, as sg.c:65 has it
              damp * rd1 * (12 * LD(SG_C6) / x ** 7 + 16 * LD(SG_C8) / x ** 9 - 18 * LD(SG_C9) / x ** 10
                            + 20 * LD(SG_C10) / x ** 11),
              damp * rd1 ** 2 * 4 * mult,
              damp * rd2 * 2 * mult]
        pre = METER2ANGSTROM ** 2 * (HBAR * HBAR / (24 * KB * LD(float(temperature)) * (AMU2KG * np.asarray(mass).astype(LD))))
        term = term + pre * (sum(d2) + 2 * sum(d1) / x)
        pieces = pieces + np.abs(pre) * (sum(np.abs(t) for t in d2) + 2 * sum(np.abs(t) for t in d1) / x)
    return term * HARTREE2KELVIN, pieces * HARTREE2KELVIN


def dreiding_pieces(rimg, s64, S, E, attractive):
    rimg = np.asarray(rimg, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ros = rimg.astype(LD) / S
        g = LD(DREIDING_GAMMA)
        t6 = ros ** -6 * (g / (g - 6))
        texp = np.where(attractive, LD(0), np.where(rimg < 0.4 * s64, MAXVALUE, np.exp(g * (1 - ros)) * (6 / (g - 6))))
        return E * (texp - t6), np.abs(E * texp) + np.abs(E * t6)


def buffered_pieces(rimg, S, E):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        rho = np.asarray(rimg, dtype=np.float64).astype(LD) / S
        t = E * (LD(1.07) / (rho + LD(0.07))) ** 7 * (LD(1.12) / (rho ** 7 + LD(0.12)) - 2)
        return t, np.abs(t)


def lj_pieces(rimg, S, E, attractive, fh_order=0, temperature=None, mi=None, mj=None):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        R = np.asarray(rimg, dtype=np.float64).astype(LD)
        t6 = (np.abs(S) / R) ** 6
        t12 = np.where(attractive, LD(0), t6 * t6)
        term = 4 * E * (t12 - t6)
        pieces = np.abs(4 * E * t12) + np.abs(4 * E * t6)
        if fh_order:
            T = LD(float(temperature))
            ir = 1 / R
            mi, mj = np.asarray(mi).astype(LD), np.asarray(mj).astype(LD)
            rm = AMU2KG * mi * mj / (mi + mj)
            dE = -24 * E * (2 * t12 - t6) * ir
            d2E = 24 * E * (26 * t12 - 7 * t6) * ir ** 2
            p2 = M2A2 * (HBAR2 / (24 * KB * T * rm))
            term = term + p2 * (d2E + 2 * dE / R)
            pieces = pieces + np.abs(p2 * d2E) + np.abs(p2 * 2 * dE / R)
            if fh_order >= 4:
                d3E = -1344 * E * (6 * t12 - t6) * ir ** 3
                d4E = 12096 * E * (10 * t12 - t6) * ir ** 4
                p4 = M2A4 * (HBAR4 / (1152 * KB2 * T * T * rm * rm))
                term = term + p4 * (15 * dE * ir ** 3 + 4 * d3E * ir + d4E)
                pieces = pieces + np.abs(p4 * 15 * dE * ir ** 3) + np.abs(p4 * 4 * d3E * ir) + np.abs(p4 * d4E)
        return term, pieces


def _lrc_term(E, S, rc, vol):
    sc = np.abs(S) / LD(rc)
    return (LD(16) / 3) * PI * E * np.abs(S) ** 3 * (sc ** 9 / 3 - sc ** 3) / LD(vol)


def _molecule_index(molecule):
    m = np.asarray(molecule)
    return np.concatenate([[0], np.cumsum(m[1:] != m[:-1])]).astype(np.int64)


def rd_terms(system, flags, form, mixing="lb"):
    """rd_energy of one configuration under `form` / `mixing`.

    system: pos, epsilon, sigma, mass, molecule, frozen, basis.  flags: pbc_cutoff (default 0 = half the shortest lattice
    vector), rd_lrc (default 1; only the lj form has a correction), feynman_hibbs, feynman_hibbs_order, temperature.
    Returns a dict: total, pair, lrc, abs_sum (longdouble); table = (i, j, rimg, term) of the pairs that take part;
    cutoff, volume; cut_margin = the smallest nonzero |rimg - cutoff| over all candidate pairs; at_cutoff = candidate
    pairs with rimg == cutoff exactly."""
    assert form in FORMS and mixing in MIXINGS
    pos = np.asarray(system["pos"], dtype=np.float64)
    n = len(pos)
    eps = np.asarray(system["epsilon"], dtype=np.float64)
    sig = np.asarray(system["sigma"], dtype=np.float64)
    mol = _molecule_index(system["molecule"])
    frz = np.asarray(system["frozen"]).astype(bool)
    molmass = np.bincount(mol, weights=np.asarray(system["mass"], dtype=np.float64))[mol]
    vol, rb, rc = box(system["basis"], flags.get("pbc_cutoff", 0.0))
    fh = bool(flags.get("feynman_hibbs"))
    T = flags.get("temperature")

    i, j = np.triu_indices(n, 1)
    k = ~(frz[i] & frz[j])  # (sg: the owned deviation -- the reference sums uninitialised distances there)
    if form != "sg":
        k &= (mol[i] != mol[j]) & (eps[i] != 0) & (sig[i] != 0) & (eps[j] != 0) & (sig[j] != 0)  # rd_excluded
    i, j = i[k], j[k]
    rimg = rimg_of(system["basis"], rb, pos[i] - pos[j]) if i.size else np.zeros(0)
    dev = np.abs(rimg - rc)
    at_cutoff = int((dev == 0.0).sum())
    cut_margin = float(dev[dev > 0.0].min()) if (dev > 0.0).any() else np.inf
    if form == "sg":
        inside = rimg < rc
    elif form == "lj":
        inside = rimg - SMALL_dR < rc
    else:
        inside = ~(rimg > rc)
    i, j, rimg = i[inside], j[inside], rimg[inside]

    if form == "sg":
        term, pieces = sg_pieces(rimg, fh, T, molmass[i])
    else:
        s64, S, E, att = mix(mixing, eps[i], sig[i], eps[j], sig[j])
        if form == "dreiding":
            term, pieces = dreiding_pieces(rimg, s64, S, E, att)
        elif form == "lj_buffered_14_7":
            term, pieces = buffered_pieces(rimg, S, E)
        else:
            term, pieces = lj_pieces(rimg, S, E, att, int(flags.get("feynman_hibbs_order", 2)) if fh else 0, T,
                                     molmass[i], molmass[j])
    pair = term.sum(dtype=LD) if i.size else LD(0)
    abs_sum = pieces.sum(dtype=LD) if i.size else LD(0)

    lrc = LD(0)
    if form == "lj" and flags.get("rd_lrc", 1):
        a, b = np.triu_indices(n, 1)
        _, S, E, _ = mix(mixing, eps[a], sig[a], eps[b], sig[b])
        k = (E != 0) & (S != 0) & ~(frz[a] & frz[b])
        t = _lrc_term(E[k], S[k], rc, vol)
        lrc += t.sum(dtype=LD)
        abs_sum += np.abs(t).sum(dtype=LD)
        k = (sig != 0) & (eps != 0) & ~frz
        t = _lrc_term(eps[k].astype(LD), sig[k].astype(LD), rc, vol)
        lrc += t.sum(dtype=LD)
        abs_sum += np.abs(t).sum(dtype=LD)
    return dict(total=pair + lrc, pair=pair, lrc=lrc, abs_sum=abs_sum, table=(i, j, rimg, term), cutoff=rc, volume=vol,
                cut_margin=cut_margin, at_cutoff=at_cutoff)
