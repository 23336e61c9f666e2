"""Brute-force reference of the rd_crystal term: Lennard-Jones summed over lattice images beyond the minimum image, what
rdc_tile_kernel, rdc_self_kernel and lj_lrc_kernel at the crystal cutoff (mpmc_amd/csrc/kernels_crystal.h) sum.  Helper
module for the tests (a plain import, not a conftest), written from the reference's formulas (energy/lj.c:11-54,
:109-276, mixing energy/pairs.c:200-211) and independent of oracle/, which has no such term.

With o = rd_crystal_order: cutoff_c = 2.0 * pbc_cutoff * (float(o) - 0.5), images n in {-(o-1) .. o-1}^3 in the
reference's loop order.

* DECISIONS are made in fp64 in the reference's operation order, which is what numpy's elementwise arithmetic does:
  a[p] = ((0 + basis[0][p] n0 + basis[1][p] n1) + basis[2][p] n2) + (pos_i[p] - pos_j[p]),
  r_n = sqrt((a0 a0 + a1 a1) + a2 a2), an image is dropped when r_n > cutoff_c and by nothing else; a pair takes part
  when rimg - 1e-12 < cutoff_c (rimg: pair_reference.minimum_image); frozen-frozen pairs are out, same-molecule pairs
  are in without their n = 0 image; the sigma < 0 / sigma == 0 branches of the mixing.
* VALUES are evaluated in numpy.longdouble from the fp64 inputs (parameters, r_n, rimg, cutoff_c, volume) and summed in
  longdouble.
"""
import numpy as np

from pair_reference import AMU2KG, HBAR2, HBAR4, KB, KB2, LD, M2A2, M2A4, PI, SMALL_dR, _molecule_index, minimum_image, pbc


def crystal_cutoff(pbc_cutoff, order):
    return 2.0 * pbc_cutoff * (float(order) - 0.5)  # lj.c:176


def translations(basis, order):
    """[(n0, n1, n2), (t0, t1, t2)] in the reference's loop order, fp64, one rounding per operation (lj.c:204-207)"""
    b = [[float(basis[q][p]) for p in range(3)] for q in range(3)]
    out = []
    rng = range(-(order - 1), order)
    for n0 in rng:
        for n1 in rng:
            for n2 in rng:
                t = []
                for p in range(3):
                    a = 0.0
                    for q, nq in enumerate((n0, n1, n2)):
                        a += b[q][p] * nq
                    t.append(a)
                out.append(((n0, n1, n2), tuple(t)))
    return out


def _mix(eps, sig, i, j):
    """pairs.c:200-211: (longdouble epsilon_ij, fp64 |sigma_ij|, attractive_only).  epsilon_ij of an attractive-only pair
    is never set in the reference: 0."""
    neg = (sig[i] < 0) | (sig[j] < 0)
    zero = (sig[i] == 0) | (sig[j] == 0)
    s = np.where(neg, 0.5 * (np.abs(sig[i]) + np.abs(sig[j])), np.where(zero, 0.0, 0.5 * (sig[i] + sig[j])))
    e = np.where(neg, LD(0), np.sqrt(eps[i].astype(LD) * eps[j].astype(LD)))
    return e, np.abs(s), neg


def _lrc_term(e, s, rc, vol):
    """lj.c:69-80 / :92-103 in longdouble from the fp64 cutoff and volume"""
    sc = s / LD(rc)
    return (LD(16) / 3) * PI * e * s ** 3 * (sc ** 9 / 3 - sc ** 3) / LD(vol)


def rd_terms(system, flags, order):
    """rd_energy under rd_crystal and everything it is made of.

    system: pos, epsilon, sigma, mass, molecule, frozen, basis.  flags: rd_lrc (default 1), feynman_hibbs,
    feynman_hibbs_order, temperature, pbc_cutoff (default 0 = half the shortest lattice vector).
    Returns a dict: pair, self, lrc, total (longdouble); abs_sum = sum |terms| counting every image's |4 eps (sigma/r)^12|
    and |4 eps (sigma/r)^6|, every Feynman-Hibbs, long-range and self term; ties = images (pair and self) with r_n exactly
    cutoff_c; pair_ties / self_ties; image_margin = the smallest NONZERO |r_n - cutoff_c| over all pair and self images;
    rimg_margin = the smallest |rimg - 1e-12 - cutoff_c| over the pairs that are not frozen-frozen; cutoff, cutoff_c,
    volume.
    """
    pos = np.asarray(system["pos"], dtype=np.float64)
    n = len(pos)
    eps = np.asarray(system["epsilon"], dtype=np.float64)
    sig = np.asarray(system["sigma"], dtype=np.float64)
    mass = np.asarray(system["mass"], dtype=np.float64)
    mol = _molecule_index(system["molecule"])
    frz = np.asarray(system["frozen"]).astype(bool)
    molmass = np.bincount(mol, weights=mass)[mol]
    vol, rb, rc = pbc(system["basis"], flags.get("pbc_cutoff", 0.0))
    cut = crystal_cutoff(rc, order)
    images = translations(system["basis"], order)
    fh = int(flags.get("feynman_hibbs_order", 0)) if flags.get("feynman_hibbs") else 0

    abs_sum = LD(0)
    margins = []

    # ---- pair part
    i, j = np.triu_indices(n, 1)
    k = ~(frz[i] & frz[j])
    i, j = i[k], j[k]
    pair = LD(0)
    pair_ties = 0
    rimg_margin = np.inf
    if i.size:
        d = pos[i] - pos[j]
        _, _, rimg, _ = minimum_image(system["basis"], rb, d)
        rimg_margin = float(np.abs((rimg - SMALL_dR) - cut).min())
        inside = rimg - SMALL_dR < cut
        i, j, d, rimg = i[inside], j[inside], d[inside], rimg[inside]
        same = mol[i] == mol[j]
        e, s, neg = _mix(eps, sig, i, j)
        sl = s.astype(LD)
        s6 = np.zeros(i.size, LD)
        s12 = np.zeros(i.size, LD)
        a6 = np.zeros(i.size, LD)
        a12 = np.zeros(i.size, LD)
        for (n0, n1, n2), t in images:
            a0, a1, a2 = t[0] + d[:, 0], t[1] + d[:, 1], t[2] + d[:, 2]
            r = np.sqrt(a0 * a0 + a1 * a1 + a2 * a2)
            live = np.ones(i.size, bool) if (n0 or n1 or n2) else ~same
            dev = np.abs(r[live] - cut)
            pair_ties += int((dev == 0.0).sum())
            if (dev > 0.0).any():
                margins.append(float(dev[dev > 0.0].min()))
            use = live & ~(r > cut)
            with np.errstate(divide="ignore", invalid="ignore"):
                x6 = np.where(use, (sl / r.astype(LD)) ** 6, LD(0))
            s6 += x6
            s12 += x6 * x6
        t12 = np.where(neg, LD(0), s12)
        term = 4 * e * (t12 - s6)
        abs_sum += (np.abs(4 * e * t12) + np.abs(4 * e * s6)).sum(dtype=LD)  # (terms of one sign: the sum of the |images|)
        if fh:
            T = LD(float(flags["temperature"]))
            R = rimg.astype(LD)
            ir = 1 / R
            mi, mj = molmass[i].astype(LD), molmass[j].astype(LD)
            rm = AMU2KG * mi * mj / (mi + mj)
            dE = -24 * e * (2 * t12 - s6) * ir
            d2E = 24 * e * (26 * t12 - 7 * s6) * ir ** 2
            corr = M2A2 * (HBAR2 / (24 * KB * T * rm)) * (d2E + 2 * dE / R)
            if fh >= 4:
                d3E = -1344 * e * (6 * t12 - s6) * ir ** 3
                d4E = 12096 * e * (10 * t12 - s6) * ir ** 4
                corr = corr + M2A4 * (HBAR4 / (1152 * KB2 * T * T * rm * rm)) * (15 * dE * ir ** 3 + 4 * d3E * ir + d4E)
            term = term + corr
            abs_sum += np.abs(corr).sum(dtype=LD)
        pair = term.sum(dtype=LD)

    # ---- self part: every atom, frozen ones included, unless sigma == 0 and epsilon == 0 (lj.c:109-162)
    l6 = l12 = LD(0)
    self_ties = 0
    for (n0, n1, n2), t in images:
        if not (n0 or n1 or n2):
            continue
        r = float(np.sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]))
        dev = abs(r - cut)
        if dev == 0.0:
            self_ties += 1
        else:
            margins.append(dev)
        if r > cut:
            continue
        l6 += LD(0.5) / LD(r) ** 6
        l12 += LD(0.5) / LD(r) ** 12
    act = ~((sig == 0) & (eps == 0))
    sa = np.abs(sig[act]).astype(LD)
    ea = eps[act].astype(LD)
    u6 = sa ** 6 * l6
    u12 = np.where(sig[act] < 0, LD(0), sa ** 12 * l12)
    self_part = (4 * ea * (u12 - u6)).sum(dtype=LD)
    abs_sum += (np.abs(4 * ea * u12) + np.abs(4 * ea * u6)).sum(dtype=LD)

    # ---- long-range correction at cutoff_c (lj.c:56-107, :188, :273)
    lrc = LD(0)
    if flags.get("rd_lrc", 1):
        i, j = np.triu_indices(n, 1)
        e, s, _ = _mix(eps, sig, i, j)
        k = (e != 0) & (s != 0) & ~(frz[i] & frz[j])
        t = _lrc_term(e[k], s[k].astype(LD), cut, vol)
        lrc += t.sum(dtype=LD)
        abs_sum += np.abs(t).sum(dtype=LD)
        k = (sig != 0) & (eps != 0) & ~frz
        t = _lrc_term(eps[k].astype(LD), np.abs(sig[k]).astype(LD), cut, vol)
        lrc += t.sum(dtype=LD)
        abs_sum += np.abs(t).sum(dtype=LD)

    return dict(pair=pair, self=self_part, lrc=lrc, total=pair + self_part + lrc, abs_sum=abs_sum,
                ties=pair_ties + self_ties, pair_ties=pair_ties, self_ties=self_ties,
                image_margin=min(margins) if margins else np.inf, rimg_margin=rimg_margin, cutoff=rc, cutoff_c=cut,
                volume=vol)
