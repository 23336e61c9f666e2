"""numpy.longdouble reference of the iterative Thole solve: the damped dipole tensor, every variant of the self-consistent
iteration and U_pol, with a DERIVED running forward-error bound next to every vector.  Helper module for the tests (a
plain import, not a conftest), written from the reference's formulas (polarization/thole_matrix.c:38-146,
polarization/thole_iterative.c:13-259, energy/polar.c:31-135, energy/pairs.c:336-360) and independent of oracle/.

Two kinds of arithmetic, as in pair_reference.py:

* DECISIONS are made in fp64 as the reference makes them, because they define the answer: the lattice image
  (pair_reference.pbc / minimum_image: rint() of the fractional displacement in the reference's operation order), the
  `rimg == 0` branch (ir3 = ir5 = MAXVALUE, damp = 0, so T = 0), the view (alpha != 0), rank_metric and the stable
  descending bubble order, and the stopping rule (fixed count, or (new - old)^2 > precision^2 DEBYE2SKA^2 on the fp64
  values of the dipoles; 128 iterations give up).
* VALUES are longdouble: the displacement d = (x_i - x_j) - sum_q b_q image_q (exact to 2^-64 from the fp64 inputs),
  r = |d|, c3 = damp1 / r^3, c5 = damp2 / r^5, T = c3 I - 3 c5 d d^T, and every recurrence.

THE BOUND.  u = 2^-53.  An fp64 evaluation of the same formulas (kernels_polar.h thole_coef, kernels_coef.h
image_displacement, the reference itself) differs from this module by at most, per pair and component, `dT`; a sweep
s = T mu of 3 nv terms in any order adds gamma_{3nv+4} |T|~ |mu| (|T|~ = |c3| delta_pq + 3 |c5| |d_p d_q| >= |T|: the
kernels form c3 mu - 3 c5 d (d.mu), whose rounding is relative to the parts, not to their difference); so, with `err` the
bound of the dipoles that enter a sweep and dE that of the field,

    err_0 = alpha dE + C_INIT u |mu_0|
    es    = |T|~ err + dT |mu| + gamma_{3nv+4} |T|~ |mu|
    err   = alpha (dE + es) + C_STEP u (|alpha E| + |alpha s|)

applied per site in sweep order for Gauss-Seidel (later sites see the new bound of earlier ones), linearly through the
SOR / ESOR mix (|w| err_new + |1 - w| err_old + C_MIX u (|w new| + |(1 - w) old|)) and once more for the Palmo product
(es(final dipoles) + the bound of ef_induced).  The counts, one per rounded fp64 operation:

* displacement: x_i - x_j (1, relative to it); the translation sum_q b_qp image_q as three products and two additions
  (5, each at most u of sum_q |b_qp image_q|; taken as C_TRANS = 6 to cover second order); the final subtraction (1,
  relative to d_p).  The FMA form of image_displacement rounds once per step and lies inside this.
      dd_p = u |x_i - x_j|_p + C_TRANS u sum_q |b_qp image_q| + u |d_p|
* r = sqrt(d.d): three squares and two additions give r^2 to 3u, the root halves it and adds u/2: C_R = 2, so
      dr = C_R u r + sum_p dd_p |d_p| / r
* E1 = exp(-l r) (l^2 r^2 / 2 + l r + 1): l*l, r*r, their product, l*r, two additions (6, all terms positive so each
  is relative to the whole), exp to 1 ulp = 2u relative (the documented OCML bound), the product (1): C_DAMP = 9; the
  rounded argument l*r moves exp by u (l r) relative.  damp1 = 1 - E1 then rounds once, relative to damp1 -- this is
  the cancellation: (C_DAMP + l r) u E1 is an error of up to 9.4 u of ONE however small damp1 is.
      ddamp1 = (C_DAMP + l r) u E1 + u |damp1|
* E2 = exp(-l r) (l^3 r^2 r / 6): l*l, *l, r*r, two products, the division (6), exp (2), the product (1): C_DAMP again.
      ddamp2 = ddamp1 + (C_DAMP + l r) u E2 + u |damp2|
* ir = 1/r, ir3 = ir ir ir, ir5 = ir3 ir ir: 3 and 5 roundings, and one for the product with damp: C_C3 = 4, C_C5 = 6.
      dc3 = ddamp1 / r^3 + C_C3 u |c3| + |dc3/dr| dr,   |dc3/dr| <= l exp(-l r) (l r)^2 / (2 r^3) + 3 |c3| / r
      dc5 = ddamp2 / r^5 + C_C5 u |c5| + |dc5/dr| dr,   |dc5/dr| <= l exp(-l r) (l r)^3 / (6 r^5) + 5 |c5| / r
* T_pq = -3 d_p d_q c5 (+ c3): the products (C_T = 4, the reference multiplies damp2 and ir5 in one by one) and the
  addition (1, relative to |T|~):
      dT_pq = delta_pq dc3 + 3 |d_p d_q| dc5 + 3 |c5| (|d_p| dd_q + |d_q| dd_p) + C_T u 3 |c5 d_p d_q| + u |T|~_pq
* C_INIT = 2 (alpha * E, * polar_gamma), C_STEP = 3 (E - s relative to |E| + |s|, * alpha, and one to spare for the
  reference's E + E_self + E_ind association), C_MIX = 4 (two products, the sum, 1 - w; exp(-gamma k) of ESOR to 1 ulp
  adds 2 more on both weights: C_ESOR = 6).
* Under Gauss-Seidel the bound of ef_induced is err / alpha + C_EIND u (|E| + |s|), C_EIND = 2: the persistent chain kernel
  holds the dipoles (through the block's cached inverse) and reports E_ind = mu / alpha - E, one division and one
  subtraction on top of the dipole's own error, so an induced field far smaller than E carries rounding of E's size.

A constant may be raised only with such a count written next to it.  The bound is first order in u except where a
second-order term is named; on the regular cases it stays below 1e-11 max|mu| (tests/test_polar_reference.py asserts
that, so that a loose bound cannot hide a failure).

solve() takes E as an input ((n, 3), fp64: exact in longdouble), so that the solver is isolated from the field, which
has its own reference (pair_reference.sums()).
"""
import numpy as np

import pair_reference as pr

LD = np.longdouble
U = LD(2.0) ** -53
UF = float(U)
MAXVALUE = 1.0e40  # include/defines.h
DEBYE2SKA = 85.10597636  # include/defines.h
MAX_ITERATION_COUNT = 128  # include/defines.h
C_TRANS, C_R, C_DAMP, C_C3, C_C5, C_T = 6, 2, 9, 4, 6, 4
C_INIT, C_STEP, C_MIX, C_ESOR, C_EIND = 2, 3, 4, 6, 2
UP = 1.0 + 2.0 ** -48  # longdouble bounds are stored in fp64: rounded up


class Tensor:
    """The view (atom indices with alpha != 0), T (3nv x 3nv longdouble, zero diagonal blocks), Tabs = |T|~ and dT (fp64,
    rounded up), per-pair rimg (fp64, nv x nv) and image (nv x nv x 3), rmin over the view's pairs."""

    def __init__(self, system, damp, chunk=64, c5_scale=None, flip=None):
        pos = np.ascontiguousarray(system["pos"], dtype=np.float64)
        alpha = np.asarray(system["alpha"], dtype=np.float64)
        basis = np.asarray(system["basis"], dtype=np.float64)
        self.n = len(alpha)
        self.view = np.flatnonzero(alpha != 0.0)
        self.alpha = alpha[self.view]
        nv = self.nv = len(self.view)
        vol, rb, rc = pr.pbc(basis)
        self.cutoff = rc
        x = pos[self.view]
        xl = x.astype(LD)
        bl = basis.astype(LD)
        l = LD(damp)
        self.T = np.zeros((3 * nv, 3 * nv), LD)
        self.Tabs = np.zeros((3 * nv, 3 * nv))
        self.dT = np.zeros((3 * nv, 3 * nv))
        self.rimg = np.zeros((nv, nv))
        self.r = np.zeros((nv, nv))
        self.image = np.zeros((nv, nv, 3), dtype=np.int64)
        self.dT_pair = np.zeros((nv, nv))  # largest component of the pair's dT block
        self.c3 = np.zeros((nv, nv))  # (for explain(): which part of a pair's term an error follows)
        self.d = np.zeros((nv, nv, 3))  # (for explain(): the displacement, to try the neighbouring images)
        self.damp, self.basis = float(damp), basis
        for i0 in range(0, nv, chunk):
            i1 = min(nv, i0 + chunk)
            d0 = x[i0:i1, None, :] - x[None, :, :]  # fp64, as the reference forms it
            img, r, rimg, _ = pr.minimum_image(basis, rb, d0)
            if flip is not None:  # test hook: (i, j, lattice direction, +-1) moves one pair to the neighbouring image
                for (fi, fj, q, sgn) in flip:
                    for a, b, s in ((fi, fj, sgn), (fj, fi, -sgn)):
                        if i0 <= a < i1:
                            img[a - i0, b, q] += s
            self.rimg[i0:i1], self.r[i0:i1], self.image[i0:i1] = rimg, r, img
            trans = img.astype(LD) @ bl  # sum_q image_q b[q][p]
            trans_abs = np.abs(img).astype(LD) @ np.abs(bl)
            dx = xl[i0:i1, None, :] - xl[None, :, :]
            d = dx - trans
            dd = U * np.abs(dx) + C_TRANS * U * trans_abs + U * np.abs(d)
            R = np.sqrt((d * d).sum(-1))
            zero = rimg == 0.0  # the reference's branch, on its own fp64 rimg (also the diagonal)
            if flip is not None:  # (the moved pair is no longer at the distance minimum_image() reported)
                self.rimg[i0:i1] = np.where(zero, 0.0, R.astype(np.float64))
            Rs = np.where(zero, LD(1), R)
            dr = C_R * U * Rs + (dd * np.abs(d)).sum(-1) / Rs
            lr = l * Rs
            e = np.exp(-lr)
            E1 = e * (LD(0.5) * lr * lr + lr + 1)
            E2 = e * (lr ** 3 / 6)
            damp1 = 1 - E1
            damp2 = damp1 - E2
            c3 = damp1 / Rs ** 3
            c5 = damp2 / Rs ** 5
            if c5_scale is not None:  # test hook: (rows, cols, factor) on the view's site indices
                rows, cols, fac = c5_scale
                sel = np.zeros((nv, nv), bool)
                sel[np.ix_(rows, cols)] = True
                sel |= sel.T
                c5 = np.where(sel[i0:i1], c5 * LD(fac), c5)
            dd1 = (C_DAMP + lr) * U * E1 + U * np.abs(damp1)
            dd2 = dd1 + (C_DAMP + lr) * U * E2 + U * np.abs(damp2)
            dc3 = dd1 / Rs ** 3 + C_C3 * U * np.abs(c3) + (l * e * lr ** 2 / (2 * Rs ** 3) + 3 * np.abs(c3) / Rs) * dr
            dc5 = dd2 / Rs ** 5 + C_C5 * U * np.abs(c5) + (l * e * lr ** 3 / (6 * Rs ** 5) + 5 * np.abs(c5) / Rs) * dr
            ad = np.abs(d)
            dyad = d[..., :, None] * d[..., None, :]
            adyad = ad[..., :, None] * ad[..., None, :]
            T = -3 * c5[..., None, None] * dyad
            Tabs = 3 * np.abs(c5)[..., None, None] * adyad
            dT = 3 * adyad * dc5[..., None, None] + C_T * U * Tabs
            dT = dT + 3 * np.abs(c5)[..., None, None] * (ad[..., :, None] * dd[..., None, :] + dd[..., :, None] * ad[..., None, :])
            for p in range(3):
                T[..., p, p] += c3
                Tabs[..., p, p] += np.abs(c3)
                dT[..., p, p] += dc3
            dT = dT + U * Tabs
            keep = ~zero
            T, Tabs, dT = (a * keep[..., None, None] for a in (T, Tabs, dT))
            m = i1 - i0
            self.T[3 * i0:3 * i1] = T.transpose(0, 2, 1, 3).reshape(3 * m, 3 * nv)
            self.Tabs[3 * i0:3 * i1] = (Tabs.transpose(0, 2, 1, 3).reshape(3 * m, 3 * nv)).astype(np.float64) * UP
            self.dT[3 * i0:3 * i1] = (dT.transpose(0, 2, 1, 3).reshape(3 * m, 3 * nv)).astype(np.float64) * UP
            self.dT_pair[i0:i1] = dT.max(axis=(-1, -2)).astype(np.float64)
            self.c3[i0:i1] = (c3 * keep).astype(np.float64)
            self.d[i0:i1] = d.astype(np.float64)
        off = ~np.eye(nv, dtype=bool)
        self.rmin = float(self.rimg[off].min()) if nv > 1 else MAXVALUE
        self.gamma = (3 * nv + 4) * UF / (1.0 - (3 * nv + 4) * UF)

    def without(self, atom):
        """the tensor of the same geometry with alpha of `atom` set to 0: that site's rows and columns leave the view"""
        k = int(np.flatnonzero(self.view == atom)[0])
        keep = np.arange(self.nv) != k
        keep3 = np.repeat(keep, 3)
        t = object.__new__(Tensor)
        t.n, t.cutoff = self.n, self.cutoff
        t.view, t.alpha = self.view[keep], self.alpha[keep]
        nv = t.nv = self.nv - 1
        t.T, t.Tabs, t.dT = (a[np.ix_(keep3, keep3)] for a in (self.T, self.Tabs, self.dT))
        t.rimg, t.r, t.dT_pair, t.c3 = (a[np.ix_(keep, keep)] for a in (self.rimg, self.r, self.dT_pair, self.c3))
        t.image, t.d = self.image[np.ix_(keep, keep)], self.d[np.ix_(keep, keep)]
        t.damp, t.basis = self.damp, self.basis
        t.rmin = float(t.rimg[~np.eye(nv, dtype=bool)].min()) if nv > 1 else MAXVALUE
        t.gamma = (3 * nv + 4) * UF / (1.0 - (3 * nv + 4) * UF)
        return t

    def sums(self, mu, err, rows=slice(None)):
        """(T mu, its bound) on the given rows: es = |T|~ err + dT |mu| + gamma |T|~ |mu|"""
        s = self.T[rows] @ mu
        am = np.abs(mu).astype(np.float64) * UP
        es = self.Tabs[rows] @ (err + self.gamma * am) + self.dT[rows] @ am
        return s, es * UP

    def rank(self, system):
        """pairs.c:336-360 on the fp64 r / rimg: rmin over pairs of polarizable atoms (rimg), one count for both atoms of
        every such pair with the UN-imaged r <= 1.5 rmin.  Full-length fp64 array."""
        nv = self.nv
        metric = np.zeros(self.n)
        if nv > 1:
            close = (self.r <= self.rmin * 1.5) & ~np.eye(nv, dtype=bool)
            metric[self.view] = close.sum(axis=1).astype(np.float64)
        return metric


def _blocks64(d, damp):
    """T blocks of displacements d[..., 3] in plain fp64 (explain() only: candidates, not reference values)"""
    r = np.sqrt((d * d).sum(-1))
    r = np.where(r == 0.0, 1.0, r)
    lr = damp * r
    e = np.exp(-lr)
    d1 = 1.0 - e * (0.5 * lr * lr + lr + 1.0)
    d2 = d1 - e * lr ** 3 / 6.0
    T = -3.0 * (d2 / r ** 5)[..., None, None] * d[..., :, None] * d[..., None, :]
    for p in range(3):
        T[..., p, p] += d1 / r ** 3
    return T


def bubble_order(order, metric):
    """update_ranking(), thole_iterative.c:143-164: bubble passes that swap on a strict `<` = a stable descending sort of
    the current order."""
    order = np.asarray(order)
    return order[np.argsort(-metric[order], kind="stable")]


def solve(tensor, system, params, E, dE=None, history=False):
    """thole_iterative() + the energy sum of polar() on the view of `tensor`, E[n, 3] given.  Returns a dict: mu,
    ef_induced, ef_induced_change ((n, 3) longdouble, zero outside the view), *_err (fp64 bounds, same shape),
    polar_iterations, iter_success, rank_metric, ranked_array (all atoms), dipole_rrms, upol, upol_terms (sum of the
    absolute products), mu_in (the dipoles that entered the last contraction) and, with history (plain Jacobi), the lists
    mus (mu_0 .. mu_n) and sums (s_1 .. s_n, s_k = T mu_{k-1}) on the view's 3nv components."""
    t = tensor
    n, nv, view = t.n, t.nv, t.view
    a = np.repeat(t.alpha, 3).astype(LD)
    af = np.repeat(t.alpha, 3)
    Ev = np.asarray(E, dtype=np.float64)[view].reshape(-1).astype(LD)
    dEv = np.zeros(3 * nv) if dE is None else np.asarray(dE, dtype=np.float64)[view].reshape(-1)
    gamma = float(params.get("polar_gamma", 1.0))
    sor, esor = bool(params.get("polar_sor")), bool(params.get("polar_esor"))
    gs_ranked = bool(params.get("polar_gs_ranked"))
    gs = bool(params.get("polar_gs")) or gs_ranked
    palmo = bool(params.get("polar_palmo"))
    rrms_on = bool(params.get("polar_rrms"))
    precision = float(params.get("polar_precision", 0.0))
    max_iter = int(params.get("polar_max_iter", 10))
    assert not params.get("polar_wolf_full")

    def absf(v):
        return np.abs(v).astype(np.float64) * UP

    aE = a * Ev
    mu = aE if (sor or esor) else aE * LD(gamma)  # init_dipoles()
    err = af * dEv + C_INIT * UF * absf(mu)
    ef_ind, ef_ind_err = np.zeros(3 * nv, LD), np.zeros(3 * nv)
    change, change_err = np.zeros(3 * nv, LD), np.zeros(3 * nv)
    metric = t.rank(system) if gs_ranked else np.zeros(n)
    ranked = np.arange(n)
    slot = np.full(n, -1)
    slot[view] = np.arange(nv)
    mus, sums = [mu.copy()], []
    mu_in = mu.copy()
    site_rrms = np.zeros(nv)
    it, success = 0, 0
    keep = not params.get("polar_zodid")
    while keep:
        it += 1
        if it >= MAX_ITERATION_COUNT and precision:
            mu, err = aE, af * dEv + UF * absf(aE)
            change, change_err = np.zeros(3 * nv, LD), np.zeros(3 * nv)
            success = 1
            break
        old, old_err = mu.copy(), err.copy()
        mu_in = old
        if gs:
            mu, err = mu.copy(), err.copy()
            new, new_err = np.zeros(3 * nv, LD), np.zeros(3 * nv)
            s_all, es_all = np.zeros(3 * nv, LD), np.zeros(3 * nv)
            for atom in ranked:
                k = slot[atom]
                if k < 0:
                    continue
                rows = slice(3 * k, 3 * k + 3)
                s, es = t.sums(mu, err, rows)
                s_all[rows], es_all[rows] = s, es
                new[rows] = a[rows] * (Ev[rows] - s)
                new_err[rows] = af[rows] * (dEv[rows] + es) + C_STEP * UF * (absf(aE[rows]) + absf(a[rows] * s))
                mu[rows], err[rows] = new[rows], new_err[rows]
            # the chain kernel reports E_ind of a site as mu / alpha - E (gs_chain_kernel's epilogue), not as the sums
            # it added: the dipole's own bound over alpha, and C_EIND roundings relative to |E| + |s|
            es_all = new_err / af + C_EIND * UF * (absf(Ev) + absf(s_all))
        else:
            s_all, es_all = t.sums(mu, err)
            new = a * (Ev - s_all)
            new_err = af * (dEv + es_all) + C_STEP * UF * (absf(aE) + absf(a * s_all))
        ef_ind, ef_ind_err = -s_all, es_all
        sums.append(s_all)
        newf, oldf = new.astype(np.float64).reshape(nv, 3), old.astype(np.float64).reshape(nv, 3)
        if rrms_on or precision > 0:  # calc_dipole_rrms()
            with np.errstate(all="ignore"):
                v = np.sqrt(((newf - oldf) ** 2).sum(1) / (newf * newf).sum(1))
            site_rrms = np.where(np.isfinite(v), v, 0.0)
        if precision == 0.0:  # are_we_done_yet()
            keep = it != max_iter
        else:
            allowed = precision * precision * DEBYE2SKA * DEBYE2SKA
            keep = bool((((newf - oldf) * (newf - oldf)) > allowed).any())
        if palmo and not keep:  # palmo_contraction(): mu is new_mu under Gauss-Seidel and still old_mu under Jacobi
            s2, es2 = t.sums(mu, err)
            change = -ef_ind - s2
            change_err = (ef_ind_err + es2 + UF * absf(change)) * UP
        if gs_ranked and keep:
            ranked = bubble_order(ranked, metric)
        if sor or esor:
            if sor:
                w, c = LD(gamma), C_MIX
            else:
                w, c = 1 - np.exp(-LD(gamma) * it), C_ESOR
            mu = w * new + (1 - w) * old
            err = (abs(float(w)) * new_err + abs(float(1 - w)) * old_err + c * UF * (absf(w * new) + absf((1 - w) * old))) * UP
        else:
            mu, err = new, new_err
        mus.append(mu.copy())

    def full(v, dtype):
        out = np.zeros((n, 3), dtype)
        out[view] = np.asarray(v).reshape(nv, 3)
        return out

    Eall = np.asarray(E, dtype=np.float64).astype(LD)
    mu_full, change_full = full(mu, LD), full(change, LD)
    terms = mu_full * Eall
    if palmo:
        terms = np.concatenate([terms, mu_full * change_full])
    out = dict(mu=mu_full, mu_err=full(err, np.float64), ef_induced=full(ef_ind, LD), ef_induced_err=full(ef_ind_err, np.float64),
               ef_induced_change=change_full, ef_induced_change_err=full(change_err, np.float64), polar_iterations=it,
               iter_success=success, rank_metric=metric, ranked_array=ranked.astype(np.int32),
               dipole_rrms=float(site_rrms.sum() / n), upol=LD(-0.5) * terms.sum(), upol_terms=LD(0.5) * np.abs(terms).sum(),
               mu_in=full(mu_in, LD), view=view)
    if history:
        out["mus"], out["sums"], out["E"] = mus, sums, Ev
    return out


def early_publish_energy(result):
    """U_pol(n) = -1/2 sum [mu_m.E - (mu_m - mu_{m-1}).s_{n-m}], m = ceil(n / 2), from the history of a plain Jacobi
    solve() (s_k = T mu_{k-1}): (U_pol, sum of |products| / 2) -- the formula the deferred path evaluates."""
    mus, sums, E = result["mus"], result["sums"], result["E"]
    n = result["polar_iterations"]
    m = (n + 1) // 2
    t1 = mus[m] * E
    t2 = (mus[m] - mus[m - 1]) * sums[n - m - 1] if n - m >= 1 else np.zeros_like(t1)
    return LD(-0.5) * (t1.sum() - t2.sum()), LD(0.5) * (np.abs(t1).sum() + np.abs(t2).sum())


def amatrix(tensor, system):
    """thole_amatrix() in the engine's layout: (3n x 3n longdouble A, fp64 bound dA).  1/alpha on the diagonal (one
    rounding: 1 ulp), MAXVALUE where alpha = 0; T between polarizable atoms.  Rows and columns of alpha = 0 atoms are not
    filled in here (the tests compare them with the oracle, not with this module)."""
    n, view = tensor.n, tensor.view
    idx = (3 * view[:, None] + np.arange(3)[None, :]).reshape(-1)
    A = np.zeros((3 * n, 3 * n), LD)
    dA = np.zeros((3 * n, 3 * n))
    A[np.ix_(idx, idx)] = tensor.T
    dA[np.ix_(idx, idx)] = tensor.dT
    alpha = np.repeat(np.asarray(system["alpha"], dtype=np.float64), 3)
    with np.errstate(divide="ignore"):
        diag = np.where(alpha != 0.0, 1 / alpha.astype(LD), LD(MAXVALUE))
    k = np.arange(3 * n)
    A[k, k] = diag
    dA[k, k] = np.where(alpha != 0.0, 2 * UF * np.abs(diag).astype(np.float64), 0.0)
    return A, dA


def explain(tensor, system, result, got, key="mu", top=3):
    """For the components of `got` ((n, 3), fp64) farthest outside result[key + '_err']: the site, its 64-block and lane
    in the view, and the partner whose single term T_ij mu_j -- removed, added, or scaled -- explains the error best."""
    t = tensor
    want, bound = result[key], result[key + "_err"]
    diff = (np.asarray(got).astype(LD) - want).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, np.abs(diff) / bound, np.where(diff != 0, np.inf, 0.0))
    ratio = np.where(np.isnan(diff), np.inf, ratio)
    slot = np.full(t.n, -1)
    slot[t.view] = np.arange(t.nv)
    mu_in = result["mu_in"][t.view].reshape(-1)
    lines = []
    for atom in np.argsort(-ratio.max(axis=1))[:top]:
        if lines and ratio[atom].max() <= 1.0:
            break
        p = int(np.argmax(ratio[atom]))
        k = slot[atom]
        head = "atom %d component %d: %s differs by %.3e, bound %.3e (ratio %.3g)" % (
            atom, p, key, diff[atom, p], bound[atom, p], ratio[atom, p])
        if k < 0:
            lines.append(head + "; not polarizable")
            continue
        head += "; view site %d = block %d lane %d" % (k, k // 64, k % 64)
        # what the pair (atom, j) adds to the sums of this site, in the units of `key`, and its c3 / c5 parts
        scale = -float(t.alpha[k]) if key == "mu" else (-1.0 if key == "ef_induced" else 1.0)
        muj = mu_in.reshape(t.nv, 3).astype(np.float64)
        term = (t.T[3 * k:3 * k + 3].reshape(3, t.nv, 3) * mu_in.reshape(1, t.nv, 3)).sum(-1).T.astype(np.float64) * scale
        term3 = t.c3[k][:, None] * muj * scale
        term[k] = term3[k] = 0.0
        parts = (("its term", term), ("the c3 part of its term", term3), ("the c5 part of its term", term - term3))
        size = max(float(np.abs(diff[atom]).max()), 1e-300)

        def fit(v):
            vv = float(v @ v)
            x = float(diff[atom] @ v) / vv if vv > 0.0 else 0.0
            return float(np.abs(diff[atom] - x * v).max()), x

        best = None
        for j in np.flatnonzero(np.abs(term).max(axis=1) > 0.0):
            for sgn, what in ((-1.0, "removing its term"), (1.0, "adding its term once more")):
                res = float(np.abs(diff[atom] - sgn * term[j]).max())
                if best is None or res < best[0]:
                    best = (res, j, what)
            for name, v in parts:
                res, x = fit(v[j])
                if abs(x) < 1e-3 and res < best[0]:
                    best = (res, j, "scaling %s by 1 %+.3e" % (name, x))
        if best is None:
            lines.append(head + "; no partner")
            continue
        for q in range(3):  # the same pair through a neighbouring image
            for sgn in (-1, 1):
                alt = t.d[k] - sgn * t.basis[q][None, :]
                v = ((_blocks64(alt, t.damp) - _blocks64(t.d[k], t.damp)) * muj[:, None, :]).sum(-1) * scale
                v[k] = 0.0
                res = np.abs(diff[atom][None, :] - v).max(axis=1)
                j = int(np.argmin(res))
                if res[j] < best[0]:
                    img = t.image[k, j].copy()
                    img[q] += sgn
                    best = (float(res[j]), j, "taking image (%d,%d,%d) instead, at %.15g," % (
                        *img, float(np.sqrt((alt[j] ** 2).sum()))))
        if best[0] > 0.05 * size:  # no single pair: a whole 64-site block of partners?
            for b0 in range(0, t.nv, 64):
                for name, v in parts:
                    res, x = fit(v[b0:b0 + 64].sum(axis=0))
                    if abs(x) < 1e-3 and res < best[0]:
                        j = b0 + int(np.argmax(np.abs(v[b0:b0 + 64]).max(axis=1)))
                        best = (res, j, "no single pair explains it; scaling %s for ALL partners of block %d by 1 %+.3e, "
                                "of which this pair's is the largest," % (name.replace("its term", "the term"), b0 // 64, x))
        res, j, what = best
        lines.append(head + "; pair (%d, %d) [partner view site %d = block %d lane %d], image (%d,%d,%d), rimg %.15g: %s "
                     "would leave %.3e (dT of the pair %.3e)" % (atom, t.view[j], j, j // 64, j % 64, *t.image[k, j],
                                                                 t.rimg[k, j], what, res, t.dT_pair[k, j]))
    return lines


def check(tensor, system, result, got, keys=("mu", "ef_induced"), what="", zero_outside=True, cap=None):
    """Componentwise |got - want| <= err on the view, exact 0 elsewhere (zero_outside = False for the oracle, which like
    the reference fills ef_induced_change on alpha = 0 sites too); returns {key: max(diff / bound)} and raises an
    AssertionError that names sites and pairs (explain()) otherwise.  A component that is not a number is outside any
    bound.  cap: {key: value} replaces the bound by min(err, value) where the running bound is known to be loose."""
    out = {}
    pol = np.zeros(tensor.n, bool)
    pol[tensor.view] = True
    if cap:
        result = dict(result)
        for key in keys:
            if key in cap:
                result[key + "_err"] = np.minimum(result[key + "_err"], cap[key])
    for key in keys:
        g = np.asarray(got[key], dtype=np.float64)
        assert not zero_outside or np.all(g[~pol] == 0.0), (what, key, "non-zero on a site without polarizability")
        diff = np.abs(g.astype(LD) - result[key]).astype(np.float64)[pol]
        bound = result[key + "_err"][pol]
        bad = ~(diff <= bound)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound > 0, diff / bound, 0.0)
        out[key] = float(r.max()) if r.size else 0.0
        if bad.any():
            raise AssertionError("%s %s: %d components outside the bound\n  %s" % (
                what, key, int(bad.sum()), "\n  ".join(explain(tensor, system, result, g, key))))
    return out


def check_energy(result, upol, what="", deferred=False, rel=1e-12):
    """|U_pol - U_ref| <= 1e-12 sum |terms|; returns the ratio to that allowance"""
    want, terms = early_publish_energy(result) if deferred else (result["upol"], result["upol_terms"])
    d, allow = abs(float(LD(upol) - want)), rel * float(terms)
    assert d <= allow, (what, "U_pol", upol, float(want), d, allow)
    return d / allow if allow else 0.0
