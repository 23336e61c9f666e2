"""numpy.longdouble reference of the dipole tensors beside the exponential one (polarization/thole_matrix.c:90-135):
`linear` (Thole's original model), `off` (undamped, with the es_excluded quirk of energy/pairs.c:61-77) and `exponential`
+ polar_wolf_full.  ModelTensor has the attributes of polar_reference.Tensor, so that solve / check / check_energy /
amatrix / explain of that module run on it as they are.  Helper module for the tests (a plain import, not a conftest).

    T = c3 I - 3 c5 d d^T,   c3 = damp1 / r^3,  c5 = damp2 / r^5                                  (linear, off)
    c3 = damp1 / r^3 - wdamp1 / rc^3,  c5 = damp2 / r^5 - wdamp2 / (r^2 rc^3)                     (wolf_full)

DECISIONS are made in fp64 as the reference makes them (polar_reference's rule): the lattice image, `rimg == 0`
(ir3 = ir5 = MAXVALUE), the exclusions of `off` (same molecule, or either charge == 0.0), and the branch `r < s` of
`linear` on the fp64 rimg and the fp64 s = polar_damp * pow(alpha_i alpha_j, 1.0 / 6.0) of this machine's libm.  VALUES are
longdouble; `linear` raises the EXACT product alpha_i alpha_j to the fp64 constant 1.0 / 6.0, as the reference's source
says.

THE BOUND dT, by the method of polar_reference (u = 2^-53, one count per rounded fp64 operation).  dd (displacement) and
dr (distance) are that module's.  1/r^3 and 1/r^5 times a damping factor are its C_C3 = 4 and C_C5 = 6 roundings.

* off.  damp is exactly 0 or 1:
      dc3 = C_C3 u |c3| + 3 |c3| dr / r,   dc5 = C_C5 u |c5| + 5 |c5| dr / r
* linear.  s: the product alpha_i alpha_j (1 rounding, which the sixth root divides by 6: counted as 1), pow to C_POW_ULP
  ulp = 2 C_POW_ULP u relative, the product with polar_damp (1): C_S = 2 + 2 C_POW_ULP.  No statement of the fp64 pow's
  error was found in the ROCm installation's documents or headers, so C_POW_ULP = 2 is ASSUMED (the largest error / bound
  ratio observed on the device is kept in profiles/thole_models/README.md).  v = r / s (1):
      dv = v (dr / r + (C_S + 1) u)
  damp1 = (4 - 3v) v v v: 3v and 4 - 3v err by at most 3u and 4u absolutely, (4 - 3v) >= 1, then three products:
  C_LIN1 = 7.  damp2 = v v v v: C_LIN2 = 3.  d damp1 / dv = 12 v^2 (1 - v), d damp2 / dv = 4 v^3:
      ddamp1 = C_LIN1 u damp1 + 12 v^2 |1 - v| dv + 6 dv^2,   ddamp2 = C_LIN2 u damp2 + 4 v^3 dv
  (6 dv^2: the second-order term that matters at v = 1, where the first derivative of damp1 vanishes.)
  THE BRANCH.  Both factors are continuous at r = s (damp1 = damp2 = 1), so an evaluation that decides r < s the other
  way -- another pow, by a rounding -- differs by what the damped formulas give within dv of v = 1.  Every pair with
  |v - 1| <= dv therefore carries the damped branch's ddamp1 / ddamp2 (with v taken as max(v, 1)) whichever side it is on.
  Pairs with v >= 1 + dv are undamped: damp = 1 exactly, as under `off`.
      dc3 = ddamp1 / r^3 + C_C3 u |c3| + 3 |c3| dr / r,   dc5 = ddamp2 / r^5 + C_C5 u |c5| + 5 |c5| dr / r
  (the dependence of damp on r is inside dv).
* wolf_full.  c3 = A3 - B3 and c5 = A5 - B5 with A the exponential model's parts (polar_reference's dc3 / dc5) and
  B3 = wdamp1 / rc^3, B5 = wdamp2 / (r^2 rc^3).  wdamp is the exponential damping at r = rc, formed once in fp64: its
  bound is that module's ddamp at r = rc, with rc exact.  rc^-3: two products and the division (3), the product with
  wdamp1 (1): C_W3 = 4.  B5 also takes 1/r (1), its square (1) and one more product: C_W5 = 7, and moves with r:
      dB3 = dwdamp1 / rc^3 + C_W3 u |B3|,   dB5 = dwdamp2 / (r^2 rc^3) + C_W5 u |B5| + 2 |B5| dr / r
  The difference rounds once, RELATIVE TO THE PARTS (near r = rc they cancel: the bound is on |A| + |B|, never on |A - B|):
      dc3 = dA3 + dB3 + u (|A3| + |B3|),   dc5 = dA5 + dB5 + u (|A5| + |B5|)
  and the assembly of T_pq rounds relative to the parts as well (the reference subtracts the two dyads entry by entry):
      dT_pq = delta_pq dc3 + 3 |d_p d_q| dc5 + 3 (|A5| + |B5|) (|d_p| dd_q + |d_q| dd_p)
              + (C_T + 1) u (3 (|A5| + |B5|) |d_p d_q| + delta_pq (|A3| + |B3|))
  The subtraction applies to EVERY pair, also beyond rc (the reference has no r < rc test; the A matrix has no cutoff).
  At rimg == 0 the dyad is 0 and damp1 MAXVALUE = 0: the block is -B3 I.
* linear / off assemble T_pq as polar_reference does: + 3 |c5| (|d_p| dd_q + |d_q| dd_p) + C_T u 3 |c5 d_p d_q| + u |T|~.

|T|~ = |c3| delta_pq + 3 |c5| |d_p d_q| of the STORED (combined) coefficients: the sweeps multiply those.
No tolerance here is fitted to any output of the engine.
"""
import numpy as np

import pair_reference as pr
import polar_reference as pref
from polar_reference import C_C3, C_C5, C_DAMP, C_R, C_T, C_TRANS, LD, MAXVALUE, U, UF, UP

C_POW_ULP = 2  # ASSUMED: no documented bound of the fp64 pow was found in the ROCm installation
C_S = 2 + 2 * C_POW_ULP
C_LIN1, C_LIN2 = 7, 3
C_W3, C_W5 = 4, 7
MODELS = ("exponential", "linear", "off")


def wolf_constants(damp, rc):
    """(wdamp1, wdamp2, dwdamp1, dwdamp2) in longdouble: thole_matrix.c:113-114 at r = rc and their fp64 bounds"""
    l, rc = LD(damp), LD(rc)
    lr = l * rc
    e = np.exp(-lr)
    E1 = e * (LD(0.5) * lr * lr + lr + 1)
    E2 = e * (lr ** 3 / 6)
    w1 = 1 - E1
    w2 = w1 - E2
    d1 = (C_DAMP + lr) * U * E1 + U * abs(w1)
    d2 = d1 + (C_DAMP + lr) * U * E2 + U * abs(w2)
    return w1, w2, d1, d2


class ModelTensor(pref.Tensor):
    """polar_reference.Tensor for damping in MODELS and, with `exponential`, wolf_full.  all_sites: the view is every atom
    (for amatrix() against download_amatrix(), which covers the alpha = 0 sites too: s = 0 there, no damping).
    cutoff: the box cutoff when it is not the one pbc() derives from the basis."""

    def __init__(self, system, damp, damping="exponential", wolf_full=False, chunk=64, all_sites=False, cutoff=None):
        assert damping in MODELS + ("none",)
        damping = "off" if damping == "none" else damping
        assert not wolf_full or damping == "exponential"
        pos = np.ascontiguousarray(system["pos"], dtype=np.float64)
        alpha_all = np.asarray(system["alpha"], dtype=np.float64)
        basis = np.asarray(system["basis"], dtype=np.float64)
        self.n = len(alpha_all)
        self.view = np.arange(self.n) if all_sites else np.flatnonzero(alpha_all != 0.0)
        self.alpha = alpha_all[self.view]
        nv = self.nv = len(self.view)
        vol, rb, rc = pr.pbc(basis)
        rc = float(rc if cutoff is None else cutoff)
        self.cutoff = rc
        self.damping, self.wolf_full = damping, bool(wolf_full)
        x = pos[self.view]
        xl = x.astype(LD)
        bl = basis.astype(LD)
        l = LD(damp)
        q = np.asarray(system["charge"], dtype=np.float64)[self.view]
        mol = np.asarray(system["molecule"])[self.view]
        self.T = np.zeros((3 * nv, 3 * nv), LD)
        self.Tabs = np.zeros((3 * nv, 3 * nv))
        self.dT = np.zeros((3 * nv, 3 * nv))
        self.rimg = np.zeros((nv, nv))
        self.r = np.zeros((nv, nv))
        self.image = np.zeros((nv, nv, 3), dtype=np.int64)
        self.dT_pair = np.zeros((nv, nv))
        self.c3 = np.zeros((nv, nv))
        self.c5 = np.zeros((nv, nv))
        self.d = np.zeros((nv, nv, 3))
        self.near_tie = np.zeros((nv, nv), bool)  # linear: pairs whose branch a rounding of s could decide either way
        self.damp, self.basis = float(damp), basis
        if wolf_full:
            w1, w2, dw1, dw2 = wolf_constants(damp, rc)
            rc3 = LD(rc) ** 3
        for i0 in range(0, nv, chunk):
            i1 = min(nv, i0 + chunk)
            d0 = x[i0:i1, None, :] - x[None, :, :]
            img, r, rimg, _ = pr.minimum_image(basis, rb, d0)
            self.rimg[i0:i1], self.r[i0:i1], self.image[i0:i1] = rimg, r, img
            trans = img.astype(LD) @ bl
            trans_abs = np.abs(img).astype(LD) @ np.abs(bl)
            dx = xl[i0:i1, None, :] - xl[None, :, :]
            d = dx - trans
            dd = U * np.abs(dx) + C_TRANS * U * trans_abs + U * np.abs(d)
            R = np.sqrt((d * d).sum(-1))
            zero = rimg == 0.0
            self_pair = np.arange(i0, i1)[:, None] == np.arange(nv)[None, :]
            Rs = np.where(zero, LD(1), R)
            dr = C_R * U * Rs + (dd * np.abs(d)).sum(-1) / Rs
            ir3, ir5 = 1 / Rs ** 3, 1 / Rs ** 5
            part3 = part5 = None  # wolf_full: |A| + |B|, what the roundings of the differences are relative to
            if damping == "off":
                excl = (mol[i0:i1, None] == mol[None, :]) | (q[i0:i1, None] == 0.0) | (q[None, :] == 0.0)
                damp12 = np.where(excl, LD(0), LD(1))
                c3, c5 = damp12 * ir3, damp12 * ir5
                dc3 = C_C3 * U * np.abs(c3) + 3 * np.abs(c3) / Rs * dr
                dc5 = C_C5 * U * np.abs(c5) + 5 * np.abs(c5) / Rs * dr
                c3 = np.where(zero, damp12 * LD(MAXVALUE), c3)  # thole_matrix.c:82-83: 1 * MAXVALUE on the diagonal of the block
                c5 = np.where(zero, LD(0), c5)  # (times a zero dyad)
            elif damping == "linear":
                aa64 = self.alpha[i0:i1, None] * self.alpha[None, :]
                s64 = float(damp) * np.power(aa64, 1.0 / 6.0)  # fp64, libm: the reference's decision
                damped = rimg < s64
                aa = self.alpha[i0:i1, None].astype(LD) * self.alpha[None, :].astype(LD)
                s = l * np.power(aa, LD(1.0 / 6.0))
                with np.errstate(divide="ignore", invalid="ignore"):
                    v = np.where(s > 0, Rs / np.where(s > 0, s, LD(1)), LD(np.inf))
                vf = np.where(np.isfinite(v.astype(np.float64)), v, LD(2))  # (s = 0: far from the branch point)
                dv = vf * (dr / Rs + (C_S + 1) * U)
                tie = np.abs(vf - 1) <= dv
                self.near_tie[i0:i1] = tie & ~zero & ~self_pair
                vb = np.where(tie, np.maximum(vf, LD(1)), vf)  # the damped branch's derivatives within dv of v = 1
                damp1 = np.where(damped, (4 - 3 * vf) * vf ** 3, LD(1))
                damp2 = np.where(damped, vf ** 4, LD(1))
                on = damped | tie
                dd1 = np.where(on, C_LIN1 * U * np.abs(damp1) + 12 * vb ** 2 * np.abs(1 - vb) * dv + 6 * dv * dv, LD(0))
                dd2 = np.where(on, C_LIN2 * U * np.abs(damp2) + 4 * vb ** 3 * dv, LD(0))
                c3, c5 = damp1 * ir3, damp2 * ir5
                dc3 = dd1 * ir3 + C_C3 * U * np.abs(c3) + 3 * np.abs(c3) / Rs * dr
                dc5 = dd2 * ir5 + C_C5 * U * np.abs(c5) + 5 * np.abs(c5) / Rs * dr
                # rimg == 0: v = 0 < s gives damp = 0 (times MAXVALUE); s = 0 (an alpha = 0 site) leaves 1 * MAXVALUE
                c3 = np.where(zero, np.where(damped, LD(0), LD(MAXVALUE)), c3)
                c5 = np.where(zero, LD(0), c5)
            else:
                lr = l * Rs
                e = np.exp(-lr)
                E1 = e * (LD(0.5) * lr * lr + lr + 1)
                E2 = e * (lr ** 3 / 6)
                damp1 = 1 - E1
                damp2 = damp1 - E2
                c3 = damp1 / Rs ** 3  # (the expressions of polar_reference.Tensor, so that the plain model is that module's to the bit)
                c5 = damp2 / Rs ** 5
                dd1 = (C_DAMP + lr) * U * E1 + U * np.abs(damp1)
                dd2 = dd1 + (C_DAMP + lr) * U * E2 + U * np.abs(damp2)
                dc3 = dd1 / Rs ** 3 + C_C3 * U * np.abs(c3) + (l * e * lr ** 2 / (2 * Rs ** 3) + 3 * np.abs(c3) / Rs) * dr
                dc5 = dd2 / Rs ** 5 + C_C5 * U * np.abs(c5) + (l * e * lr ** 3 / (6 * Rs ** 5) + 5 * np.abs(c5) / Rs) * dr
                c3, c5, dc3, dc5 = (np.where(zero, LD(0), a) for a in (c3, c5, dc3, dc5))  # damp(0) = 0, times MAXVALUE
                if wolf_full:
                    B3 = np.full(c3.shape, w1 / rc3)
                    B5 = np.where(zero, LD(0), w2 / (Rs * Rs * rc3))
                    dB3 = dw1 / rc3 + C_W3 * U * np.abs(B3)
                    dB5 = np.where(zero, LD(0), dw2 / (Rs * Rs * rc3) + C_W5 * U * np.abs(B5) + 2 * np.abs(B5) / Rs * dr)
                    part3, part5 = np.abs(c3) + np.abs(B3), np.abs(c5) + np.abs(B5)
                    dc3 = dc3 + dB3 + U * part3
                    dc5 = dc5 + dB5 + U * part5
                    c3, c5 = c3 - B3, c5 - B5
            ad = np.abs(d)
            dyad = d[..., :, None] * d[..., None, :]
            adyad = ad[..., :, None] * ad[..., None, :]
            T = -3 * c5[..., None, None] * dyad
            Tabs = 3 * np.abs(c5)[..., None, None] * adyad
            p5 = np.abs(c5) if part5 is None else part5
            p3 = np.abs(c3) if part3 is None else part3
            ct = C_T if part5 is None else C_T + 1
            Tparts = 3 * p5[..., None, None] * adyad
            dT = 3 * adyad * dc5[..., None, None] + ct * U * Tparts
            dT = dT + 3 * p5[..., None, None] * (ad[..., :, None] * dd[..., None, :] + dd[..., :, None] * ad[..., None, :])
            for p in range(3):
                T[..., p, p] += c3
                Tabs[..., p, p] += np.abs(c3)
                Tparts[..., p, p] += p3
                dT[..., p, p] += dc3
            dT = dT + U * Tparts
            keep = ~self_pair  # (a coincident pair of two sites keeps its block: -B3 I, MAXVALUE I or 0 by the model)
            T, Tabs, dT = (a * keep[..., None, None] for a in (T, Tabs, dT))
            m = i1 - i0
            self.T[3 * i0:3 * i1] = T.transpose(0, 2, 1, 3).reshape(3 * m, 3 * nv)
            self.Tabs[3 * i0:3 * i1] = (Tabs.transpose(0, 2, 1, 3).reshape(3 * m, 3 * nv)).astype(np.float64) * UP
            self.dT[3 * i0:3 * i1] = (dT.transpose(0, 2, 1, 3).reshape(3 * m, 3 * nv)).astype(np.float64) * UP
            self.dT_pair[i0:i1] = dT.max(axis=(-1, -2)).astype(np.float64)
            self.c3[i0:i1] = (c3 * keep).astype(np.float64)
            self.c5[i0:i1] = (c5 * keep).astype(np.float64)
            self.d[i0:i1] = d.astype(np.float64)
        off = ~np.eye(nv, dtype=bool)
        self.rmin = float(self.rimg[off].min()) if nv > 1 else MAXVALUE
        self.gamma = (3 * nv + 4) * UF / (1.0 - (3 * nv + 4) * UF)

    def without(self, atom):
        t = super().without(atom)
        t.__class__ = ModelTensor
        t.damping, t.wolf_full = self.damping, self.wolf_full
        k = int(np.flatnonzero(self.view == atom)[0])
        keep = np.arange(self.nv) != k
        t.c5, t.near_tie = self.c5[np.ix_(keep, keep)], self.near_tie[np.ix_(keep, keep)]
        return t


def two_site(r, alpha, damp, damping="exponential", wolf_full=False, L=40.0, charge=(1.0, -1.0), molecule=(0, 1)):
    """two equal sites r apart on the z axis in a cubic box of edge L: the system the closed forms are written for"""
    return dict(pos=np.array([[0.0, 0.0, 0.0], [0.0, 0.0, r]]), charge=np.array(charge, dtype=np.float64),
                alpha=np.array([alpha, alpha]), epsilon=np.zeros(2), sigma=np.zeros(2), mass=np.full(2, 4.0),
                molecule=np.array(molecule, dtype=np.int32), frozen=np.zeros(2, dtype=np.int32), basis=np.diag([L, L, L]))


def view_matrix(tensor):
    """the view's A (3nv x 3nv longdouble): T with 1 / alpha on the diagonal -- what the exact mode factors"""
    A = tensor.T.copy()
    k = np.arange(3 * tensor.nv)
    A[k, k] = 1 / np.repeat(tensor.alpha, 3).astype(LD)
    return A


def closed_forms(r, alpha, damp, damping="exponential", wolf_full=False, rc=None, excluded=False):
    """(T_xx, T_zz) = (c3, c3 - 3 r^2 c5) of two sites r apart on the z axis, longdouble, written out per model"""
    r, l = LD(r), LD(damp)
    if damping in ("off", "none"):
        f = LD(0) if excluded else LD(1)
        return f / r ** 3, -2 * f / r ** 3
    if damping == "linear":
        s = l * np.power(LD(alpha) * LD(alpha), LD(1.0 / 6.0))
        v = r / s
        d1, d2 = ((4 - 3 * v) * v ** 3, v ** 4) if float(r) < float(damp) * (alpha * alpha) ** (1.0 / 6.0) else (LD(1), LD(1))
        return d1 / r ** 3, (d1 - 3 * d2) / r ** 3

    def damps(x):
        e = np.exp(-l * x)
        d1 = 1 - e * ((l * x) ** 2 / 2 + l * x + 1)
        return d1, d1 - e * (l * x) ** 3 / 6

    d1, d2 = damps(r)
    txx, tzz = d1 / r ** 3, (d1 - 3 * d2) / r ** 3
    if wolf_full:
        w1, w2 = damps(LD(rc))
        txx -= w1 / LD(rc) ** 3
        tzz -= (w1 - 3 * w2) / LD(rc) ** 3
    return txx, tzz
