"""numpy.longdouble reference of the non-periodic dimer energies (the reference's surface_energy(), src/mc/surface.c:16-76):
geometry, the pair terms and the small Thole solve, with a DERIVED forward-error bound next to the dipoles and U_pol.
Helper module for the tests (a plain import, not a conftest); it shares nothing with oracle/ or the engine, and is written
from the reference's formulas: surface.c:116-125, :177-193, :383-433 (geometry), coulombic.c:198-217, lj.c:279-317,
disp_expansion.c:105-177, pairs.c:56-211, :337-359, thole_matrix.c:38-146, thole_field.c:39-68, thole_iterative.c, polar.c:107-116.

Two kinds of arithmetic, as in polar_reference.py:

* GEOMETRY and DECISIONS are fp64 in the reference's operation order, because they define the answer: the rotation matrices
  (math.cos / math.sin: the C library's, as the engine's host code calls them), the body frame, the placement (numpy fp64
  elementwise operations: one rounding each, no FMA), which pairs are in a sum, rank_metric and the stable descending
  order, and the stopping rule.  The site positions are therefore the SAME fp64 numbers on both sides of a comparison.
* VALUES are longdouble: displacements (exact from the fp64 positions), r, every pair term, c3 / c5, every recurrence.

THE BOUNDS.  u = 2^-53.
* es and rd: the project's standing bound for pair sums, 1e-12 * sum |terms| (the sums return it).
* static field, E_p = sum_j q_j d_p / r^3 over the n other-molecule sites: d_p (1), r from three squares, two additions and
  a root (C_R = 2), r r r (2 more roundings on 3 C_R), q d (1), the division (1): 11 roundings per term, and the n additions:
      dE_p = (11 + n) u sum_j |q_j d_p| / r^3
* c3, c5 and the tensor: polar_reference.py's counts without the lattice translation (dd_p = u |d_p|): C_R = 2, C_DAMP = 9,
  C_C3 = 4, C_C5 = 6, C_T = 4; the linear model's s = l (a_i a_j)^(1/6) by pow() to 2 ulp and v = r / s, (4 - 3v) v^3 and
  v^4: C_LIN = 12 relative roundings on either factor; the undamped model has damp exactly 0 or 1.
* one application g += c3 v - 3 c5 d (d.v) (kernels_dimer.h dimer_apply): the dot product (5), its products with c5, 3 and
  d_p (3), c3 v (1), the sum (1): C_APPLY = 10 roundings relative to |T|~ |v|, FMA contraction or not; a sum of N such terms
  adds N more.  With err the bound of the dipoles that enter, over the sites j != i:
      es_i = sum_j |T|~_ij err_j + dT_ij |mu_j| + (N + C_APPLY) u |T|~_ij |mu_j|
  A Gauss-Seidel sweep on the device is that pass over the OLD dipoles plus, for every site whose turn has come, the same
  application to delta_j = mu_j_new - mu_j_old (one more rounding, relative to |delta_j|); at site i's turn
      es_i = sum_j |T|~_ij err_j(current) + dT_ij |mu_j(current)| + (2 N + C_APPLY + 1) u |T|~_ij (|mu_j_old| + |delta_j|)
* a dipole: err_i = alpha_i (dE_i + es_i) + C_STEP u (|alpha_i E_i| + |alpha_i s_i|), C_STEP = 3; err_0 = alpha dE + C_INIT u
  |mu_0|, C_INIT = 2.
* U_pol = -1/2 sum mu.E (+ mu.change): dU = 1/2 sum_ip err |E| + |mu| dE + (N + 4) u |mu E|, and for the Palmo term
  err |change| + |mu| (es_used + es_now + u |change|) + (N + 4) u |mu change|.
A constant may be raised only with such a count written next to it.
"""
import math

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
MAXVALUE = 1.0e40
DEBYE2SKA = 85.10597636
MAX_ITERATION_COUNT = 128
C_R, C_DAMP, C_C3, C_C5, C_T, C_LIN = 2, 9, 4, 6, 4, 12
C_APPLY, C_STEP, C_INIT = 10, 3, 2
DISP_HK = 3.166811429 * 0.000001
DISP_REPULSION = LD("315.7750382111558307123944638")
CHUNK, MEAN_THREADS = 256, 256  # the grid form's fixed-order sum (kernels_dimer.h)


# ------------------------------------------------------------------------------------------------ geometry (fp64)
def euler_matrix(alpha, beta, gamma):
    """molecule_rotate_euler(), surface.c:116-125"""
    c, s = math.cos, math.sin
    return np.array([
        [c(gamma) * c(beta) * c(alpha) - s(gamma) * s(alpha), s(gamma) * c(beta) * c(alpha) + c(gamma) * s(alpha),
         -s(beta) * c(alpha)],
        [-c(gamma) * c(beta) * s(alpha) - s(gamma) * c(alpha), -s(gamma) * c(beta) * s(alpha) + c(gamma) * c(alpha),
         s(beta) * s(alpha)],
        [c(gamma) * s(beta), s(gamma) * s(beta), c(beta)]])


def quaternion_matrix(alpha, beta, gamma):
    """molecule_rotate_quaternion(), surface.c:177-193 with quaternion.c:45-83: the angles are divided by 57.2957795 and the
    third rotation is about x (both kept); R p = total p total*."""
    def axis(x, y, z, angle):
        angle /= 57.2957795
        sn = math.sin(angle / 2)
        return (x * sn, y * sn, z * sn, math.cos(angle / 2))

    def mul(a, b):
        ax, ay, az, aw = a
        bx, by, bz, bw = b
        return (aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz)

    t = (0.0, 0.0, 0.0, 1.0)
    t = mul(axis(0., 0., 1., alpha), t)
    t = mul(axis(0., 1., 0., beta), t)
    t = mul(axis(1., 0., 0., gamma), t)
    x, y, z, w = t
    xx, yy, zz, ww = x * x, y * y, z * z, w * w
    return np.array([[ww + xx - yy - zz, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
                     [2.0 * (x * y + w * z), ww - xx + yy - zz, 2.0 * (y * z - w * x)],
                     [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), ww - xx - yy + zz]])


def rotation(alpha, beta, gamma, global_axis=False):
    return quaternion_matrix(alpha, beta, gamma) if global_axis else euler_matrix(alpha, beta, gamma)


def body_frame(mol):
    """coordinates minus the mass-weighted centre, summed in site order (update_com(), pairs.c:364-385)"""
    pos = np.asarray(mol["pos"], dtype=np.float64).reshape(-1, 3)
    mass = np.asarray(mol["mass"], dtype=np.float64)
    tot, com = 0.0, np.zeros(3)
    for s in range(len(mass)):
        tot += mass[s]
        com = com + mass[s] * pos[s]
    com = com / tot
    return pos - com


def place(body, R, cx):
    """surface_dimer_geometry() on one molecule (surface.c:402-430): out to (cx, 0, 0), back to the centre, R times the
    vector left to right, out again; every step one fp64 rounding."""
    c = np.array([cx, 0.0, 0.0])
    p = (body + c) - c
    out = np.empty_like(p)
    for k in range(3):
        t = R[k, 0] * p[:, 0]
        t = t + R[k, 1] * p[:, 1]
        t = t + R[k, 2] * p[:, 2]
        out[:, k] = t
    return out + c


def sites(a, b, conf, global_axis=False):
    """fp64 positions [n1 + n2, 3] of the placement conf = (r, a1, b1, g1, a2, b2, g2)"""
    r = float(conf[0])
    p1 = place(body_frame(a), rotation(*[float(x) for x in conf[1:4]], global_axis=global_axis), 0.0)
    p2 = place(body_frame(b), rotation(*[float(x) for x in conf[4:7]], global_axis=global_axis), r)
    return np.vstack([p1, p2])


def loop_values(top, step):
    """the values `for (x = 0; x <= top; x += step)` visits, in double (surface.c:306-311)"""
    out, x = [], 0.0
    while x <= top:
        out.append(x)
        x += step
    return out


def scan_values(lo, hi, inc):
    """`for (r = surf_min; r <= surf_max; r += surf_inc)` (surface.c:289)"""
    out, r = [], float(lo)
    while r <= hi:
        out.append(r)
        r += inc
    return out


def angle_lists(surf_ang):
    a = loop_values(2.0 * math.pi, surf_ang)
    b = loop_values(math.pi, surf_ang)
    return [a, b, a, a, b, a]


# ------------------------------------------------------------------------------------------------ pair terms
def _col(mol, key, n):
    v = mol.get(key)
    return np.zeros(n) if v is None else np.asarray(v, dtype=np.float64)


def _merge(a, b):
    n1, n2 = len(a["charge"]), len(b["charge"])
    m = {k: np.concatenate([_col(a, k, n1), _col(b, k, n2)]) for k in ("charge", "alpha", "epsilon", "sigma", "c6", "c8", "c10")}
    m["n1"], m["n"] = n1, n1 + n2
    return m


def lj_mix(mixing, ei, si, ej, sj):
    """pairs.c:84-211 in fp64: (sigma_ij, eps_ij, attractive_only)"""
    if mixing == "waldmanhagler":
        si3, sj3 = si * si * si, sj * sj * sj
        si6, sj6 = si3 * si3, sj3 * sj3
        if si == 0 or sj == 0:
            return 0.0, math.sqrt(ei * ej), False
        return (0.5 * (si6 + sj6)) ** (1. / 6.), math.sqrt(ei * ej) * 2.0 * si3 * sj3 / (si6 + sj6), False
    if mixing == "halgren_mixing":
        sig = (si ** 3 + sj ** 3) / (si * si + sj * sj) if si > 0 and sj > 0 else 0.0
        eps = 4 * ei * ej / (math.sqrt(ei) + math.sqrt(ej)) ** 2 if ei > 0 and ej > 0 else 0.0
        return sig, eps, False
    if mixing == "c6_mixing":
        sig = 0.5 * (si + sj)
        eps = 64.0 * math.sqrt(ei * ej) * si ** 3 * sj ** 3 / (si + sj) ** 6 if sig != 0 else 0.0
        return sig, eps, False
    if si < 0 or sj < 0:
        return 0.5 * (abs(si) + abs(sj)), 0.0, True
    if si == 0 or sj == 0:
        return 0.0, math.sqrt(ei * ej), False
    return 0.5 * (si + sj), math.sqrt(ei * ej), False


def tt_damping(n, x):
    s, term = LD(0), LD(1)
    for k in range(n + 1):
        if k:
            term = term * x / k
        s += term
    f = 1 - np.exp(-x) * s
    return f if f > 0.000000001 else LD(0)


def pair_sums(m, pos, flags):
    """(es, sum |es terms|, rd, sum |rd terms|) in longdouble"""
    n1, n = m["n1"], m["n"]
    mixing = next((k for k in ("waldmanhagler", "halgren_mixing", "c6_mixing") if flags.get(k)), "lb")
    es = es_abs = rd = rd_abs = LD(0)
    P = pos.astype(LD)
    for i in range(n1):
        for j in range(n1, n):
            d = P[i] - P[j]
            r = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            qi, qj = m["charge"][i], m["charge"][j]
            if not flags.get("rd_only") and qi != 0.0 and qj != 0.0:
                t = LD(qi) * LD(qj) / r
                es += t
                es_abs += abs(t)
            ei, si, ej, sj = m["epsilon"][i], m["sigma"][i], m["epsilon"][j], m["sigma"][j]
            null_rd = ei == 0.0 or si == 0.0 or ej == 0.0 or sj == 0.0
            if flags.get("disp_expansion"):
                cs = [m[k][i] for k in ("c6", "c8", "c10")] + [m[k][j] for k in ("c6", "c8", "c10")]
                if null_rd and all(c == 0.0 for c in cs):
                    continue
                bi, bj, rhoi, rhoj = LD(ei), LD(ej), LD(si), LD(sj)
                rho = (rhoi + rhoj) / 2
                if flags.get("schmidt_mixing"):
                    bb = (bi + bj) * bi * bj / (bi * bi + bj * bj)
                else:
                    bb = 2 * bi * bj / (bi + bj)
                c6 = np.sqrt(LD(cs[0]) * LD(cs[3])) * LD(0.021958709) / LD(DISP_HK)
                c8 = np.sqrt(LD(cs[1]) * LD(cs[4])) * LD(0.0061490647) / LD(DISP_HK)
                if flags.get("extrapolate_disp_coeffs"):
                    c10 = LD(49) / 40 * c8 * c8 / c6 if c6 != 0 and c8 != 0 else LD(0)
                else:
                    c10 = np.sqrt(LD(cs[2]) * LD(cs[5])) * LD(0.0017219135) / LD(DISP_HK)
                rep = DISP_REPULSION * np.exp(-bb * (r - rho)) if bb != 0 and rho != 0 else LD(0)
                f6 = f8 = f10 = LD(1)
                if flags.get("damp_dispersion"):
                    f6, f8, f10 = (tt_damping(k, bb * r) for k in (6, 8, 10))
                terms = [-f6 * c6 / r ** 6, -f8 * c8 / r ** 8, -f10 * c10 / r ** 10, rep]
                rd += terms[0] + terms[1] + terms[2] + terms[3]
                rd_abs += sum(abs(t) for t in terms)
            else:
                if null_rd:
                    continue
                sig, eps, attractive = lj_mix(mixing, ei, si, ej, sj)
                sor6 = (abs(LD(sig)) / r) ** 6
                t12 = LD(0) if attractive else sor6 * sor6
                rd += 4 * LD(eps) * (t12 - sor6)
                rd_abs += 4 * abs(LD(eps)) * (t12 + sor6)
    return es, es_abs, rd, rd_abs


# ------------------------------------------------------------------------------------------------ the Thole system
def static_field(m, pos):
    """(E, dE): thole_field_nopbc(); the other molecule's charges, r != 0"""
    n1, n = m["n1"], m["n"]
    P = pos.astype(LD)
    E, A = np.zeros((n, 3), dtype=LD), np.zeros((n, 3), dtype=LD)
    for i in range(n):
        others = range(n1, n) if i < n1 else range(n1)
        for j in others:
            d = P[i] - P[j]
            r = np.sqrt(d @ d)
            if r != 0:
                t = LD(m["charge"][j]) * d / (r * r * r)
                E[i] += t
                A[i] += abs(t)
    nother = np.where(np.arange(n) < n1, n - n1, n1)[:, None]
    return E, ((11 + nother) * U * A).astype(np.float64) * (1 + 2.0 ** -48)


def tensors(m, pos, flags):
    """T [n, n, 3, 3] (zero diagonal blocks), |T|~ and dT (fp64, rounded up), r [n, n]"""
    n, n1 = m["n"], m["n1"]
    model = str(flags.get("polar_damp_type", "exponential")).lower()
    l = LD(flags.get("polar_damp", 0.0))
    P = pos.astype(LD)
    T = np.zeros((n, n, 3, 3), dtype=LD)
    Tabs, dT = np.zeros((n, n, 3, 3)), np.zeros((n, n, 3, 3))
    R = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            d = P[i] - P[j]
            r = np.sqrt(d @ d)
            R[i, j] = float(r)
            dd = U * abs(d)
            dr = C_R * U * r + np.sum(dd * abs(d)) / r
            if model == "exponential":
                lr = l * r
                ex = np.exp(-lr)
                E1 = ex * (lr * lr / 2 + lr + 1)
                E2 = ex * (lr * lr * lr / 6)
                damp1, damp2 = 1 - E1, 1 - E1 - E2
                ddamp1 = (C_DAMP + lr) * U * E1 + U * abs(damp1)
                ddamp2 = ddamp1 + (C_DAMP + lr) * U * E2 + U * abs(damp2)
                g3 = l * ex * lr ** 2 / (2 * r ** 3)
                g5 = l * ex * lr ** 3 / (6 * r ** 5)
            elif model == "linear":
                s = l * (LD(m["alpha"][i]) * LD(m["alpha"][j])) ** (LD(1) / 6)
                if s != 0 and float(r) < float(s):
                    v = r / s
                    damp1, damp2 = (4 - 3 * v) * v ** 3, v ** 4
                    g3, g5 = 12 * abs(1 - v) * v ** 2 / s / r ** 3, 4 * v ** 3 / s / r ** 5
                else:
                    damp1 = damp2 = LD(1)
                    g3 = g5 = LD(0)
                ddamp1, ddamp2 = C_LIN * U * abs(damp1), C_LIN * U * abs(damp2)  # (4 - 3v >= 1: no cancellation)
            else:  # off: es_excluded pairs do not couple (pairs.c:61-77)
                same = (i < n1) == (j < n1)
                excl = same or m["charge"][i] == 0.0 or m["charge"][j] == 0.0
                damp1 = damp2 = LD(0) if excl else LD(1)
                ddamp1 = ddamp2 = g3 = g5 = LD(0)
            c3, c5 = damp1 / r ** 3, damp2 / r ** 5
            dc3 = ddamp1 / r ** 3 + C_C3 * U * abs(c3) + (g3 + 3 * abs(c3) / r) * dr
            dc5 = ddamp2 / r ** 5 + C_C5 * U * abs(c5) + (g5 + 5 * abs(c5) / r) * dr
            for p in range(3):
                for q in range(3):
                    T[i, j, p, q] = -3 * d[p] * d[q] * c5 + (c3 if p == q else 0)
                    ta = 3 * abs(c5 * d[p] * d[q]) + (abs(c3) if p == q else 0)
                    Tabs[i, j, p, q] = float(ta) * (1 + 2.0 ** -48)
                    dT[i, j, p, q] = float((dc3 if p == q else 0) + 3 * abs(d[p] * d[q]) * dc5
                                           + 3 * abs(c5) * (abs(d[p]) * dd[q] + abs(d[q]) * dd[p])
                                           + C_T * U * 3 * abs(c5 * d[p] * d[q]) + U * ta) * (1 + 2.0 ** -48)
    return T, Tabs, dT, R


def rank_order(m, pos):
    """pairs.c:337-359 and update_ranking() in fp64: the stable descending order of rank_metric"""
    n = m["n"]
    pol = m["alpha"] != 0.0

    def dist(i, j):
        d = pos[i] - pos[j]
        return math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])

    rmin = MAXVALUE
    for i in range(n):
        for j in range(i + 1, n):
            if pol[i] and pol[j]:
                rmin = min(rmin, dist(i, j))
    metric = np.zeros(n)
    for i in range(n):
        for j in range(i + 1, n):
            if pol[i] and pol[j] and dist(i, j) <= rmin * 1.5:
                metric[i] += 1.0
                metric[j] += 1.0
    return sorted(range(n), key=lambda i: -metric[i]), metric


def solve(m, pos, flags):
    """The iterative solve and U_pol.  Returns dict(mu, mu_err [n, 3], polar, polar_err, iterations, not_converged, decisive):
    decisive = no stopping decision lay within the dipoles' bound of its threshold."""
    n = m["n"]
    alpha = m["alpha"].astype(LD)[:, None]
    a64 = m["alpha"][:, None]
    E, dE = static_field(m, pos)
    T, Tabs, dT, _ = tensors(m, pos, flags)
    gs = bool(flags.get("polar_gs") or flags.get("polar_gs_ranked"))
    precision = float(flags.get("polar_precision", 0.0))
    max_iter = int(flags.get("polar_max_iter", 10))
    gamma = LD(flags.get("polar_gamma", 1.0))
    allowed = precision * precision * DEBYE2SKA * DEBYE2SKA
    pol = m["alpha"] != 0.0
    order = list(range(n))
    ranked = rank_order(m, pos)[0] if flags.get("polar_gs_ranked") else None
    f64 = lambda v: np.abs(v).astype(np.float64) * (1 + 2.0 ** -48)

    def apply(i, mu):  # sum_j T_ij mu_j
        return np.einsum("jpq,jq->p", T[i], mu)

    def es_bound(i, err, mu_abs, roundings, mag_abs):
        return (np.einsum("jpq,jq->p", Tabs[i], err) + np.einsum("jpq,jq->p", dT[i], mu_abs)
                + roundings * U * np.einsum("jpq,jq->p", Tabs[i], mag_abs))

    mu = alpha * E * gamma
    err = a64 * dE + C_INIT * U * f64(mu)
    change, dchange = np.zeros((n, 3), dtype=LD), np.zeros((n, 3))
    it, keep, failed, decisive = 0, True, False, True
    while keep:
        it += 1
        if it >= MAX_ITERATION_COUNT and precision != 0.0:
            mu = alpha * E
            err = a64 * dE + U * f64(mu)
            change[:] = 0
            dchange[:] = 0
            failed = True
            break
        old, old_err = mu.copy(), err.copy()
        used, used_b = np.zeros((n, 3), dtype=LD), np.zeros((n, 3))
        if not gs:
            new, new_err = mu.copy(), err.copy()
            for i in range(n):
                s = apply(i, old)
                b = es_bound(i, old_err, f64(old), n + C_APPLY, f64(old))
                used[i], used_b[i] = s, b
                new[i] = alpha[i] * (E[i] - s)
                new_err[i] = a64[i] * (dE[i] + b) + C_STEP * U * (f64(alpha[i] * E[i]) + f64(alpha[i] * s))
            mu, err = new, new_err
        else:
            for i in order:
                if not pol[i]:
                    continue
                s = apply(i, mu)
                b = es_bound(i, err, f64(mu), 2 * n + C_APPLY + 1, f64(old) + f64(mu - old))
                used[i], used_b[i] = s, b
                mu[i] = alpha[i] * (E[i] - s)
                err[i] = a64[i] * (dE[i] + b) + C_STEP * U * (f64(alpha[i] * E[i]) + f64(alpha[i] * s))
        if precision == 0.0:
            keep = it != max_iter
        else:
            diff = (mu - old).astype(np.float64)
            keep = bool(np.any(diff * diff > allowed))
            slack = 2.0 * np.abs(diff) * (err + old_err) + (err + old_err) ** 2
            if np.any(np.abs(diff * diff - allowed) <= slack):
                decisive = False
        if flags.get("polar_palmo") and not keep and gs:
            for i in range(n):
                now = apply(i, mu)
                change[i] = used[i] - now
                nb = es_bound(i, err, f64(mu), 2 * n + C_APPLY + 1, f64(old) + f64(mu - old))
                dchange[i] = used_b[i] + nb + U * f64(change[i])
        if ranked is not None and keep:
            order = ranked
    upol = -(np.sum(mu * E) + (np.sum(mu * change) if flags.get("polar_palmo") else 0)) / 2
    dU = 0.5 * np.sum(err * f64(E) + f64(mu) * dE + (n + 4) * U * f64(mu * E))
    if flags.get("polar_palmo"):
        dU += 0.5 * np.sum(err * f64(change) + f64(mu) * dchange + (n + 4) * U * f64(mu * change))
    return dict(mu=mu, mu_err=err, polar=upol, polar_err=float(dU) * (1 + 2.0 ** -48), iterations=it, not_converged=failed,
                decisive=decisive, E=E)


def energies(a, b, conf, flags):
    """One placement: dict(es, es_abs, rd, rd_abs, polar, polar_err, mu, mu_err, iterations, not_converged, decisive)"""
    m = _merge(a, b)
    pos = sites(a, b, conf, bool(flags.get("surf_global_axis") or flags.get("global_axis")))
    es, es_abs, rd, rd_abs = pair_sums(m, pos, flags)
    out = dict(es=es, es_abs=es_abs, rd=rd, rd_abs=rd_abs, polar=LD(0), polar_err=0.0, iterations=0, not_converged=False,
               decisive=True, mu=np.zeros((m["n"], 3), dtype=LD), mu_err=np.zeros((m["n"], 3)), pos=pos)
    if not flags.get("rd_only") and np.any(m["alpha"] != 0.0):
        out.update(solve(m, pos, flags))
    return out


def fixed_order_mean(values):
    """The grid form's mean of fp64 values in placement order, in the order kernels_dimer.h states: chunk sums in ascending
    order, a strided sum of the chunks per thread, a halving tree over the threads, one division."""
    v = np.asarray(values, dtype=np.float64)
    nchunk = (len(v) + CHUNK - 1) // CHUNK
    b = np.zeros(nchunk)
    for c in range(nchunk):
        acc = 0.0
        for x in v[c * CHUNK:(c + 1) * CHUNK]:
            acc = acc + float(x)
        b[c] = acc
    d = np.zeros(MEAN_THREADS)
    for t in range(MEAN_THREADS):
        acc = 0.0
        for c in range(t, nchunk, MEAN_THREADS):
            acc = acc + b[c]
        d[t] = acc
    off = MEAN_THREADS // 2
    while off > 0:
        d[:off] = d[:off] + d[off:2 * off]
        off //= 2
    return d[0] / float(len(v))


# ------------------------------------------------------------------------------------------------ many placements at once
def _tables(mol, lists3, cx, global_axis):
    """fp64 sites [K, n, 3] of one molecule for the Cartesian product of three angle lists, the last fastest"""
    body = body_frame(mol)
    return np.array([place(body, rotation(x, y, z, global_axis=global_axis), cx)
                     for x in lists3[0] for y in lists3[1] for z in lists3[2]])


def _pair_tables(m, flags):
    """per inter-molecular pair (i on a, j on b): charge product, in-sum masks and mixed parameters (fp64 decisions)"""
    n1, n = m["n1"], m["n"]
    n2 = n - n1
    mixing = next((k for k in ("waldmanhagler", "halgren_mixing", "c6_mixing") if flags.get(k)), "lb")
    t = {k: np.zeros((n1, n2), dtype=LD) for k in ("qq", "sig", "eps", "bb", "rho", "c6", "c8", "c10", "rep")}
    t["es"], t["rd"], t["att"] = (np.zeros((n1, n2), dtype=bool) for _ in range(3))
    for i in range(n1):
        for jj in range(n2):
            j = n1 + jj
            qi, qj = m["charge"][i], m["charge"][j]
            t["es"][i, jj] = not flags.get("rd_only") and qi != 0.0 and qj != 0.0
            t["qq"][i, jj] = LD(qi) * LD(qj)
            ei, si, ej, sj = m["epsilon"][i], m["sigma"][i], m["epsilon"][j], m["sigma"][j]
            null_rd = ei == 0.0 or si == 0.0 or ej == 0.0 or sj == 0.0
            if flags.get("disp_expansion"):
                cs = [m[k][i] for k in ("c6", "c8", "c10")] + [m[k][j] for k in ("c6", "c8", "c10")]
                if null_rd and all(c == 0.0 for c in cs):
                    continue
                t["rd"][i, jj] = True
                bi, bj = LD(ei), LD(ej)
                with np.errstate(invalid="ignore", divide="ignore"):
                    bb = (bi + bj) * bi * bj / (bi * bi + bj * bj) if flags.get("schmidt_mixing") else 2 * bi * bj / (bi + bj)
                t["bb"][i, jj], t["rho"][i, jj] = bb, (LD(si) + LD(sj)) / 2
                c6 = np.sqrt(LD(cs[0]) * LD(cs[3])) * LD(0.021958709) / LD(DISP_HK)
                c8 = np.sqrt(LD(cs[1]) * LD(cs[4])) * LD(0.0061490647) / LD(DISP_HK)
                if flags.get("extrapolate_disp_coeffs"):
                    c10 = LD(49) / 40 * c8 * c8 / c6 if c6 != 0 and c8 != 0 else LD(0)
                else:
                    c10 = np.sqrt(LD(cs[2]) * LD(cs[5])) * LD(0.0017219135) / LD(DISP_HK)
                t["c6"][i, jj], t["c8"][i, jj], t["c10"][i, jj] = c6, c8, c10
                t["rep"][i, jj] = 1 if (bb != 0 and t["rho"][i, jj] != 0) else 0
            elif not null_rd:
                sig, eps, att = lj_mix(mixing, ei, si, ej, sj)
                t["rd"][i, jj], t["sig"][i, jj], t["eps"][i, jj], t["att"][i, jj] = True, abs(sig), eps, att
    return t


def _tt(n, x):
    s, term = np.ones_like(x), np.ones_like(x)
    for k in range(1, n + 1):
        term = term * x / k
        s = s + term
    f = 1 - np.exp(-x) * s
    return np.where(f > 0.000000001, f, 0)


def _solve_many(m, pos, flags):
    """U_pol [P] (longdouble) and whether any placement gave up, for fp64 sites pos [P, n, 3]: solve() without the bounds"""
    P = pos.shape[0]
    view = np.flatnonzero(m["alpha"] != 0.0)  # (sites without polarizability carry no dipole: thole_iterative.c:34-39)
    first = np.arange(m["n"]) < m["n1"]
    X = pos.astype(LD)
    # static field on the view's sites from ALL sites of the other molecule
    dq = X[:, view][:, :, None, :] - X[:, None, :, :]
    rq = np.sqrt(np.sum(dq * dq, axis=-1))
    other = (first[view][:, None] != first[None, :])[None]
    with np.errstate(divide="ignore", invalid="ignore"):
        E = np.sum(np.where((other & (rq != 0))[..., None], m["charge"].astype(LD)[None, None, :, None] * dq / (rq ** 3)[..., None], 0), axis=2)
    m = dict(m, charge=m["charge"][view], alpha=m["alpha"][view])
    pos, X = pos[:, view], X[:, view]
    n = len(view)
    d = X[:, :, None, :] - X[:, None, :, :]
    r = np.sqrt(np.sum(d * d, axis=-1))
    eye = np.eye(n, dtype=bool)
    rs = np.where(eye, LD(1), r)
    model = str(flags.get("polar_damp_type", "exponential")).lower()
    l = LD(flags.get("polar_damp", 0.0))
    if model == "exponential":
        lr = l * rs
        ex = np.exp(-lr)
        damp1 = 1 - ex * (lr * lr / 2 + lr + 1)
        damp2 = damp1 - ex * (lr * lr * lr / 6)
    elif model == "linear":
        aa = m["alpha"].astype(LD)
        s = l * (aa[:, None] * aa[None, :]) ** (LD(1) / 6)
        with np.errstate(divide="ignore", invalid="ignore"):
            v = rs / s[None]
        inside = rs.astype(np.float64) < s.astype(np.float64)[None]
        damp1 = np.where(inside, (4 - 3 * v) * v ** 3, 1)
        damp2 = np.where(inside, v ** 4, 1)
    else:
        same = first[view][:, None] == first[view][None, :]
        q0 = m["charge"] == 0.0
        excl = same | q0[:, None] | q0[None, :]
        damp1 = damp2 = np.broadcast_to(np.where(excl, LD(0), LD(1))[None], rs.shape)
    c3 = np.where(eye, 0, damp1 / rs ** 3)
    c5 = np.where(eye, 0, damp2 / rs ** 5)
    T = -3 * c5[..., None, None] * d[..., :, None] * d[..., None, :] + c3[..., None, None] * np.eye(3, dtype=LD)
    alpha = m["alpha"].astype(LD)[None, :, None]
    pol = m["alpha"] != 0.0
    gs = bool(flags.get("polar_gs") or flags.get("polar_gs_ranked"))
    precision, max_iter = float(flags.get("polar_precision", 0.0)), int(flags.get("polar_max_iter", 10))
    allowed = precision * precision * DEBYE2SKA * DEBYE2SKA
    order = np.tile(np.arange(n), (P, 1))
    if flags.get("polar_gs_ranked"):
        r64 = np.sqrt(np.sum((pos[:, :, None, :] - pos[:, None, :, :]) ** 2 * 1.0, axis=-1))  # (fp64: x^2 + y^2 + z^2 in order)
        pp = (pol[:, None] & pol[None, :] & ~eye)[None]
        rmin = np.min(np.where(pp, r64, MAXVALUE), axis=(1, 2))
        metric = np.sum(pp & (r64 <= rmin[:, None, None] * 1.5), axis=2).astype(np.float64)
        ranked = np.argsort(-metric, axis=1, kind="stable")
    mu = alpha * E * LD(flags.get("polar_gamma", 1.0))
    change = np.zeros_like(mu)
    active = np.ones(P, dtype=bool)
    failed = np.zeros(P, dtype=bool)
    rows = np.arange(P)
    it = 0
    while np.any(active):
        it += 1
        if it >= MAX_ITERATION_COUNT and precision != 0.0:
            mu[active] = (alpha * E)[active]
            change[active] = 0
            failed |= active
            break
        old = mu.copy()
        used = np.zeros_like(mu)
        if not gs:
            s = np.einsum("xijpq,xjq->xip", T, old)
            used = s
            new = alpha * (E - s)
            mu = np.where(active[:, None, None], new, mu)
        else:
            for t in range(n):
                k = order[:, t]
                s = np.einsum("xjpq,xjq->xp", T[rows, k], mu)
                new = alpha[0, k] * (E[rows, k] - s)
                upd = active & pol[k]
                used[rows[upd], k[upd]] = s[upd]
                mu[rows[upd], k[upd]] = new[upd]
        if precision == 0.0:
            done = np.full(P, it == max_iter)
        else:
            diff = (mu - old).astype(np.float64)
            done = ~np.any(diff * diff > allowed, axis=(1, 2))
        finishing = active & done
        if flags.get("polar_palmo") and gs and np.any(finishing):
            now = np.einsum("xijpq,xjq->xip", T[finishing], mu[finishing])
            change[finishing] = used[finishing] - now
        active = active & ~done
        if flags.get("polar_gs_ranked"):
            order = ranked
    u = np.sum(mu * E, axis=(1, 2))
    if flags.get("polar_palmo"):
        u = u + np.sum(mu * change, axis=(1, 2))
    return -u / 2, failed


def grid_energies(a, b, r, lists, flags, chunk=2048):
    """(es, rd, polar) [K1 K2] longdouble of the grid form's placements, in its order (the second molecule's index fastest)"""
    m = _merge(a, b)
    ga = bool(flags.get("surf_global_axis") or flags.get("global_axis"))
    t1, t2 = _tables(a, lists[:3], 0.0, ga), _tables(b, lists[3:], float(r), ga)
    K1, K2, n1 = len(t1), len(t2), m["n1"]
    pt = _pair_tables(m, flags)
    polar = not flags.get("rd_only") and np.any(m["alpha"] != 0.0)
    out = [np.zeros(K1 * K2, dtype=LD) for _ in range(3)]
    step = max(1, chunk // K2)
    for k0 in range(0, K1, step):
        p1 = t1[k0:k0 + step]
        pos = np.concatenate([np.repeat(p1, K2, axis=0), np.tile(t2, (len(p1), 1, 1))], axis=1)  # [P, n, 3]
        X = pos.astype(LD)
        d = X[:, :n1, None, :] - X[:, None, n1:, :]
        rr = np.sqrt(np.sum(d * d, axis=-1))
        sl = slice(k0 * K2, k0 * K2 + len(pos))
        out[0][sl] = np.sum(np.where(pt["es"][None], pt["qq"][None] / rr, 0), axis=(1, 2))
        if flags.get("disp_expansion"):
            f6 = f8 = f10 = 1
            if flags.get("damp_dispersion"):
                f6, f8, f10 = (_tt(k, pt["bb"][None] * rr) for k in (6, 8, 10))
            rep = pt["rep"][None] * DISP_REPULSION * np.exp(-pt["bb"][None] * (rr - pt["rho"][None]))
            term = -f6 * pt["c6"][None] / rr ** 6 - f8 * pt["c8"][None] / rr ** 8 - f10 * pt["c10"][None] / rr ** 10 + rep
        else:
            s6 = (pt["sig"][None] / rr) ** 6
            term = 4 * pt["eps"][None] * (np.where(pt["att"][None], 0, s6 * s6) - s6)
        out[1][sl] = np.sum(np.where(pt["rd"][None], term, 0), axis=(1, 2))
        if polar:
            out[2][sl] = _solve_many(m, pos, flags)[0]
    return out
