"""Brute-force reference of the coupled-dipole many-body van der Waals mode (polarvdw): what the kernels of
mpmc_amd/csrc/kernels_vdw.h sum.  Helper module for the tests (a plain import, not a conftest), written from the
reference's formulas (energy/vdw.c:101-131, :209-385, :579-632, polarization/thole_matrix.c:61-141, energy/lj.c:56-107,
:189-250, energy/energy.c:48-64) and independent of oracle/, which has no such term.

* DECISIONS are made in fp64 in the reference's operation order: the minimum image (pair_reference.minimum_image), which
  atoms enter the matrix (sqrt(alpha) * omega != 0), the Lennard-Jones cutoff rimg - 1e-12 < cutoff, the close-contact
  test rimg < scale.
* VALUES are evaluated in numpy.longdouble from the fp64 inputs and summed in longdouble.  The eigenvalues of C come from
  a cyclic Jacobi iteration in longdouble (round-robin ordering: the n / 2 disjoint rotations of a round are applied at
  once), which needs no library eigensolver and converges to the longdouble rounding level.
"""
import numpy as np

from pair_reference import LD, PI, SMALL_dR, _molecule_index, minimum_image, pbc

AU2INVSEC = LD("4.13412763705e16")  # vdw.c:22
HALF_HBAR = LD("3.81911146e-12")    # vdw.c:21
C_HBAR = LD("7.63822291e-12")       # vdw.c:20
CONV = AU2INVSEC * HALF_HBAR


def site_k(system):
    """k_i = sqrt(alpha_i) * omega_i in fp64 (getsqrtKinv, vdw.c:337); the matrix holds the atoms with k_i != 0"""
    return np.sqrt(np.asarray(system["alpha"], dtype=np.float64)) * np.asarray(system["omega"], dtype=np.float64)


def c_matrix(system, flags, atoms=None):
    """C = K A K (longdouble) over `atoms` (default: all) with k != 0, and the atom index of every site.  A: diagonal blocks
    1 / alpha, off-diagonal blocks delta_pq damp1 / r^3 - 3 x_p x_q damp2 / r^5 at the minimum image (exponential damping,
    l = polar_damp), no cutoff, every pair."""
    pos = np.asarray(system["pos"], dtype=np.float64)
    alpha = np.asarray(system["alpha"], dtype=np.float64)
    k = site_k(system)
    idx = np.arange(len(pos)) if atoms is None else np.asarray(atoms)
    idx = idx[k[idx] != 0.0]
    na = len(idx)
    Cm = np.zeros((3 * na, 3 * na), LD)
    if na == 0:
        return Cm, idx
    _, rb, _ = pbc(system["basis"], flags.get("pbc_cutoff", 0.0))
    kl = k[idx].astype(LD)
    for a in range(na):
        Cm[3 * a:3 * a + 3, 3 * a:3 * a + 3] = np.eye(3, dtype=LD) * (kl[a] * kl[a] / LD(alpha[idx[a]]))
    if na > 1:
        ia, ib = np.triu_indices(na, 1)
        d = pos[idx[ia]] - pos[idx[ib]]
        _, _, rimg, dimg = minimum_image(system["basis"], rb, d)
        r = rimg.astype(LD)
        x = dimg.astype(LD)
        l = LD(float(flags["polar_damp"]))
        ex = np.exp(-l * r)
        damp1 = 1 - ex * (l * l * r * r / 2 + l * r + 1)
        damp2 = damp1 - ex * (l ** 3 * r ** 3 / 6)
        c3 = damp1 / r ** 3
        c5 = damp2 / r ** 5
        kk = kl[ia] * kl[ib]
        for p in range(3):
            for q in range(3):
                t = (-3 * x[:, p] * x[:, q] * c5 + (c3 if p == q else 0)) * kk
                Cm[3 * ia + p, 3 * ib + q] = t
                Cm[3 * ib + q, 3 * ia + p] = t
    return Cm, idx


def _rounds(m):
    """round-robin schedule of m (even) players: m - 1 rounds of m / 2 disjoint pairs covering every pair once"""
    ring = list(range(m))
    out = []
    for _ in range(m - 1):
        p = np.array([ring[i] for i in range(m // 2)])
        q = np.array([ring[m - 1 - i] for i in range(m // 2)])
        out.append((np.minimum(p, q), np.maximum(p, q)))
        ring = [ring[0]] + [ring[-1]] + ring[1:-1]
    return out


def jacobi_eigenvalues(A, max_sweeps=40):
    """Eigenvalues (ascending, longdouble) of the symmetric matrix A by cyclic Jacobi rotations in longdouble."""
    A = np.array(A, dtype=LD)
    n = A.shape[0]
    if n == 0:
        return np.zeros(0, LD)
    if n == 1:
        return A[0].copy()
    if n > 8:
        # Start from the basis LAPACK finds in fp64, made orthogonal to the longdouble level by one Newton-Schulz step
        # (V <- V (3 - V^T V) / 2 squares the 1e-16 defect): B = V^T A V has the eigenvalues of A and an off-diagonal part of
        # 1e-16 of it, which the rotations below remove in a sweep or two instead of ten.  The eigenvalues are still those
        # the longdouble iteration converges to; fp64 only chose where it starts.
        V = np.linalg.eigh(A.astype(np.float64))[1].astype(LD)
        V = V @ (3 * np.eye(n, dtype=LD) - V.T @ V) / 2
        A = V.T @ A @ V
        A = (A + A.T) / 2
    m = n + (n & 1)  # an odd dimension gets an idle player
    sched = [(p[(q < n)], q[(q < n)]) for p, q in _rounds(m)]
    eps = np.finfo(LD).eps
    scale = np.sqrt((A * A).sum(dtype=LD))
    prev = np.inf
    for _ in range(max_sweeps):
        B = A.copy()
        np.fill_diagonal(B, 0)
        off = np.sqrt((B * B).sum(dtype=LD))
        # converged: the off-diagonal part is rounding noise (an eigenvalue moves by at most off), or it has stopped
        # shrinking below 1e-17 of the matrix -- quadratic convergence ends where the rotations' own rounding begins
        if off <= eps * scale or (off <= 1e-17 * scale and off >= 0.25 * prev):
            break
        prev = off
        for p, q in sched:
            apq = A[p, q]
            live = apq != 0
            if not live.any():
                continue
            p, q, apq = p[live], q[live], apq[live]
            theta = (A[q, q] - A[p, p]) / (2 * apq)
            t = np.where(theta >= 0, LD(1), LD(-1)) / (np.abs(theta) + np.sqrt(theta * theta + 1))
            c = 1 / np.sqrt(t * t + 1)
            s = t * c
            rp, rq = A[p, :].copy(), A[q, :].copy()
            A[p, :] = c[:, None] * rp - s[:, None] * rq
            A[q, :] = s[:, None] * rp + c[:, None] * rq
            cp, cq = A[:, p].copy(), A[:, q].copy()
            A[:, p] = cp * c[None, :] - cq * s[None, :]
            A[:, q] = cp * s[None, :] + cq * c[None, :]
    else:
        raise RuntimeError("Jacobi iteration did not converge")
    return np.sort(np.diag(A))


def eigen_energy(lam):
    """eigen2energy (vdw.c:209-221) times au2invsec * halfHBAR: negative eigenvalues are clipped to 0"""
    return CONV * np.sqrt(np.where(lam < 0, LD(0), lam)).sum(dtype=LD)


def prerotated_eigen_energy(C):
    """eigen_energy of the symmetric positive definite matrix C with a certified error, at sizes where the Jacobi iteration
    takes minutes: (e, err, info).

    V is the fp64 basis of numpy.linalg.eigh after the Newton-Schulz step of jacobi_eigenvalues, B = V^T C V in
    longdouble, e = CONV * sum sqrt(max(b_ii, 0)).  No rotation follows; instead the off-diagonal part that is left is
    turned into a bound.  With off_B = ||B - diag(B)||_F, Hoffman-Wielandt gives sum_i (mu_i - b_(i))^2 <= off_B^2 for the
    sorted eigenvalues mu of B and the sorted diagonal, so every mu_i >= b_min - off_B and
        sum_i |sqrt(mu_i) - sqrt(b_(i))| <= sum_i |mu_i - b_(i)| / (2 sqrt(b_min - off_B))
                                          <= sqrt(n) off_B / (2 sqrt(b_min - off_B)).
    Two things stand between B as computed and the spectrum of C, and both are charged:
      * V is orthogonal only to defect = ||V^T V - 1||_F.  By Ostrowski's theorem mu_i = theta_i lambda_i(C) with
        |theta_i - 1| <= defect: a relative error of defect / 2 in every square root, charged as defect * e.
      * the two longdouble products round: |fl(V^T C V) - V^T C V|_F <= 2 n eps ||C||_F (1 + O(n eps)) (||V||_2 = 1 up to
        the defect; eps = the longdouble epsilon).  This is added to off_B: off = off_B + 2 n eps ||C||_F.
    err = CONV * sqrt(n) off / (2 sqrt(b_min - off)) + defect * e.  Raises when b_min - off <= 0: the function serves the
    well-conditioned cases only.  info: b_min, b_max, off, defect, norm (= ||C||_F)."""
    C = np.array(C, dtype=LD)
    n = C.shape[0]
    assert n > 0 and C.shape == (n, n)
    eye = np.eye(n, dtype=LD)
    V = np.linalg.eigh(C.astype(np.float64))[1].astype(LD)
    V = V @ (3 * eye - V.T @ V) / 2
    G = V.T @ V - eye
    defect = np.sqrt((G * G).sum(dtype=LD))
    B = V.T @ C @ V
    B = (B + B.T) / 2
    b = np.diag(B).copy()
    np.fill_diagonal(B, 0)
    norm = np.sqrt((C * C).sum(dtype=LD))
    off = np.sqrt((B * B).sum(dtype=LD)) + 2 * n * np.finfo(LD).eps * norm
    b_min, b_max = b.min(), b.max()
    if not b_min - off > 0:
        raise ValueError("prerotated_eigen_energy: b_min - off = %g <= 0, not a well-conditioned case" % float(b_min - off))
    e = CONV * np.sqrt(b).sum(dtype=LD)
    err = CONV * np.sqrt(LD(n)) * off / (2 * np.sqrt(b_min - off)) + defect * e
    return e, err, dict(b_min=b_min, b_max=b_max, off=off, defect=defect, norm=norm)


def molecules(system):
    """[(type id, atom indices)] in upload order"""
    mol = _molecule_index(system["molecule"])
    mtype = np.asarray(system["mol_type"])
    return [(int(mtype[np.flatnonzero(mol == m)[0]]), np.flatnonzero(mol == m)) for m in range(mol.max() + 1)]


def e_iso(system, flags, cache=None):
    """sum_eiso_vdw (vdw.c:262-320): per molecule, in order, the value of its type -- computed from the first molecule of the
    type seen, and kept in `cache` (type id -> longdouble) when one is passed"""
    cache = {} if cache is None else cache
    total = LD(0)
    for t, atoms in molecules(system):
        if t not in cache:
            Cm, _ = c_matrix(system, flags, atoms)
            cache[t] = eigen_energy(jacobi_eigenvalues(Cm))
        total += cache[t]
    return total


def lr_corr(system, flags):
    """lr_vdw_corr (vdw.c:346-385): (sum, sum |terms|)"""
    if not flags.get("rd_lrc", 1):
        return LD(0), LD(0)
    alpha = np.asarray(system["alpha"], dtype=np.float64)
    w = np.asarray(system["omega"], dtype=np.float64)
    frz = np.asarray(system["frozen"]).astype(bool)
    vol, _, rc = pbc(system["basis"], flags.get("pbc_cutoff", 0.0))
    i, j = np.triu_indices(len(alpha), 1)
    keep = ~(frz[i] & frz[j]) & (alpha[i] != 0) & (alpha[j] != 0) & (w[i] != 0) & (w[j] != 0)
    i, j = i[keep], j[keep]
    w1, w2, a1, a2 = w[i].astype(LD), w[j].astype(LD), alpha[i].astype(LD), alpha[j].astype(LD)
    cC = LD(1.5) * C_HBAR * w1 * w2 / (w1 + w2) * AU2INVSEC * a1 * a2
    t = -LD(4) / 3 * PI * cC / LD(rc) ** 3 / LD(vol)
    return t.sum(dtype=LD), np.abs(t).sum(dtype=LD)


def _mix(eps, sig, i, j):
    """pairs.c:200-211: (longdouble epsilon_ij, fp64 sigma_ij); epsilon_ij of an attractive-only pair is never set: 0"""
    neg = (sig[i] < 0) | (sig[j] < 0)
    zero = (sig[i] == 0) | (sig[j] == 0)
    s = np.where(neg, 0.5 * (np.abs(sig[i]) + np.abs(sig[j])), np.where(zero, 0.0, 0.5 * (sig[i] + sig[j])))
    e = np.where(neg, LD(0), np.sqrt(eps[i].astype(LD) * eps[j].astype(LD)))
    return e, s


def repulsion(system, flags):
    """Lennard-Jones under polarvdw (lj.c:189-250 with term6 = 0): different molecules, not frozen-frozen, no zero
    parameter, rimg - 1e-12 < cutoff: 4 eps_ij (sigma_ij / rimg)^12.  Returns (sum, sum |terms|, the smallest
    |rimg - 1e-12 - cutoff| over the candidate pairs)."""
    pos = np.asarray(system["pos"], dtype=np.float64)
    eps = np.asarray(system["epsilon"], dtype=np.float64)
    sig = np.asarray(system["sigma"], dtype=np.float64)
    mol = _molecule_index(system["molecule"])
    frz = np.asarray(system["frozen"]).astype(bool)
    _, rb, rc = pbc(system["basis"], flags.get("pbc_cutoff", 0.0))
    i, j = np.triu_indices(len(pos), 1)
    keep = ~(frz[i] & frz[j]) & (mol[i] != mol[j]) & (eps[i] != 0) & (eps[j] != 0) & (sig[i] != 0) & (sig[j] != 0)
    i, j = i[keep], j[keep]
    if not i.size:
        return LD(0), LD(0), np.inf
    _, _, rimg, _ = minimum_image(system["basis"], rb, pos[i] - pos[j])
    margin = float(np.abs((rimg - SMALL_dR) - rc).min())
    inside = rimg - SMALL_dR < rc
    i, j, rimg = i[inside], j[inside], rimg[inside]
    e, s = _mix(eps, sig, i, j)
    t = 4 * e * (np.abs(s).astype(LD) / rimg.astype(LD)) ** 12
    return t.sum(dtype=LD), np.abs(t).sum(dtype=LD), margin


def repulsion_lrc(system, flags):
    """lj_lrc_corr + lj_lrc_self under polarvdw (lj.c:77-78, :100-101): (sum, sum |terms|)"""
    if not flags.get("rd_lrc", 1):
        return LD(0), LD(0)
    eps = np.asarray(system["epsilon"], dtype=np.float64)
    sig = np.asarray(system["sigma"], dtype=np.float64)
    frz = np.asarray(system["frozen"]).astype(bool)
    vol, _, rc = pbc(system["basis"], flags.get("pbc_cutoff", 0.0))

    def term(e, s):
        return LD(16) / 9 * PI * e * s ** 3 * (s / LD(rc)) ** 9 / LD(vol)

    i, j = np.triu_indices(len(eps), 1)
    e, s = _mix(eps, sig, i, j)
    k = (e != 0) & (s != 0) & ~(frz[i] & frz[j])
    t1 = term(e[k], np.abs(s[k]).astype(LD))
    k = (sig != 0) & (eps != 0) & ~frz
    t2 = term(eps[k].astype(LD), np.abs(sig[k]).astype(LD))
    return t1.sum(dtype=LD) + t2.sum(dtype=LD), np.abs(t1).sum(dtype=LD) + np.abs(t2).sum(dtype=LD)


def close_contacts(system, flags, scale):
    """cavity_absolute_check (energy.c:48-64) as a count: pairs on different molecules (frozen-frozen ones included) with
    rimg < scale.  Returns (count, the smallest |rimg - scale| over those pairs)."""
    pos = np.asarray(system["pos"], dtype=np.float64)
    mol = _molecule_index(system["molecule"])
    _, rb, _ = pbc(system["basis"], flags.get("pbc_cutoff", 0.0))
    i, j = np.triu_indices(len(pos), 1)
    keep = mol[i] != mol[j]
    i, j = i[keep], j[keep]
    if not i.size:
        return 0, np.inf
    _, _, rimg, _ = minimum_image(system["basis"], rb, pos[i] - pos[j])
    return int((rimg < scale).sum()), float(np.abs(rimg - scale).min())


def contact_table(system, flags, scale, present=None):
    """close_contacts() pair by pair: dict(i, j, rimg, counted) over the pairs i < j of two present atoms (`present`: a
    boolean mask, default all) on different molecules, in (i, j) order.  The decision rimg < scale is the fp64 one of
    close_contacts(); rimg is evaluated in longdouble from the fp64 coordinates at the lattice image the fp64 path picked,
    so that rimg - scale shows how far from the scale the decision was taken."""
    pos = np.asarray(system["pos"], dtype=np.float64)
    mol = np.asarray(system["molecule"])  # (ids, not runs: the slots of an edited context carry holes)
    ok = np.ones(len(pos), dtype=bool) if present is None else np.asarray(present, dtype=bool)
    _, rb, _ = pbc(system["basis"], flags.get("pbc_cutoff", 0.0))
    i, j = np.triu_indices(len(pos), 1)
    keep = (mol[i] != mol[j]) & ok[i] & ok[j]
    i, j = i[keep], j[keep]
    if not i.size:
        return dict(i=i, j=j, rimg=np.zeros(0, LD), counted=np.zeros(0, dtype=bool), scale=scale)
    d = pos[i] - pos[j]
    image, _, rimg64, _ = minimum_image(system["basis"], rb, d)
    shift = image.astype(LD) @ np.asarray(system["basis"], dtype=np.float64).astype(LD)
    e = d.astype(LD) - shift
    rimg = np.sqrt((e * e).sum(axis=1, dtype=LD))
    return dict(i=i, j=j, rimg=rimg, counted=rimg64 < scale, scale=scale)


def contact_tiles(table):
    """{(i // 64, j // 64): counted pairs of the tile}, the tiles with none left out"""
    out = {}
    for i, j in zip(table["i"][table["counted"]], table["j"][table["counted"]]):
        t = (int(i) // 64, int(j) // 64)
        out[t] = out.get(t, 0) + 1
    return out


def explain(got, want):
    """Lines that say which 64 x 64 tiles (i // 64, j // 64) account for the difference between two contact tables of
    the same atoms (`got`: of the input as something else saw it; `want`: the reference's), with the pairs of each such
    tile that are counted in one table only and their rimg - scale; in the style of pair_reference.explain_energy."""
    def pairs(t):
        return {(int(a), int(b)): float(r - LD(t["scale"])) for a, b, r, c in zip(t["i"], t["j"], t["rimg"], t["counted"]) if c}

    g, w = pairs(got), pairs(want)
    lines = []
    tiles = sorted(set((a // 64, b // 64) for a, b in set(g) ^ set(w)))
    for t in tiles:
        extra = sorted(p for p in set(g) - set(w) if (p[0] // 64, p[1] // 64) == t)
        missing = sorted(p for p in set(w) - set(g) if (p[0] // 64, p[1] // 64) == t)
        lines.append("tile (%d, %d): %+d (%d extra, %d missing)" % (t[0], t[1], len(extra) - len(missing), len(extra),
                                                                    len(missing)))
        lines += ["  extra pair (%d, %d), rimg - scale = %.3e" % (p[0], p[1], g[p]) for p in extra[:5]]
        lines += ["  missing pair (%d, %d), rimg - scale = %.3e" % (p[0], p[1], w[p]) for p in missing[:5]]
    if not lines:
        lines = ["the two tables count the same pairs (%d)" % len(w)]
    return lines


def vdw_terms(system, flags, iso_cache=None):
    """Everything the mode adds, in longdouble: e_total, e_iso, lr_corr, vdw_energy = e_total - e_iso + lr_corr,
    repulsion, repulsion_lrc, rd_energy; the sums of |terms| as abs_<name>; lam = the eigenvalues of C (ascending, before
    the clip); rimg_margin (see repulsion())."""
    Cm, _ = c_matrix(system, flags)
    lam = jacobi_eigenvalues(Cm)
    et = eigen_energy(lam)
    ei = e_iso(system, flags, iso_cache)
    lr, lr_abs = lr_corr(system, flags)
    rep, rep_abs, margin = repulsion(system, flags)
    rl, rl_abs = repulsion_lrc(system, flags)
    return dict(e_total=et, e_iso=ei, lr_corr=lr, vdw_energy=et - ei + lr, repulsion=rep, repulsion_lrc=rl,
                rd_energy=rep + rl, abs_e_total=et, abs_e_iso=ei, abs_lr_corr=lr_abs, abs_repulsion=rep_abs,
                abs_repulsion_lrc=rl_abs, lam=lam, rimg_margin=margin)
