"""Inputs and flag sets shared by the coupled-dipole van der Waals tests (a plain helper module).

  box(n)     n sites in a triclinic cell at liquid density (centres on a jittered 3.7 A lattice), n in SITE_COUNTS: 1 .. 130
             sites are n = 3 .. 390 matrix rows, on both sides of every 64-wide boundary of the kernels.  From 21 sites
             on: one frozen framework molecule of n // 5 atoms (every seventh without polarizability), five-site molecules
             (a centre and four satellites 1.09 A away; the last satellite has omega = 0), and one-site molecules of three
             types: active, alpha = 0, omega = 0.  Below 21 sites: one-site molecules only.
  clip()     two one-site molecules 1.2 A apart with polar_damp 10 and alpha 1.5 (2 alpha / r^3 > 1: a negative
             eigenvalue that the sum clips) beside four ordinary ones.
  contacts() molecules placed around cavity_autoreject_scale: see the function.
  large(name)  the cases of LARGE, 1023 .. 2097 matrix rows, whose references are recorded: see the function.
  axis2(), axis3(), lattice27()  spectra with exact structure (EXACT); clip_at(r), crossing()  the clip pair at the
             separation where the smallest eigenvalue changes sign, and crossing_bound() / delta_factor() for its test.

Every system carries omega and mol_type next to the arrays mpmc_amd.synth systems have.
"""
import hashlib
import os

import numpy as np

from mpmc_amd import synth

SITE_COUNTS = (1, 2, 21, 22, 43, 70, 130)
FLAGS = dict(temperature=150.0, polarization=1, polar_damp=2.1304, polar_max_iter=4, rd_lrc=1, polarvdw=1)
TOL = 1e-12       # |term - reference| <= TOL * sum |terms|, the project's convention
COND = 1e-3       # the parity cases keep lambda_min >= COND * lambda_max: a sqrt near 0 would amplify any solver's error
TYPE_FRAME, TYPE_FIVE, TYPE_ONE, TYPE_ONE_NOALPHA, TYPE_ONE_NOOMEGA = 0, 1, 2, 3, 4

_TET = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / np.sqrt(3.0)


def _cell(ncentres, spacing=3.7):
    m = max(3, int(np.ceil(ncentres ** (1.0 / 3.0) - 1e-9)))
    L = spacing * m
    basis = np.array([[L, 0.0, 0.0], [0.2 * L, 0.97 * L, 0.0], [0.12 * L, -0.17 * L, 0.95 * L]])
    return m, L, basis


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def _assemble(rows, basis, L):
    pos, q, alpha, eps, sig, mass, mol, frozen, omega, mtype = (list(c) for c in zip(*rows))
    s = synth._finish(np.array(pos), q, alpha, eps, sig, mass, mol, frozen, L)
    s["basis"] = basis
    s["omega"] = np.asarray(omega, dtype=np.float64)
    s["mol_type"] = np.asarray(mtype, dtype=np.int32)
    return s


def _one_site(c, kind, mol):
    alpha = 0.0 if kind == TYPE_ONE_NOALPHA else 1.1
    omega = 0.0 if kind == TYPE_ONE_NOOMEGA else 0.62
    return [(c, 0.0, alpha, 35.0, 3.1, 16.0, mol, 0, omega, kind)]


def _five_site(c, rot, mol):
    rows = [(c, -0.4, 1.0, 40.0, 3.2, 12.0, mol, 0, 0.71, TYPE_FIVE)]
    for k in range(4):
        rows.append((c + 1.09 * (_TET[k] @ rot.T), 0.1, 0.3, 0.0 if k == 1 else 6.0, 0.0 if k == 1 else 2.4, 1.0, mol, 0,
                     0.0 if k == 3 else 0.52, TYPE_FIVE))
    return rows


def box(n, seed=None, parts=None):
    """parts = (framework atoms, five-site molecules, one-site molecules, mixed one-site kinds?) instead of the default
    split of n; the default's random stream is untouched"""
    rng = np.random.default_rng(7000 + n if seed is None else seed)
    nframe = n // 5 if n >= 21 else 0
    nfive = (n - nframe) // 8 if n >= 21 else 0  # five-site molecules take about 5/8 of the movable sites
    none = n - nframe - 5 * nfive
    mixed = n >= 21
    if parts is not None:
        nframe, nfive, none, mixed = parts
        assert nframe + 5 * nfive + none == n
    ncent = nframe + nfive + none
    m, L, basis = _cell(ncent)
    idx = rng.permutation(m ** 3)[:ncent]
    frac = (np.stack([idx // (m * m), (idx // m) % m, idx % m], axis=1) + 0.5) / m
    cent = (frac + rng.uniform(-0.03, 0.03, frac.shape)) @ basis
    rows, mol, c = [], 1, 0
    for k in range(nframe):  # the framework: ONE frozen molecule
        rows.append((cent[c], 0.3 if k % 2 else -0.3, 0.0 if k % 7 == 3 else 0.8, 30.0 + k % 3, 3.0 + 0.01 * (k % 5), 16.0, mol,
                     1, 0.6, TYPE_FRAME))
        c += 1
    mol += 1 if nframe else 0
    kinds = [TYPE_ONE, TYPE_ONE, TYPE_ONE_NOALPHA, TYPE_ONE, TYPE_ONE_NOOMEGA]
    # one-site and five-site molecules interleaved, so that neither kind sits in one 64-atom block alone
    todo = [("five", None)] * nfive + [("one", kinds[k % 5] if mixed else TYPE_ONE) for k in range(none)]
    order = rng.permutation(len(todo))
    for o in order:
        kind, sub = todo[o]
        rows += _five_site(cent[c], _rotation(rng), mol) if kind == "five" else _one_site(cent[c], sub, mol)
        c += 1
        mol += 1
    assert len(rows) == n
    return _assemble(rows, basis, L)


CLIP_FLAGS = dict(FLAGS, polar_damp=10.0)


def clip():
    """a weakly damped close pair: r = 1.2 A, alpha = 1.5, polar_damp = 10 -> 2 alpha / r^3 = 1.74 > 1"""
    m, L, basis = _cell(27)
    c = np.array([[0.2, 0.2, 0.2], [0.2, 0.2, 0.2], [0.6, 0.3, 0.7], [0.3, 0.7, 0.5], [0.8, 0.8, 0.2], [0.7, 0.4, 0.3]]) @ basis
    c[1] += np.array([1.2, 0.0, 0.0])
    rows = []
    for k in range(6):
        rows.append((c[k], 0.0, 1.5 if k < 2 else 1.1, 35.0, 3.1, 16.0, k + 1, 0, 0.62, TYPE_ONE + (0 if k >= 2 else 5)))
    return _assemble(rows, basis, L)


# ---- the large cases: matrices past the 1024-thread strides of vdw_reflect_kernel and vdw_sum_kernel.  Their references are
# recorded (tests/golden/make_vdw_large.py -> tests/golden/vdw_large.npz): vdw_reference.prerotated_eigen_energy takes
# minutes at these sizes.
LARGE_ROWS = dict(rows1023=1023, rows1026=1026, rows1029=1029, big1=1038, big2=2097, frame=1089)
LARGE = tuple(LARGE_ROWS)
FRAME_ROWS = 1053  # the framework molecule's own active sites in `frame`: e_iso of a type above 1024 rows
LARGE_TERMS = ("e_total", "e_iso", "lr_corr", "repulsion", "repulsion_lrc")
GOLDEN_LARGE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vdw_large.npz")


def active_rows(s, atoms=None):
    k = np.sqrt(np.asarray(s["alpha"], dtype=np.float64)) * np.asarray(s["omega"], dtype=np.float64)
    return 3 * int((k != 0.0).sum() if atoms is None else (k[atoms] != 0.0).sum())


def large(name):
    """rows<n>  n / 3 one-site molecules, every site active: vdw_sum_kernel takes its second trip from n = 1025,
                vdw_reflect_kernel (mm = n - 1 at column 0, the loop starts at 1 + tid) from n = 1027
       big1     box(460): second trip with the full mix of site kinds
       big2     box(930): third trip; the second is taken by every thread
       frame    a frozen framework molecule of 410 atoms (351 active: 1053 rows of its own), two five-site and six
                one-site molecules: e_total and e_iso both large and nearly equal"""
    if name.startswith("rows"):
        n = int(name[4:]) // 3
        s = box(n, parts=(0, 0, n, False))
    elif name == "frame":
        s = box(426, parts=(410, 2, 6, True))
        assert active_rows(s, np.flatnonzero(s["mol_type"] == TYPE_FRAME)) == FRAME_ROWS
        assert len(set(np.asarray(s["molecule"])[np.asarray(s["frozen"]) == 0])) <= 8
    else:
        s = box({"big1": 460, "big2": 930}[name])
    assert active_rows(s) == LARGE_ROWS[name], (name, active_rows(s))
    return s


def input_hash(s, rows):
    """SHA-256 over a case's input arrays and its row count"""
    h = hashlib.sha256()
    for key, dt in (("pos", np.float64), ("charge", np.float64), ("alpha", np.float64), ("epsilon", np.float64),
                    ("sigma", np.float64), ("mass", np.float64), ("omega", np.float64), ("basis", np.float64),
                    ("molecule", np.int64), ("frozen", np.int64), ("mol_type", np.int64)):
        h.update(key.encode())
        h.update(np.ascontiguousarray(np.asarray(s[key]), dtype=dt).tobytes())
    h.update(np.int64(rows).tobytes())
    return h.hexdigest()


_large = {}


def large_reference(name):
    """the record of one large case: the terms and their abs_ sums in longdouble (hi + lo), err_e_total, err_e_iso (the
    certified error of the eigenvalue sums; the other terms carry none), b_min, b_max, sha256"""
    from pair_reference import LD

    if not _large:
        with np.load(GOLDEN_LARGE) as z:
            _large.update({k: z[k] for k in z.files})
    out = {}
    for t in LARGE_TERMS + tuple("abs_" + t for t in LARGE_TERMS):
        hi, lo = _large["%s/%s" % (name, t)]
        out[t] = LD(hi) + LD(lo)
    for t in ("err_e_total", "err_e_iso", "b_min", "b_max"):
        out[t] = float(_large["%s/%s" % (name, t)])
    out["sha256"] = str(_large["%s/sha256" % name])
    out["rows"] = int(_large["%s/rows" % name])
    return out


# ---- exact structure: cubic cells, coordinates exact in binary, one-site molecules of one type, no framework
def _exact(points, L):
    basis = np.diag([L, L, L]).astype(np.float64)
    rows = [(np.array(p, dtype=np.float64), 0.0, 1.1, 35.0, 3.1, 16.0, k + 1, 0, 0.62, TYPE_ONE) for k, p in enumerate(points)]
    return _assemble(rows, basis, L)


def axis2():
    """two sites 4 A apart on the x axis, cell 32 A: x, y and z decouple with exact zeros, the y and z spectra are the same
    bits, and the reduction meets a column whose tail is exactly zero (tau = 0, e_j = 0)"""
    return _exact([(8.0, 8.0, 8.0), (12.0, 8.0, 8.0)], 32.0)


def axis3():
    """three collinear sites on the same line (4 A and 6 A apart)"""
    return _exact([(8.0, 8.0, 8.0), (12.0, 8.0, 8.0), (18.0, 8.0, 8.0)], 32.0)


def lattice27():
    """a 3 x 3 x 3 lattice of 4 A spacing filling a 12 A cell: every site sees the same surroundings"""
    return _exact([(2.0 + 4.0 * i, 2.0 + 4.0 * j, 2.0 + 4.0 * k) for i in range(3) for j in range(3) for k in range(3)], 12.0)


EXACT = ("axis2", "axis3", "lattice27")


# ---- a zero crossing: the clip pair moved to where the smallest eigenvalue changes sign
CROSS_STEPS = (-1e-2, -1e-4, -1e-6, -1e-8, 1e-8, 1e-6, 1e-4, 1e-2)


def clip_at(r):
    s = clip()
    pos = np.array(s["pos"], dtype=np.float64)
    pos[1] = pos[0] + np.array([r, 0.0, 0.0])
    s["pos"] = pos
    return s


def _lambda_min(r):
    import vdw_reference as vr

    return vr.jacobi_eigenvalues(vr.c_matrix(clip_at(r), CLIP_FLAGS)[0]).min()


def crossing():
    """r*: the separation of the clip pair at which the longdouble reference's smallest eigenvalue changes sign (negative
    below, positive above), by 60 deterministic halvings of [1.2, 2.0] A"""
    if "r*" not in _cache:
        lo, hi = 1.2, 2.0
        assert _lambda_min(lo) < 0 < _lambda_min(hi)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if _lambda_min(mid) < 0:
                lo = mid
            else:
                hi = mid
        _cache["r*"] = hi
    return _cache["r*"]


def cross_name(step):
    return "cross%+.0e" % step


def delta_factor(n):
    """K(n) of DESIGN.md section 12, "Error bound of the solver as coded": every eigenvalue the kernels return is within
    K(n) * 2^-53 * max |lambda| of the reference's.  Counted from the code, not fitted:
      c(m) = 9 s1 + 8 s2 + 4 s3 + 130 per Householder column with a trailing block of m rows, where
             s1 = ceil((m - 1) / 1024) + 22   depth of the 1024-thread sum (strided trips, 6 butterfly levels, 16 waves)
             s2 = ceil(m / 64) + 6            depth of a wave's row product
             s3 = ceil(m / 256) + 10          depth of the 256-thread p.v
      K(n) = sqrt(n) * (BUILD + sum_{m = 2}^{n - 1} c(m)) + BISECT"""
    def c(m):
        return 9 * (-(-(m - 1) // 1024) + 22) + 8 * (-(-m // 64) + 6) + 4 * (-(-m // 256) + 10) + 130

    return np.sqrt(float(n)) * (BUILD_ULPS + sum(c(m) for m in range(2, n))) + BISECT_ULPS


def crossing_bound(lam):
    """CONV * sum_i [sqrt(max(lambda_i, 0) + delta) - sqrt(max(lambda_i - delta, 0))] + TOL * reference, delta =
    K(n) 2^-53 max |lambda|: what an eigenvalue error of delta can do to the clipped sum of square roots"""
    from pair_reference import LD
    from vdw_reference import CONV, eigen_energy

    delta = LD(delta_factor(len(lam))) * LD(2) ** -53 * np.abs(lam).max()
    zero = LD(0)
    spread = (np.sqrt(np.maximum(lam, zero) + delta) - np.sqrt(np.maximum(lam - delta, zero))).sum(dtype=LD)
    return float(CONV * spread + TOL * eigen_energy(lam))


BUILD_ULPS = 40   # ||C_device - C_reference||_F <= 40 * 2^-53 ||C||_F where polar_damp * r >= 10 for every pair (section 12)
BISECT_ULPS = 10  # Sturm count backward error 7, midpoint rounding 1, 64 halvings of the interval < 1, margin 1


SCALE = 1.5        # cavity_autoreject_scale of the contact cases
EDGE = 1e-9


def contacts(inside=True, outside=True, frozen_pair=True):
    """One-site and two-site molecules far apart, plus:
       inside       a different-molecule pair SCALE - 1e-9 apart                       (counts)
       outside      a different-molecule pair SCALE + 1e-9 apart                       (does not)
       always       a two-site molecule whose own sites are 0.7 A apart               (same molecule: ignored)
       frozen_pair  two frozen one-atom molecules 1.0 A apart                          (frozen-frozen: counts)"""
    m, L, basis = _cell(64)
    rows, mol = [], 1
    e = np.array([0.6, 0.0, 0.8])  # a unit vector

    def one(c, frozen=0):
        nonlocal mol
        rows.append((np.array(c, dtype=float), 0.0, 1.1, 35.0, 3.1, 16.0, mol, frozen, 0.62, TYPE_ONE + (5 if frozen else 0)))
        mol += 1

    for c in ((2.0, 2.0, 2.0), (7.0, 2.5, 2.0), (2.5, 7.0, 2.2), (2.2, 2.4, 7.0), (7.0, 7.0, 7.0)):
        one(c)
    if inside:
        one((10.0, 3.0, 3.0))
        one(np.array((10.0, 3.0, 3.0)) + (SCALE - EDGE) * e)
    if outside:
        one((3.0, 10.0, 3.0))
        one(np.array((3.0, 10.0, 3.0)) + (SCALE + EDGE) * e)
    for off in (0.0, 0.7):  # the two-site molecule
        rows.append((np.array((6.0, 10.5, 6.0)) + off * e, 0.0, 0.2, 10.0, 2.5, 8.0, mol, 0, 0.5, TYPE_FIVE + 5))
    mol += 1
    if frozen_pair:
        one((10.5, 10.5, 3.0), frozen=1)
        one(np.array((10.5, 10.5, 3.0)) + 1.0 * e, frozen=1)
    return _assemble(rows, basis, L)


def cage():
    """six one-site molecules on a line, neighbours SCALE + 1e-9 A apart: nobody is in contact, and almost any step of one
    of the inner four along the line brings it within the scale of a neighbour (a step of t along the line and p across it
    changes the distance by p^2 / (2 SCALE) - t)"""
    m, L, basis = _cell(64)
    e = np.array([0.6, 0.0, 0.8])
    rows = [(np.array((5.0, 7.0, 4.0)) + k * (SCALE + EDGE) * e, 0.0, 1.1, 35.0, 3.1, 16.0, k + 1, 0, 0.62, TYPE_ONE)
            for k in range(6)]
    return _assemble(rows, basis, L)


_cache = {}


def system(name):
    """'box<n>', 'clip', 'contacts', a name of LARGE or of EXACT, or cross_name(step): built once, never modified"""
    if name not in _cache:
        if name.startswith("box"):
            _cache[name] = box(int(name[3:]))
        elif name in LARGE_ROWS:
            _cache[name] = large(name)
        elif name.startswith("cross"):
            _cache[name] = clip_at(crossing() + float(name[5:]))
        else:
            _cache[name] = {"clip": clip, "contacts": contacts, "axis2": axis2, "axis3": axis3, "lattice27": lattice27}[name]()
    return _cache[name]


def flags_of(name):
    return CLIP_FLAGS if name == "clip" or name.startswith("cross") else FLAGS


_ref = {}


def reference(name):
    """vdw_reference.vdw_terms of one case, computed once and shared (never modified)"""
    import vdw_reference as vr

    if name not in _ref:
        _ref[name] = vr.vdw_terms(system(name), flags_of(name))
    return _ref[name]


def moved(s, molecule_index, shift, rot_seed=None):
    """a copy of system s with one molecule (index into the upload's molecule order) translated by `shift` (and rotated
    about its first site when rot_seed is given); returns (system, first atom, new positions of the molecule)"""
    from pair_reference import _molecule_index

    mol = _molecule_index(s["molecule"])
    atoms = np.flatnonzero(mol == molecule_index)
    t = dict(s)
    pos = np.array(s["pos"], dtype=np.float64)
    p = pos[atoms]
    if rot_seed is not None:
        rot = _rotation(np.random.default_rng(rot_seed))
        p = p[0] + (p - p[0]) @ rot.T
    pos[atoms] = p + np.asarray(shift, dtype=np.float64)
    t["pos"] = pos
    return t, int(atoms[0]), pos[atoms]
