"""Adversarial geometry for the pair / static-field kernels: inputs built so that the cheap screen
(prefilter_within_f / prefilter_within_d, device_common.h) and the exact fp64 path are pushed to disagree, and so that
pairs sit on the three cutoff comparisons.  Helper module for tests/test_adversarial_inputs.py (CPU: proves the inputs
are adversarial) and tests/test_gpu_screen_edges.py (GPU: engine against the per-pair reference and the oracle).

Every system is made of single-site molecules with LJ parameters, a charge of alternating sign and a small
polarizability, so each probe pair shows up in rd, es and the static field at once.  N is not a multiple of 64 and the
atom order is a seeded permutation, re-drawn until the probe pairs cover the tile positions that matter (coverage()).

Classes (last paragraph):
  T  near-tie pairs in sheared cells: one fractional component of the displacement at 0.5 -+ delta;
  E  cutoff-edge pairs in a cubic cell with an explicit cutoff: exact distances around rc;
  F  T / E plus one inert spectator atom beyond 2048 A: switches the engine to the fp64 screen (DevBox::screen64);
  B  T / E translated so that max |x| sits just below 2048 A, where fp32 coordinates are 1.2e-4 A apart.
"""
import numpy as np

import pair_reference as pr
from mpmc_amd import synth

L_T = 25.0
CELLS = {
    # the sheared cell of test_triclinic_box_polarizable
    "sheared": np.array([[L_T, 0, 0], [0.3 * L_T, 0.9 * L_T, 0], [-0.2 * L_T, 0.25 * L_T, 0.85 * L_T]]),
    "hexagonal": np.array([[L_T, 0, 0], [-0.5 * L_T, 0.5 * np.sqrt(3.0) * L_T, 0], [0, 0, L_T]]),  # gamma = 120 deg
    "monoclinic": np.array([[L_T, 0, 0], [0, L_T, 0], [L_T * np.cos(np.radians(110.0)), 0, L_T * np.sin(np.radians(110.0))]]),
}
DELTAS = (0.0, 1e-12, 1e-9, 2e-8)
T_PAIRS = 288  # probe pairs per input (>= 256): feasible directions x 2 signs x 2 sides of the tie x 4 deltas x repeats
T_INSIDE = 0.5  # the fp64 image is inside the cutoff by at least this, the competing image outside rc + 0.01 by it
MIN_DIST = 2.0  # no two atoms closer than this (keeps LJ / Coulomb / Thole terms tame)
EPS, SIG, QABS, ALPHA, MASS = 50.0, 2.0, 0.4 * synth.E2REDUCED, 0.2, 20.0

L_E, RC_E = 40.0, 9.0
E_REPEAT = 4  # 16 distances x 3 axes x 2 signs x 4 = 384 probe pairs
SCREEN_MARGIN = 0.01  # DevBox::rc2_pre
SHIFT_B = 2048.0 - 64.0  # translation of class B: every coordinate stays below kScreen32MaxCoord = 2048 A
SPECTATOR_X = 3000.0


def e_targets(rc, step):
    """The cutoff-edge distances: name -> distance.  `step` is the spacing of the representable distances (one ulp of
    rc when the anchor sits at a coordinate of 0; the coordinate spacing of the partner in class B)."""
    t = {}
    for k in (-2, -1, 0, 1, 2):
        t["rc%+dulp" % k] = rc + k * step
    for name, d in (("rc+0.5e-12", 0.5e-12), ("rc+1e-12", 1e-12), ("rc+2e-12", 2e-12)):
        t[name] = rc + d
    t["rc+1e-9-"] = rc + 1e-9 - step
    t["rc+1e-9"] = rc + 1e-9
    t["rc+1e-9+"] = rc + 1e-9 + step
    t["rc+0.005"] = rc + 0.005
    t["rc-0.005"] = rc - 0.005
    t["rc+0.0099"] = rc + 0.0099
    t["rc+0.0101"] = rc + 0.0101
    t["rc-1e-9"] = rc - 1e-9
    return t


def _min_dist(basis, placed, p):
    """true minimum distance (27 images) from point p to the placed points"""
    if not len(placed):
        return np.inf
    d = np.asarray(placed) - p
    f = d @ np.linalg.inv(basis)
    d = (f - np.rint(f)) @ basis  # (atoms may sit outside the cell: reduce first, then look at the neighbours)
    sh = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], dtype=np.float64) @ basis
    return np.sqrt(((d[:, None, :] + sh[None, :, :]) ** 2).sum(axis=2)).min()


def fractional(rb, d):
    """the argument of rint() in minimum_image (pairs.c:240-246), same operation order"""
    out = []
    for p in range(3):
        f = rb[0][p] * d[..., 0]
        f = f + rb[1][p] * d[..., 1]
        f = f + rb[2][p] * d[..., 2]
        out.append(f)
    return np.stack(out, axis=-1)


def coverage(n, probes):
    """Tile positions the probe pairs reach, as the pair kernel sees them (row = lower index: tile i // 64, lane i % 64;
    column j % 64, taken by wave (j % 64) // 8)."""
    lo, hi = np.minimum(probes[:, 0], probes[:, 1]), np.maximum(probes[:, 0], probes[:, 1])
    return dict(same_tile=bool(np.any(lo // 64 == hi // 64)), other_tile=bool(np.any(lo // 64 != hi // 64)),
                row_lane0=bool(np.any(lo % 64 == 0)), row_lane63=bool(np.any(lo % 64 == 63)),
                columns=len(set((hi % 64).tolist())), last_block=bool(np.any(hi >= 64 * (n // 64))),
                ragged=(n % 64 != 0))


def covered(c):
    return (c["same_tile"] and c["other_tile"] and c["row_lane0"] and c["row_lane63"] and c["columns"] == 64 and
            c["last_block"] and c["ragged"])


def _assemble(basis, pairs, labels, extras, seed, pbc_cutoff):
    """pairs[m,2,3] probe positions + extras[k,3] -> shuffled system; probes[m,2] = atom indices after the shuffle."""
    m = len(pairs)
    pos = np.concatenate([pairs.reshape(2 * m, 3), extras])
    n = len(pos)
    q = np.empty(n)
    q[0:2 * m:2], q[1:2 * m:2] = QABS, -QABS  # the two atoms of a probe pair carry opposite charges
    q[2 * m:] = QABS * (1 - 2 * (np.arange(n - 2 * m) % 2))
    for attempt in range(2000):
        perm = np.random.default_rng([seed, attempt]).permutation(n)  # perm[new] = old
        inv = np.empty(n, dtype=np.int64)
        inv[perm] = np.arange(n)
        probes = np.stack([inv[0:2 * m:2], inv[1:2 * m:2]], axis=1)
        if covered(coverage(n, probes)):
            break
    else:
        raise RuntimeError("no permutation covers the tile positions")
    system = dict(pos=np.ascontiguousarray(pos[perm]), charge=q[perm], alpha=np.full(n, ALPHA), epsilon=np.full(n, EPS),
                  sigma=np.full(n, SIG), mass=np.full(n, MASS), molecule=np.arange(1, n + 1, dtype=np.int32),
                  frozen=np.zeros(n, dtype=np.int32), basis=np.array(basis, dtype=np.float64))
    return dict(system=system, probes=probes, labels=list(labels), pbc_cutoff=pbc_cutoff)


def feasible_directions(basis):
    """Lattice directions k along which a near-tie pair can lie inside the cutoff at all.  A displacement with fractional
    component 0.5 along k lies on a plane at distance h_k / 2 from the origin, h_k = 1 / |column k of the reciprocal
    basis| being the spacing of the lattice planes; no point of it is closer than that, so the class conditions
    (rimg <= rc - T_INSIDE) can only be met where h_k / 2 < rc - T_INSIDE.  In a cubic cell that is no direction (a tie
    sits at >= rc); in the sheared cells here it is two of the three, and between them the three cells cover every k."""
    _, rb, rc = pr.pbc(basis)
    return [k for k in range(3) if 0.5 / np.linalg.norm(rb[:, k]) < rc - T_INSIDE]


def build_T(cell, shift=0.0, seed=7, n_extra=21):
    """Class T (class B with shift = SHIFT_B).  Every probe slot (direction k, sign, side of the tie, delta, repeat) is
    filled by drawing again until the geometric conditions hold, so the input ships exactly the planned number."""
    basis = CELLS[cell]
    vol, rb, rc = pr.pbc(basis)
    rng = np.random.default_rng([seed, 1])
    placed, pairs, labels = [], [], []
    ks = feasible_directions(basis)
    slots = [(k, sgn, side, dl) for _ in range(T_PAIRS // (16 * len(ks))) for k in ks for sgn in (1.0, -1.0)
             for side in (1.0, -1.0) for dl in DELTAS]
    assert len(slots) == T_PAIRS
    for (k, sgn, side, dl) in slots:
        done = False
        for _ in range(200):  # batches of candidates; the first one that meets every condition fills the slot
            m = 2048
            base = rng.uniform(0.0, 1.0, (m, 3)) @ basis + shift
            s = rng.uniform(-0.5, 0.5, (m, 3))
            s[:, k] = sgn * (0.5 - side * dl)
            partner = base + s @ basis
            d = base - partner
            image, _, rimg, _ = pr.minimum_image(basis, rb, d)
            f = fractional(rb, d)
            other = image.copy()
            other[:, k] = np.where(image[:, k] == np.ceil(f[:, k]), np.floor(f[:, k]), np.ceil(f[:, k]))
            r_other = np.linalg.norm(d - other @ basis, axis=1)
            ok = (rimg <= rc - T_INSIDE) & (r_other >= rc + SCREEN_MARGIN + T_INSIDE)
            ok &= np.abs(np.abs(f[:, k]) - 0.5) <= dl + 1e-10  # the rounding of the placement stays far below the deltas
            for c in np.flatnonzero(ok):
                if min(_min_dist(basis, placed, base[c]), _min_dist(basis, placed, partner[c])) < MIN_DIST:
                    continue
                placed += [base[c], partner[c]]
                pairs.append([base[c], partner[c]])
                labels.append(dict(k=k, sign=sgn, side=side, delta=dl))
                done = True
                break
            if done:
                break
        if not done:
            raise RuntimeError("could not place a class-T pair")
    extras = []
    while len(extras) < n_extra:
        p = rng.uniform(0.0, 1.0, 3) @ basis + shift
        if _min_dist(basis, placed, p) >= MIN_DIST:
            placed.append(p)
            extras.append(p)
    out = _assemble(basis, np.array(pairs), labels, np.array(extras), seed, 0.0)
    out.update(cls="T", cell=cell, shift=shift)
    return out


def build_E(shift=0.0, seed=11, n_extra=37):
    """Class E (class B with shift = SHIFT_B): the anchor has coordinate `shift` along the probe axis (0 in class E, so the
    partner coordinate IS the distance and sqrt(r * r) is exact), the partner sits at shift +- target on that axis and
    shares the other two coordinates."""
    basis = np.diag([L_E, L_E, L_E])
    rc = RC_E
    step = np.spacing(rc) if shift == 0.0 else np.spacing(shift + rc)
    targets = e_targets(rc, step)
    rng = np.random.default_rng([seed, 2])
    placed, pairs, labels = [], [], []
    for rep in range(E_REPEAT):
        for axis in range(3):
            for sgn in (1.0, -1.0):
                for name, t in targets.items():
                    for _ in range(100000):
                        a = rng.uniform(0.0, L_E, 3) + shift
                        a[axis] = shift
                        b = a.copy()
                        b[axis] = shift + sgn * t
                        if min(_min_dist(basis, placed, a), _min_dist(basis, placed, b)) < MIN_DIST:
                            continue
                        placed += [a, b]
                        pairs.append([a, b])
                        labels.append(dict(name=name, axis=axis, sign=sgn, target=t))
                        break
                    else:
                        raise RuntimeError("could not place a class-E pair")
    extras = []
    while len(extras) < n_extra:
        p = rng.uniform(0.0, L_E, 3) + shift
        if _min_dist(basis, placed, p) >= MIN_DIST:
            placed.append(p)
            extras.append(p)
    out = _assemble(basis, np.array(pairs), labels, np.array(extras), seed, rc)
    out.update(cls="E", cell="cubic", shift=shift)
    return out


def with_spectator(inp):
    """Class F: one atom with q = eps = sigma = alpha = 0 at x = 3000 A, appended (probe indices and every probe
    coordinate stay bit-identical); the engine's running max |coordinate| passes 2048 A and DevBox::screen64 switches on."""
    s = {k: np.array(v) for k, v in inp["system"].items()}
    s["pos"] = np.concatenate([s["pos"], [[SPECTATOR_X, 1.0, 2.0]]])
    for k in ("charge", "alpha", "epsilon", "sigma"):
        s[k] = np.append(s[k], 0.0)
    s["mass"] = np.append(s["mass"], MASS)
    s["molecule"] = np.append(s["molecule"], s["molecule"].max() + 1).astype(np.int32)
    s["frozen"] = np.append(s["frozen"], 0).astype(np.int32)
    out = dict(inp, system=s, cls=inp["cls"] + "F")
    assert len(s["charge"]) % 64 != 0
    return out


_CACHE = {}


def get(name):
    """Inputs by name, built once per process: T_sheared, T_hexagonal, T_monoclinic, E, their F_ and B_ forms."""
    if name not in _CACHE:
        if name.startswith("F_"):
            _CACHE[name] = with_spectator(get(name[2:]))
        elif name.startswith("B_T_"):
            _CACHE[name] = build_T(name[4:], shift=SHIFT_B)
        elif name == "B_E":
            _CACHE[name] = build_E(shift=SHIFT_B)
        elif name.startswith("T_"):
            _CACHE[name] = build_T(name[2:])
        elif name == "E":
            _CACHE[name] = build_E()
        else:
            raise KeyError(name)
    return _CACHE[name]


T_NAMES = ["T_sheared", "T_hexagonal", "T_monoclinic"]
ALL_NAMES = T_NAMES + ["E"] + ["F_" + n for n in T_NAMES + ["E"]] + ["B_" + n for n in T_NAMES + ["E"]]

# Flag sets, one per kernel variant (template instance of pair_rd_es_body / static_field_body).  ewald_alpha and
# polar_ewald_alpha are set low so that a pair AT the cutoff still weighs far more than the tolerance
# (erfc(0.12 * 9) = 0.13); polar_max_iter is small: these tests are about the field, not the solver.
_ES = dict(temperature=100.0, ewald_alpha_set=1, ewald_alpha=0.12)
_POL = dict(temperature=100.0, polarization=1, polar_damp=2.1304, polar_max_iter=2, ewald_alpha_set=1, ewald_alpha=0.12)
VARIANTS = {
    "rd_only": dict(temperature=100.0, rd_only=1),
    "ewald_fh0": dict(_ES),
    "ewald_fh2": dict(_ES, feynman_hibbs=1, feynman_hibbs_order=2),
    "ewald_fh4": dict(_ES, feynman_hibbs=1, feynman_hibbs_order=4),
    "wolf": dict(_ES, wolf=1),
    "field_bare": dict(_POL),
    "field_wolf0": dict(_POL, polar_wolf=1, polar_wolf_alpha=0.0),
    "field_wolfA": dict(_POL, polar_wolf=1, polar_wolf_alpha=0.13),
    "field_ewald": dict(_POL, polar_ewald=1, polar_ewald_alpha_set=1, polar_ewald_alpha=0.12),
}


def params_for(inp, variant):
    p = dict(VARIANTS[variant])
    if inp["pbc_cutoff"]:
        p["pbc_cutoff"] = inp["pbc_cutoff"]
    return p


# ---------------------------------------------------------------------------------------------------------------------
# numpy emulation of the fp32 screen (device_common.h: prefilter_within_f), one rounded fp32 operation per step.  The
# device contracts some of these into FMAs, so single decisions may differ; the statistics do not.
# tie_guard: None = the screen before the half-integer guard existed; a float = with the guard.
# ---------------------------------------------------------------------------------------------------------------------
def screen_f32(basis, rb, rc, pi, pj, tie_guard=None):
    f32 = np.float32
    fb, frb = np.asarray(basis).astype(f32), np.asarray(rb).astype(f32)
    d = pi.astype(f32) - pj.astype(f32)
    fr = [frb[0][k] * d[:, 0] + frb[1][k] * d[:, 1] + frb[2][k] * d[:, 2] for k in range(3)]
    im = [np.rint(x) for x in fr]
    e = [d[:, k] - (fb[0][k] * im[0] + fb[1][k] * im[1] + fb[2][k] * im[2]) for k in range(3)]
    r2 = e[0] * e[0] + e[1] * e[1] + e[2] * e[2]
    keep = ~(r2 > f32((rc + SCREEN_MARGIN) * (rc + SCREEN_MARGIN)))
    if tie_guard is not None:
        m = np.maximum(np.maximum(np.abs(fr[0] - im[0]), np.abs(fr[1] - im[1])), np.abs(fr[2] - im[2]))
        keep |= m >= f32(0.5) - f32(tie_guard)
    return keep


def tie_guard32(rb):
    """The engine's bound on the fp32 error of a fractional coordinate (device_common.h, dev_box() in engine.hip):
    11 * 2^-13 A times the largest column sum of |reciprocal basis|, rounded up by a quarter."""
    s = np.abs(np.asarray(rb)).sum(axis=0).max()
    return float(np.float32(1.25 * 11.0 * 2.0 ** -13 * s))
