"""Inputs shared by tests/test_polar_reference.py (CPU: the oracle against polar_reference) and
tests/test_gpu_polar_reference.py (the engine against it).

Sized cases come from synth.s_pol by setting chosen alpha to 0, which hits EXACT view sizes and interleaves alpha = 0
sites inside the 64-site blocks: 1, 2, 63, 64, 65, 128, 129 (block edges), 1024 / 1025 (the one-launch solver without and
with finisher workgroups), 1344 / 1345 (21 and 22 blocks: the last one-launch size and the first that defers sweeps); 1024 and 1344 are 1025 and 1345
with one more alpha set to 0, so three geometries above 1024 sites are built in all (1025, 1345 and 1345 after a move).
GS_LAG_SIZES are the views of 3 .. 7 blocks at which the Gauss-Seidel chain's cached lags first have a source and its
far-source loop first has one and two (tests/test_gpu_gs_lags.py); 'nv321_m2' is nv321 after the first two of lag_moves(321).
Special geometries are small: half-box ties in a sheared cell, polarizable sites 1e-1 .. 1e-3 A apart across a cell face,
two coincident polarizable sites, molecules moved by 10^4 lattice vectors, a frozen polarizable framework.

system(name) and tensor(name) are cached per name, so that the variants on one geometry share one tensor.
"""
import functools
import os

import numpy as np

import polar_reference as pref
from mpmc_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DAMP = 2.1304
BASE = dict(temperature=77.0, polarization=1, polar_damp=DAMP)
JACOBI4 = dict(BASE, polar_max_iter=4)
PRODUCTION = dict(BASE, polar_max_iter=4, polar_gs_ranked=1, polar_palmo=1, polar_gamma=1.03, polar_wolf=1,
                  polar_wolf_alpha=0.13)

SMALL_SIZES = (1, 2, 63, 64, 65, 128, 129)
RESIDENT_SIZES = (64, 65, 1024, 1025, 1344)
DEFERRED_SIZE = 1345
DEFERRED_ITERS = (2, 4, 5)
GS_SIZES = (129, 1025)
GS_VARIANTS = {
    "gs": dict(BASE, polar_max_iter=4, polar_gs=1),
    "gs_ranked": dict(BASE, polar_max_iter=4, polar_gs_ranked=1),
    "production": PRODUCTION,
}
# views of the chain kernel's lag machinery (option gs_lags = nlag in 2 .. 4; block t takes its sources t-1 .. t-nlag from cached
# matrices, lag k >= 2 through an auxiliary workgroup, and the sources s <= t-nlag-1 from the pair coefficients):
#   129 = 3 blocks: lag 2 first has a source; no far source under any nlag
#   193 = 4 blocks: aux(t = 3, 3) reads block 0; one far source under nlag = 2
#   256 = 4 blocks, the last one full
#   257 = 5 blocks: aux(t = 4, 4) reads block 0; one far source under nlag = 3, two under nlag = 2; a last block of one site
#   321 = 6 blocks: one far source under nlag = 4, two under nlag = 3
#   385 = 7 blocks: two far sources under nlag = 4
GS_LAG_SIZES = (129, 193, 256, 257, 321, 385)
GS_LAG_COUNTS = (2, 3, 4)
GS_LAG_VARIANTS = {"gs": GS_VARIANTS["gs"], "production": PRODUCTION}
GS_LAG_MOVED_SIZES = (321, 385)  # six and seven blocks: the incremental chain data behind a moved block
SHEARED_GS = dict(BASE, polar_max_iter=3, polar_gs=1)  # on sheared_640: the multi-block chain outside the orthorhombic branch
JACOBI_VARIANTS = {  # at 129 sites
    "sor": dict(BASE, polar_max_iter=6, polar_sor=1, polar_gamma=0.8),
    "esor": dict(BASE, polar_max_iter=6, polar_esor=1, polar_gamma=0.9),
    "palmo": dict(BASE, polar_max_iter=4, polar_palmo=1),
    "rrms": dict(BASE, polar_max_iter=5, polar_rrms=1),
    "precision": dict(BASE, polar_max_iter=0, polar_precision=1e-6),
    "zodid": dict(BASE, polar_zodid=1),
}
# atoms of the box a sized view is cut from: 3 polarizable sites per five-site molecule
_PARENT = {1024: 1750, 1025: 1750, 1344: 2300, 1345: 2300, 193: 700, 256: 700, 257: 700, 321: 700, 385: 700}


_ONE_LESS = {1024: 1025, 1344: 1345}  # the same geometry with one more alpha set to 0: one tensor serves both


@functools.lru_cache(maxsize=None)
def dropped_atom(nv):
    """the atom whose alpha sized(nv) sets to 0 on top of sized(nv + 1): from the middle of the view, inside a block"""
    return int(np.flatnonzero(sized(_ONE_LESS[nv])["alpha"] != 0.0)[nv // 2])


@functools.lru_cache(maxsize=None)
def sized(nv):
    """s_pol box with exactly nv polarizable sites: the others' alpha set to 0, chosen at random (seeded by nv).  Cached:
    callers copy what they change."""
    if nv in _ONE_LESS:
        s = dict(sized(_ONE_LESS[nv]))
        s["alpha"] = s["alpha"].copy()
        s["alpha"][dropped_atom(nv)] = 0.0
        return s
    s = dict(synth.s_pol(_PARENT.get(nv, 320)))
    alpha = s["alpha"].copy()
    pol = np.flatnonzero(alpha != 0.0)
    assert len(pol) >= nv
    rng = np.random.default_rng(9000 + nv)
    alpha[rng.choice(pol, size=len(pol) - nv, replace=False)] = 0.0
    s["alpha"] = alpha
    assert np.count_nonzero(alpha) == nv
    return s


def _ties(sheared, shift):
    """the lattice of test_gpu_parity.test_half_box_ties_use_one_image_everywhere"""
    n, L = 64, 12.0
    g = np.arange(4) * (L / 4)
    frac = np.array([[x, y, z] for x in g for y in g for z in g])
    rng = np.random.default_rng(2)
    basis = np.array([[L, 0, 0], [0.25 * L, L, 0], [0.0, 0.5 * L, L]]) if sheared else np.diag([L, L, L])
    s = dict(pos=(frac / L) @ basis + shift, charge=rng.normal(scale=60.0, size=n), alpha=rng.uniform(0.3, 1.2, size=n),
             epsilon=np.full(n, 10.0), sigma=np.full(n, 2.5), mass=np.full(n, 4.0),
             molecule=np.arange(n, dtype=np.int32), frozen=np.zeros(n, dtype=np.int32), basis=basis)
    s["charge"] -= s["charge"].mean()
    return s


CLOSE_A, CLOSE_B, CLOSE_C = 0, 35, 70  # first atoms (the polarizable centre sites) of molecules 0, 7 and 14


def _close(dist, three):
    """sized(126) (so that the view stays within 130 sites when the centres get their alpha back) with the centre of
    molecule 7 (and of molecule 14) put `dist` from the centre of molecule 0, plus 3 / -2 (and -5 / 1) lattice vectors: different molecules, across cell faces, and 3 L is not exact in fp64.  The centres carry no
    Lennard-Jones parameters here (r^-12 at 1e-3 A overflows nothing but drowns every other term)."""
    s = dict(sized(126))
    L = s["basis"][0][0]
    for k in ("pos", "alpha", "epsilon", "sigma"):
        s[k] = s[k].copy()
    moves = [(CLOSE_B, np.array([0.6, -0.64, 0.48]), np.array([3.0, -2.0, 0.0]))]
    if three:
        moves.append((CLOSE_C, np.array([-0.36, 0.48, 0.8]), np.array([0.0, -5.0, 1.0])))
    for first, direction, boxes in moves:
        s["pos"][first:first + 5] += s["pos"][CLOSE_A] + dist * direction + boxes * L - s["pos"][first]
    for a in (CLOSE_A, CLOSE_B, CLOSE_C)[:3 if three else 2]:
        s["alpha"][a] = synth.BSSP_SITES[0][4]
        s["epsilon"][a] = s["sigma"][a] = 0.0
    return s


def _coincident():
    """the centre of molecule 7 ON the centre of molecule 0 (rimg == 0: T = 0 for the pair).  Both sites carry neither
    charge nor Lennard-Jones parameters, so that no other term divides by that distance."""
    s = _close(0.0, False)
    s["charge"] = s["charge"].copy()
    s["pos"][CLOSE_B] = s["pos"][CLOSE_A]
    s["charge"][[CLOSE_A, CLOSE_B]] = 0.0
    return s


def shifted(s, nbox=10000):
    """every movable molecule moved by its own multiple (~nbox) of lattice vectors, as test_gpu_pinning.shifted does"""
    s2 = dict(s)
    pos = s["pos"].copy()
    rng = np.random.default_rng(11)
    mol = np.asarray(s["molecule"])
    for m in np.unique(mol[np.asarray(s["frozen"]) == 0]):
        k = rng.integers(-nbox, nbox + 1, size=3).astype(np.float64)
        k[rng.integers(3)] = float(nbox)
        pos[mol == m] += k @ s["basis"]
    s2["pos"] = pos
    return s2


def _sheared_pol():
    """S-POL(640) in the sheared cell of test_gpu_parity.test_triclinic_box_polarizable: 384 sites = 6 blocks, the
    general (non-orthorhombic) branch of the image arithmetic in every multi-block kernel"""
    s = dict(synth.s_pol(640))
    L = s["basis"][0, 0]
    s["basis"] = np.array([[L, 0, 0], [0.3 * L, 0.9 * L, 0], [-0.2 * L, 0.25 * L, 0.85 * L]])
    return s


SPECIAL = {
    "sheared_640": _sheared_pol,
    "ties_sheared": lambda: _ties(True, 0.0),
    "ties_sheared_shifted": lambda: _ties(True, 0.123456789),
    "close2_1e-1": lambda: _close(1e-1, False),
    "close2_1e-2": lambda: _close(1e-2, False),
    "close2_1e-3": lambda: _close(1e-3, False),
    "close3_1e-1": lambda: _close(1e-1, True),
    "close3_1e-2": lambda: _close(1e-2, True),
    "close3_1e-3": lambda: _close(1e-3, True),
    "coincident": _coincident,
    "far_10000": lambda: shifted(sized(129)),
    "mof5_frozen": lambda: dict(np.load(os.path.join(GOLD, "mof5_bssp_429.npz"))),
}
CLOSE = tuple(k for k in SPECIAL if k.startswith("close"))
# the cap on the bound (tests/test_polar_reference.py) holds on the regular cases: the close pairs are exempt by design
# (the cancellation in damp1 / r^3 IS the answer's uncertainty there), and so is far_10000 -- x_i - x_j of coordinates
# near 4e5 A is rounded to 2^-53 * 4e5 = 4e-11 A before anything else happens, in the reference too
REGULAR_SPECIAL = tuple(k for k in SPECIAL if k not in CLOSE and k != "far_10000")


def loose_bound(case, params):
    """Gauss-Seidel on the frozen framework: the worst-case recursion grows 172-fold per sweep there and the running bound
    reaches 9e-8 max|mu|, so the comparison is held to min(bound, 1e-11 max|vector|) instead (cap_of())"""
    return case == "mof5_frozen" and bool(params.get("polar_gs") or params.get("polar_gs_ranked"))


def cap_of(result):
    """{key: 1e-11 x the reference's largest component}; the field change is scaled by the induced field, as elsewhere"""
    big = lambda k: 1e-11 * float(np.abs(result[k]).max())
    return dict(mu=big("mu"), ef_induced=big("ef_induced"), ef_induced_change=big("ef_induced"))


def coincident_only():
    """the coincident case with every other alpha set to 0: a view of two sites whose only pair has rimg == 0, so the
    induced field is exactly 0 and every sweep leaves mu = alpha E (times polar_gamma at the start) to the bit"""
    s = dict(system("coincident"))
    alpha = np.zeros_like(s["alpha"])
    alpha[[CLOSE_A, CLOSE_B]] = s["alpha"][[CLOSE_A, CLOSE_B]]
    s["alpha"] = alpha
    return s


@functools.lru_cache(maxsize=None)
def system(name):
    """name: 'nv<count>', 'nv1345_moved', 'nv<count>_m<k>' (after the first k of lag_moves(count)) or a key of SPECIAL"""
    if name.startswith("nv") and "_m" in name and name.split("_m")[1].isdigit():
        nv, k = int(name[2:].split("_m")[0]), int(name.split("_m")[1])
        s = system("nv%d" % nv)
        out = dict(s)
        out["pos"] = s["pos"].copy()
        for _, first, shift, _ in lag_moves(nv)[:k]:
            out["pos"][first:first + 5] += shift
        return out
    if name == "nv1345_moved":
        s = system("nv1345")
        first, new = molecule_move(s)
        out = dict(s)
        out["pos"] = s["pos"].copy()
        out["pos"][first:first + 5] = new
        return out
    if name.startswith("nv"):
        return sized(int(name[2:]))
    return SPECIAL[name]()


def molecule_move(s, k=100, shift=(0.11, -0.07, 0.05)):
    """(first, new positions) of the k-th five-site molecule displaced rigidly"""
    first = 5 * k
    return first, np.asarray(s["pos"])[first:first + 5] + np.asarray(shift)


_LAG_SHIFTS = ((0.11, -0.07, 0.05), (-0.06, 0.09, 0.08), (0.05, 0.10, -0.07), (-0.09, -0.04, 0.10))


@functools.lru_cache(maxsize=None)
def lag_moves(nv):
    """Four rigid moves of one five-site molecule each, made one after the other on sized(nv) under plain Gauss-Seidel (the
    view is then the polarizable sites in atom order, 64 to a block): (label, first atom, displacement, view blocks of the
    molecule's polarizable sites).  A molecule all in block 0, one all in the middle block, the molecule of the last site,
    and one that straddles two inner blocks.  At 321 and 385 sites the last block holds ONE site, so no molecule lies in
    it alone: the molecule of that site reaches back into the block before it, which is asserted instead."""
    alpha = sized(nv)["alpha"]
    view = np.flatnonzero(alpha != 0.0)
    nt = (nv + 63) // 64
    blocks = {}
    for k, a in enumerate(view):
        blocks.setdefault(int(a) // 5, []).append(k // 64)
    sets = {m: tuple(sorted(set(b))) for m, b in blocks.items()}
    pick = lambda want: next(m for m in sorted(sets) if want(m, sets[m]))
    chosen = [("block 0", pick(lambda m, b: b == (0,) and len(blocks[m]) >= 2)),
              ("middle block", pick(lambda m, b: b == (nt // 2,) and len(blocks[m]) >= 2)),
              ("last block", int(view[-1]) // 5),
              ("two blocks", pick(lambda m, b: len(b) == 2 and 1 <= b[0] and b[1] < nt - 1))]
    assert len(set(m for _, m in chosen)) == 4, chosen
    assert nt - 1 in sets[chosen[2][1]], (nv, sets[chosen[2][1]])
    return tuple((label, 5 * m, np.array(shift), sets[m]) for (label, m), shift in zip(chosen, _LAG_SHIFTS))


@functools.lru_cache(maxsize=None)
def _small_tensor(name):
    return pref.Tensor(system(name), DAMP)


@functools.lru_cache(maxsize=3)  # 0.5 - 0.8 GB each: the three geometries above 1024 sites, and no more
def _large_tensor(name):
    return pref.Tensor(system(name), DAMP)


def tensor(name):
    if name.startswith("nv") and name[2:].isdigit() and int(name[2:]) in _ONE_LESS:
        nv = int(name[2:])
        return tensor("nv%d" % _ONE_LESS[nv]).without(dropped_atom(nv))
    large = int(np.count_nonzero(system(name)["alpha"])) > 1024
    return (_large_tensor if large else _small_tensor)(name)


def cpu_matrix():
    """(case name, variant name, params) of every comparison the GPU tests make"""
    out = []
    for nv in sorted(set(SMALL_SIZES) | set(RESIDENT_SIZES)):
        out.append(("nv%d" % nv, "jacobi4", JACOBI4))
    for it in DEFERRED_ITERS:
        out.append(("nv%d" % DEFERRED_SIZE, "jacobi%d" % it, dict(BASE, polar_max_iter=it)))
        out.append(("nv%d_moved" % DEFERRED_SIZE, "jacobi%d" % it, dict(BASE, polar_max_iter=it)))
    for nv in GS_SIZES:
        for name, p in GS_VARIANTS.items():
            out.append(("nv%d" % nv, name, p))
    for name, p in JACOBI_VARIANTS.items():
        out.append(("nv129", name, p))
    out.append(("sheared_640", "gs3", SHEARED_GS))
    # tests/test_gpu_gs_lags.py: gs_lags is an option of the engine, not a flag -- one row serves its three values
    for nv in GS_LAG_SIZES:
        for name, p in GS_LAG_VARIANTS.items():
            if ("nv%d" % nv, name, p) not in out:
                out.append(("nv%d" % nv, name, p))
    for nv in GS_LAG_MOVED_SIZES:
        for k in range(1, len(lag_moves(nv)) + 1):
            for name, p in GS_LAG_VARIANTS.items():
                out.append(("nv%d_m%d" % (nv, k), name, p))
    for name in SPECIAL:
        out.append((name, "jacobi4", JACOBI4))
        out.append((name, "production", PRODUCTION))
    return out


# ---------------------------------------------------------------------------------------------
# Ewald reciprocal / self energy: atom counts around the 64-atom blocks of the partial structure factors and past the 16
# reduction groups (1025 atoms = 17 blocks), a sheared cell, a frozen framework, far coordinates
# ---------------------------------------------------------------------------------------------
def _es_atoms(n):
    """the first n atoms of S-ES: rigid dimers, the last one cut in half when n is odd"""
    s = synth.s_es(2 * ((n + 1) // 2))
    return {k: (v if k == "basis" else v[:n].copy()) for k, v in s.items()}


def _es_sheared():
    s = synth.s_es(432)
    L = s["basis"][0, 0]
    s["basis"] = np.array([[L, 0, 0], [0.2 * L, 0.95 * L, 0], [0.1 * L, -0.15 * L, 0.9 * L]])
    return s


EWALD_CASES = {
    "es1": lambda: _es_atoms(1),
    "es63": lambda: _es_atoms(63),
    "es64": lambda: _es_atoms(64),
    "es65": lambda: _es_atoms(65),
    "es1025": lambda: _es_atoms(1025),
    "es432_sheared": _es_sheared,
    "mof5_frozen": SPECIAL["mof5_frozen"],
    "es65_far_10000": lambda: shifted(_es_atoms(65)),
}


@functools.lru_cache(maxsize=None)
def ewald_system(name):
    return EWALD_CASES[name]()


def ewald_move(s):
    """(first, new positions): the first movable molecule displaced rigidly"""
    mol = np.asarray(s["molecule"])
    first = int(np.flatnonzero(np.asarray(s["frozen"]) == 0)[0])
    count = int(np.count_nonzero(mol == mol[first]))
    return first, np.asarray(s["pos"])[first:first + count] + np.array([0.21, -0.13, 0.08])
