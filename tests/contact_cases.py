"""Inputs of the close-contact tests beyond one tile (tests/test_contact_cases.py on the CPU, tests/test_gpu_contacts.py on
the device): boxes of 63 .. 130 and of 2050 atoms whose close contacts are placed by hand, at the tile positions where
contact_tile_kernel (mpmc_amd/csrc/kernels_vdw.h), the dirty-block selection and the two reducers can go wrong.  A plain
helper module (no conftest).

How a box is made.  Molecules of 1, 2, 3 and 5 sites sit on a lattice of 4.5 A spacing (jitter 0.1 A, sites at most 0.7 A
from their centre): no two atoms of different background molecules come closer than 2.8 A, far above SCALE = 1.5 A.  Some
lattice sites stay vacant, and the designed atoms -- one-site molecules at chosen atom indices -- go there:

  * an ANCHOR (a one-site molecule at a vacant site, or a site of a molecule that lies across a 64-atom border) gets a
    partner SCALE - EDGE away along a unit vector (the pair counts) and a twin SCALE + EDGE away on the other side (the
    pair does not count); EDGE = 1.001e-9 A: 1e-9 A and a thousandth, so that the placement's rounding (1e-14 A) leaves
    the margin at 1e-9 A or above;
  * across a cell face, on each axis: an atom 0.5 A inside the face and its partner (or twin) 1.0 A beyond it, stored one
    lattice vector back, so that the pair needs the minimum image.

plan(n) says which atom indices those are, and why; every case lists its designed pairs in case["designed"] and the number
of them that count in case["count"].  tests/test_contact_cases.py proves on the CPU that the reference counts exactly
those, and that every case is DECISIVE: min |rimg - scale| over the different-molecule pairs >= 1e-9, before and after
every move the tests make.  The exact ties (ties()) are the designed exception.

The column position jj = j % 64 of a pair (i < j) on a DIAGONAL tile is at least 1, so jj = 0 is met on an off-diagonal
tile (column atom 64); jj = 63 needs atom 63 (or 127, ...) to be a one-site molecule, which it is at 64, 128 and 2050
atoms -- from 65 atoms on, atoms 63 and 64 belong to the molecule across the first border.
"""
import numpy as np

import tile_pass_cases as tp
import vdw_reference as vr
from mpmc_amd import synth

SCALE = 1.5
EDGE = 1.001e-9  # how far inside / outside the scale a designed pair is placed
MARGIN = 1e-9    # what "decisive" asks of min |rimg - scale|, in every configuration a test evaluates
SPACING = 4.5
SIZES = (63, 64, 65, 127, 128, 129, 130)
LARGE = 2050
BIG_SCALE = 1e3  # every different-molecule pair of present atoms counts
WIDE_SCALE = 12.0  # above half the shortest width of the sheared 130-atom box (10.2 A): only the minimum image decides
E1 = np.array([0.6, 0.0, 0.8])
E2 = np.array([-0.8, 0.0, 0.6])  # perpendicular to E1 and to the axis (y) of the molecules across a border
FLAGS = dict(temperature=150.0)  # Lennard-Jones + Ewald, no polarization
SHEARED = np.array([[1.0, 0, 0], [0.3, 0.9, 0], [-0.2, 0.25, 0.85]])  # tests/adversarial.py's sheared cell, per unit length
_TET = np.array([[1.0, 1.0, 1.0], [1.0, -1.0, -1.0], [-1.0, 1.0, -1.0], [-1.0, -1.0, 1.0]]) / np.sqrt(3.0)
# site offsets (A) of the background molecules, before their rotation
_SHAPES = {1: np.zeros((1, 3)), 2: np.array([[0, -0.35, 0], [0, 0.35, 0.0]]),
           3: np.array([[0, -0.7, 0], [0, 0, 0], [0, 0.7, 0.0]]), 5: np.concatenate([np.zeros((1, 3)), 0.6 * _TET])}
_CHARGES = {1: [0.0], 2: [0.3, -0.3], 3: [-0.2, 0.4, -0.2], 5: [-0.4, 0.1, 0.1, 0.1, 0.1]}


def plan(n):
    """What is placed by hand in a box of n atoms.
    straddlers: [(first atom, sites, frozen)]  molecules across a 64-atom border, sites 0.7 A apart along y;
    anchors:    [(name, anchor atom, direction, partner, twin, frozen atoms)]  partner / twin may be None;
    faces:      [(axis, inside atom, partner atom, counted)]  pairs across a cell face."""
    used, strad, anchors, faces = set(), [], [], []
    last = n - 1

    def take(block, lo=0, hi=64):
        """the lowest free atom index of a 64-atom block (between lanes lo and hi), else of any block from the top"""
        cand = list(range(64 * block + lo, min(64 * block + hi, n))) + list(range(n - 1, -1, -1))
        for a in cand:
            if a not in used:
                used.add(a)
                return a
        raise RuntimeError("no free atom")

    if 65 <= n < 129:
        strad.append((63, 2, False))   # the one border: a movable molecule across it
    elif n >= 129:
        strad.append((63, 2, True))    # a frozen molecule across the first border,
        strad.append((126, 3, False))  # a movable one across the second
    for first, k, _ in strad:
        used.update(range(first, first + k))

    def anchor(name, c, e, lo_block, frozen=(), slice_lo=0):
        if c not in used:
            used.add(c)
        a = take(lo_block, slice_lo)
        b = take(lo_block)
        anchors.append((name, c, e, a, b, tuple(frozen)))
        return a, b

    # the diagonal tile of block 0: column atoms at both ends of the waves' slices of eight
    reserved = {7, 8, 31, 56, last, last - 1} | ({63} if n == 64 else set())
    used |= {c for c in reserved if 0 <= c < n}
    for c in (7, 8, 31, 56):
        anchor("diag jj=%d" % c, c, E1, 0)
    # the last two real atoms, on a diagonal tile in front of the padding (jj = 63 at 64 and 128 atoms)
    if last % 64 >= 1 and not any(first <= last - 1 < first + k for first, k, _ in strad):
        anchors.append(("last two", last, E2, last - 1, take(last // 64), ()))
    if n >= 65:
        # tile (0, 1): the column atom 64 (jj = 0, wave 0) is a site of the molecule across the border, the row atom sits
        # in the last slice of eight of block 0 -- the lower-indexed atom in the higher wave slice
        anchor("blocks 0-1, jj=0, row in slice 7", 64, E1, 0, slice_lo=56)
    if n >= 129:
        # the tile of the first and the last block
        if n == 130:  # the last two real atoms: 128 (a site of the movable molecule across the border) and 129
            anchors.append(("last two", 128, E2, 129, take(1), ()))
        anchor("first and last block", 128 if n == 129 else last, E1, 0)
    if n > 1000:
        for jj in (7, 8, 31, 56, 63):  # a diagonal tile in the middle of the grid, jj = 63 included
            anchor("block 5 diag jj=%d" % jj, 320 + jj, E1, 5)
        # movers for the incremental passes (see contact_moves()): partners in a lower and in a higher clean block
        for name, c, lo in (("mover block 20", 1290, 3), ("mover block 9", 600, 31)):
            used.add(c)
            a, b = take(lo), take(32 if lo == 3 else 12)
            anchors.append((name, c, E1, a, b, ()))
    # frozen-frozen on different molecules (counts), frozen-movable (counts)
    hi = (n - 1) // 64
    c = take(hi)
    a, b = take(0), take(hi)
    anchors.append(("frozen-frozen", c, E1, a, b, (c, a, b)))
    c = take(hi)
    a, b = take(0), take(hi)
    anchors.append(("frozen-movable", c, E1, a, b, (c,)))
    if n >= 129:
        # movers of the incremental passes: a one-site molecule of block 1 with its partner in block 0 and its twin in
        # block 1, and one of block 0 with partner and twin in block 1
        c = take(1)
        anchors.append(("mover block 1", c, E1, take(0), take(1), ()))
        c = take(0)
        anchors.append(("mover block 0", c, E1, take(1), take(1), ()))
    for axis in range(3):
        for counted in (True, False):
            faces.append((axis, take(0 if counted else hi), take(hi if counted else 0), counted))
    return dict(straddlers=strad, anchors=anchors, faces=faces, designed_atoms=sorted(used))


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q


def build(n, cell="cubic", seed=None):
    """One case: dict(system, flags, designed = [(i, j, counted)], count, plan, n, cell)."""
    p = plan(n)
    rng = np.random.default_rng(9100 + n if seed is None else seed)
    designed_atoms = set(p["designed_atoms"])
    strad_first = {first: (k, frz) for first, k, frz in p["straddlers"]}
    # ---- the molecules, in atom order: (first atom, sites, kind)
    mols, a, cyc = [], 0, 0
    while a < n:
        if a in strad_first:
            mols.append((a, strad_first[a][0], "straddler"))
            a += strad_first[a][0]
        elif a in designed_atoms:
            mols.append((a, 1, "designed"))
            a += 1
        else:
            k = (1, 2, 3, 5)[cyc % 4]
            cyc += 1
            while any((a + t) in designed_atoms or (a + t) >= n for t in range(k)):  # (shrinks to what fits)
                k = {5: 3, 3: 2, 2: 1}[k]
            mols.append((a, k, "background"))
            a += k
    anchor_of = {c for _, c, _, _, _, _ in p["anchors"]}
    placed_single = {x for _, _, _, a_, b_, _ in p["anchors"] for x in (a_, b_) if x is not None}
    placed_single |= {x for _, i, j, _ in p["faces"] for x in (i, j)}
    strad_atoms = {first + t for first, k, _ in p["straddlers"] for t in range(k)}
    site_owners = [m for m in mols if m[2] != "designed" or m[0] not in placed_single]
    # ---- the lattice: face vacancies first (two sites per face pair), then one site per owner
    need = len(site_owners) + 12
    m = max(5, int(np.ceil(need ** (1.0 / 3.0) - 1e-9)))
    L = SPACING * m
    basis = (np.diag([L, L, L]) if cell == "cubic" else L * SHEARED).astype(np.float64)

    def site(t):
        return ((np.asarray(t, dtype=np.float64) + 0.5) / m) @ basis

    face_sites, taken = {}, set()
    for axis in range(3):
        for g in range(2):
            others = [2 * g + 1, axis + 1]
            lo = tuple(others[:axis] + [0] + others[axis:])
            hi = tuple(others[:axis] + [m - 1] + others[axis:])
            face_sites[axis, g] = (lo, hi)
            taken |= {lo, hi}
    free = [t for t in np.ndindex(m, m, m) if t not in taken]
    order = rng.permutation(len(free))
    assert len(free) >= len(site_owners)
    pos = np.full((n, 3), np.nan)
    q, alpha, eps, sig, mass, mol, frozen = (np.zeros(n) for _ in range(7))
    owner_site = {}
    for k, (first, sites, kind) in enumerate(site_owners):
        c = site(free[order[k]])
        owner_site[first] = c
        if kind == "background":
            c = c + rng.uniform(-0.1, 0.1, 3)
            pos[first:first + sites] = c + _SHAPES[sites] @ _rotation(rng).T
        elif kind == "straddler":
            pos[first:first + sites] = c + _SHAPES[sites]
        else:
            pos[first] = c
    for k, (first, sites, kind) in enumerate(mols):
        sl = slice(first, first + sites)
        mol[sl] = k + 1
        q[sl] = _CHARGES[sites]
        mass[sl] = 12.0 if sites > 1 else 16.0
        centre = first + (sites == 3)
        eps[centre] = 30.0 if kind != "designed" else 10.0
        sig[centre] = 2.6 if kind != "designed" else 2.0
        if kind == "straddler":
            frozen[sl] = int(strad_first[first][1])
        if kind == "background" and sites in (1, 3, 5):
            alpha[centre] = 0.6
        if kind == "designed":  # (2 alpha / r^3 = 0.24 at 1.5 A: far from the polarization catastrophe)
            alpha[centre] = 0.4
    designed = []
    pending = list(p["anchors"])
    while pending:  # (an anchor may itself be the partner of another anchor: place in dependency order)
        rest = []
        for item in pending:
            name, c, e, a_, b_, frz = item
            if np.isnan(pos[c]).any():
                rest.append(item)
                continue
            if a_ is not None:
                if np.isnan(pos[a_]).any():
                    pos[a_] = pos[c] + (SCALE - EDGE) * e
                designed.append((min(a_, c), max(a_, c), True, name))
            if b_ is not None:
                pos[b_] = pos[c] - (SCALE + EDGE) * e
                designed.append((min(b_, c), max(b_, c), False, name + " (twin)"))
            for x in frz:
                frozen[x] = 1
        assert len(rest) < len(pending), [r[0] for r in rest]
        pending = rest
    for g, (axis, inside, partner, counted) in enumerate(p["faces"]):
        lo, _ = face_sites[axis, g % 2]
        u = basis[axis] / np.linalg.norm(basis[axis])
        frac = (np.asarray(lo, dtype=np.float64) + 0.5) / m
        frac[axis] = 0.5 / np.linalg.norm(basis[axis])
        pos[inside] = frac @ basis  # 0.5 A inside the face
        pos[partner] = pos[inside] - (SCALE - EDGE if counted else SCALE + EDGE) * u + basis[axis]
        designed.append((min(inside, partner), max(inside, partner), counted, "across face %d" % axis))
    assert not np.isnan(pos).any()
    s = synth._finish(pos, q, alpha, eps, sig, mass, mol.astype(np.int32), frozen.astype(np.int32), L)
    s["basis"] = basis
    return dict(system=s, flags=dict(FLAGS), designed=designed, count=sum(1 for d in designed if d[2]), plan=p, n=n,
                cell=cell, name="%s%d" % (cell, n))


_cases = {}


def case(n, cell="cubic"):
    """built once, never modified"""
    if (n, cell) not in _cases:
        _cases[n, cell] = build(n, cell)
    return _cases[n, cell]


CASES = [(n, "cubic") for n in SIZES] + [(65, "sheared"), (130, "sheared"), (LARGE, "cubic")]
ROUTE_CASES = [(130, "cubic"), (LARGE, "cubic")]
CASE_IDS = ["%s%d" % (c, n) for n, c in CASES]


def closed_form(molecule, present=None):
    """C(n, 2) - sum_k C(m_k, 2) over the present atoms: the different-molecule pairs"""
    molecule = np.asarray(molecule)
    if present is not None:
        molecule = molecule[np.asarray(present, dtype=bool)]
    n = len(molecule)
    _, m = np.unique(molecule, return_counts=True)
    return int(n * (n - 1) // 2 - (m * (m - 1) // 2).sum())


_refs = {}


def reference(s, scale, key=None, flags=FLAGS):
    """(count, margin) of vr.close_contacts; kept under `key` when one is given"""
    if key is None or (key, scale) not in _refs:
        r = vr.close_contacts(s, flags, scale)
        if key is None:
            return r
        _refs[key, scale] = r
    return _refs[key, scale]


def near(s, scale, width=1e-6, flags=FLAGS):
    """number of different-molecule pairs within `width` of the scale"""
    t = vr.contact_table(s, flags, scale)
    return int((np.abs(t["rimg"] - np.longdouble(scale)) < width).sum())


# ---- the moves of the incremental passes
def contact_moves(c):
    """[(first atom, new coordinates)] of ONE evaluation, highest block first: tile_pass_cases.moves() of the case (a
    molecule per 64-atom block; in the 2050-atom box only those of blocks 32, 20, 9, 2, 1 and 0 -- the dirty-block list
    holds 16) with the designed movers in place of whatever it picked in their blocks' neighbourhood.  A mover is the
    anchor of a triplet: it steps 2e-9 A from its partner towards its twin, which breaks one contact and makes another in
    the same evaluation -- with a lower and a higher clean block (2050 atoms: blocks 3 / 31 and 31 / 12), with another
    dirty block (the block-1 and block-0 movers, and atom 129 / 2049 whose partners are in block 0)."""
    s, p = c["system"], c["plan"]
    n = c["n"]
    movers = [a for a in p["anchors"] if a[0].startswith("mover") or a[0] == "first and last block"]
    mv = []
    designed = set(p["designed_atoms"]) - {x for first, k, _ in p["straddlers"] for x in range(first, first + k)}
    keep_blocks = None if n < 1000 else {32, 20, 9, 2, 1, 0}
    for first, new in tp.moves(s) if n < 1000 else _moves_of_blocks(s, keep_blocks):
        if not any((first + t) in designed for t in range(len(new))):
            mv.append((first, new))
    frozen = np.asarray(s["frozen"])
    for k, (name, cidx, e, a_, b_, _) in enumerate(movers):
        if frozen[cidx]:
            continue
        if any(first <= cidx < first + len(new) for first, new in mv):
            continue  # (a site of the movable molecule across the border: it moves with its molecule)
        # every second mover steps 1e-4 A across the line instead: both distances grow by 3.3e-9 A, the contact breaks and
        # none is made, so that the total changes and not only the tiles it is made of
        step = -2 * EDGE * e if k % 2 == 0 else np.array([0.0, 1e-4, 0.0])
        mv.append((cidx, s["pos"][cidx:cidx + 1] + step))
    mv.sort(key=lambda t: -(t[0] // 64))
    assert sum(len(new) for _, new in mv) <= tp.MAX_MOVED
    return mv


def _moves_of_blocks(s, blocks):
    """tile_pass_cases.moves() restricted to the molecules of some blocks (its own rule picks one per block of the whole
    box, more than one evaluation's dirty-block list takes)"""
    mol, frozen = np.asarray(s["molecule"]), np.asarray(s["frozen"])
    rng = np.random.default_rng(23)
    out = []
    for b in sorted(blocks, reverse=True):
        atoms = np.arange(64 * b, min(64 * (b + 1), len(mol)))
        for a in atoms:
            idx = np.flatnonzero(mol == mol[a])
            if frozen[a] or idx[0] != a or idx[0] // 64 != b:
                continue
            out.append((int(a), s["pos"][idx] + rng.uniform(-0.15, 0.15, 3)))
            break
    return out


def too_many_moves(c, count=40):
    """[(first atom, new coordinates)]: background molecules of more atoms than the MoveList holds (32), each stepping
    0.05 A -- the moves cannot ride in the pair launch -- plus the block-0 mover 1e-4 A across its line, which breaks its
    contact and makes none: the count changes"""
    s, p = c["system"], c["plan"]
    mol, frozen = np.asarray(s["molecule"]), np.asarray(s["frozen"])
    designed = set(p["designed_atoms"])
    out, atoms = [], 0
    for m in np.unique(mol):
        idx = np.flatnonzero(mol == m)
        if frozen[idx].any() or set(idx.tolist()) & designed:
            continue
        out.append((int(idx[0]), s["pos"][idx] + np.array([0.05, -0.03, 0.02])))
        atoms += len(idx)
        if atoms >= count:
            break
    assert atoms >= count
    name, cidx, e, _, _, _ = [a for a in p["anchors"] if a[0] == "mover block 0"][0]
    out.append((cidx, s["pos"][cidx:cidx + 1] + np.array([0.0, 1e-4, 0.0])))
    return out


def polarizable(s, limit=None):
    """the system with only its first `limit` polarizable sites left polarizable (None: all of them)"""
    alpha = np.array(s["alpha"])
    on = np.flatnonzero(alpha != 0.0)
    if limit is not None:
        alpha[on[limit:]] = 0.0
    return dict(s, alpha=alpha)


def all_polarizable(s, alpha=0.05):
    """the system with every atom polarizable: a view large enough for the Jacobi solve to defer its last sweeps.  alpha is
    small because sites of one molecule are 0.35 .. 0.7 A apart (2 alpha / r^3 = 0.3 at 0.7 A, before the damping)"""
    return dict(s, alpha=np.full(len(s["charge"]), alpha))


# ---- exact ties: a cubic cell of edge 16, coordinates multiples of 1/8, displacement (1.125, 0, 1.5) = 1.875 exactly
TIE_SCALE = 1.875


def ties():
    """Eight one-site molecules: a tie pair inside the cell (atoms 0, 1), one across the x face (atoms 2, 3), and four far
    from everything.  rimg == 1.875 exactly for both pairs, in fp64 and in longdouble."""
    pts = [(4.0, 4.0, 4.0), (5.125, 4.0, 5.5), (15.5, 10.0, 4.0), (0.625, 10.0, 5.5), (10.0, 4.0, 10.0), (4.0, 12.0, 12.0),
           (12.0, 12.0, 8.0), (8.0, 8.0, 14.0)]
    n = len(pts)
    z = np.zeros(n)
    s = synth._finish(np.array(pts), z, z, np.full(n, 10.0), np.full(n, 2.0), np.full(n, 16.0), np.arange(1, n + 1), z, 16.0)
    return s


# ---- designed contacts on a committed case of another mode
def with_contacts(s, scale, pairs=3, seed=3):
    """A copy of system s in which `pairs` movable molecules were translated so that one atom of each sits scale - 1e-9 A
    (even pairs) or scale + 1e-9 A (odd pairs) from an atom of another molecule in another 64-atom block where there is one.
    Whatever else the translation brings close is the reference's to count; decisiveness is checked by the caller."""
    rng = np.random.default_rng(seed)
    pos = np.array(s["pos"], dtype=np.float64)
    mol, frozen = np.asarray(s["molecule"]), np.asarray(s["frozen"])
    n = len(mol)
    movable = [m for m in np.unique(mol) if not frozen[mol == m].any() and (mol == m).sum() <= 5]
    rng.shuffle(movable)
    done, touched = 0, set()
    for m in movable:
        idx = np.flatnonzero(mol == m)
        j = int(idx[0])
        others = [a for a in range(n) if mol[a] != m and mol[a] not in touched and a // 64 != j // 64] or \
                 [a for a in range(n) if mol[a] != m and mol[a] not in touched]
        i = int(others[int(rng.integers(len(others)))])
        d = (scale - EDGE) if done % 2 == 0 else (scale + EDGE)
        pos[idx] += pos[i] + d * E1 - pos[j]
        touched |= {m, mol[i]}
        done += 1
        if done == pairs:
            break
    return dict(s, pos=pos)
