"""Inputs of the cavity-grid tests: cells, seeded atom sets and darts, and the search for positions that sit exactly on
either side of the radius test.  Everything is generated (seeded), nothing is read from a file."""
import numpy as np

import cavity_reference as cr

BASES = {
    "ortho": np.array([[12.0, 0.0, 0.0], [0.0, 13.0, 0.0], [0.0, 0.0, 14.0]]),
    # sheared: no zero entry, so every product of the grid-point formula rounds
    "tric": np.array([[12.3, 0.7, -0.4], [2.1, 13.1, 0.9], [-1.3, 1.7, 14.2]]),
}
GRIDS = (1, 5, 7, 13)  # 343 points: two workgroups, the last one ragged; 2197 points: nine scan blocks
ATOM_COUNTS = (0, 1, 63, 65, 333)  # chunk edges of the 256-atom staging and of a 64-lane wave
N_DARTS = 500


def radius_for(n_atoms):
    """A radius at which a grid of more than one point has open and occupied points for this many atoms in these cells
    (~2200 A^3): the expected occupancy of a point, n * (4/3) pi R^3 / V, is 0.1 .. 1."""
    return {0: 2.0, 1: 4.0, 63: 2.0, 65: 2.0, 333: 1.0}[n_atoms]


def positions_in_cell(basis, n, rng):
    """n positions with fractional coordinates uniform in [-0.5, 0.5): what wrapall() leaves for molecules of one atom."""
    return cr.dart_positions(basis, rng.random((n, 3)))


def case(basis_name, G, n_atoms):
    """One fixture: basis, atoms [n, 3], radius, darts [N_DARTS, 3] (seeded by the case)."""
    basis = BASES[basis_name]
    rng = np.random.default_rng(1000 * G + n_atoms + (7 if basis_name == "tric" else 0))
    atoms = positions_in_cell(basis, n_atoms, rng)
    darts = cr.dart_positions(basis, rng.random((N_DARTS, 3)))
    return dict(basis=basis, G=G, atoms=atoms, radius=radius_for(n_atoms), darts=darts)


EDIT_KINDS = ("move", "insert", "remove", "same")
EDIT_GRID, EDIT_RADIUS = 7, 2.0  # the grid the edit chain is checked on (sheared cell)


def edit_sequence(basis, n_start=60, steps=40, seed=23):
    """A seeded chain of edits of a set of positions: moves of 1 .. 16 points, pure insertions, pure removals and points
    that leave and re-enter unchanged, the largest edit (16) included.  Returns the starting set [n_start, 3] and a list of
    (kind, out [k, 3], new [m, 3], set after the edit [n, 3])."""
    rng = np.random.default_rng(seed)
    current = list(positions_in_cell(basis, n_start, rng))
    start = np.array(current)
    edits = []
    for step in range(steps):
        kind = EDIT_KINDS[step % 4]
        k = 16 if step in (4, 5, 6, 7) else int(rng.integers(1, 17))
        if kind == "insert":
            out, new = [], list(positions_in_cell(basis, k, rng))
        else:
            picks = sorted(rng.choice(len(current), k, replace=False), reverse=True)
            out = [current.pop(i) for i in picks]
            if kind == "move":
                new = [w + rng.normal(0.0, 0.8, 3) for w in out]
            elif kind == "same":
                new = [w.copy() for w in out]
            else:
                new = []
        current += new
        edits.append((kind, np.array(out).reshape(-1, 3), np.array(new).reshape(-1, 3), np.array(current)))
    return start, edits


def on_threshold(point, target, radius, rng):
    """A position w with dist2(point, w) == target exactly (target ~ radius^2), found by bisection over the doubles of
    w[2]: with dx^2 + dy^2 ~ 0.95 radius^2 fixed, s = fl(fl(dx^2 + dy^2) + fl(dz^2)) is a monotone step function of dz
    whose steps are finer than an ulp of the target for dz < 0.3 radius (2 dz ulp(w) < ulp(target) and dz^2 < target / 8),
    so it takes every double on the way; should a rounding still skip the target, another direction is drawn."""
    point = np.asarray(point, dtype=np.float64)
    for _ in range(200):
        phi = rng.uniform(0.0, 2.0 * np.pi)
        rho = np.sqrt(0.95) * radius
        sx, sy, sz = rng.choice([-1.0, 1.0], 3)
        w = np.array([point[0] + sx * rho * np.cos(phi), point[1] + sy * rho * np.sin(phi), point[2]])
        near, far = point[2], point[2] + sz * 0.3 * radius  # dz = 0 and dz = 0.3 radius

        def s_of(z):
            return cr.dist2(point, np.array([w[0], w[1], z]))

        if not (s_of(near) < target <= s_of(far)):
            continue
        while True:  # invariant: s(near) < target <= s(far)
            mid = 0.5 * (near + far)
            if mid == near or mid == far:
                break
            if s_of(mid) < target:
                near = mid
            else:
                far = mid
        if s_of(far) == target:
            return np.array([w[0], w[1], far])
    raise AssertionError("no position with the wanted squared distance found")
