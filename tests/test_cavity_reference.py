"""CPU checks of the numpy restatement of the cavity grid (tests/cavity_reference.py) and of the fixtures the GPU tests use
(tests/cavity_cases.py): the restatement is the yardstick of tests/test_gpu_cavity.py, so its own corner cases are pinned
here against the definition written out the slow way."""
import numpy as np
import pytest

import cavity_cases as cc
import cavity_reference as cr


def test_a_grid_of_one_point_in_a_cubic_cell_sits_at_the_origin():
    for L in (10.0, 25.123, 1.0 / 3.0):
        pos = cr.grid_points(np.diag([L, L, L]), 1)
        assert pos.shape == (1, 3) and np.all(pos == 0.0)


def test_grid_points_follow_the_flat_index_and_the_formula():
    b = cc.BASES["tric"]
    G = 4
    pos = cr.grid_points(b, G)
    for i in range(G):
        for j in range(G):
            for k in range(G):
                c = [float(i + 1) / float(G + 1), float(j + 1) / float(G + 1), float(k + 1) / float(G + 1)]
                for p in range(3):
                    t = ((b[0][p] * c[0] + b[1][p] * c[1]) + b[2][p] * c[2])
                    t = t - 0.5 * b[0][p]
                    t = t - 0.5 * b[1][p]
                    t = t - 0.5 * b[2][p]
                    assert pos[(i * G + j) * G + k, p] == t


@pytest.mark.parametrize("radius", [1.0, 2.0, 2.5, 3.0, 4.0, 0.1, 1.0 / 3.0, np.sqrt(2.0), np.pi, 17.25, 1e-3, 123.456])
def test_threshold_brackets_the_radius(radius):
    T = cr.threshold(radius)
    assert np.sqrt(np.nextafter(T, 0.0)) < radius <= np.sqrt(T)
    # ... and it is within two ulps of the rounded square
    assert abs(T - radius * radius) <= 2 * np.spacing(radius * radius)


def test_threshold_decides_as_the_square_root_does():
    rng = np.random.default_rng(5)
    for radius in (1.0, 2.0, 2.7, np.sqrt(3.0)):
        T = cr.threshold(radius)
        s = T + np.spacing(T) * np.arange(-40, 41)  # the doubles around T
        assert np.array_equal(np.sqrt(s) < radius, s < T)
        s = rng.uniform(0.0, 2.0 * T, 2000)
        assert np.array_equal(np.sqrt(s) < radius, s < T)


def test_occupancy_equals_a_plain_triple_loop():
    b = cc.BASES["tric"]
    G, radius = 3, 1.3  # expected occupancy 150 * (4/3) pi R^3 / V = 0.6: open and occupied points
    rng = np.random.default_rng(11)
    atoms = cc.positions_in_cell(b, 150, rng)  # more than one 128-atom slab of the vectorised form
    pts = cr.grid_points(b, G)
    want = np.zeros(G ** 3, dtype=np.int32)
    for i in range(G):
        for j in range(G):
            for k in range(G):
                g = (i * G + j) * G + k
                for a in atoms:
                    r = 0.0
                    for p in range(3):
                        r += (pts[g, p] - a[p]) * (pts[g, p] - a[p])
                    if np.sqrt(r) < radius:
                        want[g] += 1
    got = cr.occupancy(pts, atoms, radius)
    assert np.array_equal(got, want) and 0 < (want == 0).sum() < G ** 3
    # the squared form the device uses gives the same counts
    T = cr.threshold(radius)
    assert np.array_equal((cr.dist2(pts[:, None, :], atoms[None, :, :]) < T).sum(axis=1), want)


def test_open_list_is_in_scan_order():
    occ = np.array([0, 2, 0, 0, 1, 0, 3, 0], dtype=np.int32)
    assert cr.open_list(occ).tolist() == [0, 2, 3, 5, 7]
    assert cr.open_list(np.ones(27, dtype=np.int32)).tolist() == []
    assert cr.open_list(np.zeros(8, dtype=np.int32)).tolist() == list(range(8))


def test_random_index_rounds_ties_to_even_and_counts_from_the_end():
    n = 11  # open - 1 = 10
    assert cr.random_index(n, 0.0) == 10
    assert cr.random_index(n, 0.5) == 5
    assert cr.random_index(n, 0.05) == 10                      # rint(0.5) = 0
    assert cr.random_index(n, 0.15) in (8, 9)                  # 10 * 0.15 rounds to 1.5 or just beside it ...
    assert cr.random_index(n, 0.15) == 10 - int(np.rint(10 * 0.15))
    assert cr.random_index(n, 0.25) == 8                       # rint(2.5) = 2: ties go to the even neighbour
    assert cr.random_index(n, 0.35) == 10 - int(np.rint(10 * 0.35))
    assert cr.random_index(n, np.nextafter(0.25, 1.0)) == 7    # just above the tie
    assert cr.random_index(n, np.nextafter(0.25, 0.0)) == 8
    assert cr.random_index(n, np.nextafter(1.0, 0.0)) == 0     # u -> 1
    assert cr.random_index(n, np.nextafter(0.95, 0.0)) == 1 and cr.random_index(n, 0.96) == 0
    assert cr.random_index(1, 0.7) == 0                        # one open point
    for u in np.random.default_rng(3).random(200):
        assert 0 <= cr.random_index(n, u) <= 10


def test_darts_and_volume():
    b = cc.BASES["ortho"]
    u = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.25, 0.75, 1.0 - 2.0 ** -53]])
    x = cr.dart_positions(b, u)
    assert np.array_equal(x[0], [-6.0, -6.5, -7.0]) and np.array_equal(x[1], [0.0, 0.0, 0.0])
    pts = cr.grid_points(b, 1)  # the origin
    assert cr.dart_hits(pts, cr.open_list(np.zeros(1)), x, 1.0) == 1
    assert cr.dart_hits(pts, cr.open_list(np.ones(1)), x, 1.0) == 0
    assert cr.cavity_volume(1, 3, 2184.0) == (1.0 / 3.0) * 2184.0


@pytest.mark.parametrize("basis", sorted(cc.BASES))
@pytest.mark.parametrize("G", cc.GRIDS)
@pytest.mark.parametrize("n", cc.ATOM_COUNTS)
def test_fixtures_have_open_and_occupied_points(basis, G, n):
    """What the GPU cases rely on: wherever it is possible at all -- more than one point, at least one atom -- some
    points are open and some are not.  (A grid of one point has 0 or 1 open points, and without atoms all are open.)"""
    c = cc.case(basis, G, n)
    pts = cr.grid_points(c["basis"], G)
    n_open = len(cr.open_list(cr.occupancy(pts, c["atoms"], c["radius"])))
    if n == 0:
        assert n_open == G ** 3
    elif G > 1:
        assert 0 < n_open < G ** 3
    if G > 1:  # some darts hit (one sphere of 1 A in 2200 A^3, a grid of one point, need not catch any of 500)
        assert cr.dart_hits(pts, cr.open_list(cr.occupancy(pts, c["atoms"], c["radius"])), c["darts"], c["radius"]) > 0


def test_edit_chain_covers_every_kind_and_keeps_open_and_occupied_points():
    basis = cc.BASES["tric"]
    pts = cr.grid_points(basis, cc.EDIT_GRID)
    start, edits = cc.edit_sequence(basis)
    assert len(edits) == 40 and {e[0] for e in edits} == set(cc.EDIT_KINDS)
    sizes = {max(len(out), len(new)) for _, out, new, _ in edits}
    assert min(sizes) >= 1 and max(sizes) == 16
    occ = cr.occupancy(pts, start, cc.EDIT_RADIUS)
    changed = 0
    for kind, out, new, current in edits:
        # the occupancy is an order-free integer sum: an edit is + entering - leaving
        occ = occ + cr.occupancy(pts, new, cc.EDIT_RADIUS) - cr.occupancy(pts, out, cc.EDIT_RADIUS)
        full = cr.occupancy(pts, current, cc.EDIT_RADIUS)
        assert np.array_equal(occ, full)
        assert 0 < (full == 0).sum() < cc.EDIT_GRID ** 3
        if kind == "same":
            assert np.array_equal(out, new)
        changed += kind != "same"
    assert changed == 30


def test_positions_on_either_side_of_the_radius_test():
    rng = np.random.default_rng(2)
    radius = 0.7
    T = cr.threshold(radius)
    below = np.nextafter(T, 0.0)
    pts = cr.grid_points(cc.BASES["tric"], 5)[:8]
    for p in pts:
        w_in = cc.on_threshold(p, below, radius, rng)
        w_out = cc.on_threshold(p, T, radius, rng)
        assert cr.dist2(p, w_in) == below and cr.dist2(p, w_out) == T
        assert cr.within(p, w_in, radius) and not cr.within(p, w_out, radius)
