"""GPU tests of the cavity grid of cavity_bias (mpmc_amd/csrc/kernels_cavity.h through mpmc_hip_set_cavity_grid,
mpmc_hip_cavity_bin, mpmc_hip_cavity_update, mpmc_hip_cavity_point, mpmc_hip_download_cavity_grid) against the numpy
restatement tests/cavity_reference.py.  Everything the grid holds is an integer or a double formed by a stated sequence of
rounded operations: every comparison is == on integers or on the bits of doubles."""
import numpy as np
import pytest

import cavity_cases as cc
import cavity_reference as cr
from mpmc_amd import engine, synth

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.fixture(scope="module")
def eng():
    e = engine.Engine(64)
    yield e
    e.close()


def check_against_reference(e, basis, G, atoms, radius, darts):
    """bin + update on the device; grid positions, occupancy, open points in order, hits and every cavity_point against
    the reference.  Returns the number of open points."""
    pts = cr.grid_points(basis, G)
    occ = cr.occupancy(pts, atoms, radius)
    opened = cr.open_list(occ)
    e.cavity_bin(atoms)
    got = e.cavity_update(darts=darts)
    assert got == (len(opened), cr.dart_hits(pts, opened, darts, radius))
    d_occ, d_pos = e.cavity_grid()
    assert same_bits(d_pos, pts)
    assert d_occ.dtype == np.int32 and np.array_equal(d_occ, occ)
    for k, g in enumerate(opened):
        dg, dp = e.cavity_point(k)
        assert dg == g and same_bits(dp, pts[g])
    for bad in (-1, len(opened)):
        with pytest.raises(engine.EngineError, match="cavity_point: index"):
            e.cavity_point(bad)
    return len(opened)


@pytest.mark.parametrize("basis", sorted(cc.BASES))
@pytest.mark.parametrize("G", cc.GRIDS)
def test_grid_occupancy_open_list_and_darts(eng, basis, G):
    """every atom count of the fixtures on one grid (tests/test_cavity_reference.py checks that the fixtures have open and
    occupied points wherever that is possible)"""
    eng.set_box(cc.BASES[basis])
    for n in cc.ATOM_COUNTS:
        c = cc.case(basis, G, n)
        eng.set_cavity_grid(G, c["radius"])
        n_open = check_against_reference(eng, c["basis"], G, c["atoms"], c["radius"], c["darts"])
        if n == 0:
            assert n_open == G ** 3
        elif G > 1:
            assert 0 < n_open < G ** 3


def test_nothing_open_and_everything_open(eng):
    basis, G = cc.BASES["tric"], 7
    c = cc.case("tric", G, 65)
    eng.set_box(basis)
    eng.set_cavity_grid(G, 40.0)  # larger than the cell: every atom covers every point
    assert check_against_reference(eng, basis, G, c["atoms"], 40.0, c["darts"]) == 0
    assert eng.cavity_update(darts=c["darts"]) == (0, 0)
    with pytest.raises(engine.EngineError, match="outside the 0 open points"):
        eng.cavity_point(0)
    eng.set_cavity_grid(G, 2.0)
    assert check_against_reference(eng, basis, G, np.zeros((0, 3)), 2.0, c["darts"]) == G ** 3
    assert eng.cavity_update() == (G ** 3, 0)  # no darts: no hits


def test_the_comparison_at_its_edge(eng):
    """for 64 grid points an atom whose squared distance is the largest double below T (counted) and one with exactly T
    (not counted); the same for darts against a single open point"""
    rng = np.random.default_rng(17)
    basis, G, radius = cc.BASES["tric"], 5, 0.7  # neighbouring points are ~2.4 A apart: an atom is near one point only
    T = cr.threshold(radius)
    below = np.nextafter(T, 0.0)
    assert np.sqrt(below) < radius <= np.sqrt(T)
    pts = cr.grid_points(basis, G)
    chosen = rng.choice(G ** 3, 64, replace=False)
    inside = np.array([cc.on_threshold(pts[g], below, radius, rng) for g in chosen])
    outside = np.array([cc.on_threshold(pts[g], T, radius, rng) for g in chosen])
    for g, w_in, w_out in zip(chosen, inside, outside):
        assert cr.dist2(pts[g], w_in) == below and cr.dist2(pts[g], w_out) == T
    want = np.zeros(G ** 3, dtype=np.int32)
    want[chosen] = 1
    assert np.array_equal(cr.occupancy(pts, inside, radius), want)
    assert not cr.occupancy(pts, outside, radius).any()
    eng.set_box(basis)
    eng.set_cavity_grid(G, radius)
    eng.cavity_bin(inside)
    assert np.array_equal(eng.cavity_grid()[0], want)
    eng.cavity_bin(outside)
    assert not eng.cavity_grid()[0].any()
    # the same through the edit: the outside atoms enter (nothing changes), the inside atoms enter, then leave again
    assert eng.cavity_update(in_pos=outside[:16]) == (G ** 3, 0)
    assert eng.cavity_update(in_pos=inside[:16]) == (G ** 3 - 16, 0)
    assert np.array_equal(np.flatnonzero(eng.cavity_grid()[0]), np.sort(chosen[:16]))
    assert eng.cavity_update(out_pos=inside[:16]) == (G ** 3, 0)
    # darts against the one (open) point of a grid of one
    eng.set_cavity_grid(1, radius)
    p = cr.grid_points(basis, 1)[0]
    hit = np.array([cc.on_threshold(p, below, radius, rng) for _ in range(64)])
    miss = np.array([cc.on_threshold(p, T, radius, rng) for _ in range(64)])
    assert cr.dart_hits(p[None, :], np.array([0]), hit, radius) == 64
    assert cr.dart_hits(p[None, :], np.array([0]), miss, radius) == 0
    eng.cavity_bin(np.zeros((0, 3)))
    assert eng.cavity_update(darts=hit) == (1, 64)
    assert eng.cavity_update(darts=miss) == (1, 0)
    assert eng.cavity_update(darts=np.concatenate([miss, hit[:5], miss])) == (1, 5)


def test_edits_keep_the_occupancy_of_a_full_bin(eng):
    rng = np.random.default_rng(29)
    basis, G, radius = cc.BASES["tric"], cc.EDIT_GRID, cc.EDIT_RADIUS
    pts = cr.grid_points(basis, G)
    start, edits = cc.edit_sequence(basis)
    assert len(edits) == 40
    eng.set_box(basis)
    eng.set_cavity_grid(G, radius)
    assert eng.cavity_update() is None  # nothing binned yet
    eng.cavity_bin(start)
    for step, (kind, out, new, current) in enumerate(edits):
        got = eng.cavity_update(out_pos=out, in_pos=new)
        occ = cr.occupancy(pts, current, radius)
        assert got == (int((occ == 0).sum()), 0), (step, kind)
        assert np.array_equal(eng.cavity_grid()[0], occ), (step, kind)
    # a from-scratch bin of the current set on the device gives the same list
    before = [eng.cavity_point(k)[0] for k in range(got[0])]
    assert before == cr.open_list(occ).tolist()
    eng.cavity_bin(current)
    assert eng.cavity_update() == got
    assert [eng.cavity_point(k)[0] for k in range(got[0])] == before
    # 17 points either way answer 1 and change nothing
    seventeen = cc.positions_in_cell(basis, 17, rng)
    assert eng.cavity_update(in_pos=seventeen) is None
    assert eng.cavity_update(out_pos=seventeen) is None
    assert eng.cavity_update() == got
    # cavity_incremental = 0: every non-empty edit answers 1; the empty one runs
    eng.set_option("cavity_incremental", 0)
    assert eng.cavity_update(in_pos=seventeen[:1]) is None
    assert eng.cavity_update() == got
    eng.set_option("cavity_incremental", 1)
    assert np.array_equal(eng.cavity_grid()[0], occ)


def test_a_box_change_moves_the_points_and_drops_the_occupancy():
    s = synth.s_pol(160, spacing=4.5)
    flags = dict(synth.FLAGS_POL_JACOBI)
    e = engine.Engine(len(s["charge"]))
    e.set_cavity_grid(6, 2.5)  # before there is a box: the setting only
    e.load_system(s, flags)
    basis = np.array(s["basis"], dtype=np.float64).reshape(3, 3)
    assert same_bits(e.cavity_grid(occupancy=False)[1], cr.grid_points(basis, 6))
    e.cavity_bin(s["pos"])
    first = e.cavity_update()
    assert first is not None
    # set_box
    bigger = basis * 1.03125
    e.set_box(bigger)
    assert e.cavity_update() is None
    with pytest.raises(engine.EngineError, match="no occupancy"):
        e.cavity_grid()
    assert same_bits(e.cavity_grid(occupancy=False)[1], cr.grid_points(bigger, 6))
    e.cavity_bin(s["pos"])
    assert e.cavity_update() == (len(cr.open_list(cr.occupancy(cr.grid_points(bigger, 6), s["pos"], 2.5))), 0)
    # scale_box (one displacement per molecule of the upload)
    n_mol = len(np.unique(s["molecule"]))
    e.energy()
    assert e.scale_box(basis, np.zeros((n_mol, 3)))
    assert e.cavity_update() is None
    assert same_bits(e.cavity_grid(occupancy=False)[1], cr.grid_points(basis, 6))
    e.cavity_bin(s["pos"])
    assert e.cavity_update() == first
    e.close()


def test_two_contexts_keep_their_own_grids():
    a, b = engine.Engine(64), engine.Engine(64)
    ca, cb = cc.case("ortho", 7, 65), cc.case("tric", 5, 63)
    for e, c in ((a, ca), (b, cb)):
        e.set_box(c["basis"])
        e.set_cavity_grid(c["G"], c["radius"])
    a.cavity_bin(ca["atoms"])
    b.cavity_bin(cb["atoms"])
    want = {}
    for name, c in (("a", ca), ("b", cb)):
        pts = cr.grid_points(c["basis"], c["G"])
        opened = cr.open_list(cr.occupancy(pts, c["atoms"], c["radius"]))
        want[name] = (pts, opened, (len(opened), cr.dart_hits(pts, opened, c["darts"], c["radius"])))
    assert a.cavity_update(darts=ca["darts"]) == want["a"][2]
    assert b.cavity_update(darts=cb["darts"]) == want["b"][2]
    for k in range(20):  # interleaved picks
        for e, (pts, opened, _) in ((a, want["a"]), (b, want["b"])):
            g, p = e.cavity_point(k)
            assert g == opened[k] and same_bits(p, pts[g])
    assert a.cavity_update(darts=ca["darts"]) == want["a"][2]
    a.close()
    assert b.cavity_update(darts=cb["darts"]) == want["b"][2]
    b.close()


def test_upload_and_energy_leave_the_grid_alone_and_the_grid_leaves_the_energy_alone():
    s = synth.s_pol(160, spacing=4.5)
    flags = dict(synth.FLAGS_POL_JACOBI)
    plain = engine.Engine(len(s["charge"]))
    plain.load_system(s, flags)
    want = plain.energy()
    moved = np.array(s["pos"][:1]) + 0.05
    plain.update_atoms(0, moved)
    want_moved = plain.energy()
    plain.close()

    e = engine.Engine(len(s["charge"]))
    e.set_cavity_grid(6, 2.5)
    e.load_system(s, flags)
    pts = cr.grid_points(s["basis"], 6)
    occ = cr.occupancy(pts, s["pos"], 2.5)
    assert 0 < (occ == 0).sum() < 6 ** 3
    e.cavity_bin(s["pos"])
    first = e.cavity_update()
    assert first == (int((occ == 0).sum()), 0)
    assert e.energy() == want  # every term, ==
    e.upload(s)
    e.energy_begin()
    for call in (e.cavity_update, lambda: e.cavity_bin(s["pos"]), lambda: e.cavity_point(0), e.cavity_grid,
                 lambda: e.set_cavity_grid(6, 2.5)):
        with pytest.raises(engine.EngineError, match="between energy_begin"):
            call()
    assert e.energy_end() == want
    assert np.array_equal(e.cavity_grid()[0], occ) and e.cavity_update() == first
    e.update_atoms(0, moved)
    assert e.cavity_update(out_pos=s["pos"][:1], in_pos=moved) is not None  # between the move and its energy
    assert e.energy() == want_moved
    assert np.array_equal(e.cavity_grid()[0], cr.occupancy(pts, np.concatenate([moved, s["pos"][1:]]), 2.5))
    e.close()


def test_refusals_by_name():
    e = engine.Engine(16)
    with pytest.raises(engine.EngineError, match="cavity grid is off"):
        e.cavity_bin(np.zeros((1, 3)))
    with pytest.raises(engine.EngineError, match="cavity_grid 65 is not supported"):
        e.set_cavity_grid(65, 1.0)
    with pytest.raises(engine.EngineError, match="invalid cavity grid or radius"):
        e.set_cavity_grid(4, 0.0)
    e.set_cavity_grid(4, 1.0)
    with pytest.raises(engine.EngineError, match="no box set"):
        e.cavity_bin(np.zeros((1, 3)))
    e.set_box(cc.BASES["ortho"])
    with pytest.raises(engine.EngineError, match="no cavity_update"):
        e.cavity_point(0)
    lib = e.lib
    assert lib.mpmc_hip_cavity_update(e.ctx, 0, None, 0, None, 0, None, None, None) < 0
    assert b"null argument" in lib.mpmc_hip_last_error()
    assert lib.mpmc_hip_download_cavity_grid(e.ctx, None, None) < 0
    assert b"null argument" in lib.mpmc_hip_last_error()
    e.set_cavity_grid(0)
    with pytest.raises(engine.EngineError, match="cavity grid is off"):
        e.cavity_update()
    e.set_cavity_grid(64, 1.0)  # the largest grid: 1024 workgroups, the scan kernel's full reach
    e.cavity_bin(np.zeros((1, 3)))
    n_open, hits = e.cavity_update(darts=np.zeros((3, 3)))
    pts = cr.grid_points(cc.BASES["ortho"], 64)
    assert n_open == int((cr.dist2(pts, np.zeros(3)) >= cr.threshold(1.0)).sum()) and 0 < n_open < 64 ** 3
    g, p = e.cavity_point(n_open - 1)
    assert g == 64 ** 3 - 1 and same_bits(p, pts[g])
    assert hits == 0  # the origin is occupied, the open points are at least 1 A away
    e.close()
