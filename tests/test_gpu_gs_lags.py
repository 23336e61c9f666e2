"""gs_chain_kernel's lag machinery (option gs_lags = 2, 3, 4: which cached matrices L(k)_t exist, how many auxiliary
workgroups a block has, the grid, the z-slices and pass widths of gs_block_inverse_kernel) against the numpy.longdouble
reference of tests/polar_reference.py, inside its derived bound, through make / evaluate / compare of
tests/test_gpu_polar_reference.py -- at the view sizes where a lag first has a source and the far-source loop first has
one and two (tests/polar_cases.py, GS_LAG_SIZES), after moves that make the builder redo single lags behind a moved block,
and across the rule that moves a view rebuilt as a whole in three consecutive calls to two lags.

The same comparisons run against the CPU oracle in tests/test_polar_reference.py (the rows of polar_cases.cpu_matrix():
gs_lags is an option of the engine, so one row serves its three values): no case can fail on its inputs alone."""
import numpy as np
import pytest

import polar_cases as pc
from test_gpu_polar_reference import compare, evaluate, make, sheared_moved_tensor

pytestmark = pytest.mark.gpu
GS = pc.GS_LAG_VARIANTS["gs"]
ENERGIES = ("energy", "polarization_energy", "rd_energy", "coulombic_energy")
VECTORS = ("mu", "ef_static", "ef_induced", "ef_induced_change")


def same_bits(a, b, what):
    """two (record, vectors) of evaluate(): every field of the record and every vector"""
    for k, v in a[0].items():
        assert v == b[0][k], (what, k, v, b[0][k])
    for k in VECTORS:
        assert np.array_equal(a[1][k], b[1][k]), (what, k, float(np.abs(a[1][k] - b[1][k]).max()))


# ---------------------------------------------------------------------------------------------
# 1. every lag count at the block-count edges
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(pc.GS_LAG_VARIANTS))
@pytest.mark.parametrize("lags", pc.GS_LAG_COUNTS)
@pytest.mark.parametrize("nv", pc.GS_LAG_SIZES)
def test_every_lag_count_at_the_block_count_edges(nv, lags, variant):
    """a fresh context and one evaluation: the whole-view build (z-slices 0 and 1, pass width min(t, gs_lags)) and the chain
    with gs_lags - 1 auxiliary workgroups per block"""
    case, p = "nv%d" % nv, pc.GS_LAG_VARIANTS[variant]
    e = make(pc.system(case), p, persistent_gs=1, gs_lags=lags)
    r, d = evaluate(e)
    assert e.timings()["resident_calls"] == 0  # (not the one-launch Jacobi solver)
    compare(case, "%s gs_lags=%d" % (variant, lags), p, r, d, e=e)
    e.close()


@pytest.mark.parametrize("nv", [129, 193, 257])
def test_the_lag_count_takes_effect_exactly_where_a_block_has_that_lag(nv):
    """The engine does not report how many lags a chain used, so that the option took effect shows in the only way it
    can: for gs_lags = a < b the dipoles differ in their bits when some block has a source a + 1 blocks in front of it
    (blocks - 1 >= a + 1: under a that source comes through the pair coefficients and M_t, under b through the cached
    L(a+1)_t) -- and are THE SAME bits when no block has.  The second half is an invariant: gs_lags enters the builder
    only as min(t, gs_lags) (which matrices of block t are built, in a pass of that many right-hand sides) and the chain
    only as min(t, gs_lags), t > gs_lags and k <= gs_lags && t >= k; with blocks - 1 <= a every block t has
    min(t, a) = min(t, b) = t, no far source and no lag beyond t under either value, so both run the same operations in
    the same order.  3 blocks: no two values differ; 4 blocks: 2 differs from 3 and 4, which agree; 5 blocks: all differ."""
    case, blocks = "nv%d" % nv, (nv + 63) // 64
    mu = {}
    for lags in pc.GS_LAG_COUNTS:
        e = make(pc.system(case), GS, persistent_gs=1, gs_lags=lags)
        mu[lags] = evaluate(e)[1]["mu"]
        e.close()
    for a in pc.GS_LAG_COUNTS:
        for b in pc.GS_LAG_COUNTS:
            if a < b:
                differ = blocks - 1 >= a + 1  # (3 blocks: no pair; 4 blocks: 2 against 3 and 4; 5 blocks: every pair)
                assert np.array_equal(mu[a], mu[b]) != differ, (case, a, b, "expected to differ: %s" % differ)


@pytest.mark.parametrize("lags", [2, 4])
def test_sheared_cell_under_the_other_lag_counts(lags):
    """six blocks in a sheared cell: the non-orthorhombic instantiations of the builder and the chain with the pass
    widths and z-slices that the default gs_lags = 3 does not reach, as a whole-view build and behind a moved molecule
    (the geometries and the move of test_gauss_seidel_in_a_sheared_cell: its tensors serve)"""
    s = pc.system("sheared_640")
    e = make(s, pc.SHEARED_GS, persistent_gs=1, gs_lags=lags)
    r, d = evaluate(e)
    compare("sheared_640", "gs3 gs_lags=%d" % lags, pc.SHEARED_GS, r, d)
    moved = dict(s)
    moved["pos"] = s["pos"].copy()
    moved["pos"][35:40] += np.array([0.31, -0.22, 0.17])
    e.update_atoms(35, moved["pos"][35:40])
    r, d = evaluate(e)
    e.close()
    compare("sheared_640_moved", "gs3 gs_lags=%d after update_atoms" % lags, pc.SHEARED_GS, r, d,
            tensor=sheared_moved_tensor(), system=moved)


# ---------------------------------------------------------------------------------------------
# 2. incremental chain data under every lag count
# ---------------------------------------------------------------------------------------------
def check_moves(nv):
    """the moves of polar_cases.lag_moves(nv), with the view blocks of each molecule's sites (from the view order, on the
    CPU) asserted to be the ones this test is about"""
    nt = (nv + 63) // 64
    moves = pc.lag_moves(nv)
    assert [m[3] for m in moves[:2]] == [(0,), (nt // 2,)], moves
    assert moves[2][3] == (nt - 2, nt - 1), moves  # (the last block holds one site: its molecule starts in the block before)
    b = moves[3][3]
    assert len(b) == 2 and b[1] == b[0] + 1 and 1 <= b[0] and b[1] < nt - 1, moves
    return moves


@pytest.mark.parametrize("lags", pc.GS_LAG_COUNTS)
@pytest.mark.parametrize("nv", pc.GS_LAG_MOVED_SIZES)
def test_chain_data_behind_a_moved_block_under_every_lag_count(nv, lags):
    """Plain Gauss-Seidel (the view is the polarizable sites in atom order), one context: a molecule in block 0 moves,
    then one in the middle block, then the molecule of the last site, then one whose sites lie in two blocks.  Behind a
    moved block b the builder redoes M_b and every L(k)_b in one pass and L(k)_{b+k} alone for k = 1 .. gs_lags (z-slice
    1 + k), as far as the view reaches.  Every evaluation is inside the reference's bound on the moved geometry and has
    every bit of a fresh context with the same gs_lags on it: each cached matrix is a function of the current
    coordinates, built by the same operations alone or with its block's others."""
    p, base = GS, "nv%d" % nv
    e = make(pc.system(base), p, persistent_gs=1, gs_lags=lags)
    r, d = evaluate(e)
    compare(base, "gs gs_lags=%d before the moves" % lags, p, r, d, e=e)
    for k, (label, first, _, blocks) in enumerate(check_moves(nv), 1):
        case = "%s_m%d" % (base, k)
        s = pc.system(case)
        what = "gs gs_lags=%d, moved: %s %s" % (lags, label, blocks)
        e.update_atoms(first, s["pos"][first:first + 5])
        r, d = evaluate(e)
        compare(case, what, p, r, d, e=e)
        fresh = make(s, p, persistent_gs=1, gs_lags=lags)
        want = evaluate(fresh)
        fresh.close()
        same_bits((r, d), want, (case, what))
    e.close()


@pytest.mark.parametrize("lags", pc.GS_LAG_COUNTS)
@pytest.mark.parametrize("nv", pc.GS_LAG_MOVED_SIZES)
def test_ranked_views_behind_the_same_moves_under_every_lag_count(nv, lags):
    """The same moves under the production flags (the molecules were chosen in atom order: in the ranked view their sites
    lie where the ranking puts them, and a move may change the ranked walk), each evaluation inside the reference's
    bound.  Bit for bit they are held where test_ranked_gauss_seidel_chain_keeps_its_view_incrementally holds its chain:
    the energies against a context that goes through the same calls and rebuilds everything in each of them -- in the
    calls in which the two run the same lag count.  That is every call under gs_lags = 2, and the first two under 3 and 4:
    a context that rebuilds its views as a whole in every call moves them to two lags at its third call
    (maintain_chain_data(), include/mpmc_hip.h "gs_lags"), and the sweeps of two and of three lags round differently
    (seen: U_pol of nv321_m2 one unit in the last place apart under gs_lags 3 and 4).  From that call on the
    rebuild-everything context must instead have the energy bits of a rebuild-everything context with gs_lags = 2,
    which by the first half has those of an incremental one."""
    p, base = pc.PRODUCTION, "nv%d" % nv
    kinds = [(1, lags), (0, lags)] + ([(0, 2)] if lags > 2 else [])  # (incremental, gs_lags)
    engs = [make(pc.system(base), p, incremental_amatrix=inc, incremental_pairs=inc, persistent_gs=1, gs_lags=n)
            for inc, n in kinds]
    cases = [(base, "before the moves", None)] + [("%s_m%d" % (base, k), "moved: " + m[0], m[1])
                                                  for k, m in enumerate(check_moves(nv), 1)]
    for call, (case, label, first) in enumerate(cases, 1):
        s = pc.system(case)
        if first is not None:
            for e in engs:
                e.update_atoms(first, s["pos"][first:first + 5])
        got = [evaluate(e) for e in engs]
        compare(case, "production gs_lags=%d, %s" % (lags, label), p, got[0][0], got[0][1], e=engs[0])
        same_count = lags == 2 or call <= 2
        a, b = (got[0][0], got[1][0]) if same_count else (got[1][0], got[2][0])
        for key in ENERGIES:
            assert a[key] == b[key], (case, lags, call, "same lag count" if same_count else "both at two lags", key, a[key], b[key])
    for e in engs:
        e.close()


# ---------------------------------------------------------------------------------------------
# 3. the switch to two lags of a view that is rebuilt as a whole in consecutive calls
# ---------------------------------------------------------------------------------------------
def edit_and_evaluate(e, s, first):
    """one grand-canonical step that changes nothing: the molecule at `first` leaves, comes back into its hole, the sweep
    order is stated anew -- and the ranked view is rebuilt as a whole"""
    sl = slice(first, first + 5)
    assert e.remove_molecule(first, 5)
    assert e.insert_molecule(s["pos"][sl], s["charge"][sl], s["alpha"][sl], s["epsilon"][sl], s["sigma"][sl],
                             s["mass"][sl]) == first
    e.set_sweep_order(np.flatnonzero(s["alpha"] != 0.0))
    return evaluate(e)


def test_a_ranked_view_rebuilt_in_three_consecutive_calls_moves_to_two_lags():
    """include/mpmc_hip.h ("gs_lags") and maintain_chain_data(): a view keeps the option's lag count through two consecutive
    whole rebuilds and uses two lags from the third on.  Production flags, 321 sites (6 blocks: the blocks 3 .. 5 have a
    third lag), default options.  Call 1 is the evaluation of the upload (a whole build; the engine takes no edit before
    it); each of the calls 2 .. 4 removes a molecule, puts it back into its hole and states the order, which rebuilds the
    RANKED view as a whole.  Every call is inside the reference's bound.  From outside the rule shows as:
      calls 1 and 2 have every bit of a fresh context (default gs_lags = 3);
      call 3 -- the third whole rebuild in a row, the second edit -- does not have the dipoles of call 2; call 4 has every
      bit of call 3;
      a context with gs_lags = 2 has the bits of a fresh gs_lags = 2 context in all four calls -- so what changes at call 3
      is the lag count and nothing else of the call history.
    Call 3 is NOT held to the bits of a fresh gs_lags = 2 context, because that is no invariant: the lag count belongs to
    a view, and these edits rebuild only the ranked view as a whole.  The atom-order view, which the first sweep of every
    call walks, keeps the blocks in front of the first changed entry of the order (set_sweep_order) and with them its
    three lags; from call 3 on the context runs sweep 1 with three lags and sweeps 2 .. 4 with two, which no fresh
    context does (tests/test_gpu_edits.py holds a restored layout to a fresh engine at 2 blocks, where no lag count differs)."""
    case, p = "nv321", pc.PRODUCTION
    s = pc.system(case)
    first = pc.lag_moves(321)[1][1]
    fresh = {}
    for lags in (2, 3):
        e = make(s, p, gs_lags=lags) if lags == 2 else make(s, p)
        fresh[lags] = evaluate(e)
        e.close()
    assert not np.array_equal(fresh[2][1]["mu"], fresh[3][1]["mu"])
    for lags in (3, 2):
        live = make(s, p, gs_lags=2) if lags == 2 else make(s, p)
        calls = []
        for call in range(1, 5):
            r, d = evaluate(live) if call == 1 else edit_and_evaluate(live, s, first)
            compare(case, "production, gs_lags %s, whole rebuild %d in a row" % ("= 2" if lags == 2 else "default", call),
                    p, r, d, e=live)
            calls.append((r, d))
        live.close()
        if lags == 2:
            for call, got in enumerate(calls, 1):
                same_bits(got, fresh[2], "gs_lags=2 call %d" % call)
        else:
            same_bits(calls[0], fresh[3], "call 1")
            same_bits(calls[1], fresh[3], "call 2")
            assert not np.array_equal(calls[2][1]["mu"], calls[1][1]["mu"]), "the third whole rebuild in a row kept three lags"
            same_bits(calls[3], calls[2], "call 4")
