"""CPU checks of the test-side Axilrod-Teller reference (tests/at_reference.py) and of the inputs the GPU tests use
(tests/at_cases.py): the literal ordered-triple loop against the unordered longdouble sum, hand-checked triangles, a
triple whose three minimum images do not close, and the condition the GPU cases have to meet."""
import numpy as np
import pytest

import at_cases
import at_reference as ref
from mpmc_amd import synth

CONV = ref.C9_NUM / ref.C9_DEN


def _three(pos, L, alpha=1.5, c9=300.0, mol=(1, 2, 3)):
    n = len(pos)
    return dict(pos=np.array(pos, dtype=np.float64), alpha=np.full(n, alpha), c9=np.full(n, c9), c6=np.full(n, 50.0),
                molecule=np.array(mol), basis=np.diag([L, L, L]).astype(np.float64))


@pytest.mark.parametrize("n", [12, 20])
@pytest.mark.parametrize("cell", ["cubic", "sheared"])
@pytest.mark.parametrize("mk", [False, True], ids=["c9", "midzuno_kihara"])
def test_literal_and_unordered_agree(n, cell, mk):
    s = synth.s_at(n)
    if cell == "sheared":
        s = ref.triclinic(s)
    a = ref.literal(s, mk)
    b = ref.unordered(s, mk)
    print("literal %.17g unordered %.17g sum|terms| %.6g" % (a, b.total, b.sum_abs))
    assert b.n_nonzero > 0 and b.sum_abs > 0.0
    assert abs(a - b.total) <= 1e-13 * b.sum_abs


def test_switched_off_sites_and_one_molecule_triples_give_exact_zeros():
    s = synth.s_at(20)
    n_active = int(np.sum((s["alpha"] != 0.0) & (s["c9"] != 0.0)))
    assert 0 < n_active < 20 and np.any(s["alpha"] == 0.0) and np.any((s["alpha"] != 0.0) & (s["c9"] == 0.0))
    act = np.flatnonzero((s["alpha"] != 0.0) & (s["c9"] != 0.0))
    mol = s["molecule"][act]
    same = sum(1 for a in range(len(act)) for b in range(a + 1, len(act)) for c in range(b + 1, len(act))
               if mol[a] == mol[b] == mol[c])
    assert same > 0  # the framework molecule has more than two atoms
    want = n_active * (n_active - 1) * (n_active - 2) // 6 - same
    assert ref.unordered(s).n_nonzero == want


def test_equilateral_triangle():
    r = 3.7
    s = _three([[0, 0, 0], [r, 0, 0], [0.5 * r, 0.5 * np.sqrt(3.0) * r, 0]], 100.0)
    want = 300.0 * CONV * (11.0 / 8.0) / r ** 9  # identical atoms: the mixed c9 is the atom's own
    assert ref.literal(s) == pytest.approx(want, rel=1e-13)
    assert ref.unordered(s).total == pytest.approx(want, rel=1e-13)


def test_collinear_triple():
    r = 3.1
    s = _three([[0, 0, 0], [r, 0, 0], [2 * r, 0, 0]], 100.0)
    want = 300.0 * CONV * (-2.0) / (r * r * 2 * r) ** 3
    assert ref.literal(s) == pytest.approx(want, rel=1e-13)
    assert ref.unordered(s).total == pytest.approx(want, rel=1e-13)


def test_three_on_one_molecule_is_excluded_and_two_are_not():
    pos = [[0, 0, 0], [3.0, 0, 0], [0, 3.5, 0]]
    assert ref.literal(_three(pos, 100.0, mol=(1, 1, 1))) == 0.0
    assert ref.unordered(_three(pos, 100.0, mol=(1, 1, 1))).n_nonzero == 0
    assert ref.literal(_three(pos, 100.0, mol=(1, 1, 2))) == ref.literal(_three(pos, 100.0, mol=(1, 2, 3))) != 0.0


def test_a_triple_whose_images_do_not_close_is_counted_as_it_is():
    # x = 0, 4, 8 in a 10 A cell: d_01 = -4, d_12 = -4 but d_02 = -8 + 10 = +2; d_01 + d_12 != d_02
    s = _three([[0, 0, 0], [4.0, 0, 0], [8.0, 0, 0]], 10.0)
    rb = ref.reciprocal(s["basis"])
    term, (dij, dik, djk) = ref.one_term(s["basis"], rb, s["pos"], s["alpha"], s["c9"], 0, 1, 2)
    assert dij[0] == -4.0 and djk[0] == -4.0 and dik[0] == 2.0
    assert not np.allclose(dij + djk, dik)
    # e_ij = -x, e_ik = +x, e_jk = -x: 1 - 3 (e_ij.e_ik)(e_ij.e_jk)(e_ik.e_jk) = 1 - 3 = -2, over (4 * 2 * 4)^3
    want = 300.0 * CONV * (-2.0) / (4.0 * 2.0 * 4.0) ** 3
    assert term == pytest.approx(want, rel=1e-13)
    assert ref.literal(s) == pytest.approx(want, rel=1e-13)
    assert ref.unordered(s).total == pytest.approx(want, rel=1e-13)


def test_periodic_cases_hold_triples_that_do_not_close():
    s = at_cases.case("n130")
    rb = ref.reciprocal(s["basis"])
    act = s["active"]
    open_triples = 0
    for a in range(len(act)):
        for b in range(a + 1, len(act)):
            for c in range(b + 1, len(act)):
                i, j, k = act[a], act[b], act[c]
                dij = ref.minimum_image(s["basis"], rb, s["pos"][i] - s["pos"][j])[0]
                djk = ref.minimum_image(s["basis"], rb, s["pos"][j] - s["pos"][k])[0]
                dik = ref.minimum_image(s["basis"], rb, s["pos"][i] - s["pos"][k])[0]
                open_triples += not np.allclose(dij + djk, dik, atol=1e-9)
    assert open_triples > 0


@pytest.mark.parametrize("name", at_cases.NAMES)
@pytest.mark.parametrize("mk", [False, True], ids=["c9", "midzuno_kihara"])
def test_gpu_cases_resolve_a_single_triple(name, mk):
    """The smallest non-zero |term| of every GPU case is at least 100 tolerances: one dropped or doubled triple fails."""
    s = at_cases.case(name)
    u = at_cases.reference(name, mk)
    tol = at_cases.TOLERANCE * u.sum_abs
    print("%s: %d sites, %d non-zero triples, smallest %.3g, sum|terms| %.6g, tolerance %.3g" %
          (name, len(s["active"]), u.n_nonzero, u.min_nonzero, u.sum_abs, tol))
    assert u.n_nonzero > 0
    assert u.min_nonzero >= at_cases.MARGIN * tol
    # the sites sit where the tiling can go wrong: both sides of every 64-atom boundary, the last two atoms, the framework
    n = len(s["alpha"])
    for b in range(64, n, 64):
        assert b - 1 in s["active"] and b in s["active"]
    assert {0, n - 2, n - 1} <= set(s["active"])
    assert sum(1 for a in s["active"] if s["frozen"][a]) >= 3
    assert any(s["molecule"][b - 1] == s["molecule"][b] for b in range(64, n, 64))  # a molecule across a boundary
    off = [i for i in range(n) if i not in s["active"]]
    assert np.all((s["alpha"][off] == 0.0) | ((s["c9"][off] == 0.0) & (s["c6"][off] == 0.0)))
