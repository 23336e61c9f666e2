"""tests/polar_reference.py against closed forms, and the CPU oracle against it WITHIN ITS DERIVED BOUND on every case and
variant that tests/test_gpu_polar_reference.py runs on the device: this validates the reference and the constants of its
bound without a GPU, and pins the oracle's solver about three orders tighter than 1e-10 max|mu|.

The last tests break the reference's input to one comparison on purpose (one pair's image flipped on a tie, c5 of one
64 x 64 tile scaled by 1 + 1e-12, one H2E dipole scaled by 1 + 1e-9) and require the comparison to fail and to name the
pair."""
import copy

import numpy as np
import pytest

import pair_reference as pr
import polar_cases as pc
import polar_reference as pref
from mpmc_amd import synth
from oracle import oracle

LD = pref.LD
EPS_LD = float(np.finfo(LD).eps)
MATRIX = pc.cpu_matrix()
IDS = ["%s-%s" % (c, v) for c, v, _ in MATRIX]
_oracle = {}


def oracle_run(case, variant, params):
    if (case, variant) not in _oracle:
        _oracle[(case, variant)] = oracle.energy(pc.system(case), params, want_vectors=True)
    return _oracle[(case, variant)]


_solved = {}


def solved(case, variant, params):
    """the reference on the oracle's static field, once per case and variant"""
    if (case, variant) not in _solved:
        _solved[(case, variant)] = pref.solve(pc.tensor(case), pc.system(case), params,
                                              oracle_run(case, variant, params)["ef_static"])
    return _solved[(case, variant)]


def keys_of(params):
    return ("mu", "ef_induced") + (("ef_induced_change",) if params.get("polar_palmo") else ())


def energy_allowance(result, E, palmo):
    """what the dipoles' own bound adds to 1e-12 sum |terms|: 1/2 sum (|E| + |dE_ind|) err_mu + |mu| err_dE_ind"""
    a = 0.5 * float((np.abs(np.asarray(E)) * result["mu_err"]).sum())
    if palmo:
        a += 0.5 * float((np.abs(result["ef_induced_change"]).astype(np.float64) * result["mu_err"]).sum())
        a += 0.5 * float((np.abs(result["mu"]).astype(np.float64) * result["ef_induced_change_err"]).sum())
    return a


# ---------------------------------------------------------------------------------------------
# 1. the module against closed forms
# ---------------------------------------------------------------------------------------------
def two_sites(r, alpha=(0.9, 1.3), box=40.0):
    pos = np.array([[1.0, 2.0, 3.0], [1.0 + r, 2.0, 3.0]])
    z = np.zeros(2)
    return dict(pos=pos, charge=z, alpha=np.array(alpha), epsilon=z, sigma=z, mass=z + 1.0,
                molecule=np.array([1, 2], dtype=np.int32), frozen=np.zeros(2, dtype=np.int32), basis=np.diag([box] * 3))


def series_damp(u):
    """damp1 = exp(-u) sum_{k>=3} u^k / k!, damp2 = exp(-u) sum_{k>=4} u^k / k!: the same functions without cancellation"""
    u = LD(u)
    term, s3, s4 = LD(1), LD(0), LD(0)
    for k in range(1, 60):
        term = term * u / k
        if k >= 3:
            s3 += term
        if k >= 4:
            s4 += term
    return np.exp(-u) * s3, np.exp(-u) * s4


@pytest.mark.parametrize("r", [1e-3, 1e-2, 1e-1, 0.4])
def test_small_u_series_of_damp1_and_damp2(r):
    """the formula in longdouble loses eps_ld / damp to its own cancellation: 2^-11 of what fp64 loses, and counted here"""
    s = two_sites(r, alpha=(1.0, 1.0))
    t = pref.Tensor(s, pc.DAMP)
    rl = LD(s["pos"][1][0]) - LD(s["pos"][0][0])
    d1, d2 = series_damp(LD(pc.DAMP) * rl)
    c3, c5 = d1 / rl ** 3, d2 / rl ** 5
    want_xx, want_yy = c3 - 3 * c5 * rl * rl, c3
    for got, want, scale in ((t.T[0, 3], want_xx, float(c3) + 3 * float(c5 * rl * rl)), (t.T[1, 4], want_yy, float(c3))):
        allow = (4 * EPS_LD / float(d2) + 16 * EPS_LD) * scale
        assert abs(float(got - want)) <= allow, (r, float(got), float(want), allow)
    assert 4 * EPS_LD < 2.0 ** -9 * pref.C_DAMP * pref.UF  # (that loss is far inside the fp64 term of dT)
    assert t.T[0, 4] == 0 and t.T[1, 5] == 0
    # and the bound of the pair is the cancellation term: about (C_DAMP u) / r^3 on c3
    assert t.dT[1, 4] >= pref.C_DAMP * pref.UF / r ** 3 * 0.99


def test_undamped_limit():
    """damp r = 120: exp(-120) (1 + u + u^2/2 + u^3/6) < 1e-46, T is the bare dipole tensor"""
    s = two_sites(3.0)
    s["pos"][1] = [2.0, 4.5, 1.0]
    t = pref.Tensor(s, 40.0)
    d = s["pos"][0].astype(LD) - s["pos"][1].astype(LD)
    r = np.sqrt((d * d).sum())
    want = np.eye(3, dtype=LD) / r ** 3 - 3 * np.outer(d, d) / r ** 5
    assert np.abs(t.T[0:3, 3:6] - want).max() <= 8 * EPS_LD * float(1 / r ** 3)


def test_tensor_is_symmetric_to_the_bit_and_blocks_are_zero_on_the_diagonal():
    t = pc.tensor("nv129")
    assert np.array_equal(t.T, t.T.T) and np.array_equal(t.dT, t.dT.T)
    for k in range(t.nv):
        assert not t.T[3 * k:3 * k + 3, 3 * k:3 * k + 3].any()
    t = pc.tensor("ties_sheared_shifted")  # ties: (i, j) and (j, i) must take opposite images of the same pair
    assert np.array_equal(t.T, t.T.T) and np.array_equal(t.image, -t.image.transpose(1, 0, 2))


def test_two_sites_on_an_axis_reach_the_analytic_fixed_point():
    """mu_1 = a_1 (E_1 - t mu_2), mu_2 = a_2 (E_2 - t mu_1) per component, t_xx = (damp1 - 3 damp2) / r^3, t_yy = damp1 / r^3"""
    r, (a1, a2) = 2.5, (0.9, 1.3)
    s = two_sites(r, (a1, a2))
    t = pref.Tensor(s, pc.DAMP)
    E = np.array([[0.3, -0.2, 0.1], [-0.15, 0.25, 0.4]])
    rl = LD(s["pos"][1][0]) - LD(s["pos"][0][0])
    d1, d2 = series_damp(LD(pc.DAMP) * rl)
    for flags in (dict(polar_max_iter=80), dict(polar_max_iter=60, polar_gs=1), dict(polar_max_iter=80, polar_sor=1, polar_gamma=0.8)):
        res = pref.solve(t, s, dict(pc.BASE, **flags), E)
        for p, tt in enumerate(((d1 - 3 * d2) / rl ** 3, d1 / rl ** 3, d1 / rl ** 3)):
            e1, e2 = LD(E[0, p]), LD(E[1, p])
            m1 = a1 * (e1 - tt * LD(a2) * e2) / (1 - LD(a1) * LD(a2) * tt * tt)
            m2 = a2 * (e2 - tt * m1)
            assert abs(float(res["mu"][0, p] - m1)) <= 1e-17 and abs(float(res["mu"][1, p] - m2)) <= 1e-17, (flags, p)
        assert float(np.abs(res["mu_err"]).max()) < 1e-13


@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 7])
def test_early_publish_identity_from_the_modules_own_sweeps(n):
    """U_pol(n) = -1/2 sum [mu_m.E - (mu_m - mu_{m-1}).s_{n-m}], m = ceil(n / 2)"""
    s, t = pc.system("nv129"), pc.tensor("nv129")
    E = np.random.default_rng(n).normal(size=(len(s["alpha"]), 3))
    res = pref.solve(t, s, dict(pc.BASE, polar_max_iter=n), E, history=True)
    u, terms = pref.early_publish_energy(res)
    assert abs(float(u - res["upol"])) <= 64 * EPS_LD * float(terms)
    prev = pref.solve(t, s, dict(pc.BASE, polar_max_iter=n - 1), E)
    assert abs(float(prev["upol"] - res["upol"])) > 1e-9 * abs(float(res["upol"]))  # (the identity is not vacuous)


def test_ranking_follows_the_reference_on_a_hand_made_view():
    """rmin from rimg, the count from the UN-imaged r <= 1.5 rmin, ties keep atom order (stable), descending"""
    z = np.zeros(5)
    pos = np.array([[0.0, 0, 0], [1.0, 0, 0], [2.2, 0, 0], [19.5, 0, 0], [10.0, 5.0, 0]])  # 3 - 0 is 0.5 through the face
    s = dict(pos=pos, charge=z, alpha=np.array([1.0, 1.0, 1.0, 1.0, 0.0]), epsilon=z, sigma=z, mass=z + 1,
             molecule=np.arange(5, dtype=np.int32), frozen=np.zeros(5, dtype=np.int32), basis=np.diag([20.0] * 3))
    t = pref.Tensor(s, pc.DAMP)
    assert t.rmin == 0.5
    metric = t.rank(s)  # r <= 0.75: no un-imaged pair is that close
    assert np.array_equal(metric, [0, 0, 0, 0, 0])
    s["pos"][3] = [0.5, 0.4, 0]  # rmin = |(0.5, 0.4)| = 0.640: pairs within 0.96 are 0-3 and 1-3
    t = pref.Tensor(s, pc.DAMP)
    metric = t.rank(s)
    assert np.array_equal(metric, [1, 1, 0, 2, 0])
    assert np.array_equal(pref.bubble_order(np.arange(5), metric), [3, 0, 1, 2, 4])


# ---------------------------------------------------------------------------------------------
# 2. the oracle within the bound, on every case and variant of the GPU tests
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,variant,params", MATRIX, ids=IDS)
def test_oracle_is_within_the_bound(case, variant, params):
    s, t = pc.system(case), pc.tensor(case)
    want = oracle_run(case, variant, params)
    res = solved(case, variant, params)
    ratios = pref.check(t, s, res, want, keys_of(params), what="%s:%s oracle" % (case, variant), zero_outside=False,
                        cap=pc.cap_of(res) if pc.loose_bound(case, params) else None)
    assert res["polar_iterations"] == want["polar_iterations"] and res["iter_success"] == want["iter_success"]
    if params.get("polar_gs_ranked"):
        assert np.array_equal(res["rank_metric"], want["rank_metric"])
        assert np.array_equal(res["ranked_array"], want["ranked_array"])
    d = abs(float(LD(want["polarization_energy"]) - res["upol"]))
    allow = 1e-12 * float(res["upol_terms"])
    if case in pc.CLOSE:  # the dipoles themselves are only known to their bound there (polar_cases.CLOSE)
        allow += energy_allowance(res, want["ef_static"], params.get("polar_palmo"))
    print("POLARREF oracle %s %s %s U_pol %.3g of its allowance" % (case, variant, " ".join(
        "%s %.3g" % kv for kv in sorted(ratios.items())), d / allow if allow else 0.0))
    assert d <= allow, (case, variant, want["polarization_energy"], float(res["upol"]), d, allow)


@pytest.mark.parametrize("nv", pc.GS_LAG_MOVED_SIZES)
def test_lag_moves_touch_the_view_blocks_they_are_named_for(nv):
    """the moves of tests/test_gpu_gs_lags.py: the blocks restated from the view order (polarizable sites in atom order,
    64 to a block), four different molecules, and each moved geometry differs from the one before in that molecule only"""
    s0 = pc.system("nv%d" % nv)
    view = np.flatnonzero(s0["alpha"] != 0.0)
    nt = (nv + 63) // 64
    assert len(view) == nv and nt in (6, 7)
    moves = pc.lag_moves(nv)
    assert len(set(first for _, first, _, _ in moves)) == 4
    for k, (label, first, shift, blocks) in enumerate(moves, 1):
        slots = [i for i, a in enumerate(view) if first <= a < first + 5]
        assert len(slots) >= 2 and tuple(sorted(set(i // 64 for i in slots))) == blocks, (label, slots)
        before, after = pc.system("nv%d_m%d" % (nv, k - 1) if k > 1 else "nv%d" % nv), pc.system("nv%d_m%d" % (nv, k))
        d = after["pos"] - before["pos"]
        assert np.array_equal(after["pos"][first:first + 5], before["pos"][first:first + 5] + shift) and shift.any()
        d[first:first + 5] = 0.0
        assert not d.any() and np.array_equal(after["alpha"], s0["alpha"])
    assert [m[3] for m in moves[:3]] == [(0,), (nt // 2,), (nt - 2, nt - 1)]  # (the last block holds one site)
    assert view[-1] // 5 == moves[2][1] // 5 and (nv - 1) // 64 == nt - 1 and nv % 64 == 1
    b = moves[3][3]
    assert len(b) == 2 and b[1] == b[0] + 1 and 1 <= b[0] and b[1] < nt - 1


def test_divergence_falls_back_to_alpha_E_at_128_iterations():
    s = synth.s_pol(320, spacing=3.0)
    s["alpha"] = s["alpha"] * 40.0
    p = dict(pc.BASE, polar_max_iter=0, polar_precision=1e-8)
    want = oracle.energy(s, p, want_vectors=True)
    with np.errstate(all="ignore"):
        res = pref.solve(pref.Tensor(s, pc.DAMP), s, p, want["ef_static"])
    assert res["iter_success"] == want["iter_success"] == 1 and res["polar_iterations"] == want["polar_iterations"] == 128
    assert np.abs(want["mu"] - res["mu"].astype(np.float64)).max() <= 2 * pref.UF * np.abs(want["mu"]).max()
    assert not res["ef_induced_change"].any()


def test_positions_to_energy_end_to_end():
    """E from pair_reference.sums() instead of the oracle's: the chain positions -> field -> dipoles -> U_pol exists in
    longdouble end to end.  The two fields differ by rounding; that difference enters as dE."""
    s = pc.system("nv129")
    for p in (pc.JACOBI4, pc.PRODUCTION, dict(pc.JACOBI4, polar_ewald=1)):
        want = oracle.energy(s, p, want_vectors=True)
        E = pr.sums(pr.pair_table(s, p), s, p)["ef_static"]
        dE = np.abs(E - want["ef_static"])
        assert dE.max() <= 1e-11 * np.abs(E).max()
        res = pref.solve(pc.tensor("nv129"), s, p, E, dE=dE)
        pref.check(pc.tensor("nv129"), s, res, want, keys_of(p), what="end to end", zero_outside=False)
        allow = 1e-12 * float(res["upol_terms"]) + energy_allowance(res, E, p.get("polar_palmo")) + \
            0.5 * float((np.abs(res["mu"]).astype(np.float64) * dE).sum())
        assert abs(float(LD(want["polarization_energy"]) - res["upol"])) <= allow


# ---------------------------------------------------------------------------------------------
# 3. conditions on the inputs (not measurements): a loose bound must not hide a failure
# ---------------------------------------------------------------------------------------------
def amplification(t, gs):
    """what one sweep of the worst-case recursion multiplies a bound by: ||alpha |T|~||_inf under Jacobi,
    ||(I - L)^-1 U||_inf of its strict triangles under Gauss-Seidel in atom order (later sites see the new bound of the
    earlier ones).  A property of the input alone."""
    A = np.repeat(t.alpha, 3)[:, None] * t.Tabs
    if gs:
        A = np.linalg.solve(np.eye(len(A)) - np.tril(A, -1), np.triu(A, 1))
    return float(np.abs(A).sum(axis=1).max()) if t.nv else 0.0


@pytest.mark.parametrize("case,variant,params", MATRIX, ids=IDS)
def test_the_bound_is_capped_on_regular_cases(case, variant, params):
    """largest bound <= 1e-11 max|mu| on every sized case and on the special geometries without a reason to exceed it.
    Exempt, each with its reason asserted on the input: the close pairs (dominated by the dT of the close pair: test
    below); coordinates near 4e5 A (x_i - x_j is rounded to 2^-53 |x| = 4e-11 A first, in any fp64 code); and
    Gauss-Seidel on the frozen framework, whose covalent distances make the worst-case recursion -- which cannot use the
    signs -- grow 172-fold per sweep (9e8 in four) while every other case stays below 10-fold; the true error does not
    grow like that, and the oracle sits at 3e-6 of that bound."""
    s, t = pc.system(case), pc.tensor(case)
    gs = bool(params.get("polar_gs") or params.get("polar_gs_ranked"))
    if case in pc.CLOSE:
        return
    if case == "far_10000":
        assert np.abs(s["pos"]).max() * pref.UF > 1e-11
        return
    if pc.loose_bound(case, params):
        assert amplification(t, True) > 100.0
        return
    if t.nv <= 129 or case == "mof5_frozen":  # (an O(nv^3) solve: the small inputs stand for their families)
        assert amplification(t, gs) < 10.0
    res = solved(case, variant, params)
    cap = 1e-11 * float(np.abs(res["mu"]).max())
    worst = float(res["mu_err"].max())
    assert worst <= cap, (case, variant, worst, cap)


@pytest.mark.parametrize("case", pc.CLOSE)
def test_close_pair_bounds_are_dominated_by_the_close_pairs_dT(case):
    s, t = pc.system(case), pc.tensor(case)
    E = oracle_run(case, "jacobi4", pc.JACOBI4)["ef_static"]
    full = pref.solve(t, s, pc.JACOBI4, E)
    t2 = copy.copy(t)
    t2.dT = t.dT.copy()
    slot = {a: k for k, a in enumerate(t.view)}
    close = [slot[a] for a in (pc.CLOSE_A, pc.CLOSE_B, pc.CLOSE_C) if a in slot and s["alpha"][a] != 0]
    pairs = [(i, j) for i in close for j in close if i != j and t.rimg[i, j] < 0.2]
    assert len(pairs) >= 2 and min(t.rimg[i, j] for i, j in pairs) <= float(case.split("_")[1]) * 1.001
    assert all(t.image[i, j].any() for i, j in pairs)  # across a cell face: the translation is not zero
    for i, j in pairs:
        t2.dT[3 * i:3 * i + 3, 3 * j:3 * j + 3] = 0.0
    rest = pref.solve(t2, s, pc.JACOBI4, E)
    assert float(rest["mu_err"].max()) <= 0.1 * float(full["mu_err"].max())


def test_coincident_pair_contributes_exactly_nothing():
    s, t = pc.system("coincident"), pc.tensor("coincident")
    slot = {a: k for k, a in enumerate(t.view)}
    i, j = slot[pc.CLOSE_A], slot[pc.CLOSE_B]
    assert t.rimg[i, j] == 0.0
    for m in (t.T, t.Tabs, t.dT):
        assert not m[3 * i:3 * i + 3, 3 * j:3 * j + 3].any() and not m[3 * j:3 * j + 3, 3 * i:3 * i + 3].any()


# ---------------------------------------------------------------------------------------------
# 4. a broken input fails its comparison and names the pair
# ---------------------------------------------------------------------------------------------
def test_flipped_image_on_a_tie_is_named():
    """atoms 0 and 36 of the sheared lattice differ by (1/2, 1/4, 0) in fractional coordinates: rint() decides between
    the images at -1/2 and +1/2 along the first lattice vector, and in this cell the two are different displacements
    (a . b != 0), so the tensor depends on the choice.  The reference is given the other one."""
    case = "ties_sheared"
    s, t = pc.system(case), pc.tensor(case)
    want = oracle_run(case, "jacobi4", pc.JACOBI4)
    i, j = 0, 36
    _, rb, _ = pr.pbc(s["basis"])
    frac = lambda d: np.array([sum(rb[q][p] * d[q] for q in range(3)) for p in range(3)])
    f = frac(t.d[i, j])
    assert abs(abs(f[0]) - 0.5) < 1e-12 and abs(abs(f[1]) - 0.25) < 1e-12, f  # a tie along direction 0, off its axis
    bad = pref.Tensor(s, pc.DAMP, flip=[(i, j, 0, int(np.sign(f[0])))])
    f2 = frac(bad.d[i, j])
    assert abs(f2[0] + f[0]) < 1e-12 and abs(f2[1] - f[1]) < 1e-12  # the tied image: -1/2 <-> +1/2, nothing else moved
    blk = (slice(3 * i, 3 * i + 3), slice(3 * j, 3 * j + 3))
    assert float(np.abs(bad.T[blk] - t.T[blk]).max()) > 1e-6 * float(np.abs(t.T[blk]).max())  # and T really differs
    others = np.ones((t.nv, t.nv), bool)
    others[i, j] = others[j, i] = False
    assert np.array_equal(np.repeat(np.repeat(others, 3, 0), 3, 1) * bad.T, np.repeat(np.repeat(others, 3, 0), 3, 1) * t.T)
    res = pref.solve(bad, s, pc.JACOBI4, want["ef_static"])
    with pytest.raises(AssertionError) as e:
        pref.check(bad, s, res, want, what="flipped")
    msg = str(e.value)
    print(msg)
    first = msg.split("\n")[1]
    assert ("pair (0, 36)" in first or "pair (36, 0)" in first) and "taking image" in first, msg


def test_a_component_that_is_not_a_number_is_outside_the_bound():
    case = "nv129"
    s, t = pc.system(case), pc.tensor(case)
    want = dict(oracle_run(case, "jacobi4", pc.JACOBI4))
    res = solved(case, "jacobi4", pc.JACOBI4)
    want["ef_induced"] = want["ef_induced"].copy()
    want["ef_induced"][t.view[5], 1] = np.nan
    with pytest.raises(AssertionError):
        pref.check(t, s, res, want, what="nan")


@pytest.mark.parametrize("flags", ["jacobi4", "production"])
def test_coincident_pair_alone_induces_exactly_nothing(flags):
    """a view of the two coincident sites only: T = 0, so ef_induced == 0 and mu == alpha E to the bit"""
    p = pc.JACOBI4 if flags == "jacobi4" else pc.PRODUCTION
    s = pc.coincident_only()
    want = oracle.energy(s, p, want_vectors=True)
    res = pref.solve(pref.Tensor(s, pc.DAMP), s, p, want["ef_static"])
    for got in (want, {k: np.asarray(res[k], dtype=np.float64) for k in ("mu", "ef_induced", "ef_induced_change")}):
        assert not got["ef_induced"][[pc.CLOSE_A, pc.CLOSE_B]].any()
        assert not got["ef_induced_change"][[pc.CLOSE_A, pc.CLOSE_B]].any()
        assert np.array_equal(got["mu"], s["alpha"][:, None] * want["ef_static"])
    assert np.abs(want["mu"]).max() > 0


def test_scaled_c5_of_one_tile_is_named():
    case = "nv129"
    s, t = pc.system(case), pc.tensor(case)
    want = oracle_run(case, "jacobi4", pc.JACOBI4)
    bad = pref.Tensor(s, pc.DAMP, c5_scale=(np.arange(0, 64), np.arange(64, 128), 1.0 + 1e-12))
    res = pref.solve(bad, s, pc.JACOBI4, want["ef_static"])
    with pytest.raises(AssertionError) as e:
        pref.check(bad, s, res, want, what="scaled c5")
    msg = str(e.value)
    print(msg)
    first = msg.split("\n")[1]
    blocks = sorted(int(w.split()[0]) for w in first.split(" = block ")[1:3])
    assert blocks == [0, 1] and "c5 part" in first, first  # the site and its partner sit in the two blocks of the scaled tile


def test_scaled_h2e_dipole_is_named():
    case = "nv129"
    s, t = pc.system(case), pc.tensor(case)
    want = dict(oracle_run(case, "jacobi4", pc.JACOBI4))
    h2e = int(np.flatnonzero(s["alpha"] == synth.BSSP_SITES[1][4])[7])
    want["mu"] = want["mu"].copy()
    want["mu"][h2e] *= 1.0 + 1e-9
    assert np.abs(want["mu"][h2e]).max() < 1e-2 * np.abs(want["mu"]).max()  # invisible to a bound scaled by max|mu|
    res = pref.solve(t, s, pc.JACOBI4, want["ef_static"])
    with pytest.raises(AssertionError) as e:
        pref.check(t, s, res, want, what="scaled H2E")
    msg = str(e.value)
    print(msg)
    assert ("atom %d component" % h2e) in msg and "pair (%d, " % h2e in msg, msg


# ---------------------------------------------------------------------------------------------
# 5. Ewald reciprocal and self energy (pair_reference.ewald_recip_energy / ewald_self_energy)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(pc.EWALD_CASES))
@pytest.mark.parametrize("kmax", [1, 7])
def test_oracle_ewald_energies_are_within_the_bound(case, kmax):
    s = pc.ewald_system(case)
    p = dict(temperature=100.0, ewald_kmax=kmax)
    want = oracle.energy(s, p)
    u, du = pr.ewald_recip_energy(s, p)
    d = abs(float(LD(want["es_recip"]) - u))
    print("POLARREF oracle ewald %s kmax %d es_recip %.3g of its bound (%.3g relative)" % (case, kmax, d / du, du / max(abs(float(u)), 1e-300)))
    assert d <= du, (want["es_recip"], float(u), d, du)
    us, nterms = pr.ewald_self_energy(s, p)
    assert abs(float(LD(want["es_self"]) - us)) <= 2 * nterms * np.spacing(abs(float(us)))
    nk = len(pr.kvector_list(kmax))  # the shapes the GPU tests want: fewer than 64 k-vectors, and no multiple of 64
    assert (nk < 64) if kmax == 1 else (nk > 64 and nk % 64 != 0)
