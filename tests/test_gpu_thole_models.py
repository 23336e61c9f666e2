"""The dipole tensors beside the exponential one on the device -- polar_damp_type linear, off / none, and exponential +
polar_wolf_full (mpmc_hip_set_thole_model) -- against the longdouble ModelTensor of tests/thole_models_reference.py, each
within that module's DERIVED bound: the downloaded A matrix entry by entry, then mu, ef_induced, ef_induced_change,
iteration count and flag on every solver path (each asserted to be the path taken, as tests/test_gpu_polar_reference.py
asserts it), U_pol to 1e-12 of its terms; incremental = fresh to the bit; the exact mode; the setting's persistence; and
the mpmc_hip driver on the golden inputs of tests/golden/thole_models/.

E is the engine's own downloaded ef_static, as in tests/test_gpu_polar_reference.py.  Every comparison prints a
`THOLEMODELS` line with max(diff / bound); profiles/thole_models/README.md keeps the largest."""
import functools
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import exact_reference as xr
import pair_reference as pr
import polar_cases as pc
import polar_reference as pref
import thole_models_reference as tm
from mpmc_amd import engine, host, synth

pytestmark = pytest.mark.gpu
LD = pref.LD
GOLD = os.path.join(os.path.dirname(__file__), "golden", "thole_models")
PRINTED = json.load(open(os.path.join(GOLD, "reference_energies.json")))

# model name -> (flags that select it, ModelTensor arguments)
MODELS = {
    "linear": (dict(polar_damp_type="linear"), dict(damping="linear")),
    "off": (dict(polar_damp_type="off"), dict(damping="off")),
    "wolf_full": (dict(polar_damp_type="exponential", polar_wolf_full=1, polar_wolf=1, polar_wolf_alpha=0.13),
                  dict(damping="exponential", wolf_full=True)),
}
NAMES = sorted(MODELS)


def flags_of(model, base):
    return dict(base, **MODELS[model][0])


def solver_params(params):
    """what polar_reference.solve() reads: the tensor's keywords are the tensor's (solve() asserts polar_wolf_full absent)"""
    return {k: v for k, v in params.items() if k not in ("polar_damp_type", "polar_wolf_full")}


def build_tensor(s, model, **kw):
    return tm.ModelTensor(s, pc.DAMP, **dict(MODELS[model][1], **kw))


@functools.lru_cache(maxsize=None)
def _small_tensor(case, model):
    return build_tensor(pc.system(case), model)


@functools.lru_cache(maxsize=1)  # 0.5 - 0.8 GB each above 1024 sites: one at a time (the tests below are ordered for it)
def _large_tensor(case, model):
    return build_tensor(pc.system(case), model)


def tensor(case, model):
    large = int(np.count_nonzero(pc.system(case)["alpha"])) > 1024
    return (_large_tensor if large else _small_tensor)(case, model)


def make(s, params, n=None, **opts):
    e = engine.Engine(len(s["charge"]) if n is None else n)
    e.load_system(s, params)
    for k, v in opts.items():
        e.set_option(k, v)
    return e


def keys_of(params):
    return ("mu", "ef_induced") + (("ef_induced_change",) if params.get("polar_palmo") else ())


def evaluate(e):
    r = e.energy()
    return r, e.dipoles()


def compare(case, model, path, params, r, d, e=None, deferred=False, t=None, s=None):
    s = pc.system(case) if s is None else s
    t = tensor(case, model) if t is None else t
    p = solver_params(params)
    res = pref.solve(t, s, p, d["ef_static"], history=deferred)
    what = "%s %s %s" % (model, case, path)
    ratios = pref.check(t, s, res, d, keys_of(p), what=what)
    if not p.get("polar_palmo"):
        assert not d["ef_induced_change"].any(), what
    assert r["polar_iterations"] == res["polar_iterations"] and r["iter_success"] == res["iter_success"], what
    if p.get("polar_gs_ranked") and e is not None:
        rank, order = e.ranking()
        assert np.array_equal(rank, res["rank_metric"]) and np.array_equal(order, res["ranked_array"]), what
    ratios["U_pol"] = pref.check_energy(res, r["polarization_energy"], what=what, deferred=deferred)
    print("THOLEMODELS %s | %s | %s | %s" % (model, case, path, " ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
    return res


def all_of(e, r=None):
    """every result field and the four per-atom vectors of one evaluation, as comparable python objects"""
    out = dict(e.energy() if r is None else r)
    for k, v in e.dipoles().items():
        out[k] = v.tobytes()
    return out


def fresh(s, params, **opts):
    e = make(s, params, **opts)
    try:
        return all_of(e)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------
# 1. the tensor itself: download_amatrix() (all atoms, alpha = 0 sites included) against amatrix(ModelTensor) within dT
# ---------------------------------------------------------------------------------------------
def cutoff_edge_system():
    """sized(65) with the centre of molecule 7 put rc (1 - 3e-10) from the centre of molecule 0 along x and that of
    molecule 14 rc (1 + 3e-10) along y (its minimum image is then 3e-10 rc INSIDE, on the other side): pairs within
    1e-9 rc of the cutoff on both sides of the half-box tie.  Pairs beyond rc (up to sqrt(3) rc) are there anyway: the A
    matrix has no cutoff."""
    s = dict(pc.sized(65))
    s["pos"] = s["pos"].copy()
    s["alpha"] = s["alpha"].copy()
    rc = 0.5 * s["basis"][0][0]
    for first, shift in ((pc.CLOSE_B, np.array([rc * (1 - 3e-10), 0.0, 0.0])), (pc.CLOSE_C, np.array([0.0, rc * (1 + 3e-10), 0.0]))):
        s["pos"][first:first + 5] += s["pos"][pc.CLOSE_A] + shift - s["pos"][first]
    for a in (pc.CLOSE_A, pc.CLOSE_B, pc.CLOSE_C):
        s["alpha"][a] = synth.BSSP_SITES[0][4]  # (sized() may have dropped them from the view)
    return s


AMATRIX_CASES = ["nv2", "nv65", "nv129", "sheared_640", "ties_sheared", "cutoff_edge"]


@pytest.mark.parametrize("case", AMATRIX_CASES)
@pytest.mark.parametrize("model", NAMES)
def test_amatrix_within_dT(model, case):
    s = cutoff_edge_system() if case == "cutoff_edge" else pc.system(case)
    t = build_tensor(s, model, all_sites=True)
    want, dA = pref.amatrix(t, s)
    e = make(s, flags_of(model, pc.JACOBI4))
    A = e.amatrix()
    e.close()
    assert np.array_equal(A, A.T), (model, case)
    diff = np.abs(A.astype(LD) - want).astype(np.float64)
    bad = np.argwhere(~(diff <= dA))  # (a NaN is outside)
    assert not len(bad), (model, case, "A outside dT", bad[:4], diff[tuple(bad[0])], dA[tuple(bad[0])], A[tuple(bad[0])])
    off_diagonal = ~np.eye(A.shape[0], dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.where((dA > 0) & off_diagonal, diff / dA, 0.0).max())  # (the diagonal is 1 / alpha: one rounding)
    assert np.abs(A[off_diagonal]).max() > 0
    note = ""
    if case == "cutoff_edge":
        rc = t.cutoff
        edge = np.abs(t.rimg - rc) <= 1e-9 * rc
        assert edge[pc.CLOSE_A, pc.CLOSE_B] and edge[pc.CLOSE_A, pc.CLOSE_C] and (t.rimg > rc * 1.2).any()
        note = " (%d pairs within 1e-9 rc of the cutoff, %d beyond it)" % (edge.sum() // 2, (t.rimg > rc).sum() // 2)
        if model == "wolf_full":  # there c3 all but cancels: the entry is far below either part, the bound is not
            i, j = 3 * pc.CLOSE_A, 3 * pc.CLOSE_B
            w1 = float(tm.wolf_constants(pc.DAMP, rc)[0])
            assert abs(A[i + 1, j + 1]) < 1e-8 * w1 / rc ** 3 and dA[i + 1, j + 1] > pref.UF * w1 / rc ** 3
    if model == "linear":
        note += " (%d pairs on the branch point r = s to a rounding)" % (t.near_tie.sum() // 2)
    if model == "off":  # the exclusions: one molecule, or either charge exactly 0.0 -- exact zeros
        mol, q = np.asarray(s["molecule"]), np.asarray(s["charge"])
        excl = (mol[:, None] == mol[None, :]) | (q[:, None] == 0.0) | (q[None, :] == 0.0)
        blocks = np.abs(A).reshape(len(q), 3, len(q), 3).max(axis=(1, 3))
        np.fill_diagonal(blocks, 0.0)
        assert not blocks[excl].any() and (blocks[~excl & ~np.eye(len(q), dtype=bool)] > 0).all()
    print("THOLEMODELS %s | %s | amatrix | A %.3g%s" % (model, case, ratio, note))


def test_linear_pairs_on_the_branch_point():
    """pairs at r = s to a rounding, and one ulp to either side: whichever way the device's pow() decides r < s, both
    factors are continuous there and the entry stays inside dT (which carries the damped branch's slope for such pairs)"""
    alpha = 0.6938
    s0 = pc.DAMP * (alpha * alpha) ** (1.0 / 6.0)
    for r in (np.nextafter(s0, 0.0), s0, np.nextafter(s0, 10.0)):
        s = tm.two_site(float(r), alpha, pc.DAMP, charge=(0.3 * synth.E2REDUCED, -0.3 * synth.E2REDUCED))
        t = build_tensor(s, "linear", all_sites=True)
        assert t.near_tie[0, 1]
        want, dA = pref.amatrix(t, s)
        e = make(s, flags_of("linear", pc.JACOBI4))
        A = e.amatrix()
        e.close()
        diff = np.abs(A.astype(LD) - want).astype(np.float64)
        assert np.all(diff <= dA), (r, diff.max(), A[0, 3], A[2, 5])
        print("THOLEMODELS linear | r = s %+d ulp | amatrix | A %.3g" % (
            round((r - s0) / np.spacing(s0)), max(diff[0, 3] / dA[0, 3], diff[2, 5] / dA[2, 5])))


def test_wolf_full_field_is_the_wolf_field_with_or_without_polar_wolf():
    """thole_field.c:32: under polar_wolf_full the static field is the Wolf field whether or not polar_wolf is set"""
    s = pc.system("nv65")
    base = dict(pc.JACOBI4, polar_damp_type="exponential", polar_wolf_full=1)
    a = fresh(s, dict(base, polar_wolf=1))
    b = fresh(s, base)
    plain = fresh(s, dict(pc.JACOBI4, polar_wolf=1))
    assert a == b
    assert a["ef_static"] == plain["ef_static"] and a["mu"] != plain["mu"]
    assert fresh(s, dict(base, polar_wolf_alpha=0.13))["ef_static"] == fresh(s, dict(pc.JACOBI4, polar_wolf=1, polar_wolf_alpha=0.13))["ef_static"]


# ---------------------------------------------------------------------------------------------
# 2. every solver path at its smallest size
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", NAMES)
def test_small_solver_paths(model):
    p = flags_of(model, pc.JACOBI4)
    # folded one-launch solver (65 sites = 2 blocks)
    e = make(pc.system("nv65"), p, resident_jacobi=1, resident_fold=16)
    r, d = evaluate(e)
    t = e.timings()
    e.close()
    assert t["resident_calls"] == 1 and t["resident_fallbacks"] == 0, t
    compare("nv65", model, "one launch, folded", p, r, d)
    # the coefficient store, one launch per sweep
    e = make(pc.system("nv65"), p, resident_jacobi=0, timing=2)
    r, d = evaluate(e)
    t = e.timings()
    e.close()
    assert t["resident_calls"] == 0 and t["sweep_count"] == 4, t
    compare("nv65", model, "coefficients, launch per sweep", p, r, d)
    # the expanded matrix: the symmetric (upper-triangle) sweep and the plain one
    for sym in (2, 0):
        e = make(pc.system("nv65"), p, pair_coefficients=0, symmetric_sweep=sym)
        r, d = evaluate(e)
        assert e.timings()["resident_calls"] == 0
        e.close()
        compare("nv65", model, "expanded matrix, symmetric_sweep=%d" % sym, p, r, d)
    # precision mode (the host reads the largest change after every sweep)
    pp = flags_of(model, pc.JACOBI_VARIANTS["precision"])
    e = make(pc.system("nv129"), pp)
    r, d = evaluate(e)
    assert e.timings()["resident_calls"] == 0
    e.close()
    res = compare("nv129", model, "precision", pp, r, d)
    assert 2 < r["polar_iterations"] < 128
    assert abs(r["dipole_rrms"] - res["dipole_rrms"]) <= 1e-9 * res["dipole_rrms"]


@pytest.mark.parametrize("model", NAMES)
def test_gauss_seidel_chain_and_literal_129(model):
    """ranked Gauss-Seidel + Palmo: the chain kernel on cached block inverses (persistent_gs = 1) and the literal
    substitution (0); that BOTH ran shows in their bits, as in tests/test_gpu_polar_reference.py"""
    p = flags_of(model, pc.PRODUCTION)
    mu = {}
    for persistent in (1, 0):
        e = make(pc.system("nv129"), p, persistent_gs=persistent)
        r, d = evaluate(e)
        assert e.timings()["resident_calls"] == 0
        compare("nv129", model, "ranked + Palmo persistent_gs=%d" % persistent, p, r, d, e=e)
        e.close()
        mu[persistent] = d["mu"]
    assert not np.array_equal(mu[1], mu[0]), (model, "persistent_gs 1 and 0 gave identical bits: one path ran twice?")


@pytest.mark.parametrize("model", NAMES)
def test_resident_with_finishers_and_chain_1025(model):
    """1025 sites = 17 blocks: the one-launch solver with finisher workgroups, and the multi-block Gauss-Seidel chain"""
    p = flags_of(model, pc.JACOBI4)
    e = make(pc.system("nv1025"), p, resident_jacobi=1, resident_fold=0)
    r, d = evaluate(e)
    t = e.timings()
    e.close()
    assert t["resident_calls"] == 1 and t["resident_fallbacks"] == 0, t
    compare("nv1025", model, "one launch, finishers", p, r, d)
    pg = flags_of(model, pc.PRODUCTION)
    e = make(pc.system("nv1025"), pg, persistent_gs=1)
    r, d = evaluate(e)
    assert e.timings()["resident_calls"] == 0
    compare("nv1025", model, "ranked + Palmo chain", pg, r, d, e=e)
    e.close()


@pytest.mark.parametrize("model", NAMES)
def test_deferred_sweeps_1345(model):
    """22 blocks: sweep + finish launches, the record published from sweep ceil(n / 2), the rest run on demand"""
    case = "nv%d" % pc.DEFERRED_SIZE
    for niter in pc.DEFERRED_ITERS:
        p = flags_of(model, dict(pc.BASE, polar_max_iter=niter))
        tail = niter - (niter + 1) // 2
        e = make(pc.system(case), p, timing=0)
        r = e.energy()
        assert e.timings()["pending_sweeps"] == tail and e.timings()["resident_calls"] == 0
        d = e.dipoles()
        assert e.timings()["pending_sweeps"] == 0
        e.close()
        compare(case, model, "deferred, %d sweeps" % niter, p, r, d, deferred=True)
    _large_tensor.cache_clear()


# ---------------------------------------------------------------------------------------------
# 3. the exact mode
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", [65, 153])
@pytest.mark.parametrize("model", NAMES)
def test_exact_cholesky(model, nv):
    """195 and 459 rows (both sides of the 64-row panel grid, one and three site blocks).  With A the REFERENCE matrix, n
    its rows and u = 2^-53: |A mu - E| <= n u (|A||mu| + |E|) + dT |mu| componentwise -- the backward bound of
    tests/test_gpu_exact.py plus what the device's matrix may differ from the reference's by; the forward bound follows
    through ||A^-1||_inf, and U_pol is held to 1e-12 of its terms."""
    case = "nv%d" % nv
    s, t = pc.system(case), tensor(case, model)
    p = flags_of(model, dict(pc.BASE, polar_iterative=0))
    e = make(s, p)
    r, d = evaluate(e)
    e.close()
    assert r["polar_iterations"] == 0 and r["iter_success"] == 0
    assert not d["ef_induced"].any() and not d["ef_induced_change"].any()
    A = tm.view_matrix(t)
    assert np.linalg.eigvalsh(A.astype(np.float64)).min() > 0.0
    E = d["ef_static"][t.view].reshape(-1)
    mu = d["mu"][t.view].reshape(-1)
    assert not d["mu"][np.asarray(s["alpha"]) == 0.0].any()
    res = np.abs(A @ mu.astype(LD) - E.astype(LD)).astype(np.float64)
    bound = xr.backward_bound(A, mu, E).astype(np.float64) + t.dT @ np.abs(mu)
    assert np.all(res <= bound), (model, case, float((res / bound).max()))
    ref = xr.solve(A, E.astype(LD))
    ninv = np.abs(np.linalg.inv(A.astype(np.float64))).sum(axis=1).max()
    err = float(np.abs(mu.astype(LD) - ref).max())
    assert err <= ninv * bound.max(), (model, case, err, ninv * bound.max())
    uref, terms = LD(-0.5) * (ref @ E.astype(LD)), LD(0.5) * np.abs(ref * E.astype(LD)).sum()
    assert abs(float(LD(r["polarization_energy"]) - uref)) <= 1e-12 * float(terms), (model, case)
    print("THOLEMODELS %s | %s | exact | backward %.3g forward %.3g U_pol %.3g" % (
        model, case, float((res / bound).max()), err / (ninv * bound.max()),
        abs(float(LD(r["polarization_energy"]) - uref)) / (1e-12 * float(terms))))


def _two_sites(r, alpha, charge=(0.0, 0.0), L=60.0):
    return tm.two_site(r, alpha, pc.DAMP, L=L, charge=charge)


@pytest.mark.parametrize("model", NAMES)
def test_polarizability_tensor_of_two_sites_is_the_closed_form(model):
    """C_xx = 2 alpha / (1 + alpha T_xx), C_zz = 2 alpha / (1 + alpha T_zz) with the model's T of the pair"""
    alpha, L = 1.1, 60.0
    # linear: inside the damped range (s = 2.1304 * 1.1^(1/3) = 2.2 A); off: charged sites on two molecules (not excluded)
    r = 1.7 if model == "linear" else 2.3
    s = _two_sites(r, alpha, charge=(0.3 * synth.E2REDUCED, -0.3 * synth.E2REDUCED), L=L)
    e = make(s, flags_of(model, dict(pc.BASE, polar_iterative=0)))
    try:
        e.energy()
        C = e.polarizability_tensor()
    finally:
        e.close()
    kw = MODELS[model][1]
    txx, tzz = tm.closed_forms(r, alpha, pc.DAMP, kw["damping"], kw.get("wolf_full", False), rc=L / 2)
    cxx, czz = float(2 * alpha / (1 + alpha * txx)), float(2 * alpha / (1 + alpha * tzz))
    print("THOLEMODELS %s | two sites | tensor | C_xx %.15g (%.15g) C_zz %.15g (%.15g)" % (model, C[0, 0], cxx, C[2, 2], czz))
    plain = [float(v) for v in xr.two_site_tensor(alpha, r, pc.DAMP)]
    assert abs(cxx - plain[0]) > 1e-6 * cxx or abs(czz - plain[1]) > 1e-6 * czz  # not the exponential model's numbers
    for got, want in ((C[0, 0], cxx), (C[1, 1], cxx), (C[2, 2], czz)):
        assert abs(got - want) <= 1e-13 * abs(want), (model, got, want)
    assert np.all(np.abs(C[~np.eye(3, dtype=bool)]) <= 1e-13 * cxx)


def test_off_polarization_catastrophe_is_reported_and_falls_back():
    """two charged single-atom molecules at r^3 = 1.5 alpha under `off`: 1/alpha - 2/r^3 < 0, no Cholesky factor --
    iter_success = 1 and the fallback dipoles alpha E"""
    alpha = 1.1
    r = (1.5 * alpha) ** (1.0 / 3.0)
    s = _two_sites(r, alpha, charge=(0.3 * synth.E2REDUCED, -0.3 * synth.E2REDUCED))
    e = make(s, flags_of("off", dict(pc.BASE, polar_iterative=0)))
    try:
        r1, d = evaluate(e)
        A = e.amatrix()
        assert np.linalg.eigvalsh(A).min() < 0.0 and abs(A[2, 5] + 2 / r ** 3) < 1e-14
        assert r1["iter_success"] == 1 and r1["polar_iterations"] == 0
        assert np.abs(d["ef_static"]).max() > 0.0
        assert np.array_equal(d["mu"], np.asarray(s["alpha"])[:, None] * d["ef_static"])
        with pytest.raises(engine.EngineError, match="not positive definite"):
            e.polarizability_tensor()
        # the same pair under the exponential model is positive definite: the catastrophe is the undamped tensor's
        e.set_thole_model("exponential")
        assert e.energy()["iter_success"] == 0
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------
# 4. incremental = fresh
# ---------------------------------------------------------------------------------------------
INCREMENTAL = {"jacobi": pc.JACOBI4, "production": pc.PRODUCTION, "exact": dict(pc.BASE, polar_iterative=0)}


@pytest.mark.parametrize("variant", sorted(INCREMENTAL))
@pytest.mark.parametrize("model", NAMES)
def test_update_atoms_and_scale_box_leave_the_bits_of_a_fresh_context(model, variant):
    s = pc.system("nv129")
    p = flags_of(model, INCREMENTAL[variant])
    e = make(s, p)
    try:
        before = all_of(e)
        assert before == fresh(s, p)
        first, new = pc.molecule_move(s, k=20)
        e.update_atoms(first, new)
        moved = dict(s, pos=s["pos"].copy())
        moved["pos"][first:first + 5] = new
        got, want = all_of(e), fresh(moved, p)
        assert got == want, (model, variant, "update_atoms", [k for k in got if got[k] != want[k]])
        assert got["polarization_energy"] != before["polarization_energy"]
        # a volume move: the store is rebuilt and, under polar_wolf_full, rc and the two Wolf constants with it
        mol = pr._molecule_index(s["molecule"])
        firsts = np.array([np.flatnonzero(mol == m)[0] for m in range(mol.max() + 1)])
        basis = np.asarray(s["basis"]) * 1.01
        delta = 0.01 * moved["pos"][firsts]
        assert e.scale_box(basis, delta)
        scaled = dict(moved, basis=basis, pos=moved["pos"] + delta[mol])
        got2, want2 = all_of(e), fresh(scaled, p)
        assert got2 == want2, (model, variant, "scale_box", [k for k in got2 if got2[k] != want2[k]])
        assert got2["polarization_energy"] != got["polarization_energy"]
    finally:
        e.close()


@pytest.mark.parametrize("model", NAMES)
def test_remove_and_insert_stay_within_the_bound(model):
    s = pc.system("nv129")
    p = flags_of(model, pc.JACOBI4)
    n = len(s["charge"])
    e = make(s, p, n=n + 64)
    try:
        e.energy()
        sl = slice(35, 40)  # molecule 7 leaves and comes back displaced to a gap in the lattice
        assert e.remove_molecule(35, 5)
        r, d = evaluate(e)
        hole = {k: (v.copy() if k != "basis" else v) for k, v in s.items()}
        for k in ("charge", "alpha", "epsilon", "sigma"):
            hole[k][sl] = 0.0
        compare("nv129 - molecule 7", model, "after remove_molecule", p, r, d, t=build_tensor(hole, model), s=hole)
        newpos = s["pos"][sl] + np.array([1.7, 1.9, -1.6])
        first = e.insert_molecule(newpos, s["charge"][sl], s["alpha"][sl], s["epsilon"][sl], s["sigma"][sl], s["mass"][sl])
        assert first is not None
        r, d = evaluate(e)
        slots = e.n
        assert d["mu"].shape[0] == slots
        back = {}
        for k, v in hole.items():
            if k == "basis":
                back[k] = v
                continue
            pad = np.zeros((slots - n,) + v.shape[1:], dtype=v.dtype)
            back[k] = np.concatenate([v, pad])
        back["molecule"][n:] = 10 ** 6 + np.arange(slots - n)  # (padding slots: every one its own empty molecule)
        back["pos"][first:first + 5] = newpos
        for k in ("charge", "alpha", "epsilon", "sigma", "mass"):
            back[k][first:first + 5] = s[k][sl]
        back["molecule"][first:first + 5] = 10 ** 7
        compare("nv129 + molecule 7 moved", model, "after insert_molecule", p, r, d, t=build_tensor(back, model), s=back)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------
# 5. the setting: persistence, and the default's bits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["jacobi", "production"])
def test_switching_models_and_back_restores_the_default_bits(variant):
    s = pc.system("nv129")
    p = INCREMENTAL[variant]
    want = fresh(s, p)  # a context never switched
    e = make(s, p)
    try:
        assert all_of(e) == want
        seen = {}
        for model in NAMES:
            kw = MODELS[model][1]
            e.set_thole_model(kw["damping"], kw.get("wolf_full", False))
            seen[model] = all_of(e)
            assert seen[model]["mu"] != want["mu"], model
            # the switch alone, on a live configuration, is the model's own fresh context (field mode aside: wolf_full
            # brings the Wolf field with it, with the polar_wolf_alpha of the parameters)
            assert seen[model] == fresh(s, dict(p, polar_damp_type=kw["damping"], polar_wolf_full=int(kw.get("wolf_full", False))))
            e.set_thole_model()  # back to the default
            assert all_of(e) == want, model
        assert len({v["mu"] for v in seen.values()}) == 3
        # the model survives an upload (a context setting); load_system() without the keys restores the default
        e.set_thole_model("linear")
        e.upload(s)
        assert all_of(e) == seen["linear"]
        e.load_system(s, p)
        assert all_of(e) == want
    finally:
        e.close()


def test_refusals_are_made_by_name():
    import vdw_cases as vc

    s = pc.system("nv65")
    e = make(s, pc.JACOBI4)
    try:
        with pytest.raises(engine.EngineError, match="polar_wolf_full needs polar_damp_type exponential"):
            e.set_thole_model("linear", wolf_full=True)
        with pytest.raises(engine.EngineError, match="damp_type"):
            e.set_thole_model(7)
        with pytest.raises(ValueError):
            e.set_thole_model("quadratic")
        e.energy_begin()
        with pytest.raises(engine.EngineError, match="between energy_begin"):
            e.set_thole_model("linear")
        e.energy_end()
        # polar_damp <= 0 is an error unless the type is off (check_input.c:406-409)
        with pytest.raises(engine.EngineError, match="damping factor"):
            e.set_params(**dict(pc.JACOBI4, polar_damp=0.0))
        e.set_thole_model("off")
        e.set_params(**dict(pc.JACOBI4, polar_damp=0.0))
        assert np.isfinite(e.energy()["polarization_energy"])
        e.set_thole_model("linear")
        with pytest.raises(engine.EngineError, match="damping factor"):
            e.energy()
    finally:
        e.close()
    sv = vc.system("box21")
    e = engine.Engine(len(sv["charge"]))
    try:
        e.load_system(sv, vc.FLAGS)
        e.energy()
        for kw in (dict(damping="linear"), dict(damping="off"), dict(damping="exponential", wolf_full=True)):
            e.set_thole_model(**kw)
            with pytest.raises(engine.EngineError, match="polarvdw with polar_damp_type linear / off or polar_wolf_full"):
                e.energy()
        e.set_thole_model()
        assert np.isfinite(e.energy()["energy"])
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------
# 6. through the host layer and the mpmc_hip driver
# ---------------------------------------------------------------------------------------------
def _driver(tmp_path, text, timeout=120):
    (tmp_path / "input").write_text(text)
    r = subprocess.run([host.EXE_PATH, "input"], cwd=str(tmp_path), capture_output=True, text=True, timeout=timeout)
    out = r.stdout + r.stderr
    vals = {m.group(1).strip(): m.group(2) for m in re.finditer(r"OUTPUT: ([a-zA-Z_/ \-]+?) *= *(\S+)", out)}
    return r.returncode, out, vals


@pytest.mark.parametrize("name", sorted(PRINTED))
def test_driver_prints_the_reference_digits(tmp_path, name):
    fx = PRINTED[name]
    shutil.copy(os.path.join(GOLD, fx["pqr"]), str(tmp_path / fx["pqr"]))
    rcode, out, vals = _driver(tmp_path, open(os.path.join(GOLD, name + ".in")).read())
    assert rcode == 0, out
    print(name, vals, fx["printed"])
    for key in ("polarization energy", "potential energy", "electrostatic energy", "repulsion/dispersion energy"):
        assert vals[key] == fx["printed"][key], (name, key, vals[key], fx["printed"][key])
    line = {"linear": "INPUT: Thole linear damping activated", "off": "INPUT: Thole linear damping is OFF",
            "wolf": "INPUT: Full polar wolf treatment activated."}[name.split("_")[1]]
    assert line in out


@pytest.mark.parametrize("ensemble", ["nvt", "npt", "uvt", "replay"])
def test_driver_runs_the_other_ensembles_under_linear(tmp_path, ensemble):
    shutil.copy(os.path.join(GOLD, "spol320.pqr"), str(tmp_path / "spol320.pqr"))
    base = open(os.path.join(GOLD, "spol320_linear_2.1304_iter10.in")).read()
    text = base.replace("ensemble total_energy", "ensemble %s" % ensemble).replace("polar_max_iter 10", "polar_max_iter 4")
    text += ("preset_seeds 20251\nnumsteps 20\ncorrtime 5\nmove_factor 0.05\nrot_factor 0.05\nenergy_output energy.dat\n"
             "pqr_output out.pqr\npqr_restart restart.pqr\ntraj_output traj.pqr\n")
    if ensemble == "npt":
        text += "pressure 1.0\nvolume_probability 0.2\nvolume_change_factor 0.05\n"
    if ensemble == "uvt":
        text += "pressure 1.0\ninsert_probability 0.5\n"
    if ensemble == "replay":
        shutil.copy(os.path.join(GOLD, "spol320.pqr"), str(tmp_path / "frames.pqr"))
        text += "traj_input frames.pqr\n"
    rcode, out, vals = _driver(tmp_path, text)
    assert rcode == 0, out
    assert "INPUT: Thole linear damping activated" in out
    rows = [l.split() for l in (tmp_path / "energy.dat").read_text().splitlines() if l.strip() and not l.startswith("#")]
    assert rows and all(np.isfinite(float(v)) for row in rows for v in row)
    polar = [float(row[4]) for row in rows]
    assert all(v < 0.0 for v in polar)
    if ensemble == "replay":  # the frame is the golden input's configuration: four sweeps of its ten-sweep -1087.337785
        assert abs(polar[0] + 1087.34) < 0.5


def test_nvt_chain_under_linear_carries_the_energy_of_its_configuration():
    """200 steps with a preset seed: every energy column finite, moves both ways, and the energy the chain carries is the
    from-scratch total_energy of its final configuration to 1e-9 relative"""
    s = synth.s_pol(320)
    f = dict(synth.FLAGS_POL_PRODUCTION, polar_damp_type="linear")
    h = host.HostSystem(s, f, seed=20251, move_factor=0.05, rot_factor=0.05)
    try:
        for _ in range(4):
            h.mc_steps(50)
            assert not h.lib.host_device_error(h.ptr)
            o = h.observables()
            assert all(np.isfinite(o[k]) for k in ("energy", "coulombic_energy", "rd_energy", "polarization_energy"))
        assert o["accept"] + o["reject"] == 200 and o["accept"] > 0 and o["reject"] > 0
        cur = dict(s, pos=h.positions())
    finally:
        h.close()
    h2 = host.HostSystem(cur, f)
    try:
        got = h2.energy()
        o2 = h2.observables()
    finally:
        h2.close()
    print("linear chain %.12g fresh %.12g" % (o["energy"], got))
    assert abs(o["energy"] - o2["energy"]) <= 1e-9 * abs(o2["energy"])
    assert abs(o["polarization_energy"] - o2["polarization_energy"]) <= 1e-9 * abs(o2["energy"])
