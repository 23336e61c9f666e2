"""The iterative Thole solve and the Ewald reciprocal / self sums on the device against numpy.longdouble references that
share nothing with the oracle (tests/polar_reference.py, tests/pair_reference.py), each within the reference's DERIVED
bound: every component of mu, ef_induced and (Palmo) ef_induced_change, U_pol to 1e-12 of the sum of its terms' magnitudes,
iteration counts, the convergence flag and the ranking -- per solver path, each asserted to be the path taken.

E is the engine's own downloaded ef_static (exact in longdouble): the solver is isolated from the field, which
tests/test_gpu_screen_edges.py holds to pair_reference.  Cases, sizes and flags: tests/polar_cases.py; the same
comparisons run against the CPU oracle in tests/test_polar_reference.py.  Every comparison prints a `POLARREF` line with
max(diff / bound) (profiles/polar_reference/README.md is that table); a component outside the bound fails with the site,
its 64-block and lane, and the pair that explains it (polar_reference.explain())."""
import numpy as np
import pytest

import pair_reference as pr
import polar_cases as pc
import polar_reference as pref
from mpmc_amd import engine, synth

pytestmark = pytest.mark.gpu
LD = pref.LD


def make(s, params, **opts):
    e = engine.Engine(len(s["charge"]))
    e.load_system(s, params)
    for k, v in opts.items():
        e.set_option(k, v)
    return e


def keys_of(params):
    return ("mu", "ef_induced") + (("ef_induced_change",) if params.get("polar_palmo") else ())


def own_sum(d, params):
    """-1/2 sum (mu.E + [palmo] mu.dE_ind) of the engine's OWN vectors in longdouble, and the sum of |products| / 2"""
    terms = d["mu"].astype(LD) * d["ef_static"].astype(LD)
    if params.get("polar_palmo"):
        terms = np.concatenate([terms, d["mu"].astype(LD) * d["ef_induced_change"].astype(LD)])
    return LD(-0.5) * terms.sum(), LD(0.5) * np.abs(terms).sum()


def energy_allowance(res, E, palmo):
    a = 0.5 * float((np.abs(E) * res["mu_err"]).sum())
    if palmo:
        a += 0.5 * float((np.abs(res["ef_induced_change"]).astype(np.float64) * res["mu_err"]).sum())
        a += 0.5 * float((np.abs(res["mu"]).astype(np.float64) * res["ef_induced_change_err"]).sum())
    return a


def compare(case, path, params, r, d, e=None, deferred=False, tensor=None, system=None):
    """one engine evaluation (record r, vectors d) against the reference on the engine's own static field"""
    s = pc.system(case) if system is None else system
    t = pc.tensor(case) if tensor is None else tensor
    res = pref.solve(t, s, params, d["ef_static"], history=deferred)
    what = "%s %s" % (case, path)
    ratios = pref.check(t, s, res, d, keys_of(params), what=what,
                        cap=pc.cap_of(res) if pc.loose_bound(case, params) else None)
    if not params.get("polar_palmo"):
        assert not d["ef_induced_change"].any(), what
    assert r["polar_iterations"] == res["polar_iterations"] and r["iter_success"] == res["iter_success"], what
    if params.get("polar_gs_ranked") and e is not None:
        rank, order = e.ranking()
        assert np.array_equal(rank, res["rank_metric"]), what
        assert np.array_equal(order, res["ranked_array"]), what
    if case in pc.CLOSE:
        # the dipoles are only known to their bound there: U_pol against the longdouble sum of the engine's own products at
        # the project's bar, and against the reference with what the dipoles' bound adds
        u, terms = own_sum(d, params)
        assert abs(float(LD(r["polarization_energy"]) - u)) <= 1e-12 * float(terms), what
        allow = 1e-12 * float(res["upol_terms"]) + energy_allowance(res, d["ef_static"], params.get("polar_palmo"))
        dU = abs(float(LD(r["polarization_energy"]) - res["upol"]))
        assert dU <= allow, (what, r["polarization_energy"], float(res["upol"]), dU, allow)
        ratios["U_pol"] = dU / allow
    else:
        ratios["U_pol"] = pref.check_energy(res, r["polarization_energy"], what=what, deferred=deferred)
    print("POLARREF gpu %s | %s | %s" % (case, path, " ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
    return res


def evaluate(e):
    r = e.energy()
    return r, e.dipoles()


# ---------------------------------------------------------------------------------------------
# 1. the expanded matrix: A itself, and both sweeps on it
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["nv65", "nv129", "ties_sheared_shifted", "coincident"] + list(pc.CLOSE))
def test_full_matrix(case):
    s, t = pc.system(case), pc.tensor(case)
    want, dA = pref.amatrix(t, s)
    idx = (3 * t.view[:, None] + np.arange(3)[None, :]).reshape(-1)
    sel = np.ix_(idx, idx)
    for sym in (2, 0):  # 2: the upper-triangle sweep whatever the size; 0: sweep_kernel on all of A
        e = make(s, pc.JACOBI4, pair_coefficients=0, symmetric_sweep=sym)
        r, d = evaluate(e)
        A = e.amatrix()
        e.close()
        assert np.array_equal(A, A.T)
        diff = np.abs(A.astype(LD) - want).astype(np.float64)[sel]
        bad = np.argwhere(~(diff <= dA[sel]))  # (a NaN is outside)
        assert not len(bad), (case, "A outside dT at view rows/columns", bad[:4], diff[tuple(bad[0])], dA[sel][tuple(bad[0])])
        diag = np.diag(A)
        alpha = np.repeat(s["alpha"], 3)
        assert np.all(diag[alpha == 0.0] == pref.MAXVALUE)
        if case == "coincident":
            i, j = 3 * pc.CLOSE_A, 3 * pc.CLOSE_B
            assert not A[i:i + 3, j:j + 3].any() and not A[j:j + 3, i:i + 3].any()
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(dA[sel] > 0, diff / dA[sel], 0.0).max()
        print("POLARREF gpu %s | amatrix symmetric_sweep=%d | A %.3g" % (case, sym, ratio))
        compare(case, "full matrix symmetric_sweep=%d" % sym, pc.JACOBI4, r, d)


# ---------------------------------------------------------------------------------------------
# 2. the coefficient store, one launch per sweep
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", pc.SMALL_SIZES + (pc.DEFERRED_SIZE,))
def test_coefficient_store_launch_per_sweep(nv):
    case = "nv%d" % nv
    e = make(pc.system(case), pc.JACOBI4, resident_jacobi=0, timing=2)
    r, d = evaluate(e)
    t = e.timings()
    e.close()
    assert t["resident_calls"] == 0 and t["sweep_count"] == 4, t
    compare(case, "coefficients, launch per sweep", pc.JACOBI4, r, d)


# ---------------------------------------------------------------------------------------------
# 3. the one-launch solvers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", pc.RESIDENT_SIZES)
def test_resident_and_folded_one_launch_solvers(nv):
    case = "nv%d" % nv
    blocks = (nv + 63) // 64
    for fold in ((16, 0) if blocks <= 16 else (0,)):
        e = make(pc.system(case), pc.JACOBI4, resident_jacobi=1, resident_fold=fold)
        r, d = evaluate(e)
        t = e.timings()
        e.close()
        assert t["resident_calls"] == 1 and t["resident_fallbacks"] == 0, (fold, t)
        compare(case, "one launch, resident_fold=%d" % fold, pc.JACOBI4, r, d)


# ---------------------------------------------------------------------------------------------
# 4. deferred sweeps and the early record
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("niter", pc.DEFERRED_ITERS)
def test_deferred_sweeps_and_early_publish(niter):
    case = "nv%d" % pc.DEFERRED_SIZE
    s = pc.system(case)
    p = dict(pc.BASE, polar_max_iter=niter)
    tail = niter - (niter + 1) // 2
    e = make(s, p, timing=0)
    r = e.energy()  # the record first: U_pol from sweep ceil(n / 2)
    assert e.timings()["pending_sweeps"] == tail and e.timings()["resident_calls"] == 0
    d = e.dipoles()  # then mu_n from the sweeps run on demand
    assert e.timings()["pending_sweeps"] == 0
    compare(case, "deferred, %d sweeps" % niter, p, r, d, deferred=True)
    first, new = pc.molecule_move(s)
    e.update_atoms(first, new)
    r = e.energy()
    assert e.timings()["pending_sweeps"] == tail
    d = e.dipoles()
    e.close()
    compare(case + "_moved", "deferred, %d sweeps, after update_atoms" % niter, p, r, d, deferred=True)


# ---------------------------------------------------------------------------------------------
# 5. Gauss-Seidel
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(pc.GS_VARIANTS))
@pytest.mark.parametrize("nv", pc.GS_SIZES)
def test_gauss_seidel(nv, variant):
    """persistent_gs = 1: the chain kernel (cached block inverses); 0: the literal substitution, two launches per block.
    The engine counts neither, so that BOTH ran shows in the only way it can: the two round differently, and their
    dipoles, each inside the bound, are not the same bits."""
    case, p = "nv%d" % nv, pc.GS_VARIANTS[variant]
    mu = {}
    for persistent in (1, 0):
        e = make(pc.system(case), p, persistent_gs=persistent)
        r, d = evaluate(e)
        assert e.timings()["resident_calls"] == 0  # (not the one-launch Jacobi solver)
        compare(case, "%s persistent_gs=%d" % (variant, persistent), p, r, d, e=e)
        e.close()
        mu[persistent] = d["mu"]
    assert not np.array_equal(mu[1], mu[0]), (case, variant, "persistent_gs 1 and 0 gave identical bits: one path ran twice?")


@pytest.mark.parametrize("persistent", [1, 0])
def test_gauss_seidel_in_a_sheared_cell(persistent):
    """six blocks in the cell of test_gpu_parity.test_triclinic_box_polarizable and that test's calls: evaluations on
    one context, then its move of one molecule through update_atoms.  (gs_chain_kernel's auxiliary-lag hand-off has an
    open timing-dependent race; with a bound of 1e-15 a recurrence fails here and names the block.)"""
    s = pc.system("sheared_640")
    e = make(s, pc.SHEARED_GS, persistent_gs=persistent)
    for call in range(3):
        r, d = evaluate(e)
        compare("sheared_640", "gs3 persistent_gs=%d call %d" % (persistent, call), pc.SHEARED_GS, r, d)
    moved = dict(s)
    moved["pos"] = s["pos"].copy()
    moved["pos"][35:40] += np.array([0.31, -0.22, 0.17])
    e.update_atoms(35, moved["pos"][35:40])
    r, d = evaluate(e)
    e.close()
    compare("sheared_640_moved", "gs3 persistent_gs=%d after update_atoms" % persistent, pc.SHEARED_GS, r, d,
            tensor=sheared_moved_tensor(), system=moved)


_moved_tensor = []


def sheared_moved_tensor():
    if not _moved_tensor:
        s = pc.system("sheared_640")
        moved = dict(s)
        moved["pos"] = s["pos"].copy()
        moved["pos"][35:40] += np.array([0.31, -0.22, 0.17])
        _moved_tensor.append(pref.Tensor(moved, pc.DAMP))
    return _moved_tensor[0]


# ---------------------------------------------------------------------------------------------
# 6. the Jacobi family's other recurrences and stopping rules
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", sorted(pc.JACOBI_VARIANTS))
def test_jacobi_variants(variant):
    p = pc.JACOBI_VARIANTS[variant]
    e = make(pc.system("nv129"), p)
    r, d = evaluate(e)
    t = e.timings()
    e.close()
    # a fixed-count Jacobi-type solve on three blocks runs as one launch; a precision-stopped one and ZODID do not
    assert t["resident_calls"] == (0 if variant in ("precision", "zodid") else 1) and t["resident_fallbacks"] == 0, t
    res = compare("nv129", variant, p, r, d)
    if variant == "precision":
        assert 2 < r["polar_iterations"] < 128
    if variant in ("rrms", "precision"):
        assert abs(r["dipole_rrms"] - res["dipole_rrms"]) <= 1e-9 * res["dipole_rrms"]


def test_divergence_falls_back_to_alpha_E():
    s = synth.s_pol(320, spacing=3.0)
    s["alpha"] = s["alpha"] * 40.0
    p = dict(pc.BASE, polar_max_iter=0, polar_precision=1e-8)
    e = make(s, p)
    r, d = evaluate(e)
    e.close()
    with np.errstate(all="ignore"):
        compare("diverging", "precision", p, r, d, tensor=pref.Tensor(s, pc.DAMP), system=s)
    assert r["iter_success"] == 1 and r["polar_iterations"] == 128


# ---------------------------------------------------------------------------------------------
# 7. special geometries
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", ["jacobi4", "production"])
@pytest.mark.parametrize("case", sorted(pc.SPECIAL))
def test_special_geometries(case, flags):
    p = pc.JACOBI4 if flags == "jacobi4" else pc.PRODUCTION
    e = make(pc.system(case), p)
    r, d = evaluate(e)
    compare(case, flags, p, r, d, e=e)
    e.close()


@pytest.mark.parametrize("path", ["one_launch", "launch_per_sweep", "full_matrix", "production", "production_literal"])
def test_coincident_pair_alone_induces_exactly_nothing(path):
    """a view of the two coincident sites only (rimg == 0, T = 0): the induced field is exactly 0 and the dipoles are
    alpha E to the bit -- any contribution of the pair, however small, shows (the chain kernel: to rounding of E, below)"""
    p, opts = {"one_launch": (pc.JACOBI4, dict(resident_jacobi=1)), "launch_per_sweep": (pc.JACOBI4, dict(resident_jacobi=0)),
               "full_matrix": (pc.JACOBI4, dict(pair_coefficients=0)), "production": (pc.PRODUCTION, dict(persistent_gs=1)),
               "production_literal": (pc.PRODUCTION, dict(persistent_gs=0))}[path]
    s = pc.coincident_only()
    e = make(s, p, **opts)
    r, d = evaluate(e)
    t = e.timings()
    e.close()
    assert t["resident_calls"] == (1 if path == "one_launch" else 0), t
    assert r["polar_iterations"] == 4 and np.abs(d["mu"]).max() > 0
    if path == "production":
        # the chain kernel forms the dipoles through the block's cached inverse (here the identity) and reports
        # E_ind = mu / alpha - E: not the bits of 0, but nothing beyond a few roundings of E -- the reference's bound with
        # T = dT = 0 is exactly that (at most 5 u |E| on the field), where a pair term would be of the order of E
        t = pref.Tensor(s, pc.DAMP)
        assert not t.T.any() and not t.dT.any()
        res = pref.solve(t, s, p, d["ef_static"])
        pref.check(t, s, res, d, keys_of(p), what="coincident pair alone, chain kernel")
        assert float(res["ef_induced_err"].max()) <= 5 * pref.UF * float(np.abs(d["ef_static"]).max()) * (1 + 1e-9)
    else:
        assert not d["ef_induced"].any() and not d["ef_induced_change"].any(), path
        assert np.array_equal(d["mu"], s["alpha"][:, None] * d["ef_static"]), path
    u, terms = own_sum(d, p)
    assert abs(float(LD(r["polarization_energy"]) - u)) <= 1e-12 * float(terms)


# ---------------------------------------------------------------------------------------------
# 8. Ewald reciprocal and self energy
# ---------------------------------------------------------------------------------------------
def check_ewald(s, p, r, what):
    u, du = pr.ewald_recip_energy(s, p)
    diff = abs(float(LD(r["es_recip"]) - u))
    print("POLARREF gpu ewald %s | es_recip %.3g of its bound (bound %.3g relative)" % (what, diff / du, du / max(abs(float(u)), 1e-300)))
    assert diff <= du, (what, r["es_recip"], float(u), diff, du)
    us, nterms = pr.ewald_self_energy(s, p)
    assert abs(float(LD(r["es_self"]) - us)) <= 2 * nterms * np.spacing(abs(float(us))), (what, r["es_self"], float(us))


@pytest.mark.parametrize("kmax", [1, 7])
@pytest.mark.parametrize("case", sorted(pc.EWALD_CASES))
def test_ewald_reciprocal_and_self_energy(case, kmax):
    s = pc.ewald_system(case)
    p = dict(temperature=100.0, ewald_kmax=kmax)
    first, new = pc.ewald_move(s)
    moved = dict(s)
    moved["pos"] = s["pos"].copy()
    moved["pos"][first:first + len(new)] = new
    for fuse in (1, 0):
        e = make(s, p, fuse_recip=fuse)
        check_ewald(s, p, e.energy(), "%s kmax %d fuse_recip=%d" % (case, kmax, fuse))
        e.update_atoms(first, new)  # the other blocks' partial structure factors stay resident
        check_ewald(moved, p, e.energy(), "%s kmax %d fuse_recip=%d after update_atoms" % (case, kmax, fuse))
        e.close()
