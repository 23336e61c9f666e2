"""mpmc_hip_insert_molecule / mpmc_hip_remove_molecule / mpmc_hip_set_sweep_order on a live context against a plain-Python
model of the bookkeeping (tests/edit_model.py) and the numpy.longdouble references that share nothing with the oracle
(tests/pair_reference.py, tests/polar_reference.py).  Scenarios: tests/edit_cases.py; the same comparisons run with the
oracle in the engine's place in tests/test_edit_model.py.

At every operation: the return value, slot_count() and n_atoms are the model's.  At every comparison point: the energies
against pair_reference.sums() and the oracle (RTOL 1e-10, ef_static to 1e-11 of its largest component, es_recip / es_self
inside their derived bounds), mu / ef_induced / ef_induced_change inside polar_reference's bound on the engine's own
ef_static, U_pol to 1e-12 of its terms, exact zeros in every hole slot, and under Gauss-Seidel the iteration count, the
flag and the ranking exactly.  Bit identity where DESIGN.md section 4 claims it: the same edits evaluated after each one or
once at the end, the listed-atoms route against the recompute-everything route, a remove + insert that restores the
upload's layout against a fresh engine, and the three forms of the Jacobi solve among themselves.  Every comparison prints
an `EDITREF` line with max(diff / bound) (profiles/edits/README.md is that table); each solver path is asserted taken."""
import numpy as np
import pytest

import edit_cases as ec
import polar_cases as pc
import polar_reference as pref
from mpmc_amd import engine

pytestmark = pytest.mark.gpu
LD = pref.LD

JACOBI_FORMS = {
    "one launch": dict(resident_jacobi=1, resident_fold=0),
    "one launch, folded": dict(resident_jacobi=1, resident_fold=16),
    "launch per sweep": dict(resident_jacobi=0, timing=2),
}


class Live(engine.Engine):
    def slot_count(self):
        return int(self.lib.mpmc_hip_slot_count(self.ctx))

    def dipoles(self):
        self.n = self.slot_count()
        return super().dipoles()

    def ranking(self):
        self.n = self.slot_count()
        return super().ranking()


def is_jacobi(s):
    p = s.params
    return ec.polarizable(s) and not (p.get("polar_gs") or p.get("polar_gs_ranked"))


def run(name, options=None, each=False, path="", compare=True):
    """one scenario on one engine; the solver path is asserted at every comparison point.  Returns play()'s results."""
    s = ec.scenario(name)
    opts = dict(s.options, **(options or {}))
    e = Live(s.max_atoms)
    e.load_system(s.system, s.params)
    for k, v in opts.items():
        e.set_option(k, v)
    seen = dict(calls=0)

    def check(op, r, d):
        t = e.timings()
        if ec.polarizable(s) and op["snap"]["live_view"] > 0:
            if not is_jacobi(s):
                assert t["resident_calls"] == 0, (name, op["label"], t)
            elif opts.get("resident_jacobi", 1) == 0:
                assert t["resident_calls"] == 0 and t["sweep_count"] == s.params["polar_max_iter"], (name, op["label"], t)
            else:
                assert t["resident_calls"] > seen["calls"] and t["resident_fallbacks"] == 0, (name, op["label"], t)
        seen["calls"] = t["resident_calls"]
        if compare:
            ec.check_point(s, op, r, d, ranking=e.ranking() if s.params.get("polar_gs_ranked") else None, path=path or "engine")

    try:
        return ec.play(s, e, refusal=engine.EngineError, check=check, each=each)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------
# 1. every scenario: model, references, path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in ec.SCENARIOS if n not in ec.JACOBI_FORMS))
def test_scenario(name):
    run(name)


@pytest.mark.parametrize("name", ec.JACOBI_FORMS)
def test_view_scenarios_in_the_three_forms_of_the_jacobi_solve(name):
    """the one-launch resident solver, its folded form and one launch per sweep: each inside the bound, each asserted
    taken, and the three bit-identical among themselves"""
    out = {form: run(name, options=o, path=form) for form, o in JACOBI_FORMS.items()}
    first = out["one launch"]
    for form in ("one launch, folded", "launch per sweep"):
        for label in first:
            ec.same_bits(first[label], out[form][label], (name, label, form))
    last = ec.scenario(name).comparison_points()[-1]
    if last["snap"]["live_view"] == 0:  # every polarizable molecule removed
        r, d = first[last["label"]]
        assert r["polarization_energy"] == 0.0 and not d["mu"].any()
        assert all(np.isfinite(v) for v in r.values()) and all(np.isfinite(d[k]).all() for k in ec.VECTORS)


@pytest.mark.parametrize("name", sorted("excluded " + k for k in ec.EXCLUDED))
def test_excluded_modes_refuse_and_change_nothing(name):
    run(name)


# ---------------------------------------------------------------------------------------------
# 2. bit identity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["order", "tiles192", "view_alpha"])
def test_evaluating_after_every_edit_or_once_at_the_end_is_the_same(name):
    end, each = run(name, compare=False), run(name, each=True, compare=False)
    for label in end:
        ec.same_bits(end[label], each[label], (name, label))


def test_the_listed_route_and_the_recompute_everything_route_agree():
    """260 edited atoms before one energy() (past 256 the engine keeps no list) against energy() after each edit"""
    label = "after 260 edited atoms"
    burst, each = run("burst", compare=False), run("burst_each", compare=False)
    ec.same_bits(burst[label], each[label], label)


@pytest.mark.parametrize("flags", ["jacobi", "production"])
def test_restoring_the_uploads_layout_equals_a_fresh_engine(flags):
    name = "restore_" + flags
    s = ec.scenario(name)
    out = run(name, compare=False)
    fresh = Live(s.max_atoms)
    fresh.load_system(s.system, s.params)
    want = (fresh.energy(), fresh.dipoles())
    fresh.close()
    ec.same_bits(out["restored"], want, name)
    ec.same_bits(out["upload"], want, name + " upload")


def test_update_atoms_of_a_hole_changes_no_bit_then_or_later():
    touched, plain = run("hole_update", compare=False), run("hole_untouched", compare=False)
    for label in plain:
        ec.same_bits(touched[label], plain[label], label)


# ---------------------------------------------------------------------------------------------
# 3. the deferred sweeps of a large view
# ---------------------------------------------------------------------------------------------
def test_deferred_sweeps_after_edits_and_their_drop_by_the_next_edit():
    """fixed-count Jacobi x 4 on a view of at least 1345 slots, timed with events (timing = 2: the call launches n - 1
    sweeps and leaves the n-th pending).  The live set is nv1345's in another slot arrangement: the committed tensor serves
    through the permutation.  The record first, then the dipoles, then one more edit, which must DROP the pending sweep."""
    s = ec.scenario("deferred")
    n, p = s.max_atoms, s.params
    e = Live(n)
    e.load_system(s.system, p)
    for k, v in s.options.items():
        e.set_option(k, v)
    out = ec.play(s, e, refusal=engine.EngineError)
    assert out == {} and e.slot_count() == n
    r = e.energy()
    t = e.timings()
    assert t["pending_sweeps"] == 1 and t["sweep_count"] == 3 and t["resident_calls"] == 0, t
    assert r["n_atoms"] == n
    d = e.dipoles()
    t = e.timings()
    assert t["pending_sweeps"] == 0 and t["sweep_count"] == 4, t
    perm = s.permutation
    full, tensor = pc.system("nv1345"), pc.tensor("nv1345")
    got = {k: d[k][perm] for k in ec.VECTORS}
    res = pref.solve(tensor, full, p, got["ef_static"], history=True)
    what = "deferred | nv1345 through a permutation | launch per sweep, last sweep on demand"
    ratios = pref.check(tensor, full, res, got, ec.keys_of(p), what=what)
    assert not got["ef_induced_change"].any() and r["polar_iterations"] == 4 and r["iter_success"] == 0
    ratios["U_pol"] = pref.check_energy(res, r["polarization_energy"], what=what, deferred=True)
    cap = 1e-11 * float(np.abs(res["mu"]).max())
    assert float(res["mu_err"].max()) <= cap
    print("EDITREF %s | n %d slots %d view %d live 1345 | %s" % (what, n, n, len(s.model.view), " ".join(
        "%s %.3g" % kv for kv in sorted(ratios.items()))))
    r2 = e.energy()
    for k, v in r.items():
        assert r2[k] == v, k
    assert e.timings()["pending_sweeps"] == 1
    assert e.remove_molecule(40, 5)  # one more edit: the pending sweep is dropped, not run on the edited state
    t = e.timings()
    assert t["pending_sweeps"] == 0 and t["sweep_count"] == 3, t
    with pytest.raises(engine.EngineError, match="no polarization energy"):
        e.dipoles()
    e.close()


# ---------------------------------------------------------------------------------------------
# 4. the expanded matrix after a re-upload into an edited context
# ---------------------------------------------------------------------------------------------
def test_full_matrix_after_a_reupload_into_an_edited_context():
    """the context of the view_alpha scenario (holes in the atom slots and in the view, 63 live atoms of 63 + 2 view
    slots) takes pair_coefficients = 0 and a fresh upload of its live atoms: A within dT, MAXVALUE on alpha = 0 diagonals"""
    s = ec.scenario("view_alpha")
    point = s.comparison_points()[2]
    stop = s.ops.index(point) + 1
    e = Live(s.max_atoms)
    e.load_system(s.system, s.params)
    short = ec.Script.__new__(ec.Script)
    short.__dict__.update(s.__dict__)
    short.ops = s.ops[:stop]
    ec.play(short, e, refusal=engine.EngineError)
    live, t = point["snap"]["system"], ec.references(s, point)["tensor"]
    e.set_option("pair_coefficients", 0)
    e.load_system(live, s.params)
    r = e.energy()
    d = e.dipoles()
    A = e.amatrix()
    e.close()
    assert e.n == len(live["charge"]) and A.shape == (3 * e.n, 3 * e.n)
    want, dA = pref.amatrix(t, live)
    idx = (3 * t.view[:, None] + np.arange(3)[None, :]).reshape(-1)
    sel = np.ix_(idx, idx)
    assert np.array_equal(A, A.T)
    diff = np.abs(A.astype(LD) - want).astype(np.float64)[sel]
    bad = np.argwhere(~(diff <= dA[sel]))
    assert not len(bad), ("A outside dT at view rows/columns", bad[:4])
    assert np.all(np.diag(A)[np.repeat(live["alpha"], 3) == 0.0] == pref.MAXVALUE)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.where(dA[sel] > 0, diff / dA[sel], 0.0).max())
    print("EDITREF view_alpha | re-upload, pair_coefficients=0 | amatrix | A %.3g" % ratio)
    slots = np.arange(e.n)
    snap = dict(point["snap"], slots=slots, holes=np.zeros(0, dtype=np.int64), slot_count=e.n)
    ec.check_point(s, dict(point, snap=snap), r, d, path="full matrix after a re-upload")
