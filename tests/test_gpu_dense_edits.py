"""GPU tests of mpmc_hip_edit_molecules: insertions and removals on a live context in the dense energy modes
(disp_expansion, axilrod_teller, rd_crystal, the pair potentials of set_rd_form), where insert_molecule / remove_molecule
answer "upload again".

After every script of tests/dense_edit_cases.py the edited configuration is rebuilt from the slots and held against the
independent references of the modes -- tests/phahst_reference.py, rdforms_reference.py, rdc_reference.py, at_reference.py --
to the bound their own GPU tests use, 1e-12 * sum |terms| (the check helpers are those tests' own, imported); the Coulomb
and polarization energies against the CPU oracle to 1e-10; and the incremental pass after the edit against a full pass over
the same slots (incremental_pairs = 0), bit for bit.  A stale long-range correction or three-body unit is no rounding
matter: one molecule missing from a correction of N atoms moves it by about 1 / N of itself, ten orders above the bound.
"""
import numpy as np
import pytest

import at_reference as ar
import dense_edit_cases as dc
import edit_model
import phahst_reference as ph
import rdc_reference as rr
import rdforms_reference as rf
import test_gpu_at as t_at
import test_gpu_phahst as t_phahst
import test_gpu_rd_crystal as t_rdc
import test_gpu_rdforms as t_rdf
import vdw_cases as vc
from mpmc_amd import engine, synth
from oracle import oracle

pytestmark = pytest.mark.gpu
FIELDS = [f for f, _ in engine.Result._fields_]
RTOL = 1e-10  # the project's bound on the oracle's terms


def _polar(f):
    return bool(f.get("polarization")) and not f.get("rd_only")


def _wire(d, f):
    """a molecule dict of dense_edit_cases as Engine.edit_molecules takes it: only the arrays the mode reads"""
    out = {k: d[k] for k in ("pos",) + edit_model.FIELDS}
    out["frozen"] = d.get("frozen", 0)
    if f.get("disp_expansion"):
        out.update({k: d[k] for k in ("c6", "c8", "c10")})
    if f.get("axilrod_teller"):
        out["c9"] = d["c9"]  # (midzuno_kihara_approx is off in every mode here: the effective c9 is c9 as read)
    return out


class Live(dc.Sim):
    """a Sim that carries every operation out on an engine too and holds the engine's answers against the model's"""

    def __init__(self, mode, n, each=True, **options):
        super().__init__(mode, n)
        self.each = each
        self.e = engine.Engine(self.cap)
        for k, v in options.items():
            self.e.set_option(k, v)
        self.e.load_system(self.start, self.flags)
        self.last = self.e.energy()

    def _apply(self, ranges, insert, firsts):
        got = self.e.edit_molecules(ranges, [_wire(d, self.flags) for d in insert])
        assert got == firsts, (got, firsts)
        assert self.e.n == self.model.slot_count
        return firsts

    def move(self, mol, shift):
        first, pos = super().move(mol, shift)
        self.e.update_atoms(first, pos)

    def scale_box(self, factor):
        nmol = len(edit_model.runs(self.start["molecule"]))
        got = self.e.scale_box(self.model.basis * factor, np.zeros((nmol, 3)))
        assert got is False
        return got

    def evaluate(self):
        super().evaluate()
        self.last = self.e.energy()
        return self.last

    def unchanged(self):
        if self.each:  # (else the previous energy() is not that of the pending edits)
            prev = self.last
            assert self.evaluate() == prev

    def all(self):
        """(result record, three-body energy, per-atom vectors or None) of an energy() now"""
        r = self.evaluate()
        return r, self.e.three_body_energy(), (self.e.dipoles() if _polar(self.flags) else None)

    def close(self):
        self.e.close()


def _same(a, b, what):
    for f in FIELDS:
        assert a[0][f] == b[0][f], (what, f, a[0][f], b[0][f])
    assert a[1] == b[1], (what, "three_body_energy", a[1], b[1])
    if a[2] is not None:
        for k in a[2]:
            assert np.array_equal(a[2][k], b[2][k]), (what, k)


def _plain(s):
    return {k: v for k, v in s.items() if k not in dc.EXTRA}


def _against_references(f, s, got, three, what):
    assert got["status"] == 0 and got["n_atoms"] == len(s["charge"])
    if f.get("disp_expansion"):
        t_phahst._check_rd(got, ph.rd_terms(s, f), what)
    elif f.get("rd_crystal"):
        t_rdc._check_rd(got, dict(rr.rd_terms(s, f, f["rd_crystal_order"]), order=f["rd_crystal_order"]), what)
    elif engine.rd_form_of(f)[0] != "off":
        form, mixing = engine.rd_form_of(f)
        t_rdf._check_rd(got, rf.rd_terms(s, f, form, mixing), what)
    if f.get("axilrod_teller"):
        t_at._check(three, ar.unordered(s, False), what)
    else:
        assert three == 0.0
    if f.get("rd_only"):
        assert got["coulombic_energy"] == 0.0 and got["polarization_energy"] == 0.0
        return
    # Coulomb and polarization: the oracle knows neither dense term, and neither enters those two energies
    bare = {k: v for k, v in f.items() if k not in engine.AT_NAMES}
    if f.get("disp_expansion"):
        want = oracle.energy(ph.without_dispersion(_plain(s)), ph.plain_flags(bare))
    else:
        want = oracle.energy(_plain(s), bare)
        assert abs(got["rd_energy"] - want["rd_energy"]) <= RTOL * max(1.0, abs(want["rd_energy"]))
    for k in ("coulombic_energy", "polarization_energy"):
        print("%s: %s %.12f oracle %.12f" % (what, k, got[k], want[k]))
        assert abs(got[k] - want[k]) <= RTOL * max(1.0, abs(want[k])), (what, k, got[k], want[k])


def _run(mode, script, each):
    n, fn = dc.SCRIPTS[script]
    live = Live(mode, n, each)
    fn(live, live.evaluate if each else (lambda: None))
    first = live.all()
    live.e.set_option("incremental_pairs", 0)  # a full pass over the same slots
    _same(first, live.all(), "%s/%s: incremental pass against a full pass over the same slots" % (mode, script))
    s = live.live_system()
    live.close()
    return first, s


@pytest.mark.parametrize("mode,script", dc.CASES, ids=["%s-%s" % c for c in dc.CASES])
def test_script(mode, script):
    at_end, s = _run(mode, script, False)
    _against_references(dc.flags(mode), s, at_end[0], at_end[1], "%s/%s" % (mode, script))
    per_edit, _ = _run(mode, script, True)
    _same(per_edit, at_end, "%s/%s: evaluating after every edit against once at the end" % (mode, script))


@pytest.mark.parametrize("mode", sorted(dc.MODES))
def test_restoring_the_layout_equals_a_fresh_engine(mode):
    live = Live(mode, 130)
    mv = live.movable()
    a = mv[len(mv) // 2]
    first, count = live.model.molecules[a]
    mol = live.molecule(a)
    assert live.edit(remove=[a]) == []
    gone = live.all()
    assert gone[0]["n_atoms"] == 130 - count
    assert live.edit(insert=[mol]) == [first]
    back = live.all()
    live.close()
    fresh = engine.Engine(live.cap)
    fresh.load_system(dc.system(mode, 130), dc.flags(mode))
    want = (fresh.energy(), fresh.three_body_energy(), fresh.dipoles() if _polar(dc.flags(mode)) else None)
    fresh.close()
    _same(back, want, "%s: a molecule removed and put back against a fresh engine" % mode)


def _old_and_new(flags, n=60):
    """the same edits through remove_molecule + insert_molecule and through edit_molecules: two engines and the model"""
    s = synth.s_pol(n)
    model = edit_model.Model(s, flags, n + 40)
    old, new = engine.Engine(n + 40), engine.Engine(n + 40)
    for e in (old, new):
        e.load_system(s, flags)
    assert old.energy() == new.energy()
    model.energy()

    def molecule(first, count, shift):
        sl = slice(first, first + count)
        return dict(pos=model.pos[sl] + shift, **{k: model.prop[k][sl].copy() for k in edit_model.FIELDS})

    def both(remove, insert):
        for first, count in remove:
            assert old.remove_molecule(first, count)
            assert model.remove(first, count)
        slots = []
        for d in insert:
            slots.append(old.insert_molecule(d["pos"], *[d[k] for k in edit_model.FIELDS]))
            assert slots[-1] == model.insert(d["pos"], *[d[k] for k in edit_model.FIELDS])
        assert new.edit_molecules(remove, insert) == slots
        for e in (old, new):
            e.set_sweep_order(model.sweep_order())
        model.set_sweep_order(model.sweep_order())
        model.energy()
        a, b = old.energy(), new.energy()
        assert a == b, (a, b)
        da, db = old.dipoles(), new.dipoles()
        for k in da:
            assert np.array_equal(da[k], db[k]), k
        return a

    half = 0.5 * 3.6
    e0 = both([(20, 5)], [])
    e1 = both([], [molecule(25, 5, half), molecule(30, 5, half)])  # the first takes the hole, the second is appended
    e2 = both([(40, 5), (10, 5)], [molecule(45, 5, half)])         # the most recent hole of the size: slots 10 .. 14
    assert model.molecules[model.mol[10]] == (10, 5) and model.holes == [(40, 5)]
    assert len({e0["energy"], e1["energy"], e2["energy"]}) == 3
    old.close()
    new.close()


def test_parity_with_the_old_entries_jacobi():
    _old_and_new(dict(synth.FLAGS_POL_JACOBI))


def test_parity_with_the_old_entries_gauss_seidel_with_set_sweep_order():
    _old_and_new(dict(synth.FLAGS_POL_PRODUCTION))


def _refused(live, text, **kw):
    before = live.last
    with pytest.raises(engine.EngineError, match=text):
        live.e.edit_molecules(**kw)
    assert live.e.energy() == before


def test_refusals_by_name_change_nothing():
    live = Live("phahst_lrc", 60)
    a = live.movable()[2]
    d = _wire(dc.grown(live.molecule(a), 3, live.gap(a)), live.flags)
    first, count = live.model.molecules[a]
    _refused(live, "c6 / c8 / c10 missing while disp_expansion is on",
             remove=[(first, count)], insert=[{k: v for k, v in d.items() if k != "c6"}])
    _refused(live, "holds no atom", remove=[(first, count), (first, count)], insert=[d])
    _refused(live, "outside", remove=[(58, 5)], insert=[d])
    # a call in flight
    live.e.energy_begin()
    with pytest.raises(engine.EngineError, match="between energy_begin\\(\\) and energy_end\\(\\)"):
        live.e.edit_molecules([(first, count)], [d])
    assert live.e.energy_end() == live.last and live.e.energy() == live.last
    # and the same molecules are taken once nothing is wrong: the refusals left no trace
    assert live.edit(remove=[a], insert=[dc.grown(live.molecule(a), 3, live.gap(a))]) == [first]
    after = live.all()
    _against_references(live.flags, live.live_system(), after[0], after[1], "after the refusals")
    # the per-atom setters keep refusing after an edit
    with pytest.raises(engine.EngineError, match="molecules were inserted or removed since the upload"):
        live.e.set_dispersion(live.start, **{k: live.flags[k] for k in engine.DISP_NAMES})
    live.close()

    live = Live("lj_at", 60)
    a = live.movable()[2]
    d = _wire(dc.grown(live.molecule(a), 2, live.gap(a)), live.flags)
    _refused(live, "c9 missing while axilrod_teller is on", insert=[{k: v for k, v in d.items() if k != "c9"}])
    _refused(live, "negative polarizability", insert=[dict(d, alpha=-np.abs(d["alpha"]) - 0.1)])
    live.close()


def test_a_negative_sigma_inserted_is_refused_under_waldman_hagler_as_after_an_upload():
    live = Live("lj_wh_fh4", 60)
    a = live.movable()[2]
    d = dc.grown(live.molecule(a), 5, live.gap(a))
    assert live.e.edit_molecules([], [dict(_wire(d, live.flags), sigma=-d["sigma"])]) == [60]
    with pytest.raises(engine.EngineError, match="waldmanhagler mixing with a negative sigma"):
        live.e.energy()
    live.close()


def _one_more(e, s, first=20, count=5):
    sl = slice(first, first + count)
    d = dict(pos=s["pos"][sl] + 1.8, **{k: s[k][sl] for k in edit_model.FIELDS})
    for k in dc.EXTRA:
        if k in s:
            d[k] = s[k][sl]
    return e.edit_molecules([(first, count)], [d])


@pytest.mark.parametrize("what", ["polarvdw", "exact", "pair_coefficients", "incremental_amatrix", "incremental_pairs",
                                  "gauss_seidel_without_the_chain_kernel"])
def test_modes_and_options_without_edits_answer_none_and_change_nothing(what):
    if what == "polarvdw":
        s, f, options = vc.system("box70"), vc.FLAGS, {}
        first, count = [(a, k) for a, k in edit_model.runs(s["molecule"]) if not s["frozen"][a] and k <= 16][3]
    else:
        s, first, count = synth.s_pol(60), 20, 5
        f = dict(synth.FLAGS_POL_JACOBI, polar_iterative=0) if what == "exact" else dict(synth.FLAGS_POL_JACOBI)
        options = {} if what == "exact" else {what: 0}
        if what.startswith("gauss"):
            f, options = dict(synth.FLAGS_POL_PRODUCTION), {"persistent_gs": 0}
    e = engine.Engine(len(s["charge"]) + 40)
    for k, v in options.items():
        e.set_option(k, v)
    e.load_system(s, f)
    before = e.energy()
    assert _one_more(e, s, first, count) is None
    assert e.energy() == before and e.n == len(s["charge"])
    e.close()
