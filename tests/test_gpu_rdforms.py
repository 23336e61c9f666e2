"""GPU tests of the pair potentials of mpmc_hip_set_rd_form -- Silvera-Goldman, DREIDING, the buffered 14-7 and
Lennard-Jones under the four mixing rules: rdform_tile_kernel<FORM> and rdform_lrc_kernel
(mpmc_amd/csrc/kernels_rdforms.h) -- against tests/rdforms_reference.py.

The tolerance of rd_energy is 1e-12 * abs_sum (the sum of |every piece| of every pair, Feynman-Hibbs addend and
long-range-correction term), that of the dense terms before this one; rdforms_reference.py writes out why an fp64
evaluation stays about two orders inside it, sg's exponential included.  The synthetic cases keep every candidate pair
1e-9 A away from the cutoff (asserted in tests/test_rdforms_reference.py); the n = 2 cases sit on it on purpose.
"""
import json
import os

import numpy as np
import pytest

import rdforms_cases as rc
import rdforms_reference as ref
from mpmc_amd import engine, synth

pytestmark = pytest.mark.gpu
FIELDS = [f for f, _ in engine.Result._fields_]
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _engine(s, flags, cap=None, **options):
    e = engine.Engine(cap or len(s["charge"]))
    for k, v in options.items():
        e.set_option(k, v)
    e.load_system(s, flags)
    return e


def _fresh(s, flags, **options):
    e = _engine(s, flags, **options)
    r = e.energy()
    e.close()
    return r


def _check_rd(got, r, what):
    want, tol = float(r["total"]), rc.RD_TOL * float(r["abs_sum"])
    err = abs(got["rd_energy"] - want)
    print("%s: rd_energy %.12g reference %.12g |diff| %.3g tol %.3g |diff| / tol %.3g" % (what, got["rd_energy"], want, err, tol,
                                                                                        err / tol if tol else 0.0))
    assert err <= tol, (what, got["rd_energy"], want, err, tol)
    assert got["status"] == 0
    assert got["cutoff"] == r["cutoff"] and got["volume"] == r["volume"]


# every case x form x mixing, and the Feynman-Hibbs variants of the two forms that have one
CASES = [(n, rc.BASE, "base", f, m) for n in rc.TILES + ("close39", "close41") for f, m in rc.COMBOS]
CASES += [(n, rc.FH4, "fh4", "lj", m) for n in ("t65", "t130") for m in rc.MIXINGS]
CASES += [(n, rc.FH2, "fh2", "lj", "waldmanhagler") for n in ("t65", "t130")]
CASES += [(n, rc.FH2, "fh2", "sg", "lb") for n in ("t65", "t130")]
CASES += [("t130", dict(rc.BASE, rd_lrc=0), "no_lrc", "lj", m) for m in rc.MIXINGS]


@pytest.mark.parametrize("name,base,variant,form,mixing", CASES, ids=["-".join((c[0], c[2], c[3], c[4])) for c in CASES])
def test_case_against_the_reference(name, base, variant, form, mixing):
    s, f = rc.system(name, form, mixing), rc.flags(name, base, form, mixing)
    got = _fresh(s, dict(f, rd_only=1))
    _check_rd(got, rc.reference(name, base, form, mixing), "%s/%s %s %s" % (name, variant, form, mixing))
    assert got["energy"] == got["rd_energy"] and got["n_atoms"] == len(s["charge"])


def test_dreiding_passes_its_1e40_through():
    got = _fresh(rc.system("close39"), dict(rc.flags("close39", rc.BASE, "dreiding"), rd_only=1))
    assert got["status"] == 0 and np.isfinite(got["rd_energy"]) and got["rd_energy"] > 1e40
    got = _fresh(rc.system("close41"), dict(rc.flags("close41", rc.BASE, "dreiding"), rd_only=1))
    assert got["status"] == 0 and abs(got["rd_energy"]) < 1e6


@pytest.mark.parametrize("form", rc.FORMS)
def test_pair_at_the_cutoff_is_in_or_out_as_the_reference_decides(form):
    for name in ("pair2_below", "pair2", "pair2_above"):
        r = rc.reference(name, rc.BASE, form)
        got = _fresh(rc.system(name, form), dict(rc.flags(name, rc.BASE, form), rd_only=1, rd_lrc=0))
        rr = ref.rd_terms(rc.system(name, form), dict(rc.flags(name, rc.BASE, form), rd_lrc=0), form)
        inside = len(r["table"][0]) == 1
        print(name, form, "inside" if inside else "outside", got["rd_energy"])
        if inside:
            _check_rd(got, rr, "%s %s" % (name, form))
            assert got["rd_energy"] != 0.0
        else:
            assert got["rd_energy"] == 0.0 and got["status"] == 0


def test_lj_form_with_lorentz_berthelot_restates_the_standard_path():
    fx = json.load(open(os.path.join(GOLD, "fixtures.json")))["mof5_buch_425"]
    boxes = [("mof5_buch_425", dict(np.load(os.path.join(GOLD, "mof5_buch_425.npz"))), dict(fx["params"])),
             ("s_pol(320) fh4", synth.s_pol(320), dict(synth.FLAGS_POL_JACOBI))]
    for what, s, f in boxes:
        e = _engine(s, f)
        std = e.energy()
        e.set_rd_form("lj", "lb")
        dense = e.energy()
        e.close()
        r = ref.rd_terms(s, f, "lj", "lb")
        _check_rd(dense, r, what + " dense")
        _check_rd(std, r, what + " standard")
        for fld in FIELDS:  # the term is invisible to the others
            if fld not in ("energy", "rd_energy"):
                assert dense[fld] == std[fld], (what, fld)
    want = fx["expected"]["rd"]
    s, f = boxes[0][1], boxes[0][2]
    got = _fresh(s, dict(f, c6_mixing=0))  # (no mixing keyword: the standard path)
    e = _engine(s, f)
    e.set_rd_form("lj")
    dense = e.energy()
    e.close()
    for g in (got, dense):
        assert "%.*f" % (fx["decimals"], g["rd_energy"]) == "%.*f" % (fx["decimals"], want)


def test_sg_computes_no_electrostatics_and_no_polarization():
    s = rc.system("t130", "sg")
    assert np.any(s["charge"] != 0) and np.any(s["alpha"] != 0)
    f = rc.flags("t130", rc.POLAR, "sg")
    got = _fresh(s, f)
    _check_rd(got, rc.reference("t130", rc.POLAR, "sg"), "t130 sg, polarization + charges present")
    assert got["coulombic_energy"] == 0.0 and got["polarization_energy"] == 0.0 and got["energy"] == got["rd_energy"]
    assert got["es_real"] == 0.0 and got["es_recip"] == 0.0 and got["es_self"] == 0.0 and got["polar_iterations"] == 0


@pytest.mark.parametrize("form,mixing", [c for c in rc.COMBOS if c[0] != "sg"])
def test_the_other_result_fields_do_not_see_the_term(form, mixing):
    """polarization + Ewald: every field but energy and rd_energy is that of the same atoms with eps = sigma = 0"""
    name = "inc320"
    s = rc.system(name, form, mixing)
    f = rc.flags(name, rc.POLAR, form, mixing)
    on = _fresh(s, f)
    _check_rd(on, rc.reference(name, rc.POLAR, form, mixing), "%s %s %s polar" % (name, form, mixing))
    z = np.zeros(len(s["charge"]))
    off = _fresh(dict(s, epsilon=z, sigma=z), f)
    assert off["rd_energy"] == 0.0
    for fld in FIELDS:
        if fld not in ("energy", "rd_energy"):
            assert on[fld] == off[fld], (fld, on[fld], off[fld])
    assert on["energy"] == on["rd_energy"] + on["coulombic_energy"] + on["polarization_energy"]


def _moves(s, count=20, seed=3):
    """single-molecule moves on inc320: the molecule in slots 63-64 (across the first block boundary) first and last"""
    rng = np.random.default_rng(seed)
    mol = np.asarray(s["molecule"])
    ids = [int(mol[63])] + [int(m) for m in rng.choice(np.unique(mol), count - 2, replace=False)] + [int(mol[64])]
    out = []
    for m in ids:
        idx = np.flatnonzero(mol == m)
        out.append((int(idx[0]), len(idx), rng.uniform(-0.3, 0.3, 3)))
    return out


@pytest.mark.parametrize("form,mixing,base", [("sg", "lb", rc.FH2), ("dreiding", "halgren_mixing", rc.BASE),
                                              ("lj_buffered_14_7", "halgren_mixing", rc.BASE),
                                              ("lj", "waldmanhagler", rc.FH4), ("lj", "c6_mixing", rc.POLAR)])
def test_incremental_pass_leaves_the_bits_of_a_fresh_context(form, mixing, base):
    name = "inc320"
    s, f = rc.system(name, form, mixing), rc.flags(name, base, form, mixing)
    assert s["molecule"][63] == s["molecule"][64]
    live = _engine(s, f)
    full = _engine(s, f, incremental_pairs=0)
    live.energy()
    full.energy()
    cur = dict(s, pos=s["pos"].copy())
    for step, (first, count, shift) in enumerate(_moves(s)):
        new = cur["pos"][first:first + count] + shift
        cur["pos"][first:first + count] = new
        live.update_atoms(first, new)
        full.update_atoms(first, new)
        a, b = live.energy(), full.energy()
        for fld in FIELDS:
            assert a[fld] == b[fld], (step, fld, a[fld], b[fld])
        if step in (0, 9, 19):
            c = _fresh(cur, f)
            for fld in FIELDS:
                assert a[fld] == c[fld], (step, fld, a[fld], c[fld])
    _check_rd(a, ref.rd_terms(cur, f, form, mixing), "%s %s after 20 moves" % (form, mixing))
    assert live.energy() == a
    live.energy_begin()
    assert live.energy_end() == a
    live.close()
    full.close()


def test_form_zero_returns_the_bits_from_before():
    """across scale_box, energy_begin / _end and two contexts at once"""
    s = rc.system("inc320")
    f = dict(rc.POLAR)
    mol = np.asarray(s["molecule"])
    ids = np.cumsum(np.concatenate([[0], mol[1:] != mol[:-1]]))
    com = np.stack([s["pos"][ids == m].mean(axis=0) for m in range(ids[-1] + 1)])
    g = 1.02 ** (1.0 / 3.0)
    delta, basis = com * (g - 1.0), s["basis"] * g
    scaled = dict(s, pos=s["pos"] + delta[ids], basis=basis)

    a = _engine(s, f, cap=384)
    b = _engine(rc.system("t130"), rc.flags("t130", rc.BASE, "lj"))
    before = a.energy()
    b_before = b.energy()

    a.set_rd_form("dreiding", "waldmanhagler")
    b.set_rd_form("sg")
    a.energy_begin()
    b.energy_begin()
    rb, ra = b.energy_end(), a.energy_end()
    _check_rd(ra, rc.reference("inc320", rc.POLAR, "dreiding", "waldmanhagler"), "context a, dreiding")
    _check_rd(rb, ref.rd_terms(rc.system("t130"), rc.BASE, "sg"), "context b, sg (frozen-frozen pairs left out)")
    # insert / remove answer "upload again" while a form is on, and change nothing
    z = np.zeros(1)
    assert a.insert_molecule(np.zeros((1, 3)), z, z, z + 30.0, z + 3.0, z + 14.0) is None
    assert a.remove_molecule(319, 1) is False
    assert a.energy() == ra
    a.set_rd_form("off")
    b.set_rd_form(None)
    a.energy_begin()
    b.energy_begin()
    assert b.energy_end() == b_before
    assert a.energy_end() == before

    # ... and the same in a scaled box; the LJ form's long-range correction follows the volume
    assert a.scale_box(basis, delta) is True
    before_scaled = a.energy()
    assert before_scaled["rd_energy"] != before["rd_energy"]
    a.set_rd_form("lj", "halgren_mixing")
    _check_rd(a.energy(), ref.rd_terms(scaled, rc.POLAR, "lj", "halgren_mixing"), "context a, lj form, scaled box")
    a.set_rd_form("off")
    assert a.energy() == before_scaled
    a.set_rd_form("lj", "halgren_mixing")
    assert a.scale_box(s["basis"], -delta) is True  # a volume move while the form is on
    back = dict(scaled, pos=scaled["pos"] - delta[ids], basis=s["basis"])
    _check_rd(a.energy(), ref.rd_terms(back, rc.POLAR, "lj", "halgren_mixing"), "context a, lj form, box scaled back")
    a.set_rd_form("off")
    a.energy()
    assert a.remove_molecule(319, 1) is True  # device-side edits are back
    a.close()
    b.close()


def test_setting_persists_across_uploads_and_is_refused_in_flight():
    s = rc.system("t65")
    e = _engine(s, dict(rc.flags("t65", rc.BASE, "lj_buffered_14_7", "halgren_mixing"), rd_only=1))
    on = e.energy()
    e.upload(s)
    assert e.energy() == on
    e.energy_begin()
    with pytest.raises(engine.EngineError, match="between energy_begin"):
        e.set_rd_form("off")
    assert e.energy_end() == on
    with pytest.raises(ValueError):
        e.set_rd_form("morse")
    with pytest.raises(engine.EngineError, match="outside 0 .. 4"):
        p = engine.RdFormParams(7, 0)
        engine._chk(e.lib.mpmc_hip_set_rd_form(e.ctx, p))
    assert e.energy() == on
    e.close()


def test_refusals_by_name():
    s = rc.system("t65")
    e = _engine(s, dict(rc.BASE, rd_only=1))
    e.set_rd_form("sg", "halgren_mixing")
    with pytest.raises(engine.EngineError, match="sg form takes no mixing rule"):
        e.energy()
    e.set_rd_form("dreiding", "waldmanhagler")  # t65 has a sigma < 0
    with pytest.raises(engine.EngineError, match="waldmanhagler mixing with a negative sigma"):
        e.energy()
    e.set_rd_form("dreiding")
    e.set_rd_crystal(2)
    with pytest.raises(engine.EngineError, match="set_rd_form with rd_crystal"):
        e.energy()
    e.set_rd_crystal(0)
    assert e.energy()["status"] == 0
    e.close()
    p = synth.s_phahst(130)
    e = _engine(p, dict(synth.FLAGS_PHAHST, dreiding=1))
    with pytest.raises(engine.EngineError, match="set_rd_form with disp_expansion"):
        e.energy()
    e.close()


def test_axilrod_teller_beside_a_form():
    s = synth.s_at(130)
    f = dict(synth.FLAGS_AT, dreiding=1)
    got = _fresh(s, f)
    lj = _fresh(s, dict(synth.FLAGS_AT))
    _check_rd(got, ref.rd_terms(s, f, "dreiding"), "s_at(130) dreiding + axilrod_teller")
    assert got["coulombic_energy"] == lj["coulombic_energy"]
    assert got["energy"] - got["rd_energy"] == pytest.approx(lj["energy"] - lj["rd_energy"], rel=1e-12)
