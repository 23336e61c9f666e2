"""GPU tests of the pair / static-field screen and of the cutoff comparisons with adversarial geometry
(tests/adversarial.py): the engine against the per-pair reference (tests/pair_reference.py) AND against the oracle,
at the bars the parity tests use (check_energies with RTOL = 1e-10; per-atom ef_static to 1e-11 of its largest
component).  A failure names the probe pairs whose removal from (or addition to) the reference table explains the
difference best.  Ordinary energy calls on boxes of <= 950 atoms; nothing here provokes a fault."""
import numpy as np
import pytest

import adversarial as adv
import pair_reference as pr
from mpmc_amd import engine
from oracle import oracle
from test_gpu_parity import RTOL, check_energies, rel

pytestmark = pytest.mark.gpu

FIELD_TOL = 1e-11
PLAIN_OPTIONS = ("fuse_field", "fuse_moves", "side_moves", "split_record", "fuse_recip")  # as test_fused_first_launch...


def probe_rows(inp, t):
    key = {(min(a, b), max(a, b)) for a, b in inp["probes"].tolist()}
    return np.array([k for k in range(len(t["i"])) if (int(t["i"][k]), int(t["j"][k])) in key], dtype=np.int64)


def compare(inp, p, got, ef_static, what=""):
    """got (Result dict) and ef_static (or None) against the reference table and the oracle; returns nothing, raises
    with the named pairs."""
    s = inp["system"]
    pol = bool(p.get("polarization")) and not p.get("rd_only")
    want = oracle.energy(s, p, want_vectors=pol)
    t = pr.pair_table(s, p)
    ref = pr.sums(t, s, p)
    rows = probe_rows(inp, t)
    msgs = []
    for key, chan in (("rd_energy", "rd"), ("es_real", "es")):
        for name, w in (("per-pair reference", ref[key]), ("oracle", want[key])):
            if not rel(got[key], w) < RTOL:
                msgs.append("%s %s: engine %.17g, %s %.17g, difference %.6e" % (what, key, got[key], name, w, got[key] - w))
                msgs += ["    " + m for m in pr.explain_energy(t, chan, got[key] - float(ref[key]), rows)]
    try:
        check_energies(got, want)
    except AssertionError as e:
        msgs.append("%s check_energies vs oracle: %s" % (what, e))
    if pol:
        for name, w in (("per-pair reference", ref["ef_static"]), ("oracle", want["ef_static"])):
            scale = np.abs(w).max()
            err = np.abs(ef_static - w).max()
            if not err <= FIELD_TOL * scale:
                msgs.append("%s ef_static vs %s: max error %.6e, allowed %.6e" % (what, name, err, FIELD_TOL * scale))
                msgs += ["    " + m for m in pr.explain_field(t, ef_static, ref["ef_static"])]
    assert not msgs, "\n".join(msgs)


def open_engine(s, p, plain=False, extra=0):
    e = engine.Engine(len(s["charge"]) + extra)
    e.load_system(s, p)
    if plain:
        for o in PLAIN_OPTIONS:
            e.set_option(o, 0)
    return e


def full(e, p):
    r = e.energy()
    ef = e.dipoles()["ef_static"] if (p.get("polarization") and not p.get("rd_only")) else None
    return r, ef


# every class x every kernel variant
FULL_INPUTS = ["T_sheared", "T_hexagonal", "T_monoclinic", "E", "F_T_sheared", "F_T_hexagonal", "F_E", "B_T_hexagonal",
               "B_T_monoclinic", "B_E"]
CASES = [(i, v) for i in FULL_INPUTS for v in sorted(adv.VARIANTS)]
CASES += [(i, v) for i in ("F_T_monoclinic", "B_T_sheared") for v in ("ewald_fh0", "field_bare")]


@pytest.mark.parametrize("name,variant", CASES)
def test_engine_matches_per_pair_reference_and_oracle(name, variant):
    inp = adv.get(name)
    p = adv.params_for(inp, variant)
    e = open_engine(inp["system"], p)
    try:
        got, ef = full(e, p)
    finally:
        e.close()
    compare(inp, p, got, ef, "%s / %s:" % (name, variant))


def _same(a, b, what):
    for k in a[0]:
        if k in b[0] and isinstance(a[0][k], (int, float)):
            assert a[0][k] == b[0][k], (what, k, a[0][k], b[0][k])
    if a[1] is not None:
        assert np.array_equal(a[1], b[1]), what


INCREMENTAL = [("T_sheared", "ewald_fh2"), ("T_hexagonal", "field_bare"), ("T_monoclinic", "field_wolfA"),
               ("E", "ewald_fh0"), ("E", "wolf"), ("E", "field_bare"), ("E", "field_ewald"), ("F_T_sheared", "field_wolf0"),
               ("B_T_hexagonal", "ewald_fh4"), ("F_E", "rd_only")]


@pytest.mark.parametrize("plain", [0, 1])
@pytest.mark.parametrize("name,variant", INCREMENTAL)
def test_moves_onto_adversarial_positions_are_bit_identical_to_a_fresh_engine(name, variant, plain):
    """The dirty-tile pass: a dozen probe partners start 1 A away and are moved ONTO their adversarial positions, one
    molecule per energy() (with the fused launches -- field_coef_kernel, pair_recip_kernel -- and, plain = 1, with every
    launch on its own).  Every result field and ef_static == a fresh engine on the final coordinates, and both follow
    the reference."""
    inp = adv.get(name)
    s, p = inp["system"], adv.params_for(inp, variant)
    pick = inp["probes"][np.linspace(0, len(inp["probes"]) - 1, 12).astype(int), 1]
    start = dict(s, pos=s["pos"].copy())
    start["pos"][pick] += np.array([0.6, -0.64, 0.48])  # |.| = 1 A
    e = open_engine(start, p, plain)
    fresh = open_engine(s, p)
    try:
        e.energy()
        for j in pick:
            e.update_atoms(int(j), s["pos"][j:j + 1])
            e.energy()
        got, want = full(e, p), full(fresh, p)
    finally:
        e.close()
        fresh.close()
    _same(got, want, "%s / %s after the moves" % (name, variant))
    compare(inp, p, got[0], got[1], "%s / %s after the moves:" % (name, variant))


@pytest.mark.parametrize("name,variant", [("T_sheared", "field_bare"), ("E", "ewald_fh0"), ("E", "field_ewald")])
def test_remove_and_insert_of_a_probe_molecule(name, variant):
    """A probe partner leaves through remove_molecule and comes back through insert_molecule into the hole it left: the
    atom order is the upload's again, so every result field == a fresh engine."""
    inp = adv.get(name)
    s, p = inp["system"], adv.params_for(inp, variant)
    j = int(inp["probes"][len(inp["probes"]) // 2, 1])
    e = open_engine(s, p, extra=64)
    fresh = open_engine(s, p)
    try:
        e.energy()
        assert e.remove_molecule(j, 1)
        without = e.energy()
        assert without["n_atoms"] == len(s["charge"]) - 1
        back = e.insert_molecule(s["pos"][j:j + 1], s["charge"][j:j + 1], s["alpha"][j:j + 1], s["epsilon"][j:j + 1],
                                 s["sigma"][j:j + 1], s["mass"][j:j + 1])
        assert back == j
        got, want = full(e, p), full(fresh, p)
    finally:
        e.close()
        fresh.close()
    _same(got, want, "%s / %s after remove + insert" % (name, variant))
    compare(inp, p, got[0], got[1], "%s / %s after remove + insert:" % (name, variant))


@pytest.mark.parametrize("variant", ["ewald_fh0", "field_bare"])
def test_scale_box_onto_a_sheared_cell_with_near_ties(variant):
    """mpmc_hip_scale_box rebuilds the screen's fp32 basis copies, rc2_pre and the half-integer guard: a class-T
    configuration loaded in a cell 3 % larger (where its pairs are no ties) and brought to its own cell by a volume move
    with zero displacements (so every coordinate keeps its bits) == a fresh engine, and follows the reference."""
    inp = adv.get("T_hexagonal")
    s, p = inp["system"], adv.params_for(inp, variant)
    big = dict(s, basis=s["basis"] * 1.03)
    e = open_engine(big, p)
    fresh = open_engine(s, p)
    try:
        e.energy()
        assert e.scale_box(s["basis"], np.zeros((len(s["charge"]), 3))) is True
        got, want = full(e, p), full(fresh, p)
    finally:
        e.close()
        fresh.close()
    _same(got, want, "T_hexagonal / %s after scale_box" % variant)
    compare(inp, p, got[0], got[1], "T_hexagonal / %s after scale_box:" % variant)
