"""CPU tests of the adversarial inputs (tests/adversarial.py): the conditions that make a GPU pass of
tests/test_gpu_screen_edges.py meaningful.  These are conditions on the inputs, checked with the per-pair reference and a
numpy emulation of the fp32 screen -- not measurements of the engine."""
import numpy as np
import pytest

import adversarial as adv
import pair_reference as pr

RTOL, FIELD_TOL = 1e-10, 1e-11  # the bars of the GPU tests
WEIGHT = 100.0  # a probe pair weighs at least this many tolerances in every channel it belongs to

T_LIKE = [n for n in adv.ALL_NAMES if "T_" in n]
E_LIKE = [n for n in adv.ALL_NAMES if n.endswith("E")]


def probe_rows(inp, t):
    index = {(int(i), int(j)): k for k, (i, j) in enumerate(zip(t["i"], t["j"]))}
    return np.array([index.get((min(a, b), max(a, b)), -1) for a, b in inp["probes"].tolist()])


@pytest.mark.parametrize("name", adv.ALL_NAMES)
def test_counts_coverage_and_nothing_filtered(name):
    inp = adv.get(name)
    s = inp["system"]
    n = len(s["charge"])
    P = inp["probes"]
    # the builder fills every planned slot by drawing again, so no filter reduces a probe set: the planned count ships
    planned = adv.T_PAIRS if "T_" in name else len(adv.e_targets(adv.RC_E, 1e-15)) * 6 * adv.E_REPEAT
    assert planned == (288 if "T_" in name else 16 * 6 * 4)
    assert len(P) == len(inp["labels"]) == planned
    assert len(P) >= 256 and len(set(map(tuple, P.tolist()))) == len(P)
    assert n % 64 != 0 and n <= 1100
    c = adv.coverage(n, P)
    assert adv.covered(c), c
    assert c["columns"] == 64  # every column index mod 64, hence all eight waves' column groups
    atoms = P.ravel()
    assert np.all(s["epsilon"][atoms] != 0) and np.all(s["sigma"][atoms] != 0) and np.all(s["alpha"][atoms] != 0)
    assert np.all(s["charge"][P[:, 0]] * s["charge"][P[:, 1]] < 0)  # charged pair, charged partner of a field site
    top = np.abs(s["pos"]).max()
    if name.startswith("F_"):
        assert top > 2048.0 and s["charge"][-1] == 0 and s["epsilon"][-1] == 0 and s["alpha"][-1] == 0
        base = adv.get(name[2:])["system"]
        assert np.array_equal(s["pos"][:-1], base["pos"])  # every probe coordinate bit-identical
    elif name.startswith("B_"):
        assert 2048.0 - 64.0 < top < 2048.0
    else:
        assert top < 64.0


@pytest.mark.parametrize("name", T_LIKE)
def test_class_T_pairs_are_near_ties_inside_the_cutoff_that_the_old_fp32_screen_loses(name):
    inp = adv.get(name)
    s, P = inp["system"], inp["probes"]
    basis = s["basis"]
    vol, rb, rc = pr.pbc(basis)
    d = s["pos"][P[:, 0]] - s["pos"][P[:, 1]]
    image, _, rimg, _ = pr.minimum_image(basis, rb, d)
    f = adv.fractional(rb, d)
    ks = np.array([l["k"] for l in inp["labels"]])
    dl = np.array([l["delta"] for l in inp["labels"]])
    fk = f[np.arange(len(P)), ks]
    assert np.all(np.abs(np.abs(fk) - 0.5) <= dl + 1e-10)
    other = image.copy()
    ik = image[np.arange(len(P)), ks]
    other[np.arange(len(P)), ks] = np.where(ik == np.ceil(fk), np.floor(fk), np.ceil(fk))
    r_other = np.linalg.norm(d - other @ basis, axis=1)
    assert np.all(rimg <= rc - adv.T_INSIDE) and np.all(r_other >= rc + adv.SCREEN_MARGIN + adv.T_INSIDE)
    # every feasible direction, both signs, both sides of the tie, every delta; the directions left out cannot hold a
    # near-tie pair inside the cutoff at all (adversarial.feasible_directions)
    feasible = adv.feasible_directions(basis)
    assert len(feasible) >= 2
    for k in range(3):
        h_half = 0.5 / np.linalg.norm(rb[:, k])
        assert (k in feasible) == (h_half < rc - adv.T_INSIDE)
    combos = {(l["k"], l["sign"], l["side"], l["delta"]) for l in inp["labels"]}
    assert combos == {(k, sg, sd, x) for k in feasible for sg in (1.0, -1.0) for sd in (1.0, -1.0) for x in adv.DELTAS}
    # the fp32 screen as it stood before the half-integer guard loses a good part of them ...
    if not name.startswith("F_"):  # (class F never runs the fp32 screen)
        lost = ~adv.screen_f32(basis, rb, rc, s["pos"][P[:, 0]], s["pos"][P[:, 1]])
        assert lost.mean() >= 0.25, lost.mean()
        # ... and with the guard, at the engine's bound, none
        assert adv.screen_f32(basis, rb, rc, s["pos"][P[:, 0]], s["pos"][P[:, 1]], adv.tie_guard32(rb)).all()


def test_the_three_cells_cover_every_tie_direction():
    assert set().union(*[adv.feasible_directions(b) for b in adv.CELLS.values()]) == {0, 1, 2}
    assert adv.feasible_directions(np.diag([25.0, 25.0, 25.0])) == []  # cubic: a tie sits at >= rc


@pytest.mark.parametrize("name", E_LIKE)
def test_class_E_distances_split_the_three_cutoff_comparisons(name):
    inp = adv.get(name)
    s = inp["system"]
    tabs = {v: pr.pair_table(s, adv.params_for(inp, v)) for v in ("ewald_fh0", "wolf", "field_bare", "field_ewald")}
    rows = probe_rows(inp, tabs["ewald_fh0"])
    assert np.all(rows >= 0)  # every probe pair is in the table (within `keep` of the cutoff)
    t = tabs["ewald_fh0"]
    rc = t["rc"]
    assert rc == adv.RC_E
    names = [l["name"] for l in inp["labels"]]
    for nm in set(names):
        assert names.count(nm) == 6 * adv.E_REPEAT  # every distance: 3 axes x 2 signs x repeats
    got = {}
    for k, l in zip(rows, inp["labels"]):
        dec = (bool(t["in_rd"][k]), bool(t["in_es"][k]), bool(tabs["wolf"]["in_es"][_row(tabs["wolf"], t, k)]),
               bool(tabs["field_bare"]["in_field"][_row(tabs["field_bare"], t, k)]),
               bool(tabs["field_ewald"]["in_field"][_row(tabs["field_ewald"], t, k)]))
        got.setdefault(l["name"], set()).add(dec)
        if inp["shift"] == 0.0:
            assert t["rimg"][k] == l["target"]  # exact distances: the partner coordinate IS the distance
        else:
            assert abs(t["rimg"][k] - l["target"]) <= np.spacing(inp["shift"] + rc)
    # (LJ `rimg - 1e-12 < rc`, Ewald `!(rimg > rc)`, Wolf `rimg < rc`, bare field as LJ, Ewald field as Ewald)
    expect = {
        "rc-2ulp": (True, True, True, True, True), "rc-1ulp": (True, True, True, True, True),
        "rc+0ulp": (True, True, False, True, True),
        "rc+1ulp": (True, False, False, True, False), "rc+2ulp": (True, False, False, True, False),
        "rc+0.5e-12": (True, False, False, True, False),
        "rc+2e-12": (False,) * 5, "rc+1e-9-": (False,) * 5, "rc+1e-9": (False,) * 5, "rc+1e-9+": (False,) * 5,
        "rc+0.005": (False,) * 5, "rc+0.0099": (False,) * 5, "rc+0.0101": (False,) * 5,
        "rc-0.005": (True,) * 5, "rc-1e-9": (True,) * 5,
    }
    for nm, want in expect.items():
        assert got[nm] == {want}, (nm, got[nm])
    assert len(got["rc+1e-12"]) == 1  # decided by fp64 rounding of (rc + 1e-12) - 1e-12; whatever it is, one answer
    # the three comparisons disagree on the edge: at rimg == rc and just above it
    assert len({expect["rc+0ulp"][c] for c in (0, 1, 2)}) == 2 and len({expect["rc+1ulp"][c] for c in (0, 1, 2)}) == 2


def _row(tab, t, k):
    """row of pair t[k] in another variant's table"""
    hit = np.flatnonzero((tab["i"] == t["i"][k]) & (tab["j"] == t["j"][k]))
    assert len(hit) == 1
    return int(hit[0])


WEIGHT_CASES = [(n, v) for n in adv.ALL_NAMES for v in sorted(adv.VARIANTS)]


@pytest.mark.parametrize("name,variant", WEIGHT_CASES)
def test_one_probe_pair_cannot_hide_in_the_tolerance(name, variant):
    """Each probe pair's term in each channel it belongs to is >= 100 x the absolute tolerance the GPU test applies to that
    channel on that input.  Exception by construction: the Wolf FIELDS are shifted so that they vanish at the cutoff
    (thole_field.c:82-83), so a pair AT the edge weighs nothing there whichever way the comparison goes; for them the
    condition is asserted on the class-T pairs (>= 0.5 A inside) and on the E pairs at rc - 0.005 only."""
    inp = adv.get(name)
    s, p = inp["system"], adv.params_for(inp, variant)
    t = pr.pair_table(s, p)
    ref = pr.sums(t, s, p)
    rows = probe_rows(inp, t)
    assert np.all(rows >= 0)  # every probe pair is in the table (inside the cutoff, or within `keep` of it)
    if "T_" in name:  # class T: every probe pair belongs to every channel of the variant
        assert t["in_rd"][rows].all()
        assert p.get("rd_only") or t["in_es"][rows].all()
        assert not pr.field_mode(p) or t["in_field"][rows].all()
    tol_rd = RTOL * max(1.0, abs(ref["rd_energy"]))
    tol_es = RTOL * max(1.0, abs(ref["es_real"]))
    k = rows[t["in_rd"][rows]]
    assert len(k) and np.abs(t["rd"][k]).min() >= WEIGHT * tol_rd, (np.abs(t["rd"][k]).min(), tol_rd)
    if not p.get("rd_only"):
        k = rows[t["in_es"][rows]]
        assert len(k) and np.abs(t["es"][k]).min() >= WEIGHT * tol_es, (np.abs(t["es"][k]).min(), tol_es)
    if pr.field_mode(p):
        tol_f = FIELD_TOL * np.abs(ref["ef_static"]).max()
        k = rows[t["in_field"][rows]]
        if pr.field_mode(p) == "wolf" and "E" == name[-1]:
            k = k[t["rimg"][k] <= t["rc"] - 0.004]
        assert len(k)
        mag = np.minimum(np.abs(t["field_i"][k]).max(axis=1), np.abs(t["field_j"][k]).max(axis=1))
        assert mag.min() >= WEIGHT * tol_f, (float(mag.min()), tol_f)
