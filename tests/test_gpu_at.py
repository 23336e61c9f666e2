"""GPU tests of the Axilrod-Teller three-body term (axilrod_teller): at_triple_kernel (mpmc_amd/csrc/kernels_at.h) through
mpmc_hip_set_axilrod_teller / mpmc_hip_get_three_body_energy, against tests/at_reference.py.

The tolerance is 1e-12 * sum |terms|, the project's own for a dense fp64 sum.  The inputs
(tests/at_cases.py) are the smallest at which the tiling can go wrong -- 130 atoms: three blocks, the last with two
atoms, so that block triples of the kinds I<J<K, I=J<K, I<J=K and I=J=K all occur; 200: several I<J<K triples; 320: the
frozen framework molecule across a block boundary; the 130 in a sheared cell -- and tests/test_at_reference.py checks
on the CPU that in each of them the smallest non-zero term is at least 100 tolerances: one dropped or doubled triple
fails the comparison.
"""
import os
import subprocess

import numpy as np
import pytest

import at_cases as ac
import at_reference as ref
from mpmc_amd import engine, host, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = [f for f, _ in engine.Result._fields_]

AT_ON = dict(axilrod_teller=1)
VARIANTS = {
    "lj": dict(synth.FLAGS_AT),
    "rd_only": dict(synth.FLAGS_LJ, **AT_ON),
    "midzuno_kihara": dict(synth.FLAGS_AT, midzuno_kihara_approx=1),
    "phahst": dict(synth.FLAGS_PHAHST, **AT_ON),
}


def _system(name, variant):
    s = ac.case(name)
    if variant == "phahst":  # the epsilon / sigma columns become the exponent b and the range rho; c8, c10 from c6
        on = s["epsilon"] != 0.0
        s = dict(s, epsilon=np.where(on, 3.2, 0.0), sigma=np.where(on, 2.9, 0.0), c8=20.0 * s["c6"], c10=500.0 * s["c6"])
    return s


def _off(flags):
    return {k: v for k, v in flags.items() if k not in engine.AT_NAMES}


def _engine(s, flags, cap=None, **options):
    e = engine.Engine(cap or len(s["charge"]))
    for k, v in options.items():
        e.set_option(k, v)
    e.load_system(s, flags)
    return e


def _fresh(s, flags):
    """(result record, three-body energy, dipoles or None) of a new context"""
    e = _engine(s, flags)
    r = e.energy()
    t = e.three_body_energy()
    d = e.dipoles() if flags.get("polarization") and not flags.get("rd_only") else None
    e.close()
    return r, t, d


def _check(three, u, what):
    tol = ac.TOLERANCE * u.sum_abs
    err = abs(three - u.total)
    print("%s: three_body %.15g reference %.15g |diff| %.3g tol %.3g (%.3g of it); smallest term %.3g" %
          (what, three, u.total, err, tol, err / tol, u.min_nonzero))
    assert err <= tol, (what, three, u.total, err, tol)


@pytest.mark.parametrize("name", ac.NAMES)
@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_three_body_energy_against_the_reference(name, variant):
    s, flags = _system(name, variant), VARIANTS[variant]
    u = ac.reference(name, bool(flags.get("midzuno_kihara_approx")))
    assert u.min_nonzero >= ac.MARGIN * ac.TOLERANCE * u.sum_abs  # (tests/test_at_reference.py: the inputs' condition)
    got, three, dip = _fresh(s, flags)
    _check(three, u, "%s/%s" % (name, variant))
    assert got["status"] == 0 and got["n_atoms"] == len(s["charge"])
    # the term is part of `energy` and of nothing else: without it, bit for bit what the same atoms give with the term off
    bare, zero, bare_dip = _fresh(s, _off(flags))
    assert zero == 0.0
    print("energy %.17g - three_body = %.17g; term off %.17g" % (got["energy"], got["energy"] - three, bare["energy"]))
    # fl(fl(E + t) - t) == E: E + t is rounded to the grid of E's binade or a finer one (t > 0 > E and |t| < |E| / 2 in
    # every case here, asserted), so the difference lies within half a grid step of E and rounds back to it
    assert bare["energy"] < 0.0 < three < -0.5 * bare["energy"]
    assert got["energy"] - three == bare["energy"]
    for f in FIELDS:
        if f != "energy":
            assert got[f] == bare[f], (f, got[f], bare[f])
    if dip is not None:
        for k in dip:
            assert np.array_equal(dip[k], bare_dip[k]), k


def test_every_site_active():
    """synth.s_at(130) as it comes -- 2.4e5 non-zero triples, every lane of every block triple busy -- to the same
    tolerance (a single triple is below it here, see tests/at_cases.py: this is a check of the sum, not of the tiling)."""
    s = synth.s_at(130)
    for mk in (False, True):
        flags = dict(synth.FLAGS_AT, midzuno_kihara_approx=int(mk))
        got, three, _ = _fresh(s, flags)
        _check(three, ref.unordered(s, mk), "s_at(130) mk=%d" % mk)
        assert got["status"] == 0


def _mover(s):
    mol = np.asarray(s["molecule"])
    frozen = np.asarray(s["frozen"])

    def move(pos, m, rng):
        idx = np.flatnonzero(mol == m)
        assert not frozen[idx].any()
        c = pos[idx].mean(axis=0)
        th = rng.uniform(-0.2, 0.2)
        rot = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
        return int(idx[0]), (pos[idx] - c) @ rot.T + c + rng.uniform(-0.15, 0.15, 3)

    return move


def _molecule_list(s, count, rng):
    """molecules to move: those of the sites that carry the term first (the sorbates across a block boundary and next to
    the framework among them), then others at random"""
    mol, frozen = np.asarray(s["molecule"]), np.asarray(s["frozen"])
    first = []
    for a in s["active"]:
        if not frozen[a] and mol[a] not in first:
            first.append(int(mol[a]))
    others = [int(m) for m in np.unique(mol[frozen == 0]) if m not in first]
    picks = first + rng.choice(others, size=max(0, count - len(first)), replace=False).tolist()
    return picks[:count]


@pytest.mark.parametrize("variant", ["lj", "phahst"])
def test_incremental_pass_leaves_the_bits_of_a_from_scratch_pass(variant):
    s, flags = _system("n320", variant), VARIANTS[variant]
    rng = np.random.default_rng(17)
    move = _mover(s)
    picks = _molecule_list(s, 20, rng)
    straddling = [int(s["molecule"][b]) for b in range(64, 320, 64)
                  if s["molecule"][b - 1] == s["molecule"][b] and not s["frozen"][b]]  # (the framework sits across one too)
    assert straddling and set(straddling) <= set(picks)
    live, full = _engine(s, flags), _engine(s, flags, incremental_pairs=0)
    assert live.energy() == full.energy() and live.three_body_energy() == full.three_body_energy()
    cur = dict(s, pos=s["pos"].copy())
    for step, m in enumerate(picks):
        first, new = move(cur["pos"], m, rng)
        cur["pos"][first:first + len(new)] = new
        live.update_atoms(first, new)
        full.update_atoms(first, new)
        a, b = live.energy(), full.energy()
        c, three, _ = _fresh(cur, flags)
        assert live.three_body_energy() == three, ("live vs fresh", step, live.three_body_energy(), three)
        assert full.three_body_energy() == three, ("incremental_pairs = 0 vs fresh", step)
        for f in FIELDS:
            assert a[f] == c[f], ("live vs fresh", step, f, a[f], c[f])
            assert b[f] == c[f], ("incremental_pairs = 0 vs fresh", step, f, b[f], c[f])
    _check(live.three_body_energy(), ref.unordered(cur), "after 20 moves")
    # the same evaluation again, and in two halves: the same bits
    assert live.energy() == a and live.three_body_energy() == three
    live.energy_begin()
    assert live.energy_end() == a and live.three_body_energy() == three
    live.close()
    full.close()


def test_scale_box_and_revert():
    s, flags = _system("n320", "lj"), VARIANTS["lj"]
    mol = np.asarray(s["molecule"])
    ids = np.cumsum(np.concatenate([[0], mol[1:] != mol[:-1]]))
    com = np.stack([s["pos"][ids == m].mean(axis=0) for m in range(ids[-1] + 1)])
    live, full = _engine(s, flags), _engine(s, flags, incremental_pairs=0)
    first = live.energy(), live.three_body_energy()
    full.energy()
    cur = dict(s, pos=s["pos"].copy(), basis=s["basis"].copy())
    for scale in (1.03, None):
        if scale is not None:
            f = scale ** (1.0 / 3.0)
            delta, basis = com * (f - 1.0), s["basis"] * f
        else:
            delta, basis = -delta, s["basis"].copy()
        cur["pos"] = cur["pos"] + delta[ids]  # the very addition the engine does
        cur["basis"] = basis
        assert live.scale_box(basis, delta) is True and full.scale_box(basis, delta) is True
        a, b = live.energy(), full.energy()
        c, three, _ = _fresh(cur, flags)
        assert live.three_body_energy() == three and full.three_body_energy() == three
        for fld in FIELDS:
            assert a[fld] == c[fld] and b[fld] == c[fld], (scale, fld, a[fld], b[fld], c[fld])
        _check(three, ref.unordered(cur), "scale %s" % scale)
    assert abs(three - first[1]) <= ac.TOLERANCE * ref.unordered(cur).sum_abs  # back where it started
    live.close()
    full.close()


def test_a_move_over_more_blocks_than_the_list_holds_is_a_full_pass():
    """update_atoms over all 18 blocks of a 1100-atom box (the dirty-block list holds 16): the same bits as a fresh
    context and as incremental_pairs = 0."""
    s, flags = synth.s_at(1100), VARIANTS["rd_only"]
    assert (1100 + 63) // 64 > 16
    live, full = _engine(s, flags), _engine(s, flags, incremental_pairs=0)
    live.energy()
    full.energy()
    rng = np.random.default_rng(5)
    new = s["pos"] + rng.uniform(-0.05, 0.05, s["pos"].shape)
    live.update_atoms(0, new)
    full.update_atoms(0, new)
    a, b = live.energy(), full.energy()
    c, three, _ = _fresh(dict(s, pos=new), flags)
    assert three != 0.0 and live.three_body_energy() == three and full.three_body_energy() == three
    assert a == c and b == c
    # ... and a single-molecule move afterwards is incremental again, with a fresh context's bits
    idx = np.flatnonzero(np.asarray(s["molecule"]) == s["molecule"][700])
    moved = new.copy()
    moved[idx] += 0.1
    live.update_atoms(int(idx[0]), moved[idx])
    a = live.energy()
    c, three, _ = _fresh(dict(s, pos=moved), flags)
    assert a == c and live.three_body_energy() == three
    live.close()
    full.close()


def test_mode_switching():
    s, flags = _system("n130", "lj"), VARIANTS["lj"]
    u = ac.reference("n130")
    bare, _, _ = _fresh(s, _off(flags))
    e = _engine(s, flags, cap=192)
    on = e.energy()
    _check(e.three_body_energy(), u, "on")
    # grand-canonical edits answer "upload again" in this mode
    idx = np.flatnonzero(np.asarray(s["molecule"]) == s["molecule"][-1])
    assert e.remove_molecule(int(idx[0]), len(idx)) is False
    z = np.zeros(1)
    assert e.insert_molecule(np.zeros((1, 3)), z, z + 1.0, z + 100.0, z + 3.4, z + 40.0) is None
    assert e.energy() == on
    # enable = 0: exact 0 and the energies of a context that never had the term
    e.set_axilrod_teller(s, enable=False)
    assert e.energy() == bare and e.three_body_energy() == 0.0
    e.set_axilrod_teller(s)
    assert e.energy() == on
    _check(e.three_body_energy(), u, "on again")
    # Midzuno-Kihara on the same context
    e.set_axilrod_teller(s, midzuno_kihara_approx=True)
    e.energy()
    _check(e.three_body_energy(), ac.reference("n130", True), "midzuno_kihara on the same context")
    # an upload without the call switches the term off
    e.load_system(s, _off(flags))
    assert e.energy() == bare and e.three_body_energy() == 0.0
    assert e.remove_molecule(int(idx[0]), len(idx)) is True  # ... and device-side edits are back
    e.load_system(s, flags)
    assert e.energy() == on
    # errors, not crashes: wrong n, null array, a negative polarizability
    c9 = np.ascontiguousarray(s["c9"])
    assert e.lib.mpmc_hip_set_axilrod_teller(e.ctx, 1, 129, c9.ctypes.data) != 0
    assert e.lib.mpmc_hip_set_axilrod_teller(e.ctx, 1, 130, None) != 0
    bad = dict(s, alpha=s["alpha"].copy())
    bad["alpha"][5] = -0.5
    e.load_system(bad, _off(flags))
    with pytest.raises(engine.EngineError, match="negative polarizability"):
        e.set_axilrod_teller(bad)
    assert e.three_body_energy() == 0.0
    e.close()


def test_two_contexts_side_by_side():
    a, b = _engine(_system("n130", "phahst"), VARIANTS["phahst"]), _engine(_system("n130_triclinic", "lj"), VARIANTS["lj"])
    a.energy_begin()
    b.energy_begin()
    b.energy_end()
    a.energy_end()
    _check(a.three_body_energy(), ac.reference("n130"), "context a")
    _check(b.three_body_energy(), ac.reference("n130_triclinic"), "context b")
    first, new = 63, _system("n130", "phahst")["pos"][63:65] + 0.1
    a.update_atoms(first, new)
    a.energy()
    assert b.energy() is not None
    _check(b.three_body_energy(), ac.reference("n130_triclinic"), "context b after a's move")
    assert a.three_body_energy() != b.three_body_energy()
    a.close()
    b.close()


def _chain(s, flags):
    h = host.HostSystem(s, flags, seed=9, move_factor=0.05, rot_factor=0.05)
    h.mc_steps(40)
    out = h.observables(), h.three_body_energy(), h.positions()
    h.close()
    return out


def test_host_layer_chain():
    """40 NVT steps through the C host layer with the term on: bit-identical run to run, and the three_body_energy it
    carries is the reference's on its final positions."""
    s, flags = ac.case("n130"), synth.FLAGS_AT
    o1, t1, p1 = _chain(s, flags)
    o2, t2, p2 = _chain(s, flags)
    assert o1 == o2 and t1 == t2 and np.array_equal(p1, p2)
    assert o1["accept"] + o1["reject"] == 40 and o1["accept"] > 0
    final = dict(s, pos=p1)
    _check(t1, ref.unordered(final), "after the chain")
    got, three, _ = _fresh(final, flags)
    assert o1["energy"] == got["energy"] and t1 == three


def _pqr_system(s):
    """s as PQR text (reference column layout: c6 c8 c10 c9 after omega and gwp_alpha) and read back the way the host
    layer reads it, so that both sides hold the same doubles"""
    lines, cols = [], []
    for i in range(len(s["charge"])):
        t = ["%.3f" % v for v in s["pos"][i]] + ["%.4f" % s["mass"][i], "%.5f" % (s["charge"][i] / synth.E2REDUCED),
                                                  "%.5f" % s["alpha"][i], "%.5f" % s["epsilon"][i], "%.5f" % s["sigma"][i],
                                                  "0.0", "0.0", "%.4f" % s["c6"][i], "0.0", "0.0", "%.4f" % s["c9"][i]]
        lines.append("ATOM  %5d X    M   %s %4d   %s" % (i + 1, "F" if s["frozen"][i] else "M", s["molecule"][i], " ".join(t)))
        cols.append([float(x) for x in t])
    c = np.array(cols)
    out = dict(s, pos=c[:, 0:3].copy(), mass=c[:, 3].copy(), charge=c[:, 4] * synth.E2REDUCED, alpha=c[:, 5].copy(),
               epsilon=c[:, 6].copy(), sigma=c[:, 7].copy(), c6=c[:, 10].copy(), c9=c[:, 13].copy())
    return "\n".join(lines) + "\nEND\n", out


def test_driver_runs_an_axilrod_teller_input(tmp_path):
    """mpmc_hip on an `axilrod_teller on` input written here: the energy column of its step-0 line is the engine's energy
    of the same numbers, three-body term included."""
    text, s = _pqr_system(ac.case("n130"))
    (tmp_path / "in.pqr").write_text(text)
    L = float(s["basis"][0, 0])
    out = tmp_path / "energy.dat"
    (tmp_path / "input").write_text(
        "job_name at\nensemble nvt\npreset_seeds 4321\nnumsteps 4\ncorrtime 2\nmove_factor 0.01\nrot_factor 0.01\n"
        "temperature 100.0\naxilrod_teller on\nbasis1 %r 0 0\nbasis2 0 %r 0\nbasis3 0 0 %r\nhip on\npqr_input in.pqr\n"
        "energy_output %s\n" % (L, L, L, out))
    r = subprocess.run([host.EXE_PATH, str(tmp_path / "input")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = out.read_text().splitlines()
    t = lines[1].split()
    got, three, _ = _fresh(s, synth.FLAGS_AT)
    bare, _, _ = _fresh(s, _off(synth.FLAGS_AT))
    _check(three, ref.unordered(s), "pqr")
    assert t[0] == "0" and t[1] == "%.6f" % got["energy"] and t[1] != "%.6f" % bare["energy"]
    assert [l.split()[0] for l in lines[1:]] == ["0", "2", "4"]
