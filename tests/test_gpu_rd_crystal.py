"""GPU tests of rd_crystal, Lennard-Jones summed over lattice images: rdc_tile_kernel + rdc_self_kernel
(mpmc_amd/csrc/kernels_crystal.h) and lj_lrc_kernel at the crystal cutoff, through mpmc_hip_set_rd_crystal, against
tests/rdc_reference.py.

The tolerance of rd_energy is 1e-12 * sum |terms| (every image's repulsive and attractive term, every Feynman-Hibbs,
long-range and self term), that of the two dense terms before this one.  The derived rounding bound is a few ulp per
term plus a log-depth sum, about 5e-15 * sum |terms|.  In the snapshots of fixture 012 up to 8 880 pair images sit on the
cutoff to the last bit (tests/test_rdc_reference.py reproduces the counts); one of them decided the other way is worth
1e-7 K or more, five orders above the tolerance there.  The synthetic cases keep every image 1e-9 A away from the
cutoff, asserted below on the CPU.
"""
import os
import subprocess

import numpy as np
import pytest

import rdc_cases as rc
import rdc_reference as rr
from mpmc_amd import engine, host, synth

pytestmark = pytest.mark.gpu
FIELDS = [f for f, _ in engine.Result._fields_]


def _engine(s, flags, cap=None, **options):
    e = engine.Engine(cap or len(s["charge"]))
    for k, v in options.items():
        e.set_option(k, v)
    e.load_system(s, flags)
    return e


def _fresh(s, flags):
    e = _engine(s, flags)
    r = e.energy()
    d = e.dipoles() if flags.get("polarization") and not flags.get("rd_only") else None
    e.close()
    return r, d


def _check_rd(got, ref, what):
    want, tol = float(ref["total"]), rc.RD_TOL * float(ref["abs_sum"])
    err = abs(got["rd_energy"] - want)
    print("%s: rd_energy %.12f reference %.12f |diff| %.3g tol %.3g (%.3g of it)" % (what, got["rd_energy"], want, err, tol,
                                                                                     err / tol))
    assert err <= tol, (what, got["rd_energy"], want, err, tol)
    assert got["status"] == 0
    # result.cutoff is the value cutoff_c was formed from
    assert got["cutoff"] == ref["cutoff"] and rr.crystal_cutoff(got["cutoff"], ref["order"]) == ref["cutoff_c"]
    assert got["volume"] == ref["volume"]


def _ref(name, variant, order):
    return dict(rc.reference(name, variant, order), order=order)


SNAP_CASES = [(n, 2) for n in rc.SNAPS] + [(n, o) for o in (1, 3) for n in rc.SNAPS[:5]]


@pytest.mark.parametrize("name,order", SNAP_CASES)
def test_fixture_012_against_the_reference(name, order):
    """the fixture's own keywords that bear on this term: rd_lrc on, no Feynman-Hibbs"""
    ref = _ref(name, "lrc", order)
    if order == 2:
        assert ref["pair_ties"] == rc.TIES_012[int(name[4:])] and ref["self_ties"] == rc.SELF_TIES_012
    got, _ = _fresh(rc.system(name), rc.flags("lrc", order))
    _check_rd(got, ref, "%s order %d (%d images on the cutoff)" % (name, order, ref["ties"]))
    assert got["energy"] == got["rd_energy"] and got["n_atoms"] == len(rc.system(name)["charge"])


@pytest.mark.parametrize("variant", sorted(rc.VARIANTS))
@pytest.mark.parametrize("name", rc.SYNTH)
def test_synthetic_cases_against_the_reference(name, variant):
    order = rc.ORDER[name]
    rc.margins(name, order)
    got, _ = _fresh(rc.system(name), rc.flags(variant, order))
    _check_rd(got, _ref(name, variant, order), "%s/%s order %d" % (name, variant, order))


@pytest.mark.parametrize("name", ["t150", "snap3"])
def test_the_other_result_fields_do_not_see_the_mode(name):
    """polarization + Ewald: every other result field and the dipoles are those of the same context with the mode off"""
    s, order = rc.system(name), 2
    f = rc.flags("polar", order)
    e = _engine(s, f)
    on, on_dip = e.energy(), e.dipoles()
    _check_rd(on, _ref(name, "polar", order), name + "/polar")
    e.set_rd_crystal(0)
    off, off_dip = e.energy(), e.dipoles()
    e.close()
    for fld in FIELDS:
        if fld not in ("energy", "rd_energy"):
            assert on[fld] == off[fld], (fld, on[fld], off[fld])
    assert on["rd_energy"] != off["rd_energy"]
    for k in on_dip:
        assert np.array_equal(on_dip[k], off_dip[k]), k
    lj, _ = _fresh(s, rc.plain_flags(f))  # ... which is what a context that never saw the mode gives
    assert off == lj


def _moves(s):
    """three single-molecule moves on t150: two small ones, and one that carries a molecule across the cell face without
    wrapping it (fractional x from inside the cell to 1.02)"""
    rng = np.random.default_rng(5)
    mol = np.asarray(s["molecule"])
    frac = s["pos"] @ np.linalg.inv(s["basis"])
    out = []
    for m in (12, 40):
        idx = np.flatnonzero(mol == m)
        out.append((int(idx[0]), len(idx), rng.uniform(-0.25, 0.25, 3)))
    inside = np.flatnonzero((mol > 1) & (frac[:, 0] < 1.0) & (frac[:, 0] > 0.0))
    a = inside[np.argmax(frac[inside, 0])]
    idx = np.flatnonzero(mol == mol[a])
    out.append((int(idx[0]), len(idx), (1.02 - frac[idx, 0].min()) * s["basis"][0]))
    return out


@pytest.mark.parametrize("variant", ["fh4", "polar"])
def test_incremental_pass_leaves_the_bits_of_a_fresh_context(variant):
    s, f = rc.system("t150"), rc.flags(variant, 2)
    live = _engine(s, f)
    live.energy()
    cur = dict(s, pos=s["pos"].copy())
    for step, (first, count, shift) in enumerate(_moves(s)):
        new = cur["pos"][first:first + count] + shift
        cur["pos"][first:first + count] = new
        live.update_atoms(first, new)
        a = live.energy()
        b, _ = _fresh(cur, f)
        for fld in FIELDS:
            assert a[fld] == b[fld], (step, fld, a[fld], b[fld])
    frac = cur["pos"][first:first + count] @ np.linalg.inv(s["basis"])
    assert frac[:, 0].max() > 1.0  # the last move left the cell, and nothing wrapped it
    _check_rd(a, dict(rr.rd_terms(cur, f, 2), order=2), "after three moves")
    # the same evaluation again, and in two halves: the same bits
    assert live.energy() == a
    live.energy_begin()
    assert live.energy_end() == a
    live.close()


def test_scale_box_gives_the_result_of_a_fresh_context():
    s, f = rc.system("t150"), rc.flags("fh2", 2)
    mol = np.asarray(s["molecule"])
    ids = np.cumsum(np.concatenate([[0], mol[1:] != mol[:-1]]))
    com = np.stack([s["pos"][ids == m].mean(axis=0) for m in range(ids[-1] + 1)])
    live = _engine(s, f)
    live.energy()
    cur = dict(s, pos=s["pos"].copy(), basis=s["basis"].copy())
    for scale in (1.03, None, 0.97):  # +3 %, revert, -3 %
        if scale is not None:
            g = scale ** (1.0 / 3.0)
            delta, basis = com * (g - 1.0), s["basis"] * g
        else:
            delta, basis = -delta, s["basis"].copy()
        cur["pos"] = cur["pos"] + delta[ids]  # the very addition the engine does
        cur["basis"] = basis
        assert live.scale_box(basis, delta) is True
        a = live.energy()
        b, _ = _fresh(cur, f)
        for fld in FIELDS:
            assert a[fld] == b[fld], (scale, fld, a[fld], b[fld])
        _check_rd(a, dict(rr.rd_terms(cur, f, 2), order=2), "scale %s" % scale)
    live.close()


def test_mode_switching():
    s = rc.system("t150")
    f = rc.flags("polar", 2)
    e = _engine(s, rc.plain_flags(f), cap=192)
    lj, lj_dip = e.energy(), e.dipoles()
    e.set_rd_crystal(2)
    on2 = e.energy()
    _check_rd(on2, _ref("t150", "polar", 2), "order 2")
    # insert / remove answer "upload again" in this mode, and change nothing
    idx = np.flatnonzero(np.asarray(s["molecule"]) == s["molecule"][-1])
    assert e.remove_molecule(int(idx[0]), len(idx)) is False
    z = np.zeros(1)
    assert e.insert_molecule(np.zeros((1, 3)), z, z, z + 30.0, z + 3.0, z + 14.0) is None
    assert e.energy() == on2
    e.set_rd_crystal(3)
    _check_rd(e.energy(), _ref("t150", "polar", 3), "order 3")
    # the setting belongs to the context: an upload keeps it
    e.set_rd_crystal(2)
    e.upload(s)
    assert e.energy() == on2
    for bad in (5, -1):
        with pytest.raises(engine.EngineError, match="outside 1 .. 4"):
            e.set_rd_crystal(bad)
    assert e.energy() == on2  # a refused order changed nothing
    e.energy_begin()
    with pytest.raises(engine.EngineError, match="between energy_begin"):
        e.set_rd_crystal(0)
    assert e.energy_end() == on2
    e.set_rd_crystal(0)
    off = e.energy()
    assert off == lj
    for k, v in e.dipoles().items():
        assert np.array_equal(v, lj_dip[k]), k
    assert e.remove_molecule(int(idx[0]), len(idx)) is True  # ... and device-side edits are back
    e.close()


def test_disp_expansion_with_rd_crystal_is_refused_by_name():
    s = synth.s_phahst(130)
    e = _engine(s, dict(synth.FLAGS_PHAHST, rd_crystal=1, rd_crystal_order=2))
    with pytest.raises(engine.EngineError, match="rd_crystal with disp_expansion"):
        e.energy()
    e.set_rd_crystal(0)
    assert e.energy()["status"] == 0
    e.close()


def test_two_contexts_side_by_side():
    a = _engine(rc.system("t150"), rc.flags("polar", 2))
    b = _engine(rc.system("snap3"), rc.flags("lrc", 3))
    a.energy_begin()
    b.energy_begin()
    rb, ra = b.energy_end(), a.energy_end()
    _check_rd(ra, _ref("t150", "polar", 2), "context a")
    _check_rd(rb, _ref("snap3", "lrc", 3), "context b")
    a.close()
    b.close()


POLAR_EWALD_IN = (  # the keywords of the reference's 012-3D-crystal-replay/polar_ewald.in
    "ensemble replay\nrd_crystal on\nrd_crystal_order 2\nrd_lrc on\nread_pqr_box on\npolarization on\npolar_damp 2.1304\n"
    "polar_damp_type exponential\npolar_ewald on\npolar_ewald_alpha 0.15\npolar_max_iter 5\npolar_iterative on\n"
    "polar_palmo on\npolar_gamma 1.03\nwrapall on\ntraj_input replay.pqr\nenergy_output %s\npqr_input /dev/null\n"
    "pqr_output /dev/null\npqr_restart /dev/null\ntraj_output /dev/null\ndipole_output /dev/null\nfield_output /dev/null\n")


def test_driver_replays_the_fixture(tmp_path):
    """mpmc_hip on the seven snapshots as a trajectory: one observables line per frame, whose rd column is the engine's
    rd_energy of that frame -- at the FIRST frame's cutoff, which a replay keeps (replay.c) -- and the reference
    program's own printed value."""
    import json

    text, systems = rc.trajectory_text()
    (tmp_path / "replay.pqr").write_text(text)
    out = tmp_path / "energy.polar_ewald"
    (tmp_path / "input").write_text(POLAR_EWALD_IN % out)
    r = subprocess.run([host.EXE_PATH, str(tmp_path / "input")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = out.read_text().splitlines()
    assert lines[0].startswith("#step #energy #coulombic #rd #polar")
    assert [l.split()[0] for l in lines[1:]] == [str(k + 1) for k in range(rc.NSNAP)]
    gold = json.load(open(os.path.join(rc.GOLD, "rd_crystal_012.json")))
    f = dict(rc.flags("polar", 2), temperature=0.0, pbc_cutoff=gold["pbc_cutoff"])
    for k, s in enumerate(systems):
        t = lines[1 + k].split()
        got, _ = _fresh(s, f)
        assert got["cutoff"] == 0.5
        _check_rd(got, dict(rr.rd_terms(s, f, 2), order=2), "frame %d" % k)
        assert t[3] == "%.6f" % got["rd_energy"] and t[1] == "%.6f" % got["energy"], (k, t, got)
        assert float(t[8]) == len(s["charge"]) / 2 and float(t[10]) == got["volume"]
        assert abs(float(t[3]) - float(gold["rd_energy"]["polar_ewald.in"][k])) <= 1.0000001e-6, (k, t[3])


def test_host_layer_chain_carries_the_engine_energy():
    """a short NVT chain through the C host layer in this mode: the energy it carries is a fresh context's energy of its
    final configuration"""
    s, f = rc.system("t150"), rc.flags("polar", 2)
    h = host.HostSystem(s, f, seed=5, move_factor=0.05, rot_factor=0.05)
    h.mc_steps(8)
    o = h.observables()
    assert o["accept"] + o["reject"] == 8
    got, _ = _fresh(dict(s, pos=h.positions()), f)
    assert o["energy"] == got["energy"] and o["rd_energy"] == got["rd_energy"]
    h.close()
