"""GPU tests of the NPT ensemble: a volume move on a LIVE device context (mpmc_hip_scale_box) must leave exactly what a
fresh context given the same box and coordinates computes; the NPT chain of the C host layer; error paths; the
driver.  Tolerances as in test_gpu_parity.py / test_gpu_host.py: 1e-10 per energy term, 1e-10 of the largest
component for per-atom vectors, 1e-9 relative on host-layer energies, == where two device paths must agree."""
import os
import subprocess

import numpy as np
import pytest

from mpmc_amd import engine, host, synth
from oracle import oracle
from test_gpu_parity import check_energies
from test_npt import centres_of_mass, scaled, volume_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

RESULT_FIELDS = [f for f, _ in engine.Result._fields_]


def _triclinic():
    s = synth.s_es(432)
    L = s["basis"][0, 0]
    s["basis"] = np.array([[L, 0, 0], [0.2 * L, 0.95 * L, 0], [0.1 * L, -0.15 * L, 0.9 * L]])
    return s


CASES = {
    "lj": lambda: (synth.s_lj(1000), dict(synth.FLAGS_LJ)),
    "lj_ewald": lambda: (synth.s_es(1024), dict(synth.FLAGS_ES)),  # default cutoff: alpha, k-vectors, self term move
    "jacobi_1024": lambda: (synth.s_pol(1024), dict(synth.FLAGS_POL_JACOBI)),  # resident one-launch solve
    "jacobi_4096": lambda: (synth.s_pol(4096), dict(synth.FLAGS_POL_JACOBI)),  # a launch per sweep
    "production_1024": lambda: (synth.s_pol(1024), dict(synth.FLAGS_POL_PRODUCTION)),
    "polar_ewald": lambda: (synth.s_pol(640), dict(synth.FLAGS_POL_JACOBI, polar_max_iter=4, polar_ewald=1)),
    "triclinic": lambda: (_triclinic(), dict(temperature=100.0, feynman_hibbs=1, feynman_hibbs_order=4)),
}


def _engine(s, p, incremental=1):
    e = engine.Engine(len(s["charge"]))
    e.load_system(s, p)
    if p.get("polar_gs_ranked"):
        # include/mpmc_hip.h ("gs_lags"): the lag count otherwise depends on the call history of a context, and the
        # rounding of the sweep with it (1e-13): a known open item, pinned on every engine compared here
        e.set_option("gs_lags", 2)
    if not incremental:
        e.set_option("incremental_amatrix", 0)
        e.set_option("incremental_pairs", 0)
    return e


def _full(e, polar, ranked=False):
    r = e.energy()
    if polar:
        r.update(e.dipoles())
    if ranked:  # (the ranking metric is only computed, and its download only defined, under polar_gs_ranked)
        r["rank"], r["order"] = e.ranking()
    return r


def _same(a, b, polar, what):
    for k in RESULT_FIELDS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    if polar:
        for k in ("mu", "ef_static", "ef_induced", "ef_induced_change"):
            assert np.array_equal(a[k], b[k]), (what, k, float(np.abs(a[k] - b[k]).max()))
    if "rank" in a or "rank" in b:
        for k in ("rank", "order"):
            assert np.array_equal(a[k], b[k]), (what, k)


def _oracle(got, s, p, polar, what):
    want = oracle.energy(s, p, want_vectors=polar)
    check_energies(got, want)
    assert abs(got["volume"] / volume_of(np.asarray(s["basis"]).tolist()) - 1.0) < 1e-14
    if polar:
        for k in ("mu", "ef_static"):
            assert np.abs(got[k] - want[k]).max() <= 1e-10 * np.abs(want[k]).max(), (what, k)


def _moved(s, pos, rng, k):
    """molecule k displaced: (first atom, new coordinates of its atoms)"""
    idx = np.flatnonzero(np.asarray(s["molecule"]) == np.asarray(s["molecule"])[k])
    first, cnt = int(idx[0]), len(idx)
    assert np.array_equal(idx, np.arange(first, first + cnt))
    return first, pos[first:first + cnt] + rng.normal(scale=0.15, size=3)


@pytest.mark.parametrize("case", sorted(CASES))
def test_live_volume_move_equals_a_fresh_context(case):
    opened = []  # every context is closed whatever happens: the resident solver of later tests needs the device alone
    try:
        _live_volume_move(case, opened)
    finally:
        for e in opened:
            e.close()


def _live_volume_move(case, opened):
    s, p = CASES[case]()
    polar = bool(p.get("polarization"))
    ranked = bool(p.get("polar_gs_ranked"))
    n = len(s["charge"])
    rng = np.random.default_rng(17)
    pos = np.array(s["pos"], dtype=np.float64)
    basis = np.asarray(s["basis"], dtype=np.float64).tolist()
    v0 = volume_of(basis)
    live = _engine(s, p)
    opened.append(live)
    live.energy()
    # a few single-molecule moves; the last one is still queued when the box is scaled
    for j, k in enumerate((7, n // 2, n - 3)):
        first, new = _moved(s, pos, rng, k)
        live.update_atoms(first, new)
        pos[first:first + len(new)] = new
        if j < 2:
            live.energy()
    for step, factor in enumerate((1.03, None, 0.97, None)):
        # the host's arithmetic: volume_change() (mc_moves.c:168-210) for a factor, revert_volume_change() (:213-248)
        # back to the first volume for None -- centres of mass as update_com() leaves them after the last energy()
        com = centres_of_mass(s, pos)
        basis, vol, delta, pos, _ = scaled(s, pos, com, basis, factor * v0 if factor else v0)
        assert live.scale_box(basis, delta) is True
        got = _full(live, polar, ranked)
        cur = dict(s, pos=pos, basis=np.array(basis))
        fresh = _engine(cur, p)
        opened.append(fresh)
        _same(got, _full(fresh, polar, ranked), polar, "%s step %d: live vs fresh" % (case, step))
        assert got["volume"] == vol
        _oracle(got, cur, p, polar, "%s step %d" % (case, step))
        fresh.close()
    # ... and the chain goes on: single-molecule moves through the incremental paths of the live context against an
    # engine that recomputes everything in every call
    full = _engine(cur, p, incremental=0)
    opened.append(full)
    full.energy()
    for j, k in enumerate((11, n // 3, n - 9, 11)):
        first, new = _moved(s, pos, rng, k)
        for e in (live, full):
            e.update_atoms(first, new)
        a, b = _full(live, polar, ranked), _full(full, polar, ranked)
        if j == 1:  # a rejected move: back, and evaluated again
            for e in (live, full):
                e.update_atoms(first, pos[first:first + len(new)])
            a, b = _full(live, polar, ranked), _full(full, polar, ranked)
        else:
            pos[first:first + len(new)] = new
        _same(a, b, polar, "%s move %d after the volume moves" % (case, j))
    _oracle(a, dict(s, pos=pos, basis=np.array(basis)), p, polar, case + " after the moves")


def test_scale_box_error_paths():
    """argument errors only: nothing here reaches a kernel with bad data"""
    s, p = synth.s_pol(320), dict(synth.FLAGS_POL_JACOBI)
    nmol = len(set(s["molecule"].tolist()))
    delta = np.zeros((nmol, 3))
    e = engine.Engine(400)
    e.set_params(**p)
    e.set_box(s["basis"])
    with pytest.raises(engine.EngineError, match="no configuration uploaded"):
        e.scale_box(s["basis"], delta)
    e.upload(s)
    with pytest.raises(engine.EngineError, match="displacements for the"):
        e.scale_box(s["basis"], delta[:-1])
    with pytest.raises(engine.EngineError, match="invalid simulation box"):
        e.scale_box(np.zeros((3, 3)), delta)
    e.energy_begin()
    with pytest.raises(engine.EngineError, match="between energy_begin"):
        e.scale_box(s["basis"], delta)
    r0 = e.energy_end()
    # a refused call changed nothing; an accepted one with zero displacements and the same box neither
    assert e.scale_box(s["basis"], delta) is True
    r1 = e.energy()
    for k in RESULT_FIELDS:
        assert r0[k] == r1[k], k
    # after a grand-canonical removal the molecule ids are no longer those of the upload: "upload again"
    assert e.remove_molecule(5, 5) is True
    assert e.scale_box(s["basis"], delta) is False
    assert e.scale_box(s["basis"], delta[:-1]) is False
    e.upload(s)
    assert e.scale_box(s["basis"], delta) is True
    e.close()


def test_coordinate_bound_is_refreshed_when_it_would_leave_the_fp32_screen():
    """the engine's bound on |coordinate| grows by max |delta| per call; a shift out and back (no net motion) would carry
    it past the fp32 screen's limit of 2048 A: there it is replaced by the true maximum.  Results == a fresh context."""
    s, p = synth.s_es(432), dict(synth.FLAGS_ES)
    nmol = len(set(s["molecule"].tolist()))
    opened = []
    try:
        live = _engine(s, p)
        opened.append(live)
        live.energy()
        pos = np.array(s["pos"])
        for sign in (1.0, -1.0):
            delta = np.tile(np.array([sign * 1200.0, 0.0, sign * -1100.0]), (nmol, 1))
            pos = pos + np.repeat(delta, 2, axis=0)  # two-site molecules
            assert live.scale_box(s["basis"], delta) is True
            got = live.energy()
            fresh = _engine(dict(s, pos=pos), p)
            opened.append(fresh)
            _same(got, fresh.energy(), False, "shift %+g" % sign)
            fresh.close()
        assert np.abs(pos - s["pos"]).max() < 1e-12
        check_energies(got, oracle.energy(dict(s, pos=pos), p))
    finally:
        for e in opened:
            e.close()


# ---- the chain ------------------------------------------------------------------------------------------------------
CHAIN = dict(n=320, seed=41, steps=80, extra={"ensemble": "npt", "pressure": "200.0", "volume_probability": "0.3",
                                              "volume_change_factor": "0.02"})


def _npt_chain(notes=True, steps=None):
    s = synth.s_pol(CHAIN["n"])
    p = dict(synth.FLAGS_POL_JACOBI)
    h = host.HostSystem(s, p, seed=CHAIN["seed"], move_factor=0.05, rot_factor=0.05, extra=CHAIN["extra"])
    h.set_volume_notes(notes)
    trace = []
    for _ in range(steps or CHAIN["steps"]):
        h.mc_steps(1)
        o = h.observables()
        trace.append((o["energy"], o["volume"], o["accept"], o["accept_volume"], o["reject_volume"]))
    return s, p, h, trace


def test_npt_chain_tracks_the_oracle_and_is_reproducible():
    """ensemble npt, 320-atom polarizable box, 80 steps, volume_probability 0.3.

    Seed 41, pressure 200 atm, volume_change_factor 0.02 were chosen on the MI355X so that both branches occur; counts
    seen there: 54 moves accepted and 26 rejected, of which volume moves 10 accepted and 8 rejected;
    volume 2985.984 -> 2906.373 A^3."""
    s, p, h, trace = _npt_chain()
    o = h.observables()
    print("npt chain: accept %d reject %d, volume moves accepted %d rejected %d, V %.3f -> %.3f" %
          (o["accept"], o["reject"], o["accept_volume"], o["reject_volume"], volume_of(s["basis"].tolist()), o["volume"]))
    assert o["accept"] + o["reject"] == CHAIN["steps"]
    assert o["accept_volume"] >= 1 and o["reject_volume"] >= 1
    assert o["volume"] != volume_of(s["basis"].tolist()) and len({t[1] for t in trace}) > 1
    cur = dict(s, pos=h.positions(), basis=h.basis())
    want = oracle.energy(cur, dict(p, pbc_cutoff=o["cutoff"]))
    assert abs(o["energy"] - want["energy"]) < 1e-9 * abs(want["energy"])
    assert abs(o["volume"] - want["volume"]) <= 1e-14 * want["volume"]
    h.close()
    # (a) the same seed gives the same chain, bit for bit
    _, _, h2, trace2 = _npt_chain()
    assert trace2 == trace
    assert np.array_equal(h2.positions(), cur["pos"]) and np.array_equal(h2.basis(), cur["basis"])
    h2.close()
    # (b) ... also when every volume step uploads the whole configuration again (no volume notes)
    _, _, h3, trace3 = _npt_chain(notes=False)
    assert trace3 == trace
    assert np.array_equal(h3.positions(), cur["pos"])
    h3.close()


@pytest.mark.parametrize("revert", [False, True])
def test_forced_volume_move_against_oracle_and_a_fresh_context(revert):
    """both branches without Metropolis: one forced change (+ its revert) on a live context, then energy()"""
    s = synth.s_pol(320)
    p = dict(synth.FLAGS_POL_JACOBI)
    h = host.HostSystem(s, p, seed=3, extra={"ensemble": "npt", "pressure": "1.0"})
    h.energy()
    v0 = h.observables()["volume"]
    h.force_volume_move(0.97 * v0, revert=revert)
    e = h.energy()
    o = h.observables()
    assert o["volume"] != v0 if not revert else abs(o["volume"] / v0 - 1.0) < 32 * 2.0 ** -52
    cur = dict(s, pos=h.positions(), basis=h.basis())
    if not revert:
        assert np.abs(cur["pos"] - s["pos"]).max() > 1e-3
    want = oracle.energy(cur, dict(p, pbc_cutoff=o["cutoff"]), want_vectors=True)
    assert abs(e - want["energy"]) < 1e-9 * abs(want["energy"])
    assert abs(o["polarization_energy"] - want["polarization_energy"]) < 1e-9 * abs(want["polarization_energy"])
    d = h.dipoles()
    assert np.abs(d["mu"] - want["mu"]).max() < 1e-10 * np.abs(want["mu"]).max()
    fresh = host.HostSystem(cur, p, seed=3, extra={"pbc_cutoff": repr(float(o["cutoff"]))})
    assert fresh.energy() == e
    assert np.array_equal(fresh.dipoles()["mu"], d["mu"])
    fresh.close()
    # the binding's host image followed the lists: a displacement afterwards takes the noted-molecule path
    h.mc_steps(3)
    o = h.observables()
    want = oracle.energy(dict(s, pos=h.positions(), basis=h.basis()), dict(p, pbc_cutoff=o["cutoff"]))
    assert abs(o["energy"] - want["energy"]) < 1e-9 * abs(want["energy"])
    h.close()


def test_driver_runs_an_npt_input(tmp_path):
    from test_reference_inputs import keyword_file

    d = keyword_file(tmp_path, "bssp_small")
    text = open(os.path.join(d, "input")).read().replace("ensemble        nvt", "ensemble        npt")
    assert "ensemble        npt" in text
    text += "pressure 1.0\nvolume_probability 0.5\nvolume_change_factor 0.25\n"
    open(os.path.join(d, "input"), "w").write(text.replace("corrtime        10", "corrtime        2"))
    r = subprocess.run([host.EXE_PATH, os.path.join(d, "input")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = open(os.path.join(d, "energy.dat")).read().splitlines()
    assert lines[0].split()[10] == "#volume"
    volumes = [l.split()[10] for l in lines[1:]]
    assert len(volumes) == 21 and volumes[0] == "%f" % 22.4567 ** 3
    assert len(set(volumes)) > 1, volumes
