"""GPU tests of cavity_bias in the C host layer (mpmc_amd/host/: the keywords, energy_hip_cavity_update(), the biased
insertion, the removal coin, the biased acceptance and the running means) against the numpy restatement
tests/cavity_reference.py, one Monte Carlo step at a time.  Counts, flags and doubles formed by stated operations are
compared with ==; the Boltzmann factor is restated with math.exp, the C library's exp the host layer calls."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import cavity_reference as cr
import reference_chain_compare as rcc
from mpmc_amd import host, synth
from oracle import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "cavity_bias", "uvt_chain_cavity_off.json")

ATM2REDUCED = 0.0073389366
G, RADIUS, CORRTIME, PRESSURE, T = 6, 2.5, 4, 300.0, 77.0
P = dict(temperature=T, polarization=1, polar_damp=2.1304, polar_max_iter=4)
UVT = {"ensemble": "uvt", "insert_probability": 0.6, "pressure": PRESSURE}
CAVITY = dict(UVT, cavity_bias="on", cavity_grid=G, cavity_radius=RADIUS, corrtime=CORRTIME)
SEED = 8  # both an insertion and a removal are accepted within 40 steps (N leaves 32 in both directions)


def start():
    s = synth.s_pol(160, spacing=4.5)
    pts = cr.grid_points(s["basis"], G)
    n_open = len(cr.open_list(cr.occupancy(pts, cr.wrapped_positions(s), RADIUS)))
    assert 0 < n_open < G ** 3  # the starting configuration has open and occupied points
    return s, pts


def chain(s, extra, seed=SEED):
    return host.HostSystem(s, P, seed=seed, move_factor=0.05, rot_factor=0.05, extra=extra)


def test_every_step_follows_the_definition():
    s, pts = start()
    basis = np.asarray(s["basis"], dtype=np.float64)
    volume = cr.reciprocal_basis(basis)[1]
    h = chain(s, CAVITY)
    assert h.cavity_flags() == dict(cavity_bias=1, cavity_grid=G, cavity_radius=RADIUS)
    h.mc_steps(0)  # the initial energy and the first checkpoint
    avg_ns, avg_obs, seen_n, kinds, biased_accepts = 0.0, 0.0, set(), set(), 0
    for step in range(1, 41):
        before = h.system(basis)            # the accepted configuration the step starts from
        move = h.next_movetype()
        energy_before = h.observables()["energy"]
        accepted = h.mc_steps(1)
        c, darts, o = h.cavity(), h.cavity_darts(), h.observables()
        # the grid of the configuration before the move, with the recorded darts
        occ = cr.occupancy(pts, cr.wrapped_positions(before), RADIUS)
        opened = cr.open_list(occ)
        assert c["n_darts"] == int(volume * 0.1) == len(darts)
        assert c["cavities_open"] == len(opened)
        assert c["hits"] == cr.dart_hits(pts, opened, darts, RADIUS)
        assert c["cavity_volume"] == cr.cavity_volume(c["hits"], c["n_darts"], volume)
        prob = float(len(opened)) / float(G ** 3)
        assert c["cavity_bias_probability"] == prob
        # biased_move: an insertion whenever a point is open; a removal by its coin, which the corrtime mean decides for
        # certain when it is 0 (pow = 1 > every draw) or leaves pow below the smallest non-zero draw, 2^-64
        if move == "insert":
            assert c["biased_move"] == (1 if len(opened) else 0)
        elif move == "remove":
            coin = math.pow(1.0 - avg_obs, float(G) * G * G)
            assert coin == 1.0 or coin < 2.0 ** -64
            assert c["biased_move"] == (0 if coin == 1.0 else 1)
        else:
            assert c["biased_move"] == 0
        # the acceptance: the running mean of the node statistics is the one of the steps before this one
        delta = c["trial_energy"] - energy_before
        n_trial = len(before["charge"]) // 5 + (1 if move == "insert" else -1 if move == "remove" else 0)
        if not math.isfinite(c["trial_energy"]):
            want = 0.0
        elif move == "insert" and c["biased_move"]:
            want = (c["cavity_volume"] * avg_ns * PRESSURE * ATM2REDUCED / (T * float(n_trial))) * math.exp(-delta / T)
        elif move == "remove" and c["biased_move"]:
            want = ((T * (float(n_trial) + 1.0)) / (c["cavity_volume"] * avg_ns * PRESSURE * ATM2REDUCED)
                    * math.exp(-delta / T))
        elif move == "insert":
            want = volume * PRESSURE * ATM2REDUCED / (T * float(n_trial)) * math.exp(-delta / T)
        elif move == "remove":
            want = T * (float(n_trial) + 1.0) / (volume * PRESSURE * ATM2REDUCED) * math.exp(-delta / T)
        else:
            want = math.exp(-delta / T)
        assert c["boltzmann_factor"] == want, (step, move, c)
        if step == 1 and move == "insert":
            assert want == 0.0  # the running mean is still 0: the reference's first biased insertion cannot be accepted
        if accepted:
            assert o["energy"] == c["trial_energy"] and o["N"] == n_trial
            biased_accepts += c["biased_move"]
        else:
            assert o["energy"] == energy_before and h.natoms() == len(before["charge"])
        # the running means: per step (average.c:55-80), and over the one walker at every corrtime (average.c:351-400)
        factor = float(step - 1) / float(step)
        avg_ns = factor * avg_ns + prob / float(step)
        assert c["avg_nodestats"] == avg_ns
        if step % CORRTIME == 0:
            avg_obs = 0.0 * 0.0 + avg_ns / 1.0
        assert c["avg_observables"] == avg_obs
        seen_n.add(h.natoms())
        kinds.add((move, c["biased_move"]))
    assert len(seen_n) > 1, "N never changed"
    assert min(seen_n) < 160 < max(seen_n)
    assert {("insert", 1), ("remove", 1), ("displace", 0)} <= kinds and biased_accepts > 0
    # the energy the chain carries is the oracle's energy of where it ended
    final = h.system(basis)
    want = oracle.energy(final, P)
    assert abs(h.observables()["energy"] - want["energy"]) < 1e-9 * max(1.0, abs(want["energy"]))
    h.close()


def test_incremental_edits_and_full_bins_walk_the_same_chain():
    s, _ = start()
    traces = []
    for incremental in (1, 0):
        h = chain(s, CAVITY)
        h.energy()  # creates the context
        h.set_option("cavity_incremental", incremental)
        trace = []
        for _ in range(40):
            acc = h.mc_steps(1)
            c = h.cavity()
            trace.append((acc, h.natoms(), h.observables()["energy"], c["cavities_open"], c["hits"], c["biased_move"],
                          c["boltzmann_factor"]))
        traces.append(trace)
        h.close()
    assert traces[0] == traces[1]
    assert len({t[1] for t in traces[0]}) > 1 and len({t[3] for t in traces[0]}) > 1


def test_cavity_bias_off_walks_the_chain_it_always_walked():
    """the chain of tests/test_gpu_host.py::test_uvt_chain_inserts_removes_and_tracks_the_oracle, block by block, against
    the bits recorded from the commit before cavity_bias existed -- with the keyword absent and with `cavity_bias off`"""
    golden = json.load(open(GOLDEN))
    s = synth.s_pol(160, spacing=4.5)
    for extra in (UVT, dict(UVT, cavity_bias="off", cavity_grid=G, cavity_radius=RADIUS)):
        h = chain(s, extra, seed=21)
        for row in golden:
            acc = h.mc_steps(10)
            o = h.observables()
            assert (acc, h.natoms(), o["N"]) == (row["accepted"], row["natoms"], row["N"])
            for k in ("energy", "coulombic_energy", "rd_energy", "polarization_energy"):
                assert float(o[k]).hex() == row[k], k
        c = h.cavity()
        assert c["n_darts"] == 0 and c["cavities_open"] == 0 and c["biased_move"] == 0 and c["avg_nodestats"] == 0.0
        h.close()


def test_driver_walks_the_reference_programs_chain(tmp_path):
    """tests/golden/cavity_bias/reference_chain: a seeded 200-step `ensemble uvt` + `cavity_bias on` run (13 frozen framework
    atoms, 12 two-site sorbates, user_fugacities) and the energy-output lines the reference program wrote for it.  The
    driver on the same input must give the same N in every line -- every insertion, removal and coin fell as in the
    reference, draw for draw -- and the energy columns to the printed digits, by the rules of
    tests/reference_chain_compare.py (the device adds its pair sums in another order)."""
    src = os.path.join(ROOT, "tests", "golden", "cavity_bias", "reference_chain")
    for name in ("input", "in.pqr"):
        shutil.copy(os.path.join(src, name), tmp_path / name)
    r = subprocess.run([host.EXE_PATH, "input"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want = rcc.energy_lines(os.path.join(src, "reference_energy.dat"))
    assert len(want) == 42
    worst = rcc.compare_energy(rcc.energy_lines(tmp_path / "energy.dat"), want)
    print("largest deviation from the reference's printed energies: %s K" % worst)
    assert len({w.split()[8] for w in want[1:]}) > 5  # N moved both ways in the reference's run
