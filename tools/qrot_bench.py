#!/usr/bin/env python3
"""What one molecule's quantum_rotation scan costs on device 0: the 256 grid energies of a molecule through
mpmc_hip_trial_energies() -- batched, and on the serial path (option trial_batched 0) -- against the only way there was
before the entry existed, 2 x 256 update_atoms() + energy() calls through the public ABI (the reference evaluates
energy_no_observables() and energy() per grid point); then a full evaluation of the sample through the host layer, split
into scan, Hamiltonian and eigen-solve + symmetry.

Two sizes: the reference's sample 007 (one BSS H2 in MOF-5, 429 atoms, tests/golden/qrot/MOF5+alpha.pdb) and a synthetic
box of 4096 atoms with five-site molecules (synth.s_pol, electrostatics without polarization).  Every figure is the
median of `--repeat` timed calls after one untimed call, timed from the host, end to end.

    python tools/qrot_bench.py [--repeat 5] [--json]

Copied into a checkout from before the entry existed (with tests/golden/qrot/MOF5+alpha.pdb beside it), it times the public
sequence alone on that build: the figure the batched call is compared with.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from mpmc_amd import engine, host, pqr, synth  # noqa: E402


def grid_placements(pos, seed=0):
    """256 rigid rotations of the molecule about its first site (the timing does not depend on which)."""
    rng = np.random.default_rng(seed)
    out = np.empty((256,) + pos.shape)
    for t in range(256):
        q = rng.normal(size=4)
        w, x, y, z = q / np.linalg.norm(q)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        out[t] = pos[0] + (pos - pos[0]) @ R.T
    return out


def timed(fn, repeat):
    fn()
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def scan_times(name, system, flags, first, k, repeat):
    xyz = grid_placements(system["pos"][first:first + k])
    eng = engine.Engine(len(system["charge"]), device=0)
    out = dict(case=name, atoms=len(system["charge"]), sites=k)
    try:
        eng.load_system(system, flags)
        eng.energy()
        if hasattr(eng, "trial_energies"):  # (a build from before the entry: the public sequence is all it has)
            out["batched_s"] = timed(lambda: eng.trial_energies(first, xyz), repeat)
            eng.set_option("trial_batched", 0)
            out["serial_s"] = timed(lambda: eng.trial_energies(first, xyz), max(1, repeat // 2))
            eng.set_option("trial_batched", 1)
        cur = system["pos"][first:first + k]

        def public_twice():  # energy_no_observables() + energy() per grid point, then the restore
            for p in xyz:
                eng.update_atoms(first, p)
                eng.energy()
                eng.energy()
            eng.update_atoms(first, cur)
            eng.energy()

        out["public_2x256_s"] = timed(public_twice, max(1, repeat // 2))
    finally:
        eng.close()
    return out


def host_split(repeat):
    system = pqr.read_pqr(os.path.join(ROOT, "tests", "golden", "qrot", "MOF5+alpha.pdb"), np.diag([25.669] * 3))
    flags = dict(temperature=50.0, rd_lrc=0, quantum_rotation=1, quantum_rotation_B=85.35060622, quantum_rotation_l_max=7,
                 quantum_rotation_level_max=64, quantum_rotation_sum=10)
    hs = host.HostSystem(system, flags, seed=1)
    try:
        hs.energy()
        rows = []
        devnull = os.open(os.devnull, os.O_WRONLY)
        saved = os.dup(1)
        for _ in range(repeat + 1):
            sys.stdout.flush()
            os.dup2(devnull, 1)  # (the 64 DEBUG_QROT lines)
            try:
                hs.qrot_evaluate()
            finally:
                os.dup2(saved, 1)
            t = np.zeros(3)
            hs.lib.host_qrot_times(t.ctypes.data)
            rows.append(t)
        rows = np.array(rows[1:])
        med = np.median(rows, axis=0)
        return dict(case="host evaluation, sample 007 alpha, l_max 7", scan_s=med[0], hamiltonian_s=med[1],
                    eigensolve_symmetry_s=med[2])
    finally:
        hs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    rows = []
    mof = pqr.read_pqr(os.path.join(ROOT, "tests", "golden", "qrot", "MOF5+alpha.pdb"), np.diag([25.669] * 3))
    movable = np.flatnonzero(np.asarray(mof["frozen"]) == 0)
    rows.append(scan_times("sample 007 alpha (MOF-5 + H2)", mof, dict(temperature=50.0, rd_lrc=0), int(movable[0]), len(movable),
                           a.repeat))
    box = synth.s_pol(4096)
    rows.append(scan_times("S-POL(4096), no polarization", box, dict(temperature=77.0), 2000, 5, a.repeat))
    if hasattr(engine.Engine, "trial_energies"):
        rows.append(host_split(a.repeat))
    for r in rows:
        if a.json:
            print(json.dumps({k: (list(v) if isinstance(v, tuple) else v) for k, v in r.items()}))
            continue
        print(r["case"])
        for k, v in r.items():
            if k.endswith("_s"):
                if isinstance(v, tuple):
                    print("  %-22s median %10.3f ms   (min %.3f, max %.3f)" % (k[:-2], 1e3 * v[0], 1e3 * v[1], 1e3 * v[2]))
                else:
                    print("  %-22s %10.3f ms" % (k[:-2], 1e3 * v))


if __name__ == "__main__":
    main()
