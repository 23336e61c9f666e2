#!/usr/bin/env python3
"""Placements per second of the dimer scans (mpmc_hip_dimer_energies / mpmc_hip_dimer_grid_means) on device 0: the
five-site N2 dimer, polarizable (polar_gs_ranked + polar_palmo, 5 sweeps) and not, through the list form and through the
grid form at surf_ang 60, 30 and -- with --full -- 15 degrees.  Every figure is the median of `--repeat` timed calls after
one untimed call; a call is timed from the host, end to end (rotation tables, launch, copy back), which is what a scan pays.

    python tools/dimer_bench.py [--repeat 5] [--full] [--json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mpmc_amd import engine  # noqa: E402

E2REDUCED = 408.7816
N2 = dict(pos=np.array([[0.0, 0, 0], [0.549, 0, 0], [-0.549, 0, 0], [0.790811, 0, 0], [-0.790811, 0, 0]]),
          charge=np.array([1.0474, -0.5237, -0.5237, 0.0, 0.0]) * E2REDUCED, alpha=np.array([1.49645, 0.4551, 0.4551, 0.0, 0.0]),
          epsilon=np.array([27.02224, 0.0, 0.0, 14.55166, 14.55166]), sigma=np.array([3.43565, 0.0, 0.0, 3.08409, 3.08409]),
          mass=np.array([0.0, 14.0067, 14.0067, 0.0, 0.0]))
POLAR = dict(polar_damp=2.1304, polar_gs_ranked=1, polar_palmo=1, polar_max_iter=5)


def loop_values(top, step):
    out, x = [], 0.0
    while x <= top:
        out.append(x)
        x += step
    return out


def timed(fn, repeat):
    fn()
    t = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--full", action="store_true", help="also the 15 degree grid (6.6e7 placements per call)")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args()
    eng = engine.Engine(64, device=0)
    rows = []
    for label, mol in (("not polarizable", dict(N2, alpha=np.zeros(5))), ("polarizable", N2)):
        rng = np.random.default_rng(1)
        for nconf in (4096, 65536, 1 << 20):
            conf = rng.uniform(0.0, 2.0 * math.pi, (nconf, 7))
            conf[:, 0] = rng.uniform(3.0, 8.0, nconf)
            med, lo, hi = timed(lambda: eng.dimer_energies(mol, mol, conf, **POLAR), args.repeat)
            rows.append(dict(form="list", molecule=label, placements=nconf, seconds=med, min=lo, max=hi, per_second=nconf / med))
        for deg in (60, 30) + ((15,) if args.full else ()):
            step = math.radians(deg)
            a, b = loop_values(2.0 * math.pi, step), loop_values(math.pi, step)
            lists = [a, b, a, a, b, a]
            count = (len(a) * len(b) * len(a)) ** 2
            med, lo, hi = timed(lambda: eng.dimer_grid_means(mol, mol, 4.0, lists, **POLAR), args.repeat if deg > 15 else 1)
            rows.append(dict(form="grid %d deg" % deg, molecule=label, placements=count, seconds=med, min=lo, max=hi,
                             per_second=count / med))
    eng.close()
    if args.json:
        print(json.dumps(rows))
        return
    for r in rows:
        print("%-12s %-16s %10d placements  %9.4f s (%.4f .. %.4f)  %.3e placements/s" % (
            r["form"], r["molecule"], r["placements"], r["seconds"], r["min"], r["max"], r["per_second"]))


if __name__ == "__main__":
    main()
