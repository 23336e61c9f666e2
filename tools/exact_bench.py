#!/usr/bin/env python3
"""What the exact Thole dipoles (polar_iterative off: mpmc_hip_set_exact_polar, kernels_exact.h) cost on one device, in one
session.  Per box, in an energy() after a one-molecule move (the matrix is updated incrementally, the factorization is
from scratch, as in every call):

  * the solve -- copy, blocked Cholesky, two substitutions, U_pol -- from the engine's own events (option "timing" = 2:
    class palmo_ms brackets exactly those launches in this mode), and the wall time of the call;
  * launches per solve, 5 np + 1 with np = ceil(3 nv / 64), hence microseconds per launch;
  * the trailing-update kernel alone (class sweep_ms: each launch's own begin / end timestamps), its share of the solve
    and its fp64 flop rate: 2 * 64^3 flops per 64 x 64 tile, sum over the panels of m (m + 1) / 2 tiles, m = np - 1 - k;
    with the bytes it moves through the memory system -- per tile two 64 x 64 operands read, the tile read and written --
    this gives bytes per second, and flops per byte = 4;
  * numpy.linalg.solve on the same downloaded matrix and field on this host with one thread: the line the reference's LU
    inversion should be compared with (that one is 2 n^3 flops and unblocked);
  * the engine's own Jacobi x4 step on the same box after the same move, for scale.

    python tools/exact_bench.py [--boxes spol256,spol1024,spol4096,pcn61] [--reps 3] [--cpu-max-rows 10000]

Prints one line per measurement and one JSON summary line; --out DIR also writes both to DIR/exact_bench.txt."""
import os

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):  # the CPU line is single-threaded
    os.environ[_v] = "1"

import argparse  # noqa: E402
import json  # noqa: E402
import sys  # noqa: E402
import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

EXACT = dict(temperature=77.0, polarization=1, polar_damp=2.1304, polar_iterative=0)
JACOBI = dict(temperature=77.0, polarization=1, polar_damp=2.1304, polar_max_iter=4)
_lines = []


def say(text):
    print(text, flush=True)
    _lines.append(text)


def load_box(name):
    from mpmc_amd import synth

    if name == "pcn61":  # the headline box of bench.py
        return dict(np.load(os.path.join(ROOT, "tests", "golden", "pcn61_bssp_4096.npz"))), dict(pbc_cutoff=8.0)
    return synth.s_pol(int(name[4:])), {}


def last_molecule(s):
    """the atoms of the last movable molecule with a polarizable site"""
    mol, frozen, alpha = np.asarray(s["molecule"]), np.asarray(s["frozen"]), np.asarray(s["alpha"])
    for m in np.unique(mol)[::-1]:
        at = np.flatnonzero(mol == m)
        if not frozen[at].any() and (alpha[at] != 0.0).any():
            return at
    raise ValueError("no movable polarizable molecule")


def median(v):
    return sorted(v)[len(v) // 2]


def run(e, s, at, reps, key):
    wall, ev, sub, cnt = [], [], [], 0
    for rep in range(reps):
        e.update_atoms(int(at[0]), s["pos"][at] + 0.01 * (rep + 1))
        t0 = time.perf_counter()
        r = e.energy()
        wall.append(1e3 * (time.perf_counter() - t0))
        t = e.timings()
        ev.append(t[key])
        sub.append(t["sweep_ms"])
        cnt = t["sweep_count"]
    return r, median(wall), median(ev), median(sub), cnt, ev


def measure(name, reps, cpu_max_rows):
    from mpmc_amd import engine

    s, extra = load_box(name)
    n = len(s["charge"])
    at = last_molecule(s)
    nv = int((np.asarray(s["alpha"]) != 0.0).sum())
    rows = 3 * nv
    npan = (rows + 63) // 64
    e = engine.Engine(n)
    e.set_option("timing", 2)
    e.load_system(s, dict(EXACT, **extra))
    t0 = time.perf_counter()
    e.energy()
    first = time.perf_counter() - t0
    r, wall, solve, trail, ntrail, solve_all = run(e, s, at, reps, "palmo_ms")
    assert r["iter_success"] == 0 and r["polar_iterations"] == 0
    launches = 5 * npan + 1
    tiles = sum(m * (m + 1) // 2 for m in range(1, npan))
    flops = 2.0 * 64 ** 3 * tiles
    nbytes = 4.0 * 64 * 64 * 8 * tiles
    out = dict(box=name, atoms=n, sites=nv, rows=rows, panels=npan, launches=launches, solve_ms=solve, solve_ms_all=solve_all,
               call_wall_ms=wall, first_call_s=first, us_per_launch=1e3 * solve / launches, trail_ms=trail,
               trail_launches=ntrail, trail_share=trail / solve if solve > 0 else 0.0,
               trail_tflops=flops / (1e-3 * trail) / 1e12 if trail > 0 else 0.0,
               trail_tb_per_s=nbytes / (1e-3 * trail) / 1e12 if trail > 0 else 0.0,
               factor_flops=rows ** 3 / 3.0, u_pol=r["polarization_energy"])
    say("solve  %-9s %5d atoms, %5d rows, %3d panels: %9.3f ms by events, %9.3f ms wall per call; %4d launches = %6.2f us "
        "each" % (name, n, rows, npan, solve, wall, launches, out["us_per_launch"]))
    say("trail  %-9s %4d launches, %9.3f ms = %4.1f %% of the solve; %.3g flop = %6.2f Tflop/s fp64; %.3g B = %5.2f TB/s" %
        (name, ntrail, trail, 100.0 * out["trail_share"], flops, out["trail_tflops"], nbytes, out["trail_tb_per_s"]))
    if rows <= cpu_max_rows:
        d = e.dipoles()
        pol = np.repeat(np.asarray(s["alpha"]) != 0.0, 3)
        A = e.amatrix()[np.ix_(pol, pol)]
        E = d["ef_static"].reshape(-1)[pol]
        t0 = time.perf_counter()
        mu = np.linalg.solve(A, E)
        dt = time.perf_counter() - t0
        diff = float(np.abs(mu - d["mu"].reshape(-1)[pol]).max() / np.abs(mu).max())
        out.update(cpu_solve_ms=1e3 * dt, cpu_max_rel_diff=diff)
        say("cpu    %-9s %5d rows: %9.3f ms numpy.linalg.solve, one thread (dipoles agree to %.2g of the largest)" %
            (name, rows, 1e3 * dt, diff))
        del A
    e.close()
    j = engine.Engine(n)
    j.set_option("timing", 2)
    j.load_system(s, dict(JACOBI, **extra))
    j.energy()
    rj, wallj, _, _, _, _ = run(j, s, at, reps, "total_ms")
    tot = j.timings()["total_ms"]
    j.close()
    out.update(jacobi4_wall_ms=wallj, jacobi4_total_ms=tot, jacobi4_u_pol=rj["polarization_energy"],
               jacobi4_rel_diff=abs(rj["polarization_energy"] - out["u_pol"]) / abs(out["u_pol"]))
    say("jacobi %-9s Jacobi x4 step: %9.3f ms wall per call (%.3f ms first launch to last kernel end); U_pol differs by "
        "%.2g relative" % (name, wallj, tot, out["jacobi4_rel_diff"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", default="spol256,spol1024,spol4096,pcn61")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-max-rows", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_solve"))
    args = ap.parse_args()
    out = [measure(b, args.reps, args.cpu_max_rows) for b in args.boxes.split(",") if b]
    say(json.dumps(out))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "exact_bench.txt"), "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
