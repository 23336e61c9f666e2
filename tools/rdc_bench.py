#!/usr/bin/env python3
"""What rd_crystal (Lennard-Jones over lattice images) costs on one device, in one session:

  * the from-scratch pass of rdc_tile_kernel (+ the sum of its partials) from the engine's own events (option
    "timing" = 2) on synth.s_pol(--atoms), at the orders of --orders: pair_ms of an rd_only evaluation with the mode on
    minus pair_ms of the same evaluation with it off (the class then holds the Lennard-Jones tile kernel only, which runs
    in both arms), and as pair images per second;
  * the incremental pass after a move of one molecule (one or two dirty blocks), the same way;
  * NVT steps/s of the same box (Lennard-Jones + Ewald) through the C host layer with the mode on (first order of
    --orders) and off, in alternating repetitions.

    python tools/rdc_bench.py [--atoms 4096] [--orders 2,3] [--steps 300] [--warmup 50] [--reps 3]

Prints one line per measurement and one JSON summary line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RD = dict(temperature=77.0, rd_only=1, rd_lrc=1)
NVT = dict(temperature=77.0, rd_lrc=1)  # Lennard-Jones + Ewald


def _stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def kernel_times(s, order, reps):
    from mpmc_amd import engine

    n = len(s["charge"])
    out = {"atoms": n, "order": order, "images": (2 * order - 1) ** 3}
    for arm, flags in (("with", dict(RD, rd_crystal=1, rd_crystal_order=order)), ("without", dict(RD))):
        e = engine.Engine(n)
        e.set_option("timing", 2)
        full, incr = [], []
        for rep in range(reps + 1):
            e.load_system(s, flags)  # an upload: every tile is redone
            e.energy()
            full.append(e.timings()["pair_ms"])
            e.update_atoms(0, s["pos"][0:5] + 0.01 * (rep + 1))  # the first five-site molecule
            e.energy()
            incr.append(e.timings()["pair_ms"])
        e.close()
        out[arm] = {"from_scratch_ms": _stats(full[1:]), "one_move_ms": _stats(incr[1:])}
    for key in ("from_scratch_ms", "one_move_ms"):
        out["rdc_" + key] = out["with"][key]["median"] - out["without"][key]["median"]
    pairs = n * (n - 1) // 2
    out["pair_images_per_s"] = pairs * out["images"] / (1e-3 * out["rdc_from_scratch_ms"])
    print("N %5d order %d (%3d images): from scratch %8.3f ms (%.3g pair images/s), one move %7.3f ms" %
          (n, order, out["images"], out["rdc_from_scratch_ms"], out["pair_images_per_s"], out["rdc_one_move_ms"]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=4096)
    ap.add_argument("--orders", default="2,3")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    from mpmc_amd import host, synth

    system = synth.s_pol(args.atoms)
    orders = [int(o) for o in args.orders.split(",") if o]
    out = {"steps": args.steps, "warmup": args.warmup, "reps": args.reps, "atoms": args.atoms,
           "kernel": [kernel_times(system, o, args.kernel_reps) for o in orders]}
    arms = {}
    for arm, flags in (("with", dict(NVT, rd_crystal=1, rd_crystal_order=orders[0])), ("without", dict(NVT))):
        h = host.HostSystem(system, flags, seed=args.seed)
        h.mc_steps(args.warmup)
        arms[arm] = (h, [])
    for rep in range(args.reps):
        for arm in ("with", "without"):  # alternating, on one device in one session
            h, rates = arms[arm]
            t0 = time.perf_counter()
            h.mc_steps(args.steps)
            rates.append(args.steps / (time.perf_counter() - t0))
            print("rep %d %-8s %9.1f steps/s" % (rep, arm, rates[-1]), flush=True)
    for arm, (h, rates) in arms.items():
        o = h.observables()
        out["nvt_" + arm] = dict(_stats(rates), accept=o["accept"], reject=o["reject"])
        h.close()
    out["nvt_order"] = orders[0]
    out["nvt_ratio_of_medians"] = out["nvt_with"]["median"] / out["nvt_without"]["median"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
