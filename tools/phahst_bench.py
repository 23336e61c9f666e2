#!/usr/bin/env python3
"""NVT steps/s of the PHAHST box (synth.s_phahst(N) + FLAGS_PHAHST) beside the Lennard-Jones polarizable box
(synth.s_pol(N) + FLAGS_POL_JACOBI) on the same build and device, in alternating repetitions after a warm-up, and the
from-scratch time of the dense tile kernel from the engine's own events.

    python tools/phahst_bench.py [--atoms 4096] [--steps 1000] [--warmup 100] [--reps 3]

Prints one line per repetition and one JSON summary line (median, min, max of each arm, the ratio of the medians).  The
two boxes differ in more than the potential (three-site against five-site molecules, a frozen third), so the ratio says what
a PHAHST user gets next to the benchmark box, not what the term costs; the kernel times say that."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_times(system, flags, reps=5):
    """pair_ms of from-scratch rd_only evaluations with every kernel class timed (option "timing" = 2): (i) in PHAHST mode,
    where the class holds the Lennard-Jones tile kernel on zero parameters plus disp_tile_kernel and the sum of its tile
    partials, and (ii) the same atoms with epsilon = sigma = 0 and no dispersion record, where it holds the Lennard-Jones
    tile kernel doing exactly the work it does in (i).  The difference is the dense kernel and its sum."""
    import numpy as np

    from mpmc_amd import engine

    out = {}
    zero = dict(system, epsilon=np.zeros(len(system["charge"])), sigma=np.zeros(len(system["charge"])))
    for arm, on in (("phahst", 1), ("lj_zero", 0)):
        f = dict(flags, rd_only=1, disp_expansion=on)
        system = system if on else zero
        e = engine.Engine(len(system["charge"]))
        e.set_option("timing", 2)
        ms = []
        for _ in range(reps + 1):
            e.load_system(system, f)  # an upload: every tile is redone
            e.energy()
            ms.append(e.timings()["pair_ms"])
        e.close()
        ms = sorted(ms[1:])
        out[arm] = {"median": ms[len(ms) // 2], "min": ms[0], "max": ms[-1]}
    out["disp_tile_kernel_ms"] = out["phahst"]["median"] - out["lj_zero"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    from mpmc_amd import host, synth

    boxes = {"phahst": (synth.s_phahst(args.atoms), dict(synth.FLAGS_PHAHST)),
             "lj_pol": (synth.s_pol(args.atoms), dict(synth.FLAGS_POL_JACOBI))}
    arms = {}
    for arm, (system, flags) in boxes.items():
        h = host.HostSystem(system, flags, seed=args.seed)
        h.mc_steps(args.warmup)
        arms[arm] = (h, [])
    for rep in range(args.reps):
        for arm in ("phahst", "lj_pol"):  # alternating, on one device in one session
            h, rates = arms[arm]
            t0 = time.perf_counter()
            h.mc_steps(args.steps)
            rates.append(args.steps / (time.perf_counter() - t0))
            print("rep %d %-7s %9.1f steps/s" % (rep, arm, rates[-1]), flush=True)
    out = {"atoms": args.atoms, "steps": args.steps, "warmup": args.warmup, "reps": args.reps}
    for arm, (h, rates) in arms.items():
        o = h.observables()
        rates = sorted(rates)
        out[arm] = {"median": rates[len(rates) // 2], "min": rates[0], "max": rates[-1], "accept": o["accept"],
                    "reject": o["reject"]}
        h.close()
    out["ratio_of_medians"] = out["phahst"]["median"] / out["lj_pol"]["median"]
    out["from_scratch_pair_ms"] = kernel_times(*boxes["phahst"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
