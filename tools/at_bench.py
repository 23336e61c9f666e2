#!/usr/bin/env python3
"""What the Axilrod-Teller term (axilrod_teller) costs on one device, in one session:

  * the from-scratch pass of at_triple_kernel (+ the sum of its partials) from the engine's own events (option
    "timing" = 2) at --sizes sites of synth.s_at: pair_ms of an rd_only evaluation with the term minus pair_ms of the
    same evaluation without it (the class then holds the Lennard-Jones tile kernel only, doing the same work in both),
    as unordered atom triples per second and as a fraction of the fp64 vector peak;
  * the incremental pass after a move of one single-site molecule (one dirty block), the same way;
  * NVT steps/s of s_at(--atoms) through the C host layer with and without the term, in alternating repetitions.

    python tools/at_bench.py [--sizes 512,1024,4096] [--atoms 512] [--steps 500] [--warmup 50] [--reps 3]

Prints one line per measurement and one JSON summary line.  The peak the fraction refers to is 78.6 TFLOP/s: half the
157.3 TFLOP/s fp32 vector rate (an fp64 FMA issues at half the fp32 rate on this chip); a triple is counted as
FLOP_PER_TRIPLE operations (three dot products, the two triple products, the 1 - 3x, the sum of the three g and the
division counted as one operation), so the fraction understates the issue slots the division really takes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FP64_VECTOR_PEAK = 78.6e12
FLOP_PER_TRIPLE = 24


def _stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def kernel_times(n, reps):
    import numpy as np

    from mpmc_amd import engine, synth

    s = synth.s_at(n)
    out = {"atoms": n, "triples": n * (n - 1) * (n - 2) // 6}
    last = n - 1  # a single-site molecule: one dirty block
    assert s["molecule"][last] != s["molecule"][last - 1]
    for arm, on in (("with", 1), ("without", 0)):
        flags = dict(synth.FLAGS_LJ, axilrod_teller=on)
        e = engine.Engine(n)
        e.set_option("timing", 2)
        full, incr = [], []
        for rep in range(reps + 1):
            e.load_system(s, flags)  # an upload: every block triple is redone
            e.energy()
            full.append(e.timings()["pair_ms"])
            e.update_atoms(last, s["pos"][last:last + 1] + 0.01 * (rep + 1))
            e.energy()
            incr.append(e.timings()["pair_ms"])
        e.close()
        out[arm] = {"from_scratch_ms": _stats(full[1:]), "one_block_ms": _stats(incr[1:])}
    for key in ("from_scratch_ms", "one_block_ms"):
        out["at_" + key] = out["with"][key]["median"] - out["without"][key]["median"]
    nb = (n + 127) // 128 * 2
    out["blocks"] = nb
    out["triples_per_s"] = out["triples"] / (1e-3 * out["at_from_scratch_ms"])
    out["fraction_of_fp64_vector_peak"] = out["triples_per_s"] * FLOP_PER_TRIPLE / FP64_VECTOR_PEAK
    # the incremental pass redoes the nb (nb + 1) / 2 block triples that hold the moved block
    out["one_block_triples_per_s"] = (nb * (nb + 1) // 2) * 64.0 ** 3 / 6.0 / (1e-3 * max(out["at_one_block_ms"], 1e-6))
    print("N %5d: from scratch %8.3f ms (%.3g triples/s, %.3f of the fp64 vector peak), one block %7.3f ms" %
          (n, out["at_from_scratch_ms"], out["triples_per_s"], out["fraction_of_fp64_vector_peak"], out["at_one_block_ms"]),
          flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,1024,4096")
    ap.add_argument("--atoms", type=int, default=512)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    from mpmc_amd import host, synth

    out = {"steps": args.steps, "warmup": args.warmup, "reps": args.reps, "nvt_atoms": args.atoms,
           "kernel": [kernel_times(int(n), args.kernel_reps) for n in args.sizes.split(",") if n]}
    system = synth.s_at(args.atoms)
    arms = {}
    for arm, on in (("with", 1), ("without", 0)):
        h = host.HostSystem(system, dict(synth.FLAGS_AT, axilrod_teller=on), seed=args.seed)
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
    out["nvt_ratio_of_medians"] = out["nvt_with"]["median"] / out["nvt_without"]["median"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
