#!/usr/bin/env python3
"""Steps/s of an NPT chain whose every step is a volume move (volume_probability 1.0), (i) with the volume notes
(the resident configuration is moved into the new box: mpmc_hip_scale_box) and (ii) without them (every step uploads
the whole configuration again, what an un-hooked caller gets), in alternating repetitions after a warm-up.

    python tools/npt_volume_bench.py [--workloads pcn61_4096,spol_1024] [--steps 300] [--warmup 50] [--reps 3]

Prints one line per repetition and one JSON summary line per workload (median, min, max of each arm)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="pcn61_4096,spol_1024")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    import bench
    from mpmc_amd import host

    for name in args.workloads.split(","):
        system, flags, label = bench.load_workload(name)
        extra = {"ensemble": "npt", "pressure": "1.0", "volume_probability": "1.0", "volume_change_factor": "0.002"}
        arms = {}
        for arm, notes in (("scale_box", True), ("full_upload", False)):
            h = host.HostSystem(system, flags, seed=args.seed, extra=extra)
            h.set_volume_notes(notes)
            h.mc_steps(args.warmup)
            arms[arm] = (h, [])
        for rep in range(args.reps):
            for arm in ("scale_box", "full_upload"):  # alternating, on one device in one session
                h, rates = arms[arm]
                t0 = time.perf_counter()
                h.mc_steps(args.steps)
                dt = time.perf_counter() - t0
                rates.append(args.steps / dt)
                print("%s rep %d %-11s %9.1f steps/s" % (name, rep, arm, rates[-1]), flush=True)
        out = {"workload": name, "label": label, "steps": args.steps, "warmup": args.warmup, "reps": args.reps}
        for arm, (h, rates) in arms.items():
            o = h.observables()
            rates = sorted(rates)
            out[arm] = {"median": rates[len(rates) // 2], "min": rates[0], "max": rates[-1],
                        "accept_volume": o["accept_volume"], "reject_volume": o["reject_volume"]}
            h.close()
        out["ratio_of_medians"] = out["scale_box"]["median"] / out["full_upload"]["median"]
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
