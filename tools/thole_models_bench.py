#!/usr/bin/env python3
"""What the dipole tensor's model (mpmc_hip_set_thole_model) costs on one device, in one session, on the 4096-atom PCN-61
box of bench.py (tests/golden/pcn61_bssp_4096.npz, its flags: Jacobi x4, rc 8 A, FH4):

  * the wall time of one energy() -- the call waits for the device's record -- after an upload (the full pass: the whole
    coefficient store is built, with everything else an upload rebuilds) and after a move of one molecule (the
    steady-state step: the moved sites' rows of the store), for polar_damp_type exponential (the default: the
    baseline), linear, off and exponential + polar_wolf_full, one context each, the arms alternating;
  * the ratio of each model's medians to the exponential model's from the same run;
  * from the engine's own events (option "timing" = 2) the A-matrix class (amatrix_ms: the coefficient build / update
    launches) of the same calls, in a second pass so that the events do not sit in the wall times.

    python tools/thole_models_bench.py [--reps 60] [--warmup 10] [--out DIR]

Only the build of the store differs between the models: every sweep reads the same {c3, c5} pairs.  Prints one line per
model and one JSON summary line; --out DIR also writes both to DIR/thole_models_bench.txt."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARMS = [("exponential", dict()), ("linear", dict(polar_damp_type="linear")), ("off", dict(polar_damp_type="off")),
        ("wolf_full", dict(polar_damp_type="exponential", polar_wolf_full=1))]
_lines = []


def say(text):
    print(text, flush=True)
    _lines.append(text)


def stats(us):
    us = np.sort(np.asarray(us))
    return dict(median_us=float(us[len(us) // 2]), min_us=float(us[0]), p90_us=float(us[int(0.9 * len(us))]), n=len(us))


def one_call(e, s, first, count, rep, full):
    """one timed energy(): after an upload (full) or after a rigid move of one molecule (the steady-state step)"""
    if full:
        e.upload(s)
    else:
        e.update_atoms(first, s["pos"][first:first + count] + 0.01 * (1 + rep % 7))
    t0 = time.perf_counter()
    r = e.energy()
    dt = time.perf_counter() - t0
    if r["status"] != 0:
        raise RuntimeError("status %d" % r["status"])
    return 1e6 * dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import bench
    from mpmc_amd import engine

    s, flags, label = bench.load_workload("pcn61_4096")
    mol, frozen = np.asarray(s["molecule"]), np.asarray(s["frozen"])
    first = int(np.flatnonzero(frozen == 0)[0])
    count = int(np.count_nonzero(mol == mol[first]))
    say("%s; the moved molecule: atoms %d .. %d" % (label, first, first + count - 1))
    engines = {}
    for name, kw in ARMS:
        e = engine.Engine(len(s["charge"]))
        e.load_system(s, dict(flags, **kw))
        engines[name] = e
    wall = {(name, full): [] for name in engines for full in (True, False)}
    for rep in range(args.warmup + args.reps):
        for full in (True, False):
            for name, e in engines.items():  # alternating, on one device in one session
                t = one_call(e, s, first, count, rep, full)
                if rep >= args.warmup:
                    wall[(name, full)].append(t)
    out = {"workload": label, "reps": args.reps, "warmup": args.warmup, "models": {}}
    for name, e in engines.items():
        m = {"full": stats(wall[(name, True)]), "one_molecule": stats(wall[(name, False)])}
        e.set_option("timing", 2)
        ev = {True: [], False: []}
        for rep in range(max(5, args.reps // 4)):
            for full in (True, False):
                one_call(e, s, first, count, rep, full)
                ev[full].append(1e3 * e.timings()["amatrix_ms"])
        m["full"]["amatrix_event_us"] = float(np.median(ev[True]))
        m["one_molecule"]["amatrix_event_us"] = float(np.median(ev[False]))
        m["polarization_energy"] = e.energy()["polarization_energy"]
        e.close()
        out["models"][name] = m
    base = out["models"]["exponential"]
    for name, m in out["models"].items():
        for k in ("full", "one_molecule"):
            m["ratio_" + k] = m[k]["median_us"] / base[k]["median_us"]
        say("%-12s full %8.1f us (min %8.1f, p90 %8.1f; store build events %7.1f)  one molecule %7.1f us (min %7.1f, p90 %7.1f; "
            "store update events %6.1f) | to exponential: full %5.3f, one molecule %5.3f | U_pol %.6f K" % (
                name, m["full"]["median_us"], m["full"]["min_us"], m["full"]["p90_us"], m["full"]["amatrix_event_us"],
                m["one_molecule"]["median_us"], m["one_molecule"]["min_us"], m["one_molecule"]["p90_us"],
                m["one_molecule"]["amatrix_event_us"], m["ratio_full"], m["ratio_one_molecule"], m["polarization_energy"]))
    say(json.dumps(out))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "thole_models_bench.txt"), "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
