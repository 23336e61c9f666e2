#!/usr/bin/env python3
"""What one pair potential of mpmc_hip_set_rd_form costs on one device, in one session, on S-LJ-style boxes
(synth.s_lj: single-site atoms, eps 120 K, sigma 3.4 A, jittered cubic lattice of spacing 3.8 A, rd_only):

  * the wall time of one energy() -- the call waits for the device's record -- after an upload (the full pass: every
    tile) and after a move of one atom (the incremental pass: the tiles of one block), for the form of --form under
    --mixing;
  * beside it the same two times of the standard Lennard-Jones path (screened, candidate lists) on the same box, the
    arms alternating, and the ratio of the medians.  The dense forms form every pair's minimum image and have no screen;
    the ratio says what that costs.
  * from the engine's own events (option "timing" = 2) the pair class of the same calls, in a second pass so that the
    events do not sit in the wall times.

    python tools/rdforms_bench.py --form dreiding [--mixing lb] [--atoms 256,1024,4096] [--reps 60] [--fh 0|2|4]
                                  [--out DIR]

One form per call.  Prints one line per box and one JSON summary line; --out DIR also writes both to
DIR/rdforms_bench_<form>_<mixing>.txt."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_lines = []


def say(text):
    print(text, flush=True)
    _lines.append(text)


def stats(us):
    us = np.sort(np.asarray(us))
    return dict(median_us=float(us[len(us) // 2]), min_us=float(us[0]), p90_us=float(us[int(0.9 * len(us))]), n=len(us))


def one_call(e, s, rep, full):
    """one timed energy(): after an upload (full) or after a move of atom 0 (incremental)"""
    if full:
        e.upload(s)
    else:
        e.update_atoms(0, s["pos"][0:1] + 0.01 * (1 + rep % 7))
    t0 = time.perf_counter()
    r = e.energy()
    dt = time.perf_counter() - t0
    if r["status"] != 0:
        raise RuntimeError("status %d" % r["status"])
    return 1e6 * dt


def box(n, form, mixing, fh, reps, warmup):
    from mpmc_amd import engine, synth

    s = synth.s_lj(n)
    flags = dict(temperature=77.0, rd_only=1, rd_lrc=1)
    if fh:
        flags.update(feynman_hibbs=1, feynman_hibbs_order=fh)
    arms = {}
    for arm in ("form", "standard"):
        e = engine.Engine(n)
        e.load_system(s, flags)
        if arm == "form":
            e.set_rd_form(form, mixing)
        arms[arm] = e
    out = {"atoms": n, "pairs": n * (n - 1) // 2, "tiles_a_side": -(-n // 128) * 2}
    wall = {(arm, full): [] for arm in arms for full in (True, False)}
    for rep in range(warmup + reps):
        for full in (True, False):
            for arm, e in arms.items():  # alternating, on one device in one session
                t = one_call(e, s, rep, full)
                if rep >= warmup:
                    wall[(arm, full)].append(t)
    for arm, e in arms.items():
        out[arm] = {"full": stats(wall[(arm, True)]), "incremental": stats(wall[(arm, False)])}
        e.set_option("timing", 2)
        ev = {True: [], False: []}
        for rep in range(max(5, reps // 4)):
            for full in (True, False):
                one_call(e, s, rep, full)
                ev[full].append(1e3 * e.timings()["pair_ms"])
        out[arm]["full"]["pair_class_event_us"] = float(np.median(ev[True]))
        out[arm]["incremental"]["pair_class_event_us"] = float(np.median(ev[False]))
        out[arm]["rd_energy"] = e.energy()["rd_energy"]
        e.close()
    for k in ("full", "incremental"):
        out["ratio_" + k] = out["form"][k]["median_us"] / out["standard"][k]["median_us"]
    say("N %5d %-16s %-14s full %8.1f us (min %8.1f, p90 %8.1f; events %8.1f)  one move %7.1f us (min %7.1f, p90 %7.1f; "
        "events %7.1f) | standard LJ path: full %7.1f us (events %7.1f), one move %6.1f us (events %6.1f) | ratio full %5.2f "
        "one move %5.2f" % (
            n, form + (" fh%d" % fh if fh else ""), mixing,
            out["form"]["full"]["median_us"], out["form"]["full"]["min_us"], out["form"]["full"]["p90_us"],
            out["form"]["full"]["pair_class_event_us"],
            out["form"]["incremental"]["median_us"], out["form"]["incremental"]["min_us"], out["form"]["incremental"]["p90_us"],
            out["form"]["incremental"]["pair_class_event_us"],
            out["standard"]["full"]["median_us"], out["standard"]["full"]["pair_class_event_us"],
            out["standard"]["incremental"]["median_us"], out["standard"]["incremental"]["pair_class_event_us"],
            out["ratio_full"], out["ratio_incremental"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--form", required=True, choices=["lj", "sg", "dreiding", "lj_buffered_14_7"])
    ap.add_argument("--mixing", default="lb", choices=["lb", "waldmanhagler", "halgren_mixing", "c6_mixing"])
    ap.add_argument("--atoms", default="256,1024,4096")
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--fh", type=int, default=0, choices=[0, 2, 4])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"form": args.form, "mixing": args.mixing, "fh": args.fh, "reps": args.reps, "warmup": args.warmup,
           "boxes": [box(int(n), args.form, args.mixing, args.fh, args.reps, args.warmup) for n in args.atoms.split(",") if n]}
    say(json.dumps(out))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "rdforms_bench_%s_%s.txt" % (args.form, args.mixing)), "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
