#!/usr/bin/env python3
"""What a grand-canonical edit costs in the dense energy modes on one device, in one session: the wall time of one
energy() -- the call waits for the device's record -- in three situations, the arms alternating after a warm-up, on one
context per mode:

  (a) after edit_molecules(): one molecule removed and inserted elsewhere in the box (it takes its own slots back);
  (b) after upload() and the mode's per-atom setter: what the same step cost while these modes had no device-side edits
      (every sum from scratch);
  (c) after update_atoms() of one molecule: an ordinary displacement.

Beside each energy() the wall time of the call in front of it (the edit, the upload + setter, the update) is reported:
(b)'s upload is part of what a chain paid.  Modes, all rd_only so that the dense terms are what is timed:

  phahst      synth.s_phahst, disp_expansion + damp_dispersion + extrapolate_disp_coeffs, rd_lrc
  at          synth.s_at, Lennard-Jones + axilrod_teller, rd_lrc
  rd_crystal  synth.s_pol, rd_crystal_order 2, rd_lrc
  rd_form     synth.s_pol, dreiding

    python tools/dense_edits_bench.py [--modes phahst,at,rd_crystal,rd_form] [--atoms 1024,4096] [--reps 40] [--warmup 5]
                                      [--at-reps 6] [--out DIR]

--at-reps: repetitions of the three-body mode from 4096 atoms on (its from-scratch pass is 1.1e10 triples).  Prints one
line per mode and box and one JSON summary line; --out DIR also writes both to DIR/dense_edits_bench.txt."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

_lines = []
FIELDS = ("charge", "alpha", "epsilon", "sigma", "mass")


def say(text):
    print(text, flush=True)
    _lines.append(text)


def stats(us):
    us = np.sort(np.asarray(us))
    return dict(median_us=float(us[len(us) // 2]), min_us=float(us[0]), p90_us=float(us[int(0.9 * len(us))]), n=len(us))


def mode_setup(mode, n):
    from mpmc_amd import synth

    rd = dict(temperature=77.0, rd_only=1, rd_lrc=1)
    if mode == "phahst":
        return synth.s_phahst(n), dict(rd, disp_expansion=1, damp_dispersion=1, extrapolate_disp_coeffs=1)
    if mode == "at":
        return synth.s_at(n), dict(rd, axilrod_teller=1)
    if mode == "rd_crystal":
        return synth.s_pol(n), dict(rd, rd_crystal=1, rd_crystal_order=2)
    if mode == "rd_form":
        return synth.s_pol(n), dict(rd, dreiding=1)
    raise ValueError(mode)


def molecules(s):
    """(first, count) of the molecules an edit may take: not frozen, at most 16 atoms"""
    mol = np.asarray(s["molecule"])
    cut = np.flatnonzero(mol[1:] != mol[:-1]) + 1
    first = np.concatenate([[0], cut])
    last = np.concatenate([cut, [len(mol)]])
    return [(int(a), int(b - a)) for a, b in zip(first, last) if not s["frozen"][a] and b - a <= 16]


def timed(call):
    t0 = time.perf_counter()
    out = call()
    return 1e6 * (time.perf_counter() - t0), out


def box(mode, n, reps, warmup):
    from mpmc_amd import engine

    s, flags = mode_setup(mode, n)
    e = engine.Engine(n + 64)
    e.load_system(s, flags)
    e.energy()
    mols = molecules(s)
    pos = s["pos"].copy()  # where the device's atoms are now
    shift = 0.37 * np.array([1.0, -1.0, 0.5])

    def molecule(first, count, rep):
        sl = slice(first, first + count)
        pos[sl] += shift * (1 if rep % 2 == 0 else -1)
        d = dict(pos=pos[sl], **{k: s[k][sl] for k in FIELDS})
        d.update({k: s[k][sl] for k in ("c6", "c8", "c10") if k in s})
        if flags.get("axilrod_teller"):
            d["c9"] = engine.effective_c9(s, False)[sl]
        return d

    def edit(rep):
        first, count = mols[(7 * rep) % len(mols)]
        got = e.edit_molecules([(first, count)], [molecule(first, count, rep)])
        if got != [first]:
            raise RuntimeError("edit_molecules answered %r for the molecule at %d" % (got, first))

    def upload(rep):
        cur = dict(s, pos=pos)
        e.upload(cur)
        if flags.get("disp_expansion"):
            e.set_dispersion(cur, **{k: flags[k] for k in engine.DISP_NAMES if k in flags})
        if flags.get("axilrod_teller"):
            e.set_axilrod_teller(cur)

    def update(rep):
        first, count = mols[(7 * rep + 3) % len(mols)]
        sl = slice(first, first + count)
        pos[sl] -= shift * (1 if rep % 2 == 0 else -1)
        e.update_atoms(first, pos[sl])

    arms = (("edit", edit), ("upload", upload), ("update", update))
    wall = {name: [] for name, _ in arms}
    prep = {name: [] for name, _ in arms}
    for rep in range(warmup + reps):
        for name, call in arms:  # alternating, on one device in one session
            # (an edit needs a context that has been evaluated since its upload: every arm ends in an energy())
            tp, _ = timed(lambda: call(rep))
            te, r = timed(e.energy)
            if r["status"] != 0:
                raise RuntimeError("status %d" % r["status"])
            if rep >= warmup:
                wall[name].append(te)
                prep[name].append(tp)
    out = {"mode": mode, "atoms": n, "blocks": -(-n // 64)}
    for name, _ in arms:
        out[name] = dict(stats(wall[name]), call_before_median_us=float(np.median(prep[name])))
    out["edit_over_upload"] = out["edit"]["median_us"] / out["upload"]["median_us"]
    out["edit_over_update"] = out["edit"]["median_us"] / out["update"]["median_us"]
    e.close()
    say("%-10s N %5d  energy() after (a) edit %9.1f us (min %9.1f, p90 %9.1f; the edit call %6.1f us)  (b) upload + setter "
        "%11.1f us (min %11.1f, p90 %11.1f; the upload %8.1f us)  (c) update %9.1f us (min %9.1f, p90 %9.1f; the update %5.1f us)"
        "  | (a)/(b) %6.3f  (a)/(c) %5.2f  [n = %d]" % (
            mode, n, out["edit"]["median_us"], out["edit"]["min_us"], out["edit"]["p90_us"], out["edit"]["call_before_median_us"],
            out["upload"]["median_us"], out["upload"]["min_us"], out["upload"]["p90_us"], out["upload"]["call_before_median_us"],
            out["update"]["median_us"], out["update"]["min_us"], out["update"]["p90_us"], out["update"]["call_before_median_us"],
            out["edit_over_upload"], out["edit_over_update"], out["edit"]["n"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="phahst,at,rd_crystal,rd_form")
    ap.add_argument("--atoms", default="1024,4096")
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--at-reps", type=int, default=6)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    boxes = []
    for mode in [m for m in args.modes.split(",") if m]:
        for n in [int(x) for x in args.atoms.split(",") if x]:
            heavy = mode == "at" and n >= 4096
            boxes.append(box(mode, n, args.at_reps if heavy else args.reps, 2 if heavy else args.warmup))
    say(json.dumps({"reps": args.reps, "warmup": args.warmup, "at_reps": args.at_reps, "boxes": boxes}))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "dense_edits_bench.txt"), "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
