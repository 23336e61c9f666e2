#!/usr/bin/env python3
"""Steps per second of a grand-canonical chain under the PHAHST potential with polarization, through the C host layer, on
the 4096-atom PCN-61 box of bench.py (tests/golden/pcn61_bssp_4096.npz, its flags and its uvt keywords: insert_probability
0.666, fugacity 70).  The file carries Lennard-Jones parameters; here every site with a non-zero epsilon gets the exponent
b = 3.2 / A and the range rho = 2.9 A in their place and C6 = 9, C8 = 180, C10 = 4500 atomic units: round numbers of the
magnitude of synth.PHAHST_SITES, a timing workload and not a parameter set.

    python tools/dense_uvt_bench.py [--tree DIR] [--steps 1500] [--warmup 100] [--seed 1234]

--tree DIR: the checkout whose mpmc_amd is measured (default: this one), so that two builds can be run alternately, one
process each, by a caller.  Prints one JSON line: steps/s over --steps steps after --warmup, the atom counts seen, and --
where the host layer has them -- the counts of full uploads, edit calls and molecules edited."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=HERE)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--seed", type=int, default=1234)
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    from mpmc_amd import host, synth

    s = dict(np.load(os.path.join(tree, "tests", "golden", "pcn61_bssp_4096.npz")))
    on = s["epsilon"] != 0.0
    s.update(epsilon=np.where(on, 3.2, 0.0), sigma=np.where(on, 2.9, 0.0), c6=np.where(on, 9.0, 0.0),
             c8=np.where(on, 180.0, 0.0), c10=np.where(on, 4500.0, 0.0))
    flags = dict(synth.FLAGS_PHAHST, polar_max_iter=4, pbc_cutoff=8.0, rd_lrc=1)
    h = host.HostSystem(s, flags, seed=args.seed,
                        extra={"ensemble": "uvt", "insert_probability": 0.666, "pressure": 70.0})
    n0 = h.natoms()
    h.mc_steps(args.warmup)
    seen = {h.natoms()}
    t0 = time.perf_counter()
    done = 0
    while done < args.steps:  # in blocks, to see N move
        k = min(100, args.steps - done)
        h.mc_steps(k)
        done += k
        seen.add(h.natoms())
    dt = time.perf_counter() - t0
    o = h.observables()
    out = dict(tree=tree, steps=args.steps, warmup=args.warmup, steps_per_s=args.steps / dt, atoms_at_start=n0,
               atoms_seen=[min(seen), max(seen)], accepted=o["accept"], rejected=o["reject"], energy=o["energy"])
    if hasattr(h, "sync_counts"):
        out["sync_counts"] = h.sync_counts()
    h.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
