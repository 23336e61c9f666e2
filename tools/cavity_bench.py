#!/usr/bin/env python3
"""What the cavity grid of cavity_bias costs, in one session, on the 4096-atom PCN-61 fixture (2016 framework atoms, 416
H2 molecules, cubic cell of 42.796 A) at cavity_radius 2.5 A and cavity_grid 10, 20, 32:

  * one mpmc_hip_cavity_update() -- one molecule's edit (5 points out, 5 in), the ordered list of the open points and
    (int)(0.1 V) = 7838 darts, the copy of the darts included: wall time of the call, which waits for its record;
  * one mpmc_hip_cavity_bin() of all 4096 wrapped positions (wall time; the call waits for the device);
  * the same update -- occupancy over all atoms, open count, darts against every point -- in a single-core C restatement
    (tools/cavity_cpu.c, gcc -O2) on this host, with its counts compared with the device's;
  * steps/s of a grand-canonical chain through the C host layer with cavity_bias on (cavity_grid 20) and off.

    python tools/cavity_bench.py [--grids 10,20,32] [--reps 200] [--steps 300] [--warmup 30]

Prints one line per measurement and one JSON summary line; --out DIR also writes both to DIR/cavity_bench.txt."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RADIUS = 2.5
FLAGS = dict(temperature=77.0, polarization=1, polar_damp=2.1304, polar_max_iter=4, pbc_cutoff=8.0, feynman_hibbs=1,
             feynman_hibbs_order=4)
_lines = []


def say(text):
    print(text, flush=True)
    _lines.append(text)


def fixture():
    s = dict(np.load(os.path.join(ROOT, "tests", "golden", "pcn61_bssp_4096.npz")))
    L = s["basis"][0, 0]
    pos = np.array(s["pos"])
    wrapped = pos.copy()
    for m in np.unique(s["molecule"]):  # wrapall(): movable molecules by the lattice vector of their centre of mass
        sel = s["molecule"] == m
        if s["frozen"][sel][0]:
            continue
        com = (s["mass"][sel, None] * pos[sel]).sum(axis=0) / s["mass"][sel].sum()
        wrapped[sel] -= L * np.rint(com / L)
    return s, wrapped


def stats(us):
    us = np.sort(np.asarray(us))
    return dict(median_us=float(us[len(us) // 2]), min_us=float(us[0]), p90_us=float(us[int(0.9 * len(us))]), n=len(us))


def cpu_library():
    d = tempfile.mkdtemp(prefix="cavity_cpu")
    so = os.path.join(d, "cavity_cpu.so")
    subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "cavity_cpu.c"), "-lm"])
    lib = C.CDLL(so)
    lib.cavity_cpu_update.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_void_p,
                                      C.c_void_p]
    return lib


def grid_times(s, wrapped, G, reps, cpu):
    from mpmc_amd import engine

    rng = np.random.default_rng(G)
    L = s["basis"][0, 0]
    n_darts = int(L ** 3 * 0.1)
    darts = np.ascontiguousarray((rng.random((n_darts, 3)) - 0.5) * L)
    e = engine.Engine(len(wrapped))
    e.set_box(s["basis"], 8.0)
    e.set_cavity_grid(G, RADIUS)
    cols = [np.ascontiguousarray(wrapped[:, k]) for k in range(3)]
    lib, ctx = e.lib, e.ctx
    bins = []
    for _ in range(max(5, reps // 10)):
        t0 = time.perf_counter()
        rc = lib.mpmc_hip_cavity_bin(ctx, len(wrapped), *[c.ctypes.data for c in cols])
        bins.append(1e6 * (time.perf_counter() - t0))
        assert rc == 0
    movable = np.flatnonzero(s["frozen"] == 0)
    first = int(movable[0])
    mol = np.flatnonzero(s["molecule"] == s["molecule"][first])
    here = np.ascontiguousarray(wrapped[mol])
    there = np.ascontiguousarray(here + 0.3)
    n_open, hits = C.c_int(), C.c_int()
    upd = []
    for rep in range(reps + 10):
        a, b = (here, there) if rep % 2 == 0 else (there, here)  # the molecule steps to and fro
        t0 = time.perf_counter()
        rc = lib.mpmc_hip_cavity_update(ctx, len(mol), a.ctypes.data, len(mol), b.ctypes.data, n_darts, darts.ctypes.data,
                                        C.byref(n_open), C.byref(hits))
        dt = 1e6 * (time.perf_counter() - t0)
        assert rc == 0
        if rep >= 10:
            upd.append(dt)
    picks = []
    for rep in range(reps):
        t0 = time.perf_counter()
        e.cavity_point(rep % max(1, n_open.value))
        picks.append(1e6 * (time.perf_counter() - t0))
    # the configuration is the starting one again (an even number of steps): compare with the CPU restatement
    occ_dev, pos_dev = e.cavity_grid()
    e.close()
    occ = np.zeros(G ** 3, dtype=np.int32)
    o = C.c_int()
    flat = np.ascontiguousarray(wrapped)
    t0 = time.perf_counter()
    h = cpu.cavity_cpu_update(G ** 3, pos_dev.ctypes.data, len(flat), flat.ctypes.data, n_darts, darts.ctypes.data, RADIUS,
                              occ.ctypes.data, C.byref(o))
    cpu_ms = 1e3 * (time.perf_counter() - t0)
    same = bool(np.array_equal(occ, occ_dev) and o.value == n_open.value and h == hits.value)
    out = dict(grid=G, points=G ** 3, atoms=len(flat), darts=n_darts, open=n_open.value, hits=hits.value,
               update=stats(upd), bin=stats(bins), point=stats(picks), cpu_ms=cpu_ms, cpu_counts_equal=same)
    say("grid %2d (%5d points, %4d open, %4d of %d darts hit): update %7.1f us (min %7.1f, p90 %7.1f; n = %d), full bin "
        "%7.1f us, cavity_point %5.1f us; one core: %8.1f ms (counts equal: %s)" %
        (G, G ** 3, n_open.value, hits.value, n_darts, out["update"]["median_us"], out["update"]["min_us"],
         out["update"]["p90_us"], len(upd), out["bin"]["median_us"], out["point"]["median_us"], cpu_ms, same))
    return out


def chain(s, on, steps, warmup, G=20):
    from mpmc_amd import host

    extra = {"ensemble": "uvt", "insert_probability": 0.3, "pressure": 10.0}
    if on:
        extra.update(cavity_bias="on", cavity_grid=G, cavity_radius=RADIUS)
    h = host.HostSystem(s, FLAGS, seed=7, move_factor=0.02, rot_factor=0.02, extra=extra)
    h.mc_steps(warmup)
    t0 = time.perf_counter()
    h.mc_steps(steps)
    dt = time.perf_counter() - t0
    o = h.observables()
    n = h.natoms()
    h.close()
    say("chain cavity_bias %-3s: %8.1f uvt steps/s over %d steps (%d accepted, %d rejected, %d atoms at the end)" %
        ("on" if on else "off", steps / dt, steps, o["accept"], o["reject"], n))
    return dict(cavity_bias=bool(on), grid=G if on else 0, steps=steps, steps_per_s=steps / dt, accept=o["accept"],
                reject=o["reject"], natoms=n)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", default="10,20,32")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cavity_bias"))
    args = ap.parse_args()
    s, wrapped = fixture()
    cpu = cpu_library()
    out = {"radius": RADIUS, "grids": [grid_times(s, wrapped, int(g), args.reps, cpu) for g in args.grids.split(",") if g]}
    if args.steps > 0:
        out["chain"] = [chain(s, on, args.steps, args.warmup) for on in (0, 1, 0, 1)]
    say(json.dumps(out))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "cavity_bench.txt"), "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
