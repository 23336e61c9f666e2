#!/usr/bin/env python3
"""What the coupled-dipole many-body van der Waals term (polarvdw) costs on one device, in one session:

  * the eigenvalue-sum solve (build, Householder tridiagonalisation, bisection, sum) of a box of one-site molecules at
    liquid density, at the site counts of --sites: the engine's own events around the solve's launches (option
    "timing" = 2, class other_ms, in a call after a one-atom move, when nothing else of that class runs) and the wall time
    of that energy() call; with the launch count 3 (n - 2) + 4 and the bytes the unblocked reduction moves
    (sum over columns of one read of the trailing block by the matrix-vector product and one read + one write by the
    rank-2 update, 8 B each) this gives microseconds per launch and bytes per second, the two figures that say whether the
    reduction is launch-bound or HBM-bound at a size;
  * NVT steps/s of a short chain at --chain-sites through the C host layer (polarization, Ewald, autoreject: everything a
    production step runs);
  * numpy.linalg.eigvalsh of the same matrix (fp64) on this host with one BLAS thread, up to --cpu-max-sites, as the CPU
    line: what the reference's dsyev call costs per step.

    python tools/vdw_bench.py [--sites 256,1070,4096] [--chain-sites 1070] [--steps 20] [--cpu-max-sites 1070]

Prints one line per measurement and one JSON summary line; --out DIR also writes both to DIR/vdw_bench.txt."""
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

SOLVE = dict(temperature=150.0, polar_damp=2.1304, rd_lrc=1, polarvdw=1)  # no polarization: the term alone
CHAIN = dict(temperature=150.0, polarization=1, polar_damp=2.1304, polar_max_iter=4, rd_lrc=1, polarvdw=1,
             cavity_autoreject_absolute=1, cavity_autoreject_scale=1.5)
ALPHA, OMEGA, DAMP = 1.1, 0.62, 2.1304
_lines = []


def say(text):
    print(text, flush=True)
    _lines.append(text)


def box(n, seed=1):
    """n one-site molecules on a jittered cubic lattice, spacing 3.7 A"""
    rng = np.random.default_rng(seed + n)
    m = int(np.ceil(n ** (1.0 / 3.0) - 1e-9))
    L = 3.7 * m
    idx = rng.permutation(m ** 3)[:n]
    pos = (np.stack([idx // (m * m), (idx // m) % m, idx % m], axis=1) + 0.5) * 3.7 + rng.uniform(-0.3, 0.3, (n, 3))
    return dict(pos=pos, charge=np.zeros(n), alpha=np.full(n, ALPHA), epsilon=np.full(n, 35.0), sigma=np.full(n, 3.1),
                mass=np.full(n, 16.0), molecule=np.arange(1, n + 1, dtype=np.int32), frozen=np.zeros(n, dtype=np.int32),
                basis=np.eye(3) * L, omega=np.full(n, OMEGA), mol_type=np.zeros(n, dtype=np.int32))


def matrix(s):
    """C = K A K in fp64 (cubic cell), for the CPU line"""
    pos, n = s["pos"], len(s["pos"])
    L = s["basis"][0, 0]
    k2 = ALPHA * OMEGA * OMEGA
    Cm = np.zeros((3 * n, 3 * n))
    for i in range(n):
        d = pos[i] - pos
        d -= L * np.rint(d / L)
        r = np.sqrt((d * d).sum(axis=1))
        r[i] = 1.0
        ex = np.exp(-DAMP * r)
        d1 = 1.0 - ex * (0.5 * DAMP ** 2 * r * r + DAMP * r + 1.0)
        d2 = d1 - ex * (DAMP ** 3 * r ** 3 / 6.0)
        c3, c5 = d1 / r ** 3, d2 / r ** 5
        t = -3.0 * d[:, :, None] * d[:, None, :] * c5[:, None, None] + np.eye(3)[None] * c3[:, None, None]
        t[i] = np.eye(3) / ALPHA
        Cm[3 * i:3 * i + 3] = (k2 * t).transpose(1, 0, 2).reshape(3, 3 * n)
    return Cm


def solve_times(n, reps):
    from mpmc_amd import engine

    s = box(n)
    e = engine.Engine(n)
    e.set_option("timing", 2)
    e.load_system(s, SOLVE)
    t0 = time.perf_counter()
    e.energy()
    first = time.perf_counter() - t0
    ev, wall = [], []
    for rep in range(reps):
        e.update_atoms(0, s["pos"][0:1] + 0.01 * (rep + 1))
        t0 = time.perf_counter()
        e.energy()
        wall.append(1e3 * (time.perf_counter() - t0))
        ev.append(e.timings()["other_ms"])
    terms = e.vdw_terms()
    e.close()
    dim = 3 * n
    launches = 3 * (dim - 2) + 4
    nbytes = 8.0 * 3.0 * sum(float(m) * m for m in range(2, dim))
    ms = sorted(ev)[len(ev) // 2]
    out = dict(sites=n, matrix=dim, launches=launches, solve_ms=ms, solve_ms_all=ev, call_wall_ms=sorted(wall)[len(wall) // 2],
               first_call_s=first, us_per_launch=1e3 * ms / launches, bytes=nbytes, tb_per_s=nbytes / (1e-3 * ms) / 1e12,
               e_total=terms["e_total"])
    say("solve  %5d sites (n = %5d): %10.3f ms by events, %10.3f ms wall per call; %6d launches = %6.2f us each; "
        "%.3g B moved = %5.2f TB/s" % (n, dim, ms, out["call_wall_ms"], launches, out["us_per_launch"], nbytes, out["tb_per_s"]))
    return out, s


def cpu_time(s):
    Cm = matrix(s)
    t0 = time.perf_counter()
    w = np.linalg.eigvalsh(Cm)
    dt = time.perf_counter() - t0
    e_total = 4.13412763705e16 * 3.81911146e-12 * np.sqrt(np.clip(w, 0.0, None)).sum()
    say("cpu    %5d sites (n = %5d): %10.3f ms numpy.linalg.eigvalsh, one thread" % (len(s["pos"]), Cm.shape[0], 1e3 * dt))
    return dict(sites=len(s["pos"]), eigvalsh_ms=1e3 * dt, e_total=float(e_total))


def chain(n, steps, warmup):
    from mpmc_amd import host

    h = host.HostSystem(box(n), CHAIN, seed=5, move_factor=0.02, rot_factor=0.02)
    h.mc_steps(warmup)
    t0 = time.perf_counter()
    h.mc_steps(steps)
    dt = time.perf_counter() - t0
    o, v = h.observables(), h.vdw()
    h.close()
    say("chain  %5d sites: %8.2f NVT steps/s over %d steps (%d accepted, %d rejected, %d autorejects)" %
        (n, steps / dt, steps, o["accept"], o["reject"], v["count_autorejects"]))
    return dict(sites=n, steps=steps, steps_per_s=steps / dt, accept=o["accept"], reject=o["reject"],
                autorejects=v["count_autorejects"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", default="256,1070,4096")
    ap.add_argument("--chain-sites", type=int, default=1070)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu-max-sites", type=int, default=1070)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "coupled_dipole_vdw"))
    args = ap.parse_args()
    out = {"solve": [], "cpu": []}
    for n in [int(x) for x in args.sites.split(",") if x]:
        r, s = solve_times(n, args.reps)
        out["solve"].append(r)
        if n <= args.cpu_max_sites:
            c = cpu_time(s)
            c["relative_difference"] = abs(c["e_total"] - r["e_total"]) / abs(c["e_total"])
            out["cpu"].append(c)
    if args.chain_sites > 0:
        out["chain"] = chain(args.chain_sites, args.steps, args.warmup)
    say(json.dumps(out))
    if args.out:
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "vdw_bench.txt"), "w") as f:
            f.write("\n".join(_lines) + "\n")


if __name__ == "__main__":
    main()
