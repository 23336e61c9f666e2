"""The HIP calls of a fixed, seeded tour through the engine's modes, for holding one build's launch sequence against another's.

Run (one build per run, no counters):
    rocprofv3 --hip-trace --kernel-trace --output-format csv -d OUT -- python3 tools/launch_sequence.py [--lib PATH]
then reduce the trace to what must not differ between two builds of the same device code:
    python3 tools/launch_sequence.py --reduce OUT --tag NAME --into profiles/step_phases
Two sequences are compared: the HIP API function names in call order (hipStreamQuery rows dropped: wait_sequence() polls by
elapsed spins) and, per queue in dispatch order, kernel name, grid size and workgroup size.  NAME_api.txt and
NAME_kernels.txt hold, for each, the sha256 of the ordered sequence (one line per call, "\n" behind each) and how often
every distinct line occurs: two builds whose files are equal made the same calls in the same order.  With --full the
sequences themselves are written beside them (NAME_api_full.txt, NAME_kernels_full.txt, runs of equal lines as "N x line"),
to find where two builds part; they run to thousands of lines and are not meant to be kept.

The tour, at 320 atoms: for each mode upload, energy(), two single-molecule moves each followed by energy(),
download_dipoles().  Every energy is printed as a hex float, so two runs can also be compared bit for bit.  At its end the
script prints resident_fallbacks and spec_rank_redos summed over the contexts: a shared device can make the resident launch
give up, and the sequences of such a run are not comparable in that mode.
"""
import argparse
import collections
import csv
import glob
import hashlib
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 320


def molecule_atoms(system, k):
    """(first, count) of the molecule that holds atom k (molecules are contiguous in the synthetic systems)."""
    idx = np.flatnonzero(system["molecule"] == system["molecule"][k])
    assert idx[-1] - idx[0] + 1 == len(idx)
    return int(idx[0]), len(idx)


def tour(engine, name, system, flags, options=(), calls=3, edit=False, order=False):
    eng = engine.Engine(len(system["pos"]) + 16, device=0)
    for opt, value in options:
        eng.set_option(opt, value)
    eng.load_system(system, flags)
    pos = np.array(system["pos"], dtype=np.float64)
    n = len(pos)
    out = [eng.energy()["energy"]]
    if edit:
        first, count = molecule_atoms(system, 0)
        assert eng.remove_molecule(first, count)
        got = eng.insert_molecule(pos[first:first + count] + 0.05,
                                  *[system[k][first:first + count] for k in ("charge", "alpha", "epsilon", "sigma", "mass")])
        assert got == first, got  # (the hole it left)
        pos[first:first + count] += 0.05
        if order:
            eng.set_sweep_order(np.flatnonzero(system["alpha"] != 0.0))
        out.append(eng.energy()["energy"])
    for step in range(1, calls):
        first, count = molecule_atoms(system, (step * (n // 3) + 7) % n)
        pos[first:first + count] += np.array([0.11, -0.07, 0.05]) * step
        eng.update_atoms(first, pos[first:first + count])
        out.append(eng.energy()["energy"])
    if flags.get("polarization") and not flags.get("rd_only"):
        out.append(float(np.sum(eng.dipoles()["mu"])))
    t = eng.timings()
    eng.close()
    print("%-28s %s" % (name, " ".join(float(v).hex() for v in out)), flush=True)
    return t["resident_fallbacks"], t["spec_rank_redos"]


def run(lib):
    from mpmc_amd import engine, synth
    if lib:
        engine.LIB_PATH = os.path.abspath(lib)
    pol = synth.s_pol(N)
    J = dict(synth.FLAGS_POL_JACOBI)
    GS = dict(J, polar_gs=1)
    modes = [
        ("jacobi", pol, J, {}),
        ("jacobi_multi_4", pol, dict(J, polar_max_iter=4), dict(options=[("resident_jacobi", 0)])),
        ("jacobi_multi_5", pol, dict(J, polar_max_iter=5), dict(options=[("resident_jacobi", 0)])),
        ("jacobi_timing_2", pol, J, dict(options=[("timing", 2)])),
        ("jacobi_precision", pol, dict(J, polar_precision=1.0e-3, polar_max_iter=0), {}),
        ("gs_build_fork_2", pol, GS, dict(options=[("gs_build_fork", 2)])),
        ("gs_not_persistent", pol, GS, dict(options=[("persistent_gs", 0)])),
        ("gs_ranked_5_calls", pol, dict(J, polar_gs_ranked=1), dict(calls=5)),
        ("palmo", pol, dict(J, polar_palmo=1), {}),
        ("zodid", pol, dict(J, polar_zodid=1), {}),
        ("production_wolf", pol, dict(synth.FLAGS_POL_PRODUCTION), {}),
        ("polar_ewald", pol, dict(J, polar_ewald=1), {}),
        ("exact_dipoles", pol, dict(J, polar_iterative=0), {}),
        ("rd_only", synth.s_lj(N), dict(synth.FLAGS_LJ), {}),
        ("electrostatics", synth.s_es(N), dict(synth.FLAGS_ES), {}),
        ("phahst", synth.s_phahst(N), dict(synth.FLAGS_PHAHST), {}),
        ("axilrod_teller", synth.s_at(N), dict(synth.FLAGS_AT), {}),
        ("jacobi_one_stream", pol, J, dict(options=[("overlap_streams", 0)])),
        ("jacobi_remove_insert", pol, J, dict(edit=True)),
        ("gs_remove_insert_order", pol, GS, dict(edit=True, order=True)),
        ("step_graph_6_steps", pol, J, dict(options=[("step_graph", 1)], calls=7)),
    ]
    fallbacks = redos = 0
    for name, system, flags, kw in modes:
        f, r = tour(engine, name, system, flags, **kw)
        fallbacks += f
        redos += r
    print("resident_fallbacks %d spec_rank_redos %d" % (fallbacks, redos), flush=True)


def run_lengths(lines):
    """Consecutive equal lines as one, "N x line"."""
    out = []
    for line in lines:
        if out and out[-1][1] == line:
            out[-1][0] += 1
        else:
            out.append([1, line])
    return ["%d x %s" % (k, line) if k > 1 else line for k, line in out]


def reduce_trace(d, tag, into, full=False):
    def rows(pattern):
        out = []
        for f in sorted(glob.glob(os.path.join(d, "**", pattern), recursive=True)):
            out += list(csv.DictReader(open(f)))
        if not out:
            sys.exit("no %s under %s" % (pattern, d))
        return out

    api = sorted(rows("*hip_api_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Function"] for r in api if r["Function"] != "hipStreamQuery"]
    kern = rows("*kernel_trace.csv")
    key = "Dispatch_Id" if "Dispatch_Id" in kern[0] else "Start_Timestamp"
    kern.sort(key=lambda r: int(r[key]))
    queues = {}  # numbered in order of first use: the runtime's ids are not the same from run to run
    for r in kern:
        q = queues.setdefault((r.get("Agent_Id"), r.get("Queue_Id")), [])
        name = re.sub(r"\s*\[clone .*", "", r["Kernel_Name"]).replace("mpmc::", "")
        q.append("%s grid %s,%s,%s block %s,%s,%s" % ((name,) + tuple(r[a + "_" + x] for a in ("Grid_Size", "Workgroup_Size")
                                                                      for x in "XYZ")))
    os.makedirs(into, exist_ok=True)

    def digest(seq):
        return hashlib.sha256("".join(line + "\n" for line in seq).encode()).hexdigest()

    def table(seq):
        count = collections.Counter(seq)
        return ["%7d  %s" % (count[line], line) for line in sorted(count)]

    with open(os.path.join(into, tag + "_api.txt"), "w") as f:
        f.write("%d HIP API calls, sha256 of the sequence %s\n" % (len(names), digest(names)))
        f.write("\n".join(table(names)) + "\n")
    with open(os.path.join(into, tag + "_kernels.txt"), "w") as f:
        for k, q in enumerate(queues.values()):
            f.write("queue %d: %d dispatches, sha256 of the sequence %s\n" % (k, len(q), digest(q)))
        f.write("\n".join(table([line for q in queues.values() for line in q])) + "\n")
    if full:
        with open(os.path.join(into, tag + "_api_full.txt"), "w") as f:
            f.write("\n".join(run_lengths(names)) + "\n")
        with open(os.path.join(into, tag + "_kernels_full.txt"), "w") as f:
            for k, q in enumerate(queues.values()):
                f.write("queue %d: %d dispatches\n" % (k, len(q)))
                f.write("\n".join(run_lengths(q)) + "\n")
    print("%s: %d API calls, %d dispatches on %d queues" % (tag, len(names), len(kern), len(queues)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="the engine library to load instead of the tree's own build")
    ap.add_argument("--reduce", metavar="DIR", help="reduce the rocprofv3 csv trace under DIR instead of running the tour")
    ap.add_argument("--tag", default="trace")
    ap.add_argument("--into", default=".")
    ap.add_argument("--full", action="store_true", help="with --reduce: also write the sequences themselves")
    a = ap.parse_args()
    if a.reduce:
        reduce_trace(a.reduce, a.tag, a.into, a.full)
    else:
        run(a.lib)
