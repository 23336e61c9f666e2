#!/usr/bin/env python3
"""Fixtures of tests/golden/thole_models/: `ensemble total_energy` inputs for the dipole tensors beside the exponential one
(polar_damp_type linear, off, and exponential + polar_wolf_full), their PQR files and what the reference program printed.

    python tests/golden/make_thole_models.py [path/to/the/reference/program]

Without an argument only the inputs and the PQR files are (re)written.  With one, every input is run once in a scratch
copy and the values of the program's `OUTPUT:` lines and the row of its energy file go into reference_energies.json
(data only; nothing of the program is copied).  The program is the unmodified reference built out of tree (SURVEY.md section 8c has the cmake line).

Systems: `bssp10.pqr` is tests/golden/bssp_small_10.npz (two five-site BSSP H2 in a 22.4567 A box), `spol320.pqr` is
synth.s_pol(320); under `off` too ten Jacobi sweeps converge there (they agree with the direct solve to the printed
digits).  Every number is written by repr(); the charges are in e, as the format has them, so a reader of the PQR -- not
of the arrays -- gets the doubles the program ran on.
"""
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "thole_models")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from mpmc_amd import synth  # noqa: E402

MODELS = {
    "linear_1.662": ["polar_damp_type linear", "polar_damp 1.662"],
    "linear_2.1304": ["polar_damp_type linear", "polar_damp 2.1304"],
    "off": ["polar_damp_type off"],
    "wolf_full": ["polar_damp_type exponential", "polar_damp 2.1304", "polar_wolf_full on", "polar_wolf on"],
}
SOLVERS = {"iter10": ["polar_iterative on", "polar_max_iter 10"], "exact": ["polar_iterative off"]}


def systems():
    return {"bssp10": dict(np.load(os.path.join(HERE, "bssp_small_10.npz"))), "spol320": synth.s_pol(320)}


def pqr_text(s):
    lines = []
    for i in range(len(s["charge"])):
        q = float(s["charge"][i]) / synth.E2REDUCED
        lines.append("ATOM %6d X%-3d MOL %s %5d %r %r %r %r %r %r %r %r" % (
            i + 1, i % 5, "F" if s["frozen"][i] else "M", int(s["molecule"][i]), float(s["pos"][i][0]), float(s["pos"][i][1]),
            float(s["pos"][i][2]), float(s["mass"][i]), q, float(s["alpha"][i]), float(s["epsilon"][i]), float(s["sigma"][i])))
    return "\n".join(lines) + "\nEND\n"


def inputs():
    out = {}
    for sname, s in systems().items():
        for mname, mk in MODELS.items():
            for vname, vk in SOLVERS.items():
                name = "%s_%s_%s" % (sname, mname, vname)
                b = s["basis"]
                text = ["job_name %s" % name, "ensemble total_energy", "temperature 77.0", "polarization on"] + mk + vk
                text += ["basis%d %r %r %r" % (k + 1, float(b[k][0]), float(b[k][1]), float(b[k][2])) for k in range(3)]
                text += ["pqr_input %s.pqr" % sname]
                out[name] = dict(text="\n".join(text) + "\n", pqr=sname + ".pqr", keywords=mk + vk)
    return out


def main():
    os.makedirs(OUT, exist_ok=True)
    for sname, s in systems().items():
        open(os.path.join(OUT, sname + ".pqr"), "w").write(pqr_text(s))
    cases = inputs()
    for name, c in cases.items():
        open(os.path.join(OUT, name + ".in"), "w").write(c["text"])
    if len(sys.argv) < 2:
        return
    prog = os.path.abspath(sys.argv[1])
    result = {}
    for name, c in cases.items():
        with tempfile.TemporaryDirectory() as tmp:
            for f in (name + ".in", c["pqr"]):
                shutil.copy(os.path.join(OUT, f), tmp)
            run = subprocess.run([prog, name + ".in"], cwd=tmp, capture_output=True, text=True)
            printed = {}
            for line in (run.stdout + run.stderr).splitlines():
                m = re.match(r"OUTPUT: (.*?) = (\S+)", line)
                if m:
                    printed[m.group(1).strip()] = m.group(2)
            assert "polarization energy" in printed, (name, run.stdout[-2000:], run.stderr[-2000:])
            rows = [l.split() for l in open(os.path.join(tmp, name + ".energy.dat")).read().splitlines() if l.strip()]
            head = [t.lstrip("#") for t in rows[0]]
            result[name] = dict(keywords=c["keywords"], pqr=c["pqr"], printed=printed, energy_dat=dict(zip(head, rows[1])))
    json.dump(result, open(os.path.join(OUT, "reference_energies.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
