"""GPU tests of sg / dreiding / lj_buffered_14_7 and the Lennard-Jones mixing rules through the C host layer and the
mpmc_hip driver: the reference program's printed energies of tests/golden/rd_forms/, a Monte Carlo chain per form, and the
other ensembles."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rdforms_cases as rc
import rdforms_reference as ref
from mpmc_amd import engine, host

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", "rd_forms")
PRINTED = json.load(open(os.path.join(GOLD, "reference_energies.json")))


def _driver(tmp_path, text, timeout=120):
    (tmp_path / "input").write_text(text)
    r = subprocess.run([host.EXE_PATH, "input"], cwd=str(tmp_path), capture_output=True, text=True, timeout=timeout)
    out = r.stdout + r.stderr
    vals = {m.group(1).strip(): m.group(2) for m in re.finditer(r"OUTPUT: ([a-zA-Z_/ \-]+?) *= *(\S+)", out)}
    return r.returncode, out, vals


@pytest.mark.parametrize("name", sorted(PRINTED))
def test_driver_prints_the_reference_digits(tmp_path, name):
    fx = PRINTED[name]
    shutil.copy(os.path.join(GOLD, fx["pqr"]), str(tmp_path / fx["pqr"]))
    rcode, out, vals = _driver(tmp_path, open(os.path.join(GOLD, name + ".in")).read())
    assert rcode == 0, out
    print(name, vals, fx["printed"], fx["energy_dat"])
    assert vals["potential energy"] == fx["printed"]["potential energy"]
    if "electrostatic energy" in fx["printed"]:
        assert vals["electrostatic energy"] == fx["printed"]["electrostatic energy"]
    else:  # sg: the reference computes (and prints) no electrostatics
        assert float(vals["electrostatic energy"]) == 0.0 and float(vals["polarization energy"]) == 0.0
    # the driver prints 5 decimals, the reference's energy file 6: half a unit of each
    assert abs(float(vals["repulsion/dispersion energy"]) - float(fx["energy_dat"]["rd"])) <= 0.55000001e-5


CHAINS = [("sg", "lb", rc.FH2), ("dreiding", "lb", rc.BASE), ("lj_buffered_14_7", "halgren_mixing", rc.BASE),
          ("lj", "waldmanhagler", rc.FH4)]


@pytest.mark.parametrize("form,mixing,base", CHAINS, ids=[c[0] + "-" + c[1] for c in CHAINS])
def test_nvt_chain_carries_the_energy_of_its_configuration(form, mixing, base):
    """200 steps with a preset seed: no failure, moves both ways, and the energy the chain carries is the from-scratch
    energy of its final configuration"""
    s, f = rc.system("inc320", form, mixing), rc.flags("inc320", base, form, mixing)
    h = host.HostSystem(s, f, seed=20251, move_factor=0.05, rot_factor=0.05)
    h.mc_steps(200)
    assert not h.lib.host_device_error(h.ptr)
    o = h.observables()
    assert o["accept"] + o["reject"] == 200 and o["accept"] > 0 and o["reject"] > 0
    cur = dict(s, pos=h.positions())
    h.close()
    e = engine.Engine(len(s["charge"]))
    e.load_system(cur, f)
    got = e.energy()
    e.close()
    assert got["status"] == 0 and np.isfinite(o["energy"])
    r = ref.rd_terms(cur, f, form, mixing)
    tol = rc.RD_TOL * (float(r["abs_sum"]) + abs(got["es_real"]) + abs(got["es_recip"]) + abs(got["es_self"]))
    print(form, mixing, "chain %.12g fresh %.12g |diff| %.3g tol %.3g" % (o["energy"], got["energy"],
                                                                       abs(o["energy"] - got["energy"]), tol))
    assert abs(o["energy"] - got["energy"]) <= tol and abs(o["rd_energy"] - got["rd_energy"]) <= tol
    assert abs(got["rd_energy"] - float(r["total"])) <= rc.RD_TOL * float(r["abs_sum"])
    if form == "sg":
        assert o["coulombic_energy"] == 0.0 and o["polarization_energy"] == 0.0 and o["energy"] == o["rd_energy"]


ENSEMBLE = ("job_name run\nensemble %s\npreset_seeds 20251\nnumsteps 60\ncorrtime 10\ntemperature 77.0\nmove_factor 0.1\n"
            "rot_factor 0.1\n%s%spqr_input %s\nenergy_output energy.dat\npqr_output out.pqr\npqr_restart restart.pqr\n"
            "traj_output traj.pqr\n")


def _basis_lines(name):
    return "".join(l + "\n" for l in open(os.path.join(GOLD, name + ".in")).read().splitlines() if l.startswith("basis"))


@pytest.mark.parametrize("ensemble,extra,name", [
    ("uvt", "user_fugacities 40.0\ninsert_probability 0.5\nsg on\n", "sg_fh0"),
    ("npt", "pressure 1.0\nvolume_probability 0.3\nvolume_change_factor 0.1\ndreiding on\nhalgren_mixing on\n",
     "dreiding_halgren"),
    ("uvt", "pressure 20.0\ninsert_probability 0.5\nc6_mixing on\nfeynman_hibbs on\nfeynman_hibbs_order 4\n", "lj_c6_fh4"),
])
def test_driver_runs_the_other_ensembles(tmp_path, ensemble, extra, name):
    fx = PRINTED[name]
    shutil.copy(os.path.join(GOLD, fx["pqr"]), str(tmp_path / fx["pqr"]))
    rcode, out, _ = _driver(tmp_path, ENSEMBLE % (ensemble, extra, _basis_lines(name), fx["pqr"]))
    assert rcode == 0, out
    rows = [l.split() for l in (tmp_path / "energy.dat").read_text().splitlines() if not l.startswith("#")]
    assert len(rows) >= 6
    assert all(np.isfinite(float(v)) for row in rows for v in row)
    # the first row is the reference program's energy of the same input
    assert abs(float(rows[0][3]) - float(fx["energy_dat"]["rd"])) <= 1.0000001e-6, (rows[0], fx["energy_dat"])


def test_driver_refuses_by_name(tmp_path):
    shutil.copy(os.path.join(GOLD, "mixed.pqr"), str(tmp_path / "mixed.pqr"))
    text = open(os.path.join(GOLD, "dreiding_lb.in")).read()
    for extra, words in (("waldmanhagler on\n", "waldmanhagler with a negative sigma"),
                         ("sg on\n", "sg with two or more frozen atoms")):
        rcode, out, _ = _driver(tmp_path, text.replace("dreiding on\n", extra))
        assert rcode != 0 and words in out, out
