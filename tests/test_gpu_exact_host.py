"""The exact Thole dipoles (polar_iterative off) through the C host layer and the driver: the 10-atom reference-style input
of tests/data/bssp_small as a single point, as an NVT chain whose every accepted energy is the energy of its
configuration, and `polarizability_tensor on` for one five-site molecule."""
import os
import re
import subprocess

import numpy as np
import pytest

from mpmc_amd import engine, host, pqr
from test_reference_inputs import DATA, keyword_file

pytestmark = pytest.mark.gpu

BASIS = np.diag([22.4567] * 3)
FLAGS = dict(temperature=77.0, polarization=1, polar_damp=2.1304, polar_iterative=0, feynman_hibbs=1, feynman_hibbs_order=4)
TERMS = ("energy", "rd_energy", "coulombic_energy", "polarization_energy")


def _input(tmp_path, ensemble, extra="", pqr_text=None):
    """tests/data/bssp_small/input with polar_iterative off and another ensemble; returns the keyword file's path"""
    d = keyword_file(tmp_path, "bssp_small")
    lines = []
    for line in open(os.path.join(d, "input")).read().splitlines():
        key = line.split()[0] if line.split() else ""
        if key == "polar_iterative":
            line = "polar_iterative off"
        elif key == "ensemble":
            line = "ensemble        " + ensemble
        elif key == "pqr_input" and pqr_text is not None:
            with open(os.path.join(d, "one.pqr"), "w") as f:
                f.write(pqr_text)
            line = "pqr_input       " + os.path.join(d, "one.pqr")
        lines.append(line)
    path = os.path.join(d, "input")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n" + extra)
    return path


def _fresh(s):
    e = engine.Engine(len(s["charge"]))
    try:
        e.load_system(s, FLAGS)
        return e.energy()
    finally:
        e.close()


def test_total_energy_is_the_engines_value_for_the_same_atoms(tmp_path):
    path = _input(tmp_path, "total_energy")
    s = pqr.read_pqr(os.path.join(DATA, "bssp_small", "small.initial.pqr"), BASIS)
    want = _fresh(s)
    assert want["polar_iterations"] == 0 and want["iter_success"] == 0 and want["polarization_energy"] < 0.0
    lib = host.load()
    p = lib.setup_system(path.encode())
    assert p
    try:
        assert lib.host_unsupported(p) is None
        e = lib.energy(p)
        obs = np.zeros(8)
        lib.host_get_observables(p, obs.ctypes.data)
    finally:
        lib.free_system(p)
    assert obs[3] == want["polarization_energy"]
    assert e == obs[0] and obs[5] == 0.0  # no iteration ran
    # not what the iterative solver of the original input gives: ten Jacobi sweeps stop a few 1e-7 short
    it = engine.Engine(len(s["charge"]))
    it.load_system(s, dict(FLAGS, polar_iterative=1, polar_max_iter=10))
    jac = it.energy()["polarization_energy"]
    it.close()
    print("exact %.12g, ten Jacobi sweeps %.12g" % (obs[3], jac))
    assert jac != obs[3] and abs(jac - obs[3]) <= 1e-3 * abs(obs[3])
    # ... and the driver prints it
    r = subprocess.run([host.EXE_PATH, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "INPUT: Matrix polarization activated" in r.stdout
    assert "OUTPUT: polarization energy = %.5f K" % want["polarization_energy"] in r.stdout


def test_nvt_chain_carries_the_energy_of_its_configuration():
    s = pqr.read_pqr(os.path.join(DATA, "bssp_small", "small.initial.pqr"), BASIS)
    h = host.HostSystem(s, FLAGS, seed=12345, move_factor=0.01, rot_factor=0.01)
    try:
        accepted = 0
        for step in range(20):
            h.mc_steps(1)
            obs = h.observables()
            if obs["accept"] == accepted:
                continue
            accepted = obs["accept"]
            want = _fresh(h.system(BASIS))
            for k in TERMS:
                assert obs[k] == want[k], (step, k, obs[k], want[k])
            assert obs["polar_iterations"] == 0
        assert accepted >= 3 and obs["accept"] + obs["reject"] == 20
    finally:
        h.close()


def test_driver_prints_the_polarizability_tensor_and_leaves(tmp_path):
    one = "".join(open(os.path.join(DATA, "bssp_small", "small.initial.pqr")).readlines()[:5]) + "END\n"
    path = _input(tmp_path, "nvt", "polarizability_tensor on\n", pqr_text=one)
    s = pqr.read_pqr(os.path.join(os.path.dirname(path), "one.pqr"), BASIS)
    assert len(s["charge"]) == 5
    e = engine.Engine(5)
    try:
        e.load_system(s, FLAGS)
        e.energy()
        C = e.polarizability_tensor()
    finally:
        e.close()
    r = subprocess.run([host.EXE_PATH, path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr  # the reference's die(0)
    assert "INPUT: Polarizability tensor calculation activated" in r.stdout
    out = r.stdout[r.stdout.index("POLARIZATION: polarizability tensor (A^3):"):]
    block = out.splitlines()
    rule = "#" * 26
    assert block[1] == rule and block[5] == rule
    for p in range(3):
        assert block[2 + p] == "".join("%.4f " % C[p, q] for q in range(3))
    assert block[6] == "isotropic = %.4f" % (np.trace(C) / 3.0)
    assert block[7] == "XX/ZZ = %.4f" % (C[0, 0] / C[2, 2])
    assert len(block) == 8  # the run ends with the block: no step was taken, no matrix dump in front of it
    assert not re.search(r"OUTPUT: .* sec/step", r.stdout)
    # a hydrogen molecule: the tensor is that of three sites on a line (to the file's three decimals), larger along it
    w = np.linalg.eigvalsh(0.5 * (C + C.T))
    assert w[0] > 0.0 and abs(w[0] - w[1]) <= 1e-6 * w[2] and w[2] > w[1] + 1e-4
