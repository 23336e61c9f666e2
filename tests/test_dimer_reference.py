"""CPU checks of the dimer scans: closed forms of tests/dimer_reference.py; the loop-bound restatement against the grid
sizes the reference program ran; the longdouble model against the stored lines of every fixture of tests/golden/surf/; the
new keywords of the host layer's parser; and every refusal of `ensemble surf`, by name."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import dimer_cases as dc
import dimer_reference as dr
import surf_fixtures as sf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "mpmc_amd", "host", "mpmc_hip")
HOSTLIB = os.path.join(ROOT, "mpmc_amd", "host", "libmpmc_host.so")


def atom(x, charge=0.0, alpha=0.0, epsilon=0.0, sigma=0.0, mass=1.0):
    return dict(pos=np.array([[x, 0.0, 0.0]]), charge=np.array([charge]), alpha=np.array([alpha]),
                epsilon=np.array([epsilon]), sigma=np.array([sigma]), mass=np.array([mass]))


# ---------------------------------------------------------------------------------------------- closed forms
def test_two_charges():
    o = dr.energies(atom(0.3, charge=2.0), atom(-1.0, charge=-3.0), [4.0, 0.4, 1.0, 2.0, 0.1, 0.2, 0.3], {})
    assert abs(float(o["es"]) + 6.0 / 4.0) < 1e-18 and o["rd"] == 0 and o["polar"] == 0


def test_two_lennard_jones_atoms_at_the_minimum():
    sigma, eps = 3.4, 120.0
    r = 2.0 ** (1.0 / 6.0) * sigma
    o = dr.energies(atom(0.0, epsilon=eps, sigma=sigma), atom(0.0, epsilon=eps, sigma=sigma), [r, 0, 0, 0, 0, 0, 0], {})
    assert abs(float(o["rd"]) + eps) < 1e-13 * eps and o["es"] == 0


def test_two_polarizable_atoms_converged():
    """a charge polarizing a neutral polarizable atom, undamped: U = -1/2 alpha q^2 / r^4"""
    q, alpha, r = 50.0, 1.5, 5.0
    flags = dict(polar_damp_type="off", polar_damp=0.0, polar_max_iter=3)
    o = dr.energies(atom(0.0, charge=q), atom(0.0, charge=1e-300, alpha=alpha), [r, 0, 0, 0, 0, 0, 0], flags)
    assert abs(float(o["polar"]) + 0.5 * alpha * q * q / r ** 4) < 1e-15 * alpha * q * q


def test_rotation_identity_and_reverse():
    assert np.array_equal(dr.euler_matrix(0.0, 0.0, 0.0), np.eye(3))
    assert np.array_equal(dr.quaternion_matrix(0.0, 0.0, 0.0), np.eye(3))
    a, b, g = 0.7, 1.9, 4.2
    fwd, back = dr.euler_matrix(a, b, g), dr.euler_matrix(-g, -b, -a)  # the reference's reverse_flag (surface.c:87-96)
    assert np.max(np.abs(back @ fwd - np.eye(3))) < 4e-16
    for R in (fwd, dr.quaternion_matrix(40.0, 70.0, 200.0)):
        assert np.max(np.abs(R @ R.T - np.eye(3))) < 4e-16 and abs(np.linalg.det(R) - 1.0) < 4e-16


def test_placement_keeps_the_molecule_rigid():
    m = dc.molecule(16, 3)
    pos = dr.sites(m, m, [6.0, 0.3, 1.0, 2.0, 4.0, 0.5, 6.0])
    body = dr.body_frame(m)
    for half in (pos[:16], pos[16:]):
        d0 = np.linalg.norm(body[:, None] - body[None, :], axis=-1)
        assert np.max(np.abs(np.linalg.norm(half[:, None] - half[None, :], axis=-1) - d0)) < 1e-14


def test_fixed_order_mean_small_cases():
    assert dr.fixed_order_mean([3.5]) == 3.5
    v = np.arange(1.0, 1001.0)
    assert dr.fixed_order_mean(v) == 500.5
    rng = np.random.default_rng(5)
    w = rng.normal(size=70000)
    assert abs(dr.fixed_order_mean(w) - float(np.sum(w.astype(dr.LD)) / len(w))) < 1e-15


# ---------------------------------------------------------------------------------------------- the fixtures
def test_fixture_set_is_complete():
    assert len(sf.names()) == 12
    for name in sf.names():
        lines = sf.reference_lines(name)
        assert 3 <= len(lines) <= 5, name
        for f in ("input", "dimer.pqr", "reference.out"):
            assert os.path.getsize(os.path.join(sf.GOLD, name, f)) < 4096


def test_loop_bounds_give_the_grid_sizes_the_reference_ran():
    """38 416 = 196^2 dimers per separation at surf_ang 1.0; the separations the reference printed are the ones the
    double-precision loop visits (3.2 + 4 * 0.4 > 4.8: the last point of that scan is not run)"""
    assert [len(x) for x in dr.angle_lists(1.0)] == [7, 4, 7, 7, 4, 7] and 7 * 4 * 7 == 196 and 196 ** 2 == 38416
    for name in sf.names():
        cfg = sf.read_input(name)
        rs = dr.scan_values(cfg["surf_min"], cfg["surf_max"], cfg["surf_inc"])
        assert ["%.5f" % r for r in rs] == [l.split()[0] for l in sf.reference_lines(name)], name
    assert len(sf.reference_lines("ar_ar_phahst")) == 4


@pytest.mark.parametrize("name", sf.names())
def test_longdouble_model_reproduces_the_reference_lines(name):
    """every separation of the cheap cases; the first separation of the isotropic polarizable ones (3 s each; the fixture
    maker holds all of them)"""
    cfg = sf.read_input(name)
    first_only = bool(cfg.get("polarization")) and not cfg.get("surf_preserve")
    got = sf.model_lines(name, first_only)
    want = sf.reference_lines(name)[:len(got)]
    exits, total = sf.compare_lines(want, got)
    assert exits == 0, (name, want, got)  # (the maker's cap is 1 in 50 over the set; as stored, none differs)


# ---------------------------------------------------------------------------------------------- parser and refusals
@pytest.fixture(scope="module")
def driver():
    import __graft_entry__ as g

    if not (os.path.exists(DRIVER) and os.path.exists(HOSTLIB)):
        g.build()
    return DRIVER


def run_input(driver, tmp_path, lines, pqr=None):
    (tmp_path / "dimer.pqr").write_text(pqr or open(os.path.join(sf.GOLD, "n2_total", "dimer.pqr")).read())
    (tmp_path / "input").write_text("\n".join(["job_name t", "ensemble surf", "pqr_input dimer.pqr"] + lines) + "\n")
    return subprocess.run([driver, str(tmp_path / "input")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def test_new_keywords_parse(driver):
    lib = C.CDLL(HOSTLIB)
    lib.surface_loop_count.restype = C.c_int
    lib.surface_loop_count.argtypes = [C.c_double, C.c_double]
    for top, step in ((2.0 * math.pi, 1.0), (math.pi, 1.0), (2.0 * math.pi, math.pi / 6), (math.pi, math.pi / 12)):
        assert lib.surface_loop_count(top, step) == len(dr.loop_values(top, step))
    lib.read_config.restype = C.c_void_p
    for name in sf.names():
        assert lib.read_config(os.path.join(sf.GOLD, name, "input").encode()), name


POLAR = ["polarization on", "polar_damp 2.1304", "polar_damp_type exponential", "polar_iterative on"]
BASE = ["surf_min 3.0", "surf_max 4.0", "surf_inc 0.5", "surf_ang 1.0"]
REFUSALS = [
    (["surf_virial on"], "surf_virial"),
    (["surf_output traj.pqr"], "surf_output"),
    (["surf_print_level 3"], "surf_print_level"),
    (["read_pqr_box on"], "read_pqr_box"),
    (POLAR + ["polar_wolf on"], "polar_wolf"),
    (POLAR + ["polar_wolf_full on"], "polar_wolf_full"),
    (POLAR + ["polar_ewald on"], "polar_ewald"),
    (["polarization on", "polar_damp 2.1304", "polar_damp_type exponential", "polar_iterative off"], "polar_iterative off"),
    (POLAR + ["polar_sor on"], "polar_sor"),
    (POLAR + ["polar_esor on"], "polar_esor"),
    (POLAR + ["polar_zodid on"], "polar_zodid"),
    (POLAR + ["polar_rrms on"], "polar_rrms"),
    (["polarvdw on", "polar_damp 2.1304", "polar_damp_type exponential", "cavity_autoreject_absolute on",
      "cavity_autoreject_scale 1.0"], "polarvdw"),
    (["cdvdw_exp_repulsion on"], "cdvdw_"),
    (["sg on"], "sg"),
    (["dreiding on"], "dreiding"),
    (["lj_buffered_14_7 on"], "lj_buffered_14_7"),
    (["axilrod_teller on"], "axilrod_teller"),
]


@pytest.mark.parametrize("lines,word", REFUSALS, ids=[w for _, w in REFUSALS])
def test_refusals_by_name(driver, tmp_path, lines, word):
    res = run_input(driver, tmp_path, BASE + lines)
    assert res.returncode != 0 and word in res.stderr, (res.returncode, res.stderr)
    assert not [l for l in res.stdout.splitlines() if l[:1].isdigit()]  # (no energy line is printed)


@pytest.mark.parametrize("ensemble", ["surf_fit", "nve"])
def test_other_ensembles_are_refused_by_name(driver, tmp_path, ensemble):
    (tmp_path / "input").write_text("job_name t\nensemble %s\n" % ensemble)
    res = subprocess.run([driver, str(tmp_path / "input")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert res.returncode != 0 and ("ensemble %s is not implemented" % ensemble) in res.stderr


def test_molecule_count_size_and_frozen_refusals(driver, tmp_path):
    pqr = open(os.path.join(sf.GOLD, "n2_total", "dimer.pqr")).read().splitlines()
    atoms = [l for l in pqr if l.startswith("ATOM")]
    one = "\n".join(atoms[:5] + ["END"]) + "\n"
    res = run_input(driver, tmp_path, BASE, one)
    assert res.returncode != 0 and "only a single molecule" in res.stderr
    three = "\n".join(atoms + [l.replace(" M    2 ", " M    3 ") for l in atoms[5:]] + ["END"]) + "\n"
    res = run_input(driver, tmp_path, BASE, three)
    assert res.returncode != 0 and "exactly two molecules" in res.stderr
    big = "\n".join(atoms[:5] * 4 + atoms[5:] + ["END"]) + "\n"
    res = run_input(driver, tmp_path, BASE, big)
    assert res.returncode != 0 and "more than 16 sites" in res.stderr
    frozen = "\n".join([l.replace(" M    1 ", " F    1 ").replace(" M    2 ", " F    2 ") for l in atoms] + ["END"]) + "\n"
    res = run_input(driver, tmp_path, BASE, frozen)
    assert res.returncode != 0 and ("frozen" in res.stderr or "moveable" in res.stderr)
    res = run_input(driver, tmp_path, ["surf_min 3.0", "surf_max 4.0", "surf_inc 0.5"])
    assert res.returncode != 0 and "surf_ang is less than or equal to 0" in res.stderr
    res = run_input(driver, tmp_path, ["surf_min 5.0", "surf_max 4.0", "surf_ang 1.0"])
    assert res.returncode != 0 and "surf_max" in res.stderr
