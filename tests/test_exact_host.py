"""CPU-only checks of the exact-dipole plumbing (polar_iterative off, polarizability_tensor): the keywords through the C
host layer, every refusal by its name, the new C-ABI entries and the Python flag handling."""
import ctypes as C
import os

import numpy as np
import pytest

from mpmc_amd import engine, host

PQR = (
    "ATOM      1 H2G  H2  M    1     -4.353  -9.818   2.557   0.0000  -0.7464  0.69380 12.76532  3.15528\n"
    "ATOM      2 H2E  H2  M    1     -4.640  -9.822   2.323   1.0080   0.3732  0.00044  0.00000  0.00000\n"
    "ATOM      3 H2E  H2  M    1     -4.066  -9.813   2.791   1.0080   0.3732  0.00044  0.00000  0.00000\n"
    "ATOM      4 AR   AR  M    2      4.000   0.000   0.000  39.9480   0.0000  1.64110 119.80000  3.40500 0.70000\n"
    "END\n")
BASE = ("ensemble nvt\ntemperature 77\nnumsteps 1\ncorrtime 1\nbasis1 20 0 0\nbasis2 0 20 0\nbasis3 0 0 20\n"
        "polarization on\npolar_damp_type exponential\npolar_damp 2.1304\npqr_input in.pqr\n")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    if not (os.path.exists(host.LIB_PATH) and os.path.exists(engine.LIB_PATH)):
        g.build()


def _setup(tmp_path, extra):
    (tmp_path / "in.pqr").write_text(PQR)
    (tmp_path / "input").write_text(BASE + extra)
    return host.load().setup_system(str(tmp_path / "input").encode())


def _why(lib, p):
    w = lib.host_unsupported(p)
    return None if w is None else w.decode()


@pytest.mark.parametrize("extra", ["polar_iterative off\n", "", "polar_iterative off\npolar_max_iter 4\npolar_gs on\n"])
def test_polar_iterative_off_parses_and_is_supported(tmp_path, capfd, extra):
    """absent = off, as in the reference (its system_t starts zeroed): polarization then means the direct solve; the
    solver keywords may stay in the file, the engine ignores them in this mode"""
    lib = host.load()
    p = _setup(tmp_path, extra)
    assert p
    assert _why(lib, p) is None
    assert "INPUT: Matrix polarization activated" in capfd.readouterr().out  # check_input.c:486-488
    lib.free_system(p)


def test_polar_iterative_on_is_what_it_was(tmp_path, capfd):
    lib = host.load()
    p = _setup(tmp_path, "polar_iterative on\npolar_max_iter 4\n")
    assert p and _why(lib, p) is None
    assert "Matrix polarization" not in capfd.readouterr().out
    lib.free_system(p)


def test_tensor_keyword(tmp_path, capfd):
    lib = host.load()
    p = _setup(tmp_path, "polar_iterative off\npolarizability_tensor on\n")
    assert p and _why(lib, p) is None
    assert "INPUT: Polarizability tensor calculation activated" in capfd.readouterr().out  # check_input.c:489-491
    lib.free_system(p)
    # with the iterative solver: the reference's message (check_input.c:343-347), at set-up ...
    assert not _setup(tmp_path, "polar_iterative on\npolar_max_iter 4\npolarizability_tensor on\n")
    assert "INPUT: iterative polarizability tensor method not implemented" in capfd.readouterr().err
    assert not _setup(tmp_path, "polarizability_tensor maybe\n")
    assert not _setup(tmp_path, "polar_iterative perhaps\n")


def test_zodid_with_the_direct_solve_is_refused_at_set_up(tmp_path, capfd):
    assert not _setup(tmp_path, "polar_iterative off\npolar_zodid on\n")
    assert "INPUT: ZODID and matrix inversion cannot both be set!" in capfd.readouterr().err  # check_input.c:349-353


S2 = dict(pos=np.array([[0.0, 0, 0], [4.0, 0, 0]]), charge=np.array([0.3, -0.3]), alpha=np.ones(2), epsilon=np.ones(2),
          sigma=np.ones(2), mass=np.ones(2), molecule=np.array([1, 2]), frozen=np.zeros(2, dtype=np.int32),
          basis=np.eye(3) * 20, omega=np.full(2, 0.5), mol_type=np.zeros(2, dtype=np.int32))
F = dict(temperature=77.0, polarization=1, polar_damp=2.1304)
REFUSED = [
    (dict(F, polar_iterative=0, polar_zodid=1), "ZODID and matrix inversion cannot both be set!"),
    (dict(F, polar_iterative=0, polar_zodid=1), "polar_zodid with polar_iterative off"),
    (dict(F, polar_iterative=0, polar_palmo=1), "polar_palmo with polar_iterative off"),
    (dict(F, polarvdw=1, cavity_autoreject_absolute=1, cavity_autoreject_scale=1.5, polar_iterative=0),
     "polarvdw with polar_iterative off"),
    (dict(F, polar_max_iter=4, polarizability_tensor=1), "iterative polarizability tensor method not implemented"),
]


@pytest.mark.parametrize("flags,name", REFUSED)
def test_every_refusal_names_itself(flags, name):
    """systems built from arrays do not pass check_system(): energy_hip.c states the refusals itself"""
    h = host.HostSystem(S2, flags)
    try:
        why = _why(h.lib, h.ptr)
        assert why is not None and name in why, why
    finally:
        h.close()


def test_array_built_systems_iterate_unless_told_otherwise():
    for flags, want in ((dict(F, polar_max_iter=4), None), (dict(F, polar_iterative=0), None),
                        (dict(F, polar_iterative=0, polarizability_tensor=1), None)):
        h = host.HostSystem(S2, flags)
        assert _why(h.lib, h.ptr) is want
        h.close()
    txt = host.config_text(dict(F, polar_iterative=0))
    assert "polar_iterative off" in txt and "polar_iterative on" not in txt
    assert "polar_iterative on" in host.config_text(F)
    assert "polarizability_tensor on" in host.config_text(dict(F, polar_iterative=0, polarizability_tensor=1))


def test_library_exports_the_entries_and_null_arguments_are_errors():
    lib = engine.load()
    names = ("mpmc_hip_set_exact_polar", "mpmc_hip_get_polarizability_tensor")
    for name in names:
        assert hasattr(lib, name) and name in engine.EXPORTS
    assert lib.mpmc_hip_abi_version() == 1
    assert lib.mpmc_hip_set_exact_polar(None, 1) != 0 and b"set_exact_polar" in lib.mpmc_hip_last_error()
    t = (C.c_double * 9)()
    assert lib.mpmc_hip_get_polarizability_tensor(None, t) != 0
    assert b"get_polarizability_tensor" in lib.mpmc_hip_last_error()
    header = open(os.path.join(os.path.dirname(engine.__file__), "..", "include", "mpmc_hip.h")).read()
    for name in names:
        assert name + "(" in header
    # the records did not grow
    assert "polar_iterative" not in engine.PARAM_NAMES
    p = engine.make_params(**dict(F, polar_iterative=0))  # left to Engine.load_system()
    assert p.polarization == 1
