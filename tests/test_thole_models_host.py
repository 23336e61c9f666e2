"""CPU: the host layer's side of the dipole tensors beside the exponential one -- polar_damp_type none | off | linear |
exponential and polar_wolf_full are read as the reference reads them, announced with its lines, sent to the engine
(mpmc_hip_set_thole_model) and refused by name only where the device has nothing to offer."""
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
        "polarization on\npolar_iterative on\npolar_max_iter 4\npqr_input in.pqr\n")
OFF, LINEAR, EXPONENTIAL = 0, 1, 2  # the reference's DAMPING_* values


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


def _thole(lib, p):
    out = (C.c_int * 3)()
    lib.host_get_thole_flags(p, out)
    return list(out)


@pytest.mark.parametrize("extra,want,line", [
    ("polar_damp_type linear\npolar_damp 1.662\n", [LINEAR, 0, 0], "INPUT: Thole linear damping activated"),
    ("polar_damp_type LINEAR\npolar_damp 2.1304\n", [LINEAR, 0, 0], "INPUT: Thole linear damping activated"),
    ("polar_damp_type off\n", [OFF, 0, 0], "INPUT: Thole linear damping is OFF"),
    ("polar_damp_type none\n", [OFF, 0, 0], "INPUT: Thole linear damping is OFF"),
    ("polar_damp_type off\npolar_damp 0\n", [OFF, 0, 0], "INPUT: Thole linear damping is OFF"),  # check_input.c:406
    ("", [OFF, 0, 0], "INPUT: Thole linear damping is OFF"),  # absent = off, as there (a zeroed system_t)
    ("polar_damp_type exponential\npolar_damp 2.1304\npolar_wolf_full on\n", [EXPONENTIAL, 1, 0],
     "INPUT: Full polar wolf treatment activated."),
    ("polar_damp_type exponential\npolar_damp 2.1304\npolar_wolf_full on\npolar_wolf on\npolar_wolf_alpha 0.13\n",
     [EXPONENTIAL, 1, 0], "INPUT: Full polar wolf treatment activated."),
    ("polar_damp_type exponential\npolar_damp 2.1304\npolar_wolf_full off\n", [EXPONENTIAL, 0, 0], None),
])
def test_every_spelling_is_read_and_supported(tmp_path, capfd, extra, want, line):
    lib = host.load()
    p = _setup(tmp_path, extra)
    assert p, capfd.readouterr().err
    out = capfd.readouterr().out
    assert _thole(lib, p) == want
    assert _why(lib, p) is None
    if line:
        assert line in out
    else:
        assert "Full polar wolf" not in out and "linear damping" not in out
    lib.free_system(p)


def test_what_set_up_still_refuses(tmp_path, capfd):
    assert not _setup(tmp_path, "polar_damp_type quadratic\n")  # input.c:1231-1232
    assert not _setup(tmp_path, "polar_wolf_full maybe\n")
    capfd.readouterr()
    # a damping factor is needed unless the type is off (check_input.c:406-409)
    for extra in ("polar_damp_type linear\n", "polar_damp_type exponential\npolar_damp 0\n", "polar_damp_type linear\npolar_damp -1\n"):
        assert not _setup(tmp_path, extra)
        assert "INPUT: damping factor must be specified" in capfd.readouterr().err


def test_refusals_that_remain_are_made_by_name(tmp_path):
    lib = host.load()
    for extra, name in (
            ("polar_damp_type exponential\npolar_damp 2.1304\npolar_ewald_full on\n", "polar_ewald_full"),
            ("polar_damp_type linear\npolar_damp 2.1304\npolar_wolf_full on\n", "polar_wolf_full needs polar_damp_type exponential"),
            ("polar_damp_type off\npolar_wolf_full on\n", "polar_wolf_full needs polar_damp_type exponential"),
            ("polar_damp_type linear\npolar_damp 2.1304\npolarvdw on\ncavity_autoreject_absolute on\ncavity_autoreject_scale 0.5\n",
             "polarvdw with polar_damp_type linear / off or polar_wolf_full is not on the device"),
            ("polar_damp_type exponential\npolar_damp 2.1304\npolar_wolf_full on\npolarvdw on\ncavity_autoreject_absolute on\n"
             "cavity_autoreject_scale 0.5\n", "polarvdw with polar_damp_type linear / off or polar_wolf_full is not on the device")):
        p = _setup(tmp_path, extra)
        assert p
        why = _why(lib, p)
        assert why is not None and name in why, (extra, why)
        lib.free_system(p)


S2 = dict(pos=np.array([[0.0, 0, 0], [4.0, 0, 0]]), charge=np.array([0.3, -0.3]), alpha=np.ones(2), epsilon=np.ones(2),
          sigma=np.ones(2), mass=np.ones(2), molecule=np.array([1, 2]), frozen=np.zeros(2, dtype=np.int32),
          basis=np.eye(3) * 20, omega=np.full(2, 0.5), mol_type=np.zeros(2, dtype=np.int32))
F = dict(temperature=77.0, polarization=1, polar_damp=2.1304, polar_max_iter=4)


def test_config_text_round_trips():
    """a given polar_damp_type is written as a bare word in place of the built-in exponential line, polar_wolf_full as
    on / off; without the keys the text is what it was"""
    assert host.config_text(F).count("polar_damp_type") == 1 and "polar_damp_type exponential\n" in host.config_text(F)
    assert "polar_wolf_full" not in host.config_text(F)
    for word, want in (("linear", LINEAR), ("off", OFF), ("none", OFF), ("exponential", EXPONENTIAL)):
        txt = host.config_text(dict(F, polar_damp_type=word))
        assert txt.count("polar_damp_type") == 1 and ("polar_damp_type %s\n" % word) in txt
        h = host.HostSystem(S2, dict(F, polar_damp_type=word))
        assert _thole(h.lib, h.ptr) == [want, 0, 0] and _why(h.lib, h.ptr) is None
        h.close()
    for v, word in ((1, "on"), (0, "off")):
        txt = host.config_text(dict(F, polar_wolf_full=v))
        assert ("polar_wolf_full %s\n" % word) in txt and "polar_damp_type exponential\n" in txt
        h = host.HostSystem(S2, dict(F, polar_wolf_full=v))
        assert _thole(h.lib, h.ptr) == [EXPONENTIAL, v, 0] and _why(h.lib, h.ptr) is None
        h.close()
    # a system built from arrays keeps the exponential tensor unless the text names another
    h = host.HostSystem(S2, dict(temperature=77.0, polarvdw=1, polar_damp=2.1304, polar_max_iter=4, cavity_autoreject_absolute=1,
                                 cavity_autoreject_scale=0.5))
    assert _thole(h.lib, h.ptr) == [EXPONENTIAL, 0, 0] and _why(h.lib, h.ptr) is None
    h.close()
    h = host.HostSystem(S2, dict(F, polar_damp_type="linear", polar_wolf_full=1))
    assert "polar_wolf_full needs polar_damp_type exponential" in _why(h.lib, h.ptr)
    h.close()


def test_library_exports_the_entry_and_refuses_bad_records():
    lib = engine.load()
    assert hasattr(lib, "mpmc_hip_set_thole_model") and "mpmc_hip_set_thole_model" in engine.EXPORTS
    assert lib.mpmc_hip_abi_version() == 1
    assert lib.mpmc_hip_set_thole_model(None, None) != 0 and b"set_thole_model" in lib.mpmc_hip_last_error()
    header = open(os.path.join(os.path.dirname(engine.__file__), "..", "include", "mpmc_hip.h")).read()
    assert "int mpmc_hip_set_thole_model(mpmc_hip_ctx *ctx, const mpmc_hip_thole_model *m);" in header
    assert engine.THOLE_DAMPINGS == dict(off=0, none=0, linear=1, exponential=2)
    assert set(engine.THOLE_NAMES) <= engine.NOT_PARAMS  # the two keywords are no fields of mpmc_hip_params
