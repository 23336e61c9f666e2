"""CPU-only checks of the coupled-dipole van der Waals plumbing: the keywords, the omega PQR column and the forced sigma
through the C host layer and back out through its writer, every refusal by its name, the new C-ABI entries."""
import ctypes as C
import os

import numpy as np
import pytest

from mpmc_amd import engine, host

#                                              x       y       z      mass    charge    alpha    epsilon    sigma  omega
PQR = (
    "ATOM      1 C    CH4 M    1      0.000   0.000   0.000  12.0110  -0.4000  1.00000  40.00000  1.00000 0.71000\n"
    "ATOM      2 H    CH4 M    1      1.090   0.000   0.000   1.0079   0.1000  0.30000   6.00000  2.40000 0.52000 0.0 1.0 2.0 3.0 4.0\n"
    "ATOM      3 AR   AR  M    2      4.000   0.000   0.000  39.9480   0.0000  1.64110 119.80000  3.40500\n"
    "ATOM      4 C    MOF F    3      5.000   5.000   5.000  12.0110   0.0000  1.20000  50.00000  1.00000 0.60000\n"
    "END\n")
BASE = ("ensemble nvt\ntemperature 150\nnumsteps 1\ncorrtime 1\nbasis1 20 0 0\nbasis2 0 20 0\nbasis3 0 0 20\n"
        "polar_damp_type exponential\npolar_damp 2.1304\npolar_max_iter 4\npqr_input in.pqr\n")
VDW = "polarvdw on\ncavity_autoreject_absolute on\ncavity_autoreject_scale 1.5\n"


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    if not (os.path.exists(host.LIB_PATH) and os.path.exists(engine.LIB_PATH)):
        g.build()


def _setup(tmp_path, extra, pqr=PQR, name="in.pqr", base=BASE):
    (tmp_path / name).write_text(pqr)
    (tmp_path / "input").write_text(base.replace("in.pqr", name) + extra)
    return host.load().setup_system(str(tmp_path / "input").encode())


def _vdw(lib, p):
    out = np.zeros(5)
    lib.host_get_vdw(p, out.ctypes.data)
    return out.tolist()


def _omega(lib, p, n):
    out = np.zeros(n)
    lib.host_get_omega(p, out.ctypes.data)
    return out.tolist()


def _sigma(lib, p, n):
    f = [np.zeros(n) for _ in range(5)]
    pos, mol, frz = np.zeros((n, 3)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    lib.host_get_system(p, pos.ctypes.data, *[a.ctypes.data for a in f], mol.ctypes.data, frz.ctypes.data)
    return f[3].tolist()


def _why(lib, p):
    w = lib.host_unsupported(p)
    return None if w is None else w.decode()


@pytest.mark.parametrize("keyword", ["polarvdw", "cdvdw"])
def test_keywords_omega_column_and_forced_sigma(tmp_path, capfd, keyword):
    lib = host.load()
    p = _setup(tmp_path, VDW.replace("polarvdw", keyword))
    assert p
    err = capfd.readouterr().err
    assert _vdw(lib, p) == [1.0, 1.0, 1.5, 0.0, 0.0]
    # column 15, behind sigma; absent columns read as 0
    assert _omega(lib, p, 4) == [0.71, 0.52, 0.0, 0.6]
    # read_pqr.c:266-271: every sigma becomes 1.0, with the reference's warning for the two that were not
    assert _sigma(lib, p, 4) == [1.0, 1.0, 1.0, 1.0]
    assert err.count("warning: setting sigma to 1.0 (due to polarvdw)") == 2
    assert _why(lib, p) is None
    lib.free_system(p)


def test_mode_off_reads_and_writes_what_it_always_did(tmp_path, capfd):
    lib = host.load()
    lib.write_molecules.argtypes = [C.c_void_p, C.c_char_p]
    p = _setup(tmp_path, "")
    assert p and _vdw(lib, p) == [0.0, 0.0, 0.0, 0.0, 0.0] and _why(lib, p) is None
    assert "warning" not in capfd.readouterr().err
    assert _sigma(lib, p, 4) == [1.0, 2.4, 3.405, 1.0]
    off = tmp_path / "off.pqr"
    assert lib.write_molecules(p, str(off).encode()) == 0
    lib.free_system(p)
    rows = [ln.split() for ln in off.read_text().splitlines() if ln.startswith("ATOM")]
    assert [len(r) for r in rows] == [20] * 4
    assert [float(r[14]) for r in rows] == [0.0] * 4  # omega is not written while the mode is off
    assert [float(r[16]) for r in rows] == [0.0, 1.0, 0.0, 0.0]
    # ... and with the mode on the column carries it, so that a restart keeps the frequencies
    p = _setup(tmp_path, VDW)
    on = tmp_path / "on.pqr"
    assert lib.write_molecules(p, str(on).encode()) == 0
    lib.free_system(p)
    rows_on = [ln.split() for ln in on.read_text().splitlines() if ln.startswith("ATOM")]
    assert [float(r[14]) for r in rows_on] == [0.71, 0.52, 0.0, 0.6]
    for a, b in zip(rows, rows_on):  # nothing else differs but the forced sigma
        assert a[:13] == b[:13] and a[15:] == b[15:] and float(b[13]) == 1.0
    q = _setup(tmp_path, VDW, pqr=on.read_text(), name="again.pqr")
    assert q and _omega(lib, q, 4) == [0.71, 0.52, 0.0, 0.6]
    lib.free_system(q)


def test_keyword_values(tmp_path):
    lib = host.load()
    assert not _setup(tmp_path, "polarvdw maybe\n")
    assert not _setup(tmp_path, "cavity_autoreject_absolute perhaps\n")
    assert not _setup(tmp_path, "cavity_autoreject_scale wide\n")
    # the reference's range check of the scale: 0 < scale <= 1.78
    for bad in ("", "cavity_autoreject_scale 0\n", "cavity_autoreject_scale 1.79\n", "cavity_autoreject_scale -1\n"):
        assert not _setup(tmp_path, "cavity_autoreject_absolute on\n" + bad)
    p = _setup(tmp_path, "cavity_autoreject_absolute on\ncavity_autoreject_scale 1.78\n")  # usable without polarvdw
    assert p and _vdw(lib, p)[:3] == [0.0, 1.0, 1.78] and _why(lib, p) is None
    lib.free_system(p)
    p = _setup(tmp_path, "polarvdw off\n")
    assert p and _vdw(lib, p)[0] == 0.0
    lib.free_system(p)
    # polarvdw outside replay demands cavity_autoreject_absolute: the reference's message (check_input.c:216-219)
    assert not _setup(tmp_path, "polarvdw on\n")


REFUSED = [
    ("polarvdw evects\n", "polarvdw evects"),
    ("polarvdw comp\n", "polarvdw comp"),
    ("polarvdw on\ncdvdw_exp_repulsion on\n", "cdvdw_exp_repulsion"),
    ("polarvdw on\ncdvdw_sig_repulsion on\n", "cdvdw_sig_repulsion"),
    ("polarvdw on\ncdvdw_9th_repulsion on\n", "cdvdw_9th_repulsion"),
    ("polarvdw on\nfeynman_hibbs on\n", "feynman_hibbs with polarvdw"),
    ("polarvdw on\npolarization off\n", "polarvdw without polarization"),
    ("polarvdw on\ndisp_expansion on\n", "disp_expansion with polarvdw"),
    ("polarvdw on\nrd_crystal on\nrd_crystal_order 2\n", "rd_crystal with polarvdw"),
    ("polarvdw on\naxilrod_teller on\n", "axilrod_teller with polarvdw"),
]


@pytest.mark.parametrize("extra,name", REFUSED)
def test_every_refusal_names_itself(tmp_path, extra, name):
    lib = host.load()
    p = _setup(tmp_path, extra + "cavity_autoreject_absolute on\ncavity_autoreject_scale 1.5\n")
    assert p
    why = _why(lib, p)
    assert why is not None and name in why, why
    lib.free_system(p)


def test_missing_autoreject_is_refused_with_the_references_message():
    # a system built from arrays does not pass check_system(): energy_hip.c refuses it itself
    s = dict(pos=np.array([[0.0, 0, 0], [4.0, 0, 0]]), charge=np.zeros(2), alpha=np.ones(2), epsilon=np.ones(2),
             sigma=np.ones(2), mass=np.ones(2), molecule=np.array([1, 2]), frozen=np.zeros(2, dtype=np.int32),
             basis=np.eye(3) * 20, omega=np.full(2, 0.5), mol_type=np.zeros(2, dtype=np.int32))
    h = host.HostSystem(s, dict(temperature=150.0, polarvdw=1, polar_damp=2.1304, polar_max_iter=4))
    why = _why(h.lib, h.ptr)
    assert why == "cavity_autoreject_absolute must be used with polarvdw + Feynman Hibbs."
    assert h.vdw()["polarvdw"] == 1 and _omega(h.lib, h.ptr, 2) == [0.5, 0.5]
    h.close()
    h = host.HostSystem(s, dict(temperature=150.0, polarvdw=1, polar_damp=2.1304, polar_max_iter=4,
                                cavity_autoreject_absolute=1, cavity_autoreject_scale=1.5))
    assert _why(h.lib, h.ptr) is None
    h.close()
    with pytest.raises(ValueError):
        host.HostSystem(s, dict(temperature=150.0, cavity_autoreject_absolute=1, cavity_autoreject_scale=2.0))


def test_library_exports_the_entries_and_null_arguments_are_errors():
    lib = engine.load()
    names = ("mpmc_hip_set_vdw", "mpmc_hip_get_vdw_energy", "mpmc_hip_get_vdw_terms", "mpmc_hip_set_autoreject",
             "mpmc_hip_get_close_contacts")
    for name in names:
        assert hasattr(lib, name) and name in engine.EXPORTS
    assert lib.mpmc_hip_set_vdw(None, 1, 0, None, None) != 0 and b"set_vdw" in lib.mpmc_hip_last_error()
    v = C.c_double(1.0)
    assert lib.mpmc_hip_get_vdw_energy(None, C.byref(v)) != 0 and b"get_vdw_energy" in lib.mpmc_hip_last_error()
    assert lib.mpmc_hip_set_autoreject(None, 1.0) != 0 and b"set_autoreject" in lib.mpmc_hip_last_error()
    n = C.c_longlong(0)
    assert lib.mpmc_hip_get_close_contacts(None, C.byref(n)) != 0 and b"get_close_contacts" in lib.mpmc_hip_last_error()
    # the result record did not grow: the term has its own getter
    assert "vdw_energy" not in [f for f, _ in engine.Result._fields_]
    header = open(os.path.join(os.path.dirname(engine.__file__), "..", "include", "mpmc_hip.h")).read()
    for name in names:
        assert name + "(" in header


def test_config_text_and_make_params_leave_the_keys_to_their_calls():
    flags = dict(temperature=150.0, polarization=1, polar_damp=2.1304, polarvdw=1, cavity_autoreject_absolute=1,
                 cavity_autoreject_scale=1.5)
    txt = host.config_text(flags)
    assert "polarvdw on" in txt and "cavity_autoreject_absolute on" in txt and "cavity_autoreject_scale 1.5" in txt
    assert "polarvdw evects" in host.config_text(dict(polarvdw="evects"))
    p = engine.make_params(**flags)
    assert p.polarization == 1 and p.rd_only == 0
