"""CPU-only checks of the cavity_bias plumbing: the keywords through the C host layer, the check's messages, every
refusal by its name, the default (off), the new C-ABI entries, and the random numbers the grid update takes before there
is a device context."""
import ctypes as C
import os

import numpy as np
import pytest

from mpmc_amd import engine, host

PQR = (
    "ATOM      1 H2G  H2  M    1      0.000   0.000   0.000   2.0160   0.0000  0.00000  34.20000  2.96000\n"
    "ATOM      2 H2G  H2  M    2      4.000   1.000   0.000   2.0160   0.0000  0.00000  34.20000  2.96000\n"
    "ATOM      3 C    MOF F    3      5.000   5.000   5.000  12.0110   0.0000  0.00000  50.00000  3.40000\n"
    "END\n")
BASE = ("ensemble uvt\ntemperature 77\npressure 1.0\ninsert_probability 0.5\nnumsteps 1\ncorrtime 1\n"
        "basis1 20 0 0\nbasis2 0 20 0\nbasis3 0 0 20\npqr_input in.pqr\n")
CAVITY = "cavity_bias on\ncavity_grid 5\ncavity_radius 2.5\n"


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    if not (os.path.exists(host.LIB_PATH) and os.path.exists(engine.LIB_PATH)):
        g.build()


def _setup(tmp_path, extra, base=BASE):
    (tmp_path / "in.pqr").write_text(PQR)
    (tmp_path / "input").write_text(base + extra)
    return host.load().setup_system(str(tmp_path / "input").encode())


def _flags(lib, p):
    out = np.zeros(3)
    lib.host_get_cavity_flags(p, out.ctypes.data)
    return out.tolist()


def _state(lib, p):
    out = np.zeros(10)
    n = lib.host_get_cavity(p, out.ctypes.data)
    return n, out.tolist()


def test_keywords_and_the_banner(tmp_path, capfd):
    lib = host.load()
    p = _setup(tmp_path, CAVITY)
    assert p
    text = "".join(capfd.readouterr())
    assert "INPUT: cavity-biased umbrella sampling activated" in text
    assert "INPUT: cavity grid size is 5x5x5 points with a sphere radius of 2.500 A" in text
    assert _flags(lib, p) == [1.0, 5.0, 2.5]
    assert lib.host_unsupported(p) is None
    lib.free_system(p)
    p = _setup(tmp_path, "CAVITY_BIAS On\nCavity_Grid 64\ncavity_radius 1e0\n")  # keywords ignore case; 64 is the largest
    assert p and _flags(lib, p) == [1.0, 64.0, 1.0]
    lib.free_system(p)


def test_keyword_values(tmp_path):
    assert not _setup(tmp_path, "cavity_bias maybe\n")
    assert not _setup(tmp_path, "cavity_grid five\n")
    assert not _setup(tmp_path, "cavity_grid 5.5\n")
    assert not _setup(tmp_path, "cavity_radius wide\n")


@pytest.mark.parametrize("extra", ["cavity_bias on\n", "cavity_bias on\ncavity_grid 5\n", "cavity_bias on\ncavity_radius 2.5\n",
                                   "cavity_bias on\ncavity_grid 0\ncavity_radius 2.5\n",
                                   "cavity_bias on\ncavity_grid -3\ncavity_radius 2.5\n",
                                   "cavity_bias on\ncavity_grid 5\ncavity_radius 0\n",
                                   "cavity_bias on\ncavity_grid 5\ncavity_radius -1.0\n"])
def test_the_check_uses_the_references_words(tmp_path, capfd, extra):
    assert not _setup(tmp_path, extra)
    text = "".join(capfd.readouterr())
    assert "INPUT: invalid cavity grid or radius specified" in text
    assert "umbrella sampling activated" not in text


def test_refusals_by_name(tmp_path, capfd):
    assert not _setup(tmp_path, CAVITY, base=BASE.replace("ensemble uvt", "ensemble nvt"))
    assert "INPUT: cavity_bias needs ensemble uvt" in "".join(capfd.readouterr())
    assert not _setup(tmp_path, CAVITY, base=BASE.replace("ensemble uvt", "ensemble npt"))
    assert "INPUT: cavity_bias needs ensemble uvt" in "".join(capfd.readouterr())
    assert not _setup(tmp_path, "cavity_bias on\ncavity_grid 65\ncavity_radius 2.5\n")
    assert "INPUT: cavity_grid above 64 is not on the device" in "".join(capfd.readouterr())
    # a system built from arrays goes through the same check
    s = dict(pos=np.array([[0.0, 0, 0], [4.0, 0, 0]]), charge=np.zeros(2), alpha=np.zeros(2), epsilon=np.ones(2),
             sigma=np.ones(2), mass=np.ones(2), molecule=np.array([1, 2]), frozen=np.zeros(2, dtype=np.int32),
             basis=np.eye(3) * 20)
    uvt = {"ensemble": "uvt", "pressure": 1.0, "insert_probability": 0.5}
    with pytest.raises(ValueError):
        host.HostSystem(s, dict(temperature=77.0, cavity_bias=1, cavity_grid=5, cavity_radius=2.5))  # nvt
    with pytest.raises(ValueError):
        host.HostSystem(s, dict(temperature=77.0, cavity_bias=1, cavity_grid=65, cavity_radius=2.5), extra=uvt)
    with pytest.raises(ValueError):
        host.HostSystem(s, dict(temperature=77.0, cavity_bias=1, cavity_grid=5), extra=uvt)
    h = host.HostSystem(s, dict(temperature=77.0, cavity_bias=1, cavity_grid=5, cavity_radius=2.5), extra=uvt)
    assert h.cavity_flags() == dict(cavity_bias=1, cavity_grid=5, cavity_radius=2.5)
    h.close()


def test_the_default_is_off_and_reads_and_writes_what_it_always_did(tmp_path, capfd):
    lib = host.load()
    lib.write_molecules.argtypes = [C.c_void_p, C.c_char_p]
    files = []
    for k, extra in enumerate(("", "cavity_bias off\ncavity_grid 5\ncavity_radius 2.5\n", CAVITY)):
        p = _setup(tmp_path, extra)
        assert p and _flags(lib, p)[0] == (1.0 if extra == CAVITY else 0.0)
        text = "".join(capfd.readouterr())
        assert ("umbrella sampling" in text) == (extra == CAVITY)
        n, state = _state(lib, p)
        assert n == 0 and state[:9] == [0.0] * 9  # nothing has run
        out = tmp_path / ("out%d.pqr" % k)
        assert lib.write_molecules(p, str(out).encode()) == 0
        files.append(out.read_text())
        lib.free_system(p)
    assert files[0] == files[1] == files[2] and files[0].count("ATOM") == 3
    # off: outside uvt the keywords may stay in the file, and the grid and radius are not checked
    p = _setup(tmp_path, "cavity_bias off\ncavity_grid 500\ncavity_radius -1\n", base=BASE.replace("ensemble uvt", "ensemble nvt"))
    assert p
    lib.free_system(p)


def test_library_exports_the_entries_and_null_arguments_are_errors():
    lib = engine.load()
    names = ("mpmc_hip_set_cavity_grid", "mpmc_hip_cavity_bin", "mpmc_hip_cavity_update", "mpmc_hip_cavity_point",
             "mpmc_hip_download_cavity_grid")
    for name in names:
        assert hasattr(lib, name) and name in engine.EXPORTS
    n, g = C.c_int(0), C.c_int(0)
    pos = (C.c_double * 3)()
    assert lib.mpmc_hip_set_cavity_grid(None, 5, 2.5) != 0 and b"set_cavity_grid" in lib.mpmc_hip_last_error()
    assert lib.mpmc_hip_cavity_bin(None, 0, None, None, None) != 0 and b"cavity_bin" in lib.mpmc_hip_last_error()
    assert lib.mpmc_hip_cavity_update(None, 0, None, 0, None, 0, None, C.byref(n), C.byref(g)) != 0
    assert b"cavity_update" in lib.mpmc_hip_last_error()
    assert lib.mpmc_hip_cavity_point(None, 0, C.byref(g), pos) != 0 and b"cavity_point" in lib.mpmc_hip_last_error()
    assert lib.mpmc_hip_download_cavity_grid(None, None, None) != 0
    assert b"download_cavity_grid" in lib.mpmc_hip_last_error()
    header = open(os.path.join(os.path.dirname(engine.__file__), "..", "include", "mpmc_hip.h")).read()
    for name in names:
        assert name + "(" in header
    assert '"cavity_incremental"' in header
    hl = host.load()
    for name in ("energy_hip_cavity_update", "energy_hip_cavity_point", "energy_hip_cavity_darts", "host_get_cavity",
                 "host_get_cavity_darts", "host_get_cavity_flags", "update_nodestats", "update_root_nodestats",
                 "clear_avg_nodestats"):
        assert hasattr(hl, name), name


def test_config_text_and_make_params_leave_the_keys_to_their_calls():
    flags = dict(temperature=77.0, cavity_bias=1, cavity_grid=5, cavity_radius=2.5)
    txt = host.config_text(flags)
    assert "cavity_bias on" in txt and "cavity_grid 5" in txt and "cavity_radius 2.5" in txt
    assert "cavity_bias off" in host.config_text(dict(cavity_bias=0))


def test_the_grid_update_before_the_first_energy_takes_its_darts_and_nothing_else(tmp_path):
    """mc() updates the grid once in front of the first energy() (mc.c:245): 3 * (int)(0.1 V) draws, three per dart, in
    order.  A second stream with the same seed that skips that many numbers continues where the first one does."""
    lib = host.load()
    lib.energy_hip_cavity_update.argtypes = [C.c_void_p]
    a, b = _setup(tmp_path, CAVITY), _setup(tmp_path, "")
    assert a and b
    for p in (a, b):
        lib.host_seed(p, 12345)
    first = lib.host_get_rand(a)
    assert first == lib.host_get_rand(b)
    assert lib.energy_hip_cavity_update(a) == 0  # no device context yet: the draws only
    n_darts = int(20.0 * 20.0 * 20.0 * 0.1)
    assert n_darts == 800
    skipped = [lib.host_get_rand(b) for _ in range(3 * n_darts)]
    assert lib.host_get_rand(a) == lib.host_get_rand(b)
    n, state = _state(lib, a)
    assert n == n_darts and state[0] == 0.0 and state[1] == 0.0 and state[3] == 0.0  # nothing reads that call's results
    # the darts it recorded are those draws: f = -0.5 + u, x = 20 f in this cubic cell
    darts = np.zeros((n, 3))
    lib.host_get_cavity_darts(a, darts.ctypes.data)
    assert np.array_equal(darts, 20.0 * (-0.5 + np.array(skipped).reshape(n, 3)))
    # with the keyword off nothing is drawn
    lib.host_seed(b, 777)
    lib.host_seed(a, 777)
    a_off = _setup(tmp_path, "cavity_bias off\n")
    lib.host_seed(a_off, 777)
    if engine.load().mpmc_hip_device_count() == 0:
        # without a device the chain stops at its first energy(): the cavity-biased one behind its darts, the plain one
        # before any draw
        assert lib.host_mc_steps(a, 0) == -1 and lib.host_mc_steps(a_off, 0) == -1
        for _ in range(3 * n_darts):
            lib.host_get_rand(b)
        assert lib.host_get_rand(a) == lib.host_get_rand(b)
        lib.host_seed(b, 777)
        assert lib.host_get_rand(a_off) == lib.host_get_rand(b)
    for p in (a, b, a_off):
        lib.free_system(p)
