"""CPU-only checks of the rd_crystal / replay plumbing: the keywords through the C host layer, what it refuses, the
replay frame reader on a trajectory written from the fixture's arrays, and the new C-ABI entry."""
import os

import numpy as np
import pytest

import rdc_cases as rc
from mpmc_amd import engine, host, synth

PQR = (
    "ATOM      1 AR   AR  M    1      0.000   0.000   0.000  39.9480   0.0000  1.64110 119.80000  3.40500\n"
    "ATOM      2 N    N2  M    2      4.000   0.000   0.000  14.0067   0.2000  0.80000  36.00000  3.31000\n"
    "ATOM      3 N    N2  M    2      5.100   0.000   0.000  14.0067  -0.2000  0.80000  36.00000  3.31000\n"
    "END\n")
BASE = ("ensemble nvt\ntemperature 77\nnumsteps 1\ncorrtime 1\nbasis1 20 0 0\nbasis2 0 20 0\nbasis3 0 0 20\n"
        "pqr_input in.pqr\n")


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
    out = np.zeros(2, dtype=np.int32)
    lib.host_get_rdc_flags(p, out.ctypes.data)
    return out.tolist()


def test_keywords(tmp_path):
    lib = host.load()
    p = _setup(tmp_path, "")
    assert _flags(lib, p) == [0, 0] and lib.host_unsupported(p) is None
    lib.free_system(p)
    p = _setup(tmp_path, "rd_crystal on\nrd_crystal_order 3\n")
    assert _flags(lib, p) == [1, 3] and lib.host_unsupported(p) is None
    lib.free_system(p)
    p = _setup(tmp_path, "rd_crystal off\nrd_crystal_order 3\n")
    assert _flags(lib, p) == [0, 3] and lib.host_unsupported(p) is None
    lib.free_system(p)
    # the reference's input check: the order must be positive (and it has no default)
    assert not _setup(tmp_path, "rd_crystal on\n")
    assert not _setup(tmp_path, "rd_crystal on\nrd_crystal_order 0\n")
    assert not _setup(tmp_path, "rd_crystal on\nrd_crystal_order -2\n")
    assert not _setup(tmp_path, "rd_crystal maybe\n")
    assert not _setup(tmp_path, "rd_crystal_order two\n")


def test_refusals_name_themselves(tmp_path):
    lib = host.load()
    p = _setup(tmp_path, "rd_crystal on\nrd_crystal_order 2\ndisp_expansion on\n")
    why = lib.host_unsupported(p)
    assert why is not None and "rd_crystal with disp_expansion" in why.decode()
    lib.free_system(p)
    p = _setup(tmp_path, "rd_crystal on\nrd_crystal_order 5\n")
    why = lib.host_unsupported(p)
    assert why is not None and "rd_crystal_order above 4" in why.decode()
    lib.free_system(p)
    p = _setup(tmp_path, "rd_crystal on\nrd_crystal_order 4\naxilrod_teller on\n")
    assert lib.host_unsupported(p) is None
    lib.free_system(p)
    # an order that is switched off is nobody's business
    p = _setup(tmp_path, "rd_crystal off\nrd_crystal_order 9\ndisp_expansion on\n")
    assert lib.host_unsupported(p) is None
    lib.free_system(p)


def test_replay_keywords(tmp_path):
    traj, _ = rc.trajectory_text([0, 1])
    (tmp_path / "traj.pqr").write_text(traj)
    replay = BASE.replace("ensemble nvt", "ensemble replay").replace("pqr_input in.pqr", "pqr_input /dev/null")
    lib = host.load()
    assert not _setup(tmp_path, "", base=replay)  # no traj_input
    assert not _setup(tmp_path, "traj_input nowhere.pqr\n", base=replay)
    assert not _setup(tmp_path, "traj_input traj.pqr\ncalc_pressure on\n", base=replay)  # refused by name (stderr)
    p = _setup(tmp_path, "traj_input traj.pqr\nread_pqr_box on\ncalc_pressure off\n", base=replay)
    assert p and lib.host_natoms(p) == 2  # the first frame, as the reference's setup_system() reads it
    lib.free_system(p)
    assert not _setup(tmp_path, "ensemble sideways\n")


def test_frame_reader_on_the_fixture(tmp_path):
    """every frame of a trajectory written from the fixture: atoms, box, and the cutoff a replay holds there -- the first
    frame's, because pbc() keeps a cutoff that is set (as in the reference)"""
    traj, systems = rc.trajectory_text()
    path = tmp_path / "traj.pqr"
    path.write_text(traj)
    s0 = systems[0]
    h = host.HostSystem(s0, dict(temperature=77.0), extra={"read_pqr_box": "on"})
    first_cutoff = None
    for k, s in enumerate(systems):
        assert h.lib.host_read_frame(h.ptr, str(path).encode(), k) == 0
        n = len(s["charge"])
        assert h.lib.host_natoms(h.ptr) == n == rc.META["atoms_per_snapshot"][k]
        h.n = n
        assert np.array_equal(h.positions(), s["pos"])
        assert np.array_equal(h.basis(), s["basis"])
        o = h.observables()
        assert o["volume"] == abs(np.linalg.det(s["basis"])) or abs(o["volume"] - np.linalg.det(s["basis"])) < 1e-9
        first_cutoff = o["cutoff"] if k == 0 else first_cutoff
        assert o["cutoff"] == first_cutoff == 0.5
    assert h.lib.host_read_frame(h.ptr, str(path).encode(), len(systems)) == 1  # past the end: out of frames
    assert h.lib.host_natoms(h.ptr) == 0
    h.close()
    # without read_pqr_box the REMARK BOX lines are not read: the box stays
    h = host.HostSystem(s0, dict(temperature=77.0))
    assert h.lib.host_read_frame(h.ptr, str(path).encode(), 3) == 0
    assert np.array_equal(h.basis(), s0["basis"]) and h.lib.host_natoms(h.ptr) == 128
    h.close()


def test_library_exports_the_entry_and_a_null_context_is_an_error():
    lib = engine.load()
    assert hasattr(lib, "mpmc_hip_set_rd_crystal") and "mpmc_hip_set_rd_crystal" in engine.EXPORTS
    assert lib.mpmc_hip_abi_version() == 1
    assert lib.mpmc_hip_set_rd_crystal(None, 2) != 0
    assert b"set_rd_crystal" in lib.mpmc_hip_last_error()


def test_config_text_and_params_carry_the_new_flags():
    f = rc.flags("fh2", 3)
    txt = host.config_text(f)
    assert "rd_crystal on" in txt and "rd_crystal_order 3" in txt
    h = host.HostSystem(synth.s_lj(8), f)
    assert _flags(h.lib, h.ptr) == [1, 3]
    h.close()
    with pytest.raises(ValueError):
        host.HostSystem(synth.s_lj(8), dict(f, rd_crystal_order=0))
    assert engine.make_params(**f).rd_only == 1  # make_params() leaves the two keys to set_rd_crystal()
