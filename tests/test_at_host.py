"""CPU-only checks of the Axilrod-Teller plumbing: the two keywords and the c9 PQR column through the C host layer and
back out through its writer, the refusal list, the two new C-ABI entries, and the effective-c9 arithmetic."""
import ctypes as C
import os

import numpy as np
import pytest

import at_reference as ref
from mpmc_amd import engine, host, synth

PQR = (
    "ATOM      1 AR   AR  M    1      0.000   0.000   0.000  39.9480   0.0000  1.64110 119.80000  3.40500 0.0 0.0 64.3 0.0 0.0 518.3\n"
    "ATOM      2 N    N2  M    2      4.000   0.000   0.000  14.0067   0.2000  0.80000  36.00000  3.31000 0.0 0.0 24.0 0.0 0.0 100.0\n"
    "ATOM      3 N    N2  M    2      5.100   0.000   0.000  14.0067  -0.2000  0.80000  36.00000  3.31000 0.0 0.0 24.0 0.0 0.0\n"
    "ATOM      4 C    MOF F    3      5.000   5.000   5.000  12.0110   0.0000  1.20000  50.00000  3.40000\n"
    "END\n")
BASE = ("ensemble nvt\ntemperature 77\nnumsteps 1\ncorrtime 1\nbasis1 20 0 0\nbasis2 0 20 0\nbasis3 0 0 20\n"
        "pqr_input in.pqr\n")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    if not (os.path.exists(host.LIB_PATH) and os.path.exists(engine.LIB_PATH)):
        g.build()


def _setup(tmp_path, extra, pqr=PQR, name="in.pqr"):
    (tmp_path / name).write_text(pqr)
    (tmp_path / "input").write_text(BASE.replace("in.pqr", name) + extra)
    return host.load().setup_system(str(tmp_path / "input").encode())


def _at_flags(lib, p):
    out = np.zeros(2, dtype=np.int32)
    lib.host_get_at_flags(p, out.ctypes.data)
    return out.tolist()


def _c9(lib, p, n):
    out = np.zeros(n)
    lib.host_get_c9(p, out.ctypes.data)
    return out.tolist()


def test_keywords_and_c9_column_round_trip(tmp_path):
    lib = host.load()
    lib.write_molecules.argtypes = [C.c_void_p, C.c_char_p]
    p = _setup(tmp_path, "axilrod_teller on\nmidzuno_kihara_approx on\n")
    assert p
    assert _at_flags(lib, p) == [1, 1]
    # column 20, behind c10; absent columns read as 0
    assert _c9(lib, p, 4) == [518.3, 100.0, 0.0, 0.0]
    assert lib.host_unsupported(p) is None
    out = tmp_path / "out.pqr"
    assert lib.write_molecules(p, str(out).encode()) == 0
    lib.free_system(p)
    rows = [ln.split() for ln in out.read_text().splitlines() if ln.startswith("ATOM")]
    assert [len(r) for r in rows] == [20] * 4 and [float(r[19]) for r in rows] == [518.3, 100.0, 0.0, 0.0]
    q = _setup(tmp_path, "axilrod_teller on\n", pqr=out.read_text(), name="again.pqr")
    assert q and _at_flags(lib, q) == [1, 0] and _c9(lib, q, 4) == [518.3, 100.0, 0.0, 0.0]
    c6 = [np.zeros(4) for _ in range(3)]
    lib.host_get_dispersion(q, *[a.ctypes.data for a in c6])
    assert c6[0].tolist() == [64.3, 24.0, 24.0, 0.0]
    lib.free_system(q)


def test_keywords_default_to_off_and_reject_nonsense(tmp_path):
    lib = host.load()
    p = _setup(tmp_path, "")
    assert _at_flags(lib, p) == [0, 0] and lib.host_unsupported(p) is None
    lib.free_system(p)
    p = _setup(tmp_path, "axilrod_teller off\nmidzuno_kihara_approx off\n")
    assert _at_flags(lib, p) == [0, 0]
    lib.free_system(p)
    assert not _setup(tmp_path, "axilrod_teller maybe\n")


def test_other_refusals_still_name_themselves(tmp_path):
    lib = host.load()
    p = _setup(tmp_path, "axilrod_teller on\ndisp_expansion on\ndisp_expansion_mbvdw on\n")
    why = lib.host_unsupported(p)
    assert why is not None and "disp_expansion_mbvdw" in why.decode()
    lib.free_system(p)
    p = _setup(tmp_path, "axilrod_teller on\ndisp_expansion on\ngilbert_smith_mixing on\n")
    why = lib.host_unsupported(p)
    assert why is not None and "gilbert_smith_mixing" in why.decode()
    lib.free_system(p)
    p = _setup(tmp_path, "axilrod_teller on\ndisp_expansion on\n")
    assert lib.host_unsupported(p) is None
    lib.free_system(p)


def test_library_exports_the_two_entries_and_null_arguments_are_errors():
    lib = engine.load()
    for name in ("mpmc_hip_set_axilrod_teller", "mpmc_hip_get_three_body_energy"):
        assert hasattr(lib, name) and name in engine.EXPORTS
    assert lib.mpmc_hip_abi_version() == 1
    assert lib.mpmc_hip_set_axilrod_teller(None, 1, 0, None) != 0
    assert b"set_axilrod_teller" in lib.mpmc_hip_last_error()
    v = C.c_double(1.0)
    assert lib.mpmc_hip_get_three_body_energy(None, C.byref(v)) != 0
    assert b"get_three_body_energy" in lib.mpmc_hip_last_error()
    # the result record did not grow: the term has its own getter
    assert "three_body_energy" not in [f for f, _ in engine.Result._fields_]


def test_effective_c9_matches_the_reference_arithmetic():
    s = synth.s_at(40)
    assert np.array_equal(engine.effective_c9(s, False), ref.effective_c9(s, False))
    assert np.array_equal(engine.effective_c9(s, False), s["c9"])
    mk = engine.effective_c9(s, True)
    assert np.array_equal(mk, ref.effective_c9(s, True))
    i = int(np.flatnonzero(s["alpha"] != 0.0)[0])
    assert mk[i] == 3.0 / 4.0 * s["alpha"][i] * 6.7483345 * s["c6"][i] != 0.0
    assert np.all(mk[s["alpha"] == 0.0] == 0.0)


def test_config_text_and_arrays_carry_the_new_fields():
    flags = dict(synth.FLAGS_AT, midzuno_kihara_approx=1)
    txt = host.config_text(flags)
    assert "axilrod_teller on" in txt and "midzuno_kihara_approx on" in txt
    s = synth.s_at(30)
    h = host.HostSystem(s, flags)
    assert _at_flags(h.lib, h.ptr) == [1, 1]
    assert np.array_equal(np.array(_c9(h.lib, h.ptr, 30)), s["c9"])
    assert h.three_body_energy() == 0.0
    h.close()
    # make_params() leaves the three-body keys to set_axilrod_teller()
    assert engine.make_params(**flags).rd_only == 0
