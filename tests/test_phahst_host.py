"""CPU-only checks of the PHAHST plumbing: the keywords and PQR columns through the C host layer, the refusals of the
sub-flags the engine does not have, the new C-ABI entry and its parameter record."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mpmc_amd import engine, host, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PQR = (
    "ATOM      1 H2G  H2  M    1      0.000   0.000   0.000   2.0160  -0.7464  0.69380  3.50000  2.60000 0.0 0.0 9.0 160.0 4000.0\n"
    "ATOM      2 H2N  H2  M    1      0.363   0.000   0.000   0.0000   0.0000  0.00000  0.00000  0.00000 0.0 0.0 1.5 20.0\n"
    "ATOM      3 H2E  H2  M    1     -0.371   0.000   0.000   0.0000   0.7464  0.00044  0.00000  0.00000\n"
    "ATOM      4 C    MOF F    2      5.000   5.000   5.000  12.0110   0.0000  1.20000  3.20000  3.10000 0.0 0.0 25.0 600.0 18000.0\n"
    "END\n")
BASE = ("ensemble nvt\ntemperature 77\nnumsteps 1\ncorrtime 1\nbasis1 20 0 0\nbasis2 0 20 0\nbasis3 0 0 20\n"
        "pqr_input in.pqr\n")


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    if not (os.path.exists(host.LIB_PATH) and os.path.exists(engine.LIB_PATH)):
        g.build()


def _setup(tmp_path, extra):
    (tmp_path / "in.pqr").write_text(PQR)
    (tmp_path / "input").write_text(BASE + extra)
    return host.load().setup_system(str(tmp_path / "input").encode())


def _flags(lib, p):
    out = np.zeros(8, dtype=np.int32)
    lib.host_get_disp_flags(p, out.ctypes.data)
    return out.tolist()


def test_keywords_and_pqr_columns_are_read(tmp_path):
    lib = host.load()
    p = _setup(tmp_path, "disp_expansion on\ndamp_dispersion on\nextrapolate_disp_coeffs on\nschmidt_mixing on\n")
    assert p
    assert _flags(lib, p) == [1, 1, 1, 1, 0, 0, 0, 0]
    c6, c8, c10 = np.zeros(4), np.zeros(4), np.zeros(4)
    lib.host_get_dispersion(p, c6.ctypes.data, c8.ctypes.data, c10.ctypes.data)
    # columns 17-19 (after omega and gwp_alpha); absent columns read as 0
    assert c6.tolist() == [9.0, 1.5, 0.0, 25.0]
    assert c8.tolist() == [160.0, 20.0, 0.0, 600.0]
    assert c10.tolist() == [4000.0, 0.0, 0.0, 18000.0]
    assert lib.host_unsupported(p) is None
    lib.free_system(p)


def test_keywords_default_to_off_and_take_off(tmp_path):
    lib = host.load()
    p = _setup(tmp_path, "")
    assert _flags(lib, p) == [0] * 8 and lib.host_unsupported(p) is None
    lib.free_system(p)
    p = _setup(tmp_path, "disp_expansion on\ndamp_dispersion off\nschmidt_mixing off\n")
    assert _flags(lib, p) == [1, 0, 0, 0, 0, 0, 0, 0]
    lib.free_system(p)
    assert not _setup(tmp_path, "disp_expansion maybe\n")


@pytest.mark.parametrize("flag", ["disp_expansion_mbvdw", "gilbert_smith_mixing", "bohm_ahlrichs_mixing",
                                  "wilson_popelier_mixing"])
def test_refused_sub_flag_gives_its_message(tmp_path, flag):
    lib = host.load()
    p = _setup(tmp_path, "disp_expansion on\n%s on\n" % flag)
    assert p
    why = lib.host_unsupported(p)
    assert why is not None and flag in why.decode() and "not on the device" in why.decode()
    lib.free_system(p)


def test_library_exports_set_dispersion_and_the_record_matches(tmp_path):
    lib = engine.load()
    assert hasattr(lib, "mpmc_hip_set_dispersion") and "mpmc_hip_set_dispersion" in engine.EXPORTS
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpmc_hip.h"\n'
                    'int main(void){printf("%zu %zu %d\\n", sizeof(mpmc_hip_disp_params),'
                    ' offsetof(mpmc_hip_disp_params, schmidt_mixing), MPMC_HIP_ABI_VERSION);return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(engine.DispParams), engine.DispParams.schmidt_mixing.offset, 1]
    assert [f for f, _ in engine.DispParams._fields_] == ["disp_expansion", "damp_dispersion", "extrapolate_disp_coeffs",
                                                          "schmidt_mixing"]
    # a null context is an error, not a crash
    assert lib.mpmc_hip_set_dispersion(None, None, 0, None, None, None) != 0


def test_config_text_and_arrays_carry_the_new_fields():
    txt = host.config_text(synth.FLAGS_PHAHST)
    assert "disp_expansion on" in txt and "damp_dispersion on" in txt and "schmidt_mixing off" in txt
    s = synth.s_phahst(30)
    h = host.HostSystem(s, synth.FLAGS_PHAHST)
    c6, c8, c10 = np.zeros(30), np.zeros(30), np.zeros(30)
    h.lib.host_get_dispersion(h.ptr, c6.ctypes.data, c8.ctypes.data, c10.ctypes.data)
    assert np.array_equal(c6, s["c6"]) and np.array_equal(c8, s["c8"]) and np.array_equal(c10, s["c10"])
    assert _flags(h.lib, h.ptr)[:4] == [1, 1, 1, 0]
    h.close()
    # make_params() leaves the dispersion keys to set_dispersion()
    assert engine.make_params(**synth.FLAGS_PHAHST).polarization == 1
