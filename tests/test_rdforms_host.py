"""CPU-only checks of the plumbing of sg / dreiding / lj_buffered_14_7 and the Lennard-Jones mixing rules: the keywords
through the C host layer, the refusals by name, the new C-ABI entry and its parameter record."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from mpmc_amd import engine, host, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PQR = (
    "ATOM      1 H2G  H2  M    1      0.000   0.000   0.000   2.0160   0.0000  0.00000 34.20000  2.96000\n"
    "ATOM      2 H2G  H2  M    2      3.500   0.000   0.000   2.0160   0.0000  0.00000 34.20000  2.96000\n"
    "ATOM      3 C    MOF %s    3      5.000   5.000   5.000  12.0110   0.0000  1.20000 30.00000 %s\n"
    "ATOM      4 C    MOF %s    4      9.000   5.000   5.000  12.0110   0.0000  1.20000 30.00000  3.10000\n"
    "END\n")
BASE = ("ensemble nvt\ntemperature 77\nnumsteps 1\ncorrtime 1\nbasis1 20 0 0\nbasis2 0 20 0\nbasis3 0 0 20\n"
        "pqr_input in.pqr\n")
NAMES = ["sg", "dreiding", "lj_buffered_14_7", "waldmanhagler", "halgren_mixing", "c6_mixing"]


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as g

    if not (os.path.exists(host.LIB_PATH) and os.path.exists(engine.LIB_PATH)):
        g.build()


def _setup(tmp_path, extra, frozen=("M", "M"), sigma=" 3.10000"):
    (tmp_path / "in.pqr").write_text(PQR % (frozen[0], sigma, frozen[1]))
    (tmp_path / "input").write_text(BASE + extra)
    return host.load().setup_system(str(tmp_path / "input").encode())


def _flags(lib, p):
    out = np.zeros(6, dtype=np.int32)
    lib.host_get_rdform_flags(p, out.ctypes.data)
    return out.tolist()


def test_keywords_are_read_and_default_to_off(tmp_path):
    lib = host.load()
    p = _setup(tmp_path, "")
    assert _flags(lib, p) == [0] * 6 and lib.host_unsupported(p) is None
    lib.free_system(p)
    for k, name in enumerate(NAMES):
        p = _setup(tmp_path, "%s on\n" % name)
        assert p, name
        assert _flags(lib, p) == [int(j == k) for j in range(6)]
        assert lib.host_unsupported(p) is None, name
        lib.free_system(p)
        p = _setup(tmp_path, "%s on\n%s off\n" % (name, name))
        assert _flags(lib, p) == [0] * 6
        lib.free_system(p)
        assert not _setup(tmp_path, "%s maybe\n" % name)
    p = _setup(tmp_path, "dreiding on\nhalgren_mixing on\nfeynman_hibbs on\nfeynman_hibbs_order 2\n")
    assert _flags(lib, p) == [0, 1, 0, 0, 1, 0] and lib.host_unsupported(p) is None
    lib.free_system(p)


@pytest.mark.parametrize("two", [("waldmanhagler", "halgren_mixing"), ("waldmanhagler", "c6_mixing"),
                                 ("halgren_mixing", "c6_mixing")])
def test_two_mixing_rules_are_the_reference_input_error(tmp_path, two):
    (tmp_path / "in.pqr").write_text(PQR % ("M", " 3.10000", "M"))
    (tmp_path / "input").write_text(BASE + "%s on\n%s on\n" % two)
    r = subprocess.run([host.EXE_PATH, str(tmp_path / "input")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "INPUT: more than one mixing rule specified" in r.stdout + r.stderr  # check_input.c:1277-1281
    assert not _setup(tmp_path, "%s on\n%s on\n" % two)
    with pytest.raises(ValueError, match="more than one mixing rule specified"):
        engine.rd_form_of({two[0]: 1, two[1]: 1})


@pytest.mark.parametrize("extra,frozen,sigma,words", [
    ("sg on\nwaldmanhagler on\n", ("M", "M"), " 3.10000", ["sg with waldmanhagler", "ignores the mixing rule"]),
    ("sg on\nc6_mixing on\n", ("M", "M"), " 3.10000", ["sg with waldmanhagler", "c6_mixing"]),
    ("sg on\n", ("F", "F"), " 3.10000", ["sg with two or more frozen atoms"]),
    ("waldmanhagler on\n", ("M", "M"), "-3.10000", ["waldmanhagler with a negative sigma"]),
    ("dreiding on\nwaldmanhagler on\n", ("M", "M"), "-3.10000", ["waldmanhagler with a negative sigma"]),
    ("dreiding on\nrd_crystal on\nrd_crystal_order 2\n", ("M", "M"), " 3.10000", ["rd_crystal with sg / dreiding"]),
    ("c6_mixing on\nrd_crystal on\nrd_crystal_order 2\n", ("M", "M"), " 3.10000", ["rd_crystal with", "mixing rule"]),
    ("lj_buffered_14_7 on\ndisp_expansion on\n", ("M", "M"), " 3.10000", ["disp_expansion with sg / dreiding"]),
    ("sg on\npolarvdw on\npolar_damp_type exponential\npolar_damp 2.1304\npolar_max_iter 4\ncavity_autoreject_absolute on\ncavity_autoreject_scale 0.5\n",
     ("M", "M"), " 3.10000", ["polarvdw with sg / dreiding"]),
])
def test_each_named_refusal_is_hit(tmp_path, extra, frozen, sigma, words):
    lib = host.load()
    p = _setup(tmp_path, extra, frozen, sigma)
    assert p
    why = lib.host_unsupported(p)
    assert why is not None
    for w in words:
        assert w in why.decode(), why
    lib.free_system(p)


def test_what_is_allowed_is_not_refused(tmp_path):
    lib = host.load()
    for extra, frozen, sigma in (("sg on\n", ("F", "M"), " 3.10000"),  # one frozen atom: no frozen-frozen pair
                                 ("dreiding on\n", ("F", "F"), "-3.10000"),
                                 ("halgren_mixing on\n", ("F", "F"), "-3.10000"),
                                 ("lj_buffered_14_7 on\naxilrod_teller on\n", ("M", "M"), " 3.10000")):
        p = _setup(tmp_path, extra, frozen, sigma)
        assert p and lib.host_unsupported(p) is None, extra
        lib.free_system(p)


def test_library_exports_set_rd_form_and_the_record_matches(tmp_path):
    lib = engine.load()
    assert hasattr(lib, "mpmc_hip_set_rd_form") and "mpmc_hip_set_rd_form" in engine.EXPORTS
    assert lib.mpmc_hip_abi_version() == 1
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpmc_hip.h"\n'
                    'int main(void){printf("%zu %zu %zu %d %d %d %d %d %d %d %d %d\\n", sizeof(mpmc_hip_rd_form_params),'
                    ' offsetof(mpmc_hip_rd_form_params, form), offsetof(mpmc_hip_rd_form_params, mixing),'
                    ' MPMC_HIP_ABI_VERSION, MPMC_HIP_RD_LJ, MPMC_HIP_RD_SG, MPMC_HIP_RD_DREIDING, MPMC_HIP_RD_BUFFERED_14_7,'
                    ' MPMC_HIP_RD_MIX_LB, MPMC_HIP_RD_MIX_WALDMAN_HAGLER, MPMC_HIP_RD_MIX_HALGREN, MPMC_HIP_RD_MIX_C6);'
                    'return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    F, M = engine.RD_FORMS, engine.RD_MIXINGS
    assert got == [C.sizeof(engine.RdFormParams), engine.RdFormParams.form.offset, engine.RdFormParams.mixing.offset, 1,
                   F["lj"], F["sg"], F["dreiding"], F["lj_buffered_14_7"],
                   M["lb"], M["waldmanhagler"], M["halgren_mixing"], M["c6_mixing"]]
    assert [f for f, _ in engine.RdFormParams._fields_] == ["form", "mixing"] and F["off"] == 0
    # a null context is an error, not a crash
    assert lib.mpmc_hip_set_rd_form(None, None) != 0


def test_flag_sets_map_to_form_and_mixing():
    assert engine.rd_form_of({}) == ("off", "lb")
    assert engine.rd_form_of(dict(sg=1)) == ("sg", "lb")
    assert engine.rd_form_of(dict(dreiding=1, halgren_mixing=1)) == ("dreiding", "halgren_mixing")
    assert engine.rd_form_of(dict(lj_buffered_14_7=1, sg=0)) == ("lj_buffered_14_7", "lb")
    assert engine.rd_form_of(dict(waldmanhagler=1)) == ("lj", "waldmanhagler")
    assert engine.rd_form_of(dict(c6_mixing=1, halgren_mixing=0)) == ("lj", "c6_mixing")
    # make_params() leaves the keys to set_rd_form()
    assert engine.make_params(temperature=77.0, sg=1, c6_mixing=1).temperature == 77.0
    txt = host.config_text(dict(temperature=77.0, dreiding=1, waldmanhagler=1, sg=0))
    assert "dreiding on" in txt and "waldmanhagler on" in txt and "sg off" in txt


def test_host_system_from_arrays_carries_the_flags():
    s = synth.s_lj(30)
    h = host.HostSystem(s, dict(temperature=77.0, lj_buffered_14_7=1, halgren_mixing=1))
    assert _flags(h.lib, h.ptr) == [0, 0, 1, 0, 1, 0]
    h.close()
    with pytest.raises(Exception):
        host.HostSystem(s, dict(temperature=77.0, halgren_mixing=1, c6_mixing=1))
