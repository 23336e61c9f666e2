"""How the binding (mpmc_amd/host/energy_hip.c) keeps the device in line with the molecule lists -- full upload, one-molecule
update, edit call or nothing; the order of the setters; the limits of the walk; the volume notes -- on a CPU:
tests/shim_sync_check.c, a stand-alone program, is compiled together with the binding against a recording engine, with
AddressSanitizer and UBSan, and run.  No GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "mpmc_amd", "host")
SRC = [os.path.join(ROOT, "tests", "shim_sync_check.c"), os.path.join(HOST, "energy_hip.c")]
COMPILERS = ["gcc", "/opt/rocm/lib/llvm/bin/clang"]


@pytest.mark.parametrize("compiler", COMPILERS)
def test_the_binding_sends_what_the_lists_ask_for(compiler, tmp_path):
    cc = shutil.which(compiler)
    assert cc, "no %s on this machine" % compiler
    exe = str(tmp_path / "shim_sync_check")
    # (the sanitizer runtimes linked statically: the program is whole, whatever the environment it is started in loads)
    static = "-static-libasan" if compiler == "gcc" else "-static-libsan"
    subprocess.check_call([cc, "-std=gnu99", "-O1", "-g", "-Wall", "-Werror", "-DMPMC_SHIM_HOST_MIRROR",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", static, "-I", os.path.join(ROOT, "include"),
                           "-I", HOST, "-o", exe] + SRC + ["-lm"])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout.endswith("every check held\n")


def test_the_binding_keeps_one_record_and_one_column_table():
    """what the walk and the upload read is named: no image member beside the column table, no literal column index, and
    nothing that an upload sends remembered outside the settings record"""
    import re

    text = open(SRC[1]).read()
    for name in ("x", "y", "z", "q", "alpha", "eps", "sig", "mass", "c6", "c8", "c10", "c9", "omega",
                 "params", "disp", "rd_form", "thole", "rdc_order", "vdw_on", "exact", "ar_scale"):
        assert not re.search(r"\bst->%s\b" % name, text), "st->%s" % name
    assert not re.search(r"\bbuf\[\d+\]\[", text) and not re.search(r"\bcol\[\d", text)
