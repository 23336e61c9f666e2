"""The host's step plans (mpmc_amd/csrc/step_plan.h: which chain data a move invalidates, the ranked walk, what each Jacobi
sweep's finish does, blocks_of, chunking, molecule placement; step_pods.h: the chain kernel's ticket count per block) on a CPU: tests/step_plan_check.cpp, a stand-alone program,
is compiled against the header alone -- plain host C++17, no HIP header -- with AddressSanitizer and UBSan, and run.  No GPU,
nothing loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mpmc_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "step_plan_check.cpp")
COMPILERS = ["g++", "/opt/rocm/lib/llvm/bin/clang++"]


@pytest.mark.parametrize("compiler", COMPILERS)
def test_step_plans_hold_their_descriptions(compiler, tmp_path):
    cxx = shutil.which(compiler)
    assert cxx, "no %s on this machine" % compiler
    exe = str(tmp_path / "step_plan_check")
    # (the sanitizer runtimes linked statically: the program is whole, whatever the environment it is started in loads)
    static = "-static-libasan" if compiler == "g++" else "-static-libsan"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", static, "-I", CSRC, "-o", exe, SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout


def test_the_header_needs_no_hip():
    for name in ("step_plan.h", "step_pods.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "__device__" not in text and "__global__" not in text, name
