"""Register, scratch and LDS budget of the trial-placement kernels, read from the code object inside libmpmc_hip.so (no
GPU needed): the figures DESIGN.md section 19 states.  trial_pair_kernel keeps a partner atom and one site's pair terms in
registers -- no scratch, no spilled vector register -- and 960 bytes of LDS (16 sites x 7 doubles + the wave sums), so by
registers three (feynman_hibbs 4) or four workgroups of 4 waves share a compute unit.  The VGPR counts are held at the
figures the document states, so that a change of them is seen and the document follows."""
import os
import re
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM, kernel_notes  # noqa: F401  (the fixture that reads the code object's notes)

KERNELS = {  # name: (instances, VGPRs per instance in the order of the template argument, LDS bytes): DESIGN.md section 19
    "trial_pair_kernelILi": (3, {"ILi0E": 109, "ILi2E": 115, "ILi4E": 141}, 960),  # feynman_hibbs off / 2 / 4
    "trial_recip_prepare_kernel": (1, {"": 78}, 4096),
    "trial_recip_kernel": (1, {"": 70}, 512),
    "trial_assemble_kernel": (1, {"": 14}, 0),
}
VGPR_CEILING = 168  # 3 waves per SIMD: what the mapping needs whatever a later compiler allocates


@pytest.fixture(scope="module")
def lds_bytes(tmp_path_factory):
    d = tmp_path_factory.mktemp("codeobj_trial")
    fat, co = str(d / "fat.bin"), str(d / "mpmc.co")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", LIB, fat])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co, "--unbundle"])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    out = {}
    for block in text.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", block).group(1))
    return out


def test_trial_kernels_are_in_the_code_object(kernel_notes):  # noqa: F811
    for kernel, (instances, _, _) in KERNELS.items():
        assert sum(kernel in k for k in kernel_notes) == instances, kernel


def test_trial_kernels_have_no_scratch_and_hold_the_stated_figures(kernel_notes, lds_bytes):  # noqa: F811
    seen = 0
    for name, r in kernel_notes.items():
        for kernel, (_, vgprs, lds) in KERNELS.items():
            if kernel in name:
                seen += 1
                assert r["scratch"] == 0 and r["vgpr_spills"] == 0, (name, r)
                want = [v for tag, v in vgprs.items() if tag in name]
                assert len(want) == 1 and r["vgprs"] == want[0] <= VGPR_CEILING, (name, r)
                assert lds_bytes[name] == lds, (name, lds_bytes[name])
    assert seen == 6
