"""Register budget of the dimer kernels, read from the code object inside libmpmc_hip.so (no GPU needed): the three
instances of dimer_energy_kernel keep their per-site state in registers -- no scratch, no spilled vector registers -- and
their LDS stays within what DESIGN.md section 18 states (one wave per workgroup, 12 workgroups per compute unit by
registers)."""
import re

import pytest

from test_kernel_resources import kernel_notes  # noqa: F401  (the fixture that reads the code object's notes)


def test_dimer_kernels_are_in_the_code_object(kernel_notes):  # noqa: F811
    assert sum("dimer_energy_kernel" in k for k in kernel_notes) == 3  # exponential, linear, undamped tensor
    assert sum("dimer_rotate_kernel" in k for k in kernel_notes) == 1
    assert sum("dimer_mean_kernel" in k for k in kernel_notes) == 1


def test_dimer_energy_kernel_has_no_scratch(kernel_notes):  # noqa: F811
    for name, r in kernel_notes.items():
        if re.search("dimer_(energy|rotate|mean)_kernel", name):
            assert r["scratch"] == 0 and r["vgpr_spills"] == 0, (name, r)
            assert r["vgprs"] <= 168, (name, r)  # 3 waves per SIMD (512 / 168), 12 per compute unit
