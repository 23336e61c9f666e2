"""Register budget of the PHAHST kernels, read from the code object inside libmpmc_hip.so as tests/test_kernel_resources.py
does (no GPU needed).  disp_tile_kernel is a dense fp64 loop -- two exp, three sqrt, a reciprocal and an eleven-term
series per pair with the row atom's eight parameters live across it: a spill there is a scratch round trip per pair."""
import pytest

from test_kernel_resources import kernel_notes  # noqa: F401  (the module-scoped fixture)


def test_new_kernels_are_in_the_code_object(kernel_notes):
    assert sum("disp_tile_kernel" in k for k in kernel_notes) == 1
    assert sum("disp_lrc_kernel" in k for k in kernel_notes) == 1
    # the kernels tests/test_kernel_resources.py counts are still that many
    assert sum("gs_block_inverse_kernel" in k for k in kernel_notes) == 6
    assert sum("gs_chain_kernel" in k for k in kernel_notes) == 2


@pytest.mark.parametrize("kernel", ["disp_tile_kernel", "disp_lrc_kernel"])
def test_no_scratch_and_no_spilled_vector_registers(kernel_notes, kernel):
    hits = {k: v for k, v in kernel_notes.items() if kernel in k}
    assert hits
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0, (name, r)
        assert r["vgprs"] <= 128, (name, r)  # two 8-wave workgroups stay resident per compute unit
