"""Register budget of the kernels of mpmc_hip_set_rd_form, read from the code object inside libmpmc_hip.so as
tests/test_kernel_resources.py does (no GPU needed).  rdform_tile_kernel runs fp64 exponentials, divisions and a square
root per pair in its innermost loop: a spill there is a scratch round trip per pair."""
from test_kernel_resources import kernel_notes  # noqa: F401  (the module-scoped fixture)


def test_new_kernels_are_in_the_code_object_once_per_instantiation(kernel_notes):
    tile = [k for k in kernel_notes if "rdform_tile_kernel" in k]
    assert len(tile) == 4 and len(set(tile)) == 4  # LJ, SG, DREIDING, BUFFERED_14_7
    assert sum("rdform_lrc_kernel" in k for k in kernel_notes) == 1
    # the dense kernels the other resource tests count are still that many
    assert sum("disp_tile_kernel" in k for k in kernel_notes) == 1
    assert sum("disp_lrc_kernel" in k for k in kernel_notes) == 1
    assert sum("rdc_tile_kernel" in k for k in kernel_notes) == 1
    assert sum("lj_lrc_kernel" in k for k in kernel_notes) == 1
    assert sum("at_triple_kernel" in k for k in kernel_notes) == 1


def test_no_scratch_and_no_spills(kernel_notes):
    hits = {k: v for k, v in kernel_notes.items() if "rdform_tile_kernel" in k or "rdform_lrc_kernel" in k}
    assert len(hits) == 5
    for name, r in hits.items():
        # (the instantiations that mix park 4 scalar registers in vector lanes around pow(): no memory traffic)
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0, (name, r)
        assert r["vgprs"] <= 128, (name, r)  # two 8-wave workgroups per compute unit (512 / 4 registers a lane)
