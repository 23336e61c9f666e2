"""Register budget of the rd_crystal kernels, read from the code object inside libmpmc_hip.so as
tests/test_kernel_resources.py does (no GPU needed).  rdc_tile_kernel runs an fp64 division per image in its innermost
loop, up to 343 images per pair: a spill there is a scratch round trip per image."""
from test_kernel_resources import kernel_notes  # noqa: F401  (the module-scoped fixture)


def test_new_kernels_are_in_the_code_object_once(kernel_notes):
    assert sum("rdc_tile_kernel" in k for k in kernel_notes) == 1  # not a template: one instantiation
    assert sum("rdc_self_kernel" in k for k in kernel_notes) == 1
    # the kernels the other resource tests count are still that many
    assert sum("gs_block_inverse_kernel" in k for k in kernel_notes) == 6
    assert sum("gs_chain_kernel" in k for k in kernel_notes) == 2
    assert sum("disp_tile_kernel" in k for k in kernel_notes) == 1
    assert sum("disp_lrc_kernel" in k for k in kernel_notes) == 1
    assert sum("at_triple_kernel" in k for k in kernel_notes) == 1
    assert sum("lj_lrc_kernel" in k for k in kernel_notes) == 1


def test_no_scratch_and_no_spills(kernel_notes):
    hits = {k: v for k, v in kernel_notes.items() if "rdc_tile_kernel" in k or "rdc_self_kernel" in k}
    assert len(hits) == 2
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, (name, r)
    tile = [v for k, v in hits.items() if "rdc_tile_kernel" in k][0]
    assert tile["vgprs"] <= 128, tile  # two 8-wave workgroups per compute unit (512 / 4 registers a lane)
