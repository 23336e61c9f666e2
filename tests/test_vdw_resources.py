"""Register budget of the coupled-dipole van der Waals kernels (mpmc_amd/csrc/kernels_vdw.h), read from the code object
inside libmpmc_hip.so as tests/test_kernel_resources.py does (no GPU needed).  The Householder reduction launches
vdw_symv_kernel and vdw_rank2_kernel once per column of the matrix, thousands of times per energy(), and
vdw_bisect_kernel runs an fp64 division per matrix row and halving: a spill in any of them is a scratch round trip in an
innermost loop."""
from test_kernel_resources import kernel_notes  # noqa: F401  (the module-scoped fixture)

NEW_KERNELS = ["vdw_build_kernel", "vdw_reflect_kernel", "vdw_symv_kernel", "vdw_rank2_kernel", "vdw_bisect_kernel",
               "vdw_sum_kernel", "vdw_lrc_kernel", "rep_tile_kernel", "rep_lrc_kernel", "contact_tile_kernel"]


def test_new_kernels_are_in_the_code_object_once(kernel_notes):
    for name in NEW_KERNELS:
        assert sum(name in k for k in kernel_notes) == 1, name  # none is a template: one instantiation each
    # the kernels the other resource tests count are still that many
    assert sum("gs_block_inverse_kernel" in k for k in kernel_notes) == 6
    assert sum("gs_chain_kernel" in k for k in kernel_notes) == 2
    assert sum("disp_tile_kernel" in k for k in kernel_notes) == 1
    assert sum("disp_lrc_kernel" in k for k in kernel_notes) == 1
    assert sum("at_triple_kernel" in k for k in kernel_notes) == 1
    assert sum("rdc_tile_kernel" in k for k in kernel_notes) == 1
    assert sum("rdc_self_kernel" in k for k in kernel_notes) == 1
    assert sum("lj_lrc_kernel" in k for k in kernel_notes) == 1


def test_no_scratch_and_no_spills(kernel_notes):
    hits = {k: v for k, v in kernel_notes.items() if any(name in k for name in NEW_KERNELS)}
    assert len(hits) == len(NEW_KERNELS)
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, (name, r)
        assert r["vgprs"] <= 128, (name, r)  # at least four waves per SIMD
