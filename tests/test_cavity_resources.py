"""Register budget of the cavity-grid kernels (mpmc_amd/csrc/kernels_cavity.h), read from the code object inside
libmpmc_hip.so as tests/test_kernel_resources.py does (no GPU needed).  The update of the grid runs in every Monte Carlo
step of a cavity-biased chain; its kernels stage positions through LDS and must not touch scratch."""
from test_kernel_resources import kernel_notes  # noqa: F401  (the module-scoped fixture)

NEW_KERNELS = ("cavity_points_kernel", "cavity_bin_kernel", "cavity_edit_kernel", "cavity_scan_kernel",
               "cavity_scatter_kernel", "cavity_darts_kernel", "cavity_publish_kernel", "cavity_pick_kernel")


def test_new_kernels_are_in_the_code_object(kernel_notes):
    for name in NEW_KERNELS:  # no templates: one instantiation each
        assert sum(name in k for k in kernel_notes) == 1, name
    assert sum("cavity_" in k for k in kernel_notes) == len(NEW_KERNELS)
    # the kernels the other resource tests count are still that many
    assert sum("gs_block_inverse_kernel" in k for k in kernel_notes) == 6
    assert sum("gs_chain_kernel" in k for k in kernel_notes) == 2
    for name in ("disp_tile_kernel", "disp_lrc_kernel", "at_triple_kernel", "rdc_tile_kernel", "rdc_self_kernel",
                 "lj_lrc_kernel", "vdw_build_kernel", "vdw_reflect_kernel", "vdw_symv_kernel", "vdw_rank2_kernel",
                 "vdw_bisect_kernel", "vdw_sum_kernel", "vdw_lrc_kernel", "rep_tile_kernel", "rep_lrc_kernel",
                 "contact_tile_kernel", "chol_copy_kernel", "chol_diag_kernel", "chol_panel_kernel", "chol_trail_kernel",
                 "chol_energy_kernel", "chol_tensor_kernel"):
        assert sum(name in k for k in kernel_notes) == 1, name
    for name in ("chol_rhs_kernel", "chol_fwd_kernel", "chol_bwd_kernel"):
        assert sum(name in k for k in kernel_notes) == 2, name
    assert sum("chol_" in k for k in kernel_notes) == 12
    # no older kernel's name contains a new one, and no new name contains an older kernel's: counts by substring stay
    old = [k for k in kernel_notes if "cavity_" not in k]
    new = [k for k in kernel_notes if "cavity_" in k]
    for name in NEW_KERNELS:
        assert not any(name in k for k in old)
    for name in ("publish_result_kernel", "publish_side_kernel", "contact_tile_kernel"):
        assert not any(name in k for k in new)


def test_no_scratch_and_no_spills(kernel_notes):
    hits = {k: v for k, v in kernel_notes.items() if "cavity_" in k}
    assert len(hits) == len(NEW_KERNELS)
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, (name, r)
        assert r["vgprs"] <= 128, (name, r)  # the project's bound: at least four waves per SIMD
