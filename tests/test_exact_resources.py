"""Register budget of the exact-dipole kernels (mpmc_amd/csrc/kernels_exact.h), read from the code object inside
libmpmc_hip.so as tests/test_kernel_resources.py does (no GPU needed).  A factorization launches the diagonal, panel and
trailing kernels once per 64-row panel and the substitutions once per panel and direction: a spill in any of them is a
scratch round trip in a loop that runs hundreds of times per energy()."""
from test_kernel_resources import kernel_notes  # noqa: F401  (the module-scoped fixture)

# name -> instantiations: the substitution kernels and the right-hand-side kernel exist for 1 (E_static) and 3 (the
# tensor's unit fields) right-hand sides
NEW_KERNELS = {"chol_copy_kernel": 1, "chol_diag_kernel": 1, "chol_panel_kernel": 1, "chol_trail_kernel": 1,
               "chol_rhs_kernel": 2, "chol_fwd_kernel": 2, "chol_bwd_kernel": 2, "chol_energy_kernel": 1,
               "chol_tensor_kernel": 1}


def test_new_kernels_are_in_the_code_object(kernel_notes):
    for name, count in NEW_KERNELS.items():
        assert sum(name in k for k in kernel_notes) == count, name
    assert sum("chol_" in k for k in kernel_notes) == sum(NEW_KERNELS.values())
    for n in ("ILi1E", "ILi3E"):  # the template arguments, as mangled
        for name in ("chol_rhs_kernel", "chol_fwd_kernel", "chol_bwd_kernel"):
            assert sum(name + n in k for k in kernel_notes) == 1, (name, n)
    # the kernels the other resource tests count are still that many
    assert sum("gs_block_inverse_kernel" in k for k in kernel_notes) == 6
    assert sum("gs_chain_kernel" in k for k in kernel_notes) == 2
    assert sum("disp_tile_kernel" in k for k in kernel_notes) == 1
    assert sum("disp_lrc_kernel" in k for k in kernel_notes) == 1
    assert sum("at_triple_kernel" in k for k in kernel_notes) == 1
    assert sum("rdc_tile_kernel" in k for k in kernel_notes) == 1
    assert sum("rdc_self_kernel" in k for k in kernel_notes) == 1
    assert sum("lj_lrc_kernel" in k for k in kernel_notes) == 1
    for name in ("vdw_build_kernel", "vdw_reflect_kernel", "vdw_symv_kernel", "vdw_rank2_kernel", "vdw_bisect_kernel",
                 "vdw_sum_kernel", "vdw_lrc_kernel", "rep_tile_kernel", "rep_lrc_kernel", "contact_tile_kernel"):
        assert sum(name in k for k in kernel_notes) == 1, name
    # no older kernel's name contains a new one: the counts by substring stay what they were
    old = [k for k in kernel_notes if "chol_" not in k]
    for name in NEW_KERNELS:
        assert not any(name in k for k in old)


def test_no_scratch_and_no_spills(kernel_notes):
    hits = {k: v for k, v in kernel_notes.items() if "chol_" in k}
    assert len(hits) == sum(NEW_KERNELS.values())
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0 and r["sgpr_spills"] == 0, (name, r)
        if "chol_trail_kernel" in name:
            assert r["vgprs"] <= 256, (name, r)  # arch + acc registers: two waves per SIMD
        else:
            assert r["vgprs"] <= 128, (name, r)  # the project's bound: at least four waves per SIMD
