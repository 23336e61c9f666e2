"""Register budget of the Axilrod-Teller kernel, read from the code object inside libmpmc_hip.so as
tests/test_kernel_resources.py does (no GPU needed).  at_triple_kernel keeps the (i, j) pair data of eight j atoms -- 32
doubles -- in registers across its k loop, next to an fp64 division per triple: a spill there is a scratch round trip in
the innermost loop of an O(N^3) sum."""
from test_kernel_resources import kernel_notes  # noqa: F401  (the module-scoped fixture)


def test_new_kernel_is_in_the_code_object_once(kernel_notes):
    assert sum("at_triple_kernel" in k for k in kernel_notes) == 1  # not a template: one instantiation
    # the kernels tests/test_kernel_resources.py and tests/test_phahst_resources.py count are still that many
    assert sum("gs_block_inverse_kernel" in k for k in kernel_notes) == 6
    assert sum("gs_chain_kernel" in k for k in kernel_notes) == 2
    assert sum("disp_tile_kernel" in k for k in kernel_notes) == 1
    assert sum("disp_lrc_kernel" in k for k in kernel_notes) == 1


def test_no_scratch_no_spills_and_the_designed_residency(kernel_notes):
    hits = {k: v for k, v in kernel_notes.items() if "at_triple_kernel" in k}
    assert hits
    for name, r in hits.items():
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0, (name, r)
        # designed for 4 waves per SIMD: two 8-wave workgroups resident per compute unit (512 / 4 = 128 registers a
        # lane; their 2 x 47 KB of LDS fit the 160 KB), so that one workgroup's table fill overlaps the other's triple loop
        assert r["vgprs"] <= 128, (name, r)
