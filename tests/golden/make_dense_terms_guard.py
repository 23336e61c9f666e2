"""Writes tests/golden/dense_terms_guard.npz, the fixture of
tests/test_gpu_tile_passes.py::test_dense_terms_give_the_bits_of_the_parent_commit: the result fields (and the three-body
energy) of the dense-term cases of tests/tile_pass_cases.py, at the first evaluation and after the multi-block move, and of
an LJ + Ewald + rd_lrc box before and after remove_molecule / insert_molecule.  It must be run on an MI355X with the package
of the commit BEFORE mpmc_amd/csrc/kernels_tile.h first on sys.path (a checkout of that commit, built):

    PYTHONPATH=<that checkout> python make_dense_terms_guard.py dense_terms_guard.npz
"""
import os
import sys

from mpmc_amd import engine

assert not os.path.exists(os.path.join(os.path.dirname(engine.__file__), "csrc", "kernels_tile.h")) and \
    not hasattr(engine, "NOT_PARAMS"), "this must be the parent commit's package"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # tests/: the cases

import numpy as np

import tile_pass_cases as tp

print("library:", engine.LIB_PATH)
d = {k: np.float64(v) if isinstance(v, float) else np.int64(v) for k, v in tp.guard_entries(engine).items()}
np.savez(sys.argv[1], **d)
for k in sorted(d):
    if k.endswith(":energy") or k.endswith(":three_body"):
        print("%-48s %.17g" % (k, d[k]))
print("wrote", sys.argv[1], len(d), "entries")
