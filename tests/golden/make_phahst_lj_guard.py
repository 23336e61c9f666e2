"""Writes tests/golden/phahst_lj_guard.npz, the fixture of
tests/test_gpu_phahst.py::test_lennard_jones_results_are_those_of_the_parent_commit: the result fields of an LJ + Ewald +
Jacobi box of 320 atoms before and after three single-molecule moves.  It must be run on an MI355X with the package of the
commit BEFORE the disp_expansion term first on sys.path (a checkout of that commit, built):

    PYTHONPATH=<that checkout> python make_phahst_lj_guard.py phahst_lj_guard.npz
"""
import sys

import numpy as np

out = sys.argv[1]
from mpmc_amd import engine, synth

print("library:", engine.LIB_PATH)
assert not hasattr(engine, "DispParams"), "this must be the parent commit's package"
s, flags = synth.s_pol(320), dict(synth.FLAGS_POL_JACOBI)
e = engine.Engine(320)
e.load_system(s, flags)
first = e.energy()
rng = np.random.default_rng(3)
pos = s["pos"].copy()
for k in (7, 23, 41):
    new = pos[5 * k:5 * k + 5] + rng.uniform(-0.1, 0.1, 3)
    pos[5 * k:5 * k + 5] = new
    e.update_atoms(5 * k, new)
    last = e.energy()
dip = e.dipoles()
e.close()
d = {"first_" + k: np.float64(v) if isinstance(v, float) else np.int64(v) for k, v in first.items()}
d.update({"last_" + k: np.float64(v) if isinstance(v, float) else np.int64(v) for k, v in last.items()})
d.update(mu=dip["mu"], ef_static=dip["ef_static"])
np.savez(out, **d)
print("wrote", out, first["energy"], last["energy"])
