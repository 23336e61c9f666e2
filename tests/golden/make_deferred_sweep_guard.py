"""Writes tests/golden/deferred_sweep_guard.npz, the fixture of tests/test_gpu_deferred_sweep.py: the energies of the solver
modes the deferred last sweep does NOT apply to (tests/deferred_sweep_cases.py, EXCLUDED) and the headline flags' energies
and dipoles at 2300 and 2560 atoms, as the commit BEFORE the deferral computes them.  It must be run on an MI355X with the
package of that commit first on sys.path (a checkout of it, built):

    PYTHONPATH=<that checkout> python make_deferred_sweep_guard.py deferred_sweep_guard.npz
"""
import os
import sys

from mpmc_amd import engine

_CSRC = os.path.join(os.path.dirname(engine.__file__), "csrc")
assert "defer_last_sweep" not in open(os.path.join(_CSRC, "engine_polar.inc")).read(), \
    "this must be the parent commit's package"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # tests/: the cases

import numpy as np

import deferred_sweep_cases as dc

print("library:", engine.LIB_PATH)
d = {}
for k, v in dc.guard_entries(engine).items():
    d[k] = v if isinstance(v, np.ndarray) else (np.float64(v) if isinstance(v, float) else np.int64(v))
np.savez(sys.argv[1], **d)
for k in sorted(d):
    if k.endswith(":polarization_energy") or k.endswith(":polar_iterations"):
        print("%-48s %.17g" % (k, d[k]))
print("wrote", sys.argv[1], len(d), "entries")
