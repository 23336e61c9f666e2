"""Inputs shared by tests/test_gpu_deferred_sweep.py and tests/golden/make_deferred_sweep_guard.py.

A fixed-count plain Jacobi solve on a view of 22 blocks or more launches n - 1 of its n sweeps and takes U_pol from
    -1/2 sum mu_0.E + 1/2 (T mu_0).mu_{n-1}
(DESIGN.md section 3); the last sweep runs when somebody asks for the dipoles.  Shapes: S-POL(2300) has 1380
polarizable sites = 22 blocks, the last one ragged (36 sites): the smallest view the rule applies to on a 256-CU
device; S-POL(2560) has 1536 = 24 full blocks.
"""
import numpy as np

from mpmc_amd import synth

SIZES = (2300, 2560)
# the headline's flags (bench.py, pcn61_4096) on the synthetic boxes
FLAGS = dict(temperature=77.0, polarization=1, polar_damp=2.1304, polar_max_iter=4, feynman_hibbs=1,
             feynman_hibbs_order=4)
# the same call sequence on the untouched path: polar_rrms runs all n sweeps and the old sum
FLAGS_ALL_SWEEPS = dict(FLAGS, polar_rrms=1)

# what keeps a solve on the old path (test 4); pair_coefficients is an engine option, the rest are flags
EXCLUDED = {
    "gamma_1.03": (dict(FLAGS, polar_gamma=1.03), {}),
    "sor": (dict(FLAGS, polar_sor=1, polar_gamma=0.9), {}),
    "palmo": (dict(FLAGS, polar_palmo=1), {}),
    "precision": (dict(FLAGS, polar_max_iter=0, polar_precision=1e-4), {}),
    "expanded_matrix": (dict(FLAGS), {"pair_coefficients": 0}),
}


def system(n):
    return synth.s_pol(n)


def blocks(s):
    return (int(np.count_nonzero(np.asarray(s["alpha"]) != 0.0)) + 63) // 64


def molecule_move(s, k, shift=(0.11, -0.07, 0.05)):
    """(first, new positions) of the k-th five-site molecule displaced rigidly"""
    first = 5 * k
    return first, np.asarray(s["pos"])[first:first + 5] + np.asarray(shift)


def big_move(s, first=40, count=40, shift=(0.03, 0.02, -0.04)):
    """more atoms than the engine's move list holds (32): update_atoms copies them at once"""
    return first, np.asarray(s["pos"])[first:first + count] + np.asarray(shift)


def moved(s, first, new):
    out = dict(s)
    out["pos"] = np.array(s["pos"], dtype=np.float64, copy=True)
    out["pos"][first:first + len(new)] = new
    return out


ENERGY_KEYS = ("energy", "rd_energy", "coulombic_energy", "polarization_energy", "polar_iterations")


def guard_entries(engine):
    """{key: value} of everything tests/golden/deferred_sweep_guard.npz holds: the energies of the excluded modes at 2560
    atoms (first evaluation and after a one-molecule move), and the headline flags' energies and dipoles at both sizes."""
    out = {}
    s = system(2560)
    first, new = molecule_move(s, 100)
    for name, (flags, opts) in sorted(EXCLUDED.items()):
        e = engine.Engine(2560)
        e.load_system(s, flags)
        for k, v in opts.items():
            e.set_option(k, v)
        for tag in ("first", "moved"):
            if tag == "moved":
                e.update_atoms(first, new)
            r = e.energy()
            for f in ENERGY_KEYS:
                out["%s:%s:%s" % (name, tag, f)] = r[f]
        e.close()
    for n in SIZES:
        s = system(n)
        first, new = molecule_move(s, 100)
        e = engine.Engine(n)
        e.load_system(s, FLAGS)
        for tag in ("first", "moved"):
            if tag == "moved":
                e.update_atoms(first, new)
            r = e.energy()
            for f in ENERGY_KEYS:
                out["headline_%d:%s:%s" % (n, tag, f)] = r[f]
            out["headline_%d:%s:mu" % (n, tag)] = e.dipoles()["mu"]
        e.close()
    return out
