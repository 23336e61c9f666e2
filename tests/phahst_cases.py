"""Inputs and flag sets shared by the PHAHST tests (a plain helper module): the smallest shapes that still take every
path of the dense tile kernel.

  c130  130 atoms, cubic 18 A cell: npad = 256, so four 64-blocks of which the third holds 2 atoms and the fourth none
        (padding, J < I tiles, empty tiles);
  c320  320 atoms, cubic 21.6 A cell: five blocks, three-site molecules straddling block borders, a frozen third;
  t130  the 130 atoms in a sheared triclinic cell (molecules moved rigidly with their lattice site).
The cutoff is half the shortest lattice vector, so about half of all pairs lie beyond it: a kernel that applied the
cutoff to the pair sum would lose them.
"""
import numpy as np

from mpmc_amd import synth

RD = dict(temperature=77.0, rd_only=1, disp_expansion=1)
VARIANTS = {
    "damp_extrapolate": dict(RD, damp_dispersion=1, extrapolate_disp_coeffs=1),
    "damp": dict(RD, damp_dispersion=1, extrapolate_disp_coeffs=0),
    "extrapolate": dict(RD, damp_dispersion=0, extrapolate_disp_coeffs=1),
    "plain": dict(RD, damp_dispersion=0, extrapolate_disp_coeffs=0),
    "schmidt": dict(RD, damp_dispersion=1, extrapolate_disp_coeffs=1, schmidt_mixing=1),
    "no_lrc": dict(RD, damp_dispersion=1, extrapolate_disp_coeffs=1, rd_lrc=0),
    "ewald": dict(temperature=77.0, disp_expansion=1, damp_dispersion=1, extrapolate_disp_coeffs=1),
    "polarizable": dict(synth.FLAGS_PHAHST),
}
INPUTS = ("c130", "c320", "t130")


def sheared(s):
    """The same molecules in a sheared cell: every molecule is moved rigidly so that its first atom keeps its fractional
    coordinates."""
    L = s["basis"][0, 0]
    basis = np.array([[L, 0.0, 0.0], [0.3 * L, L, 0.0], [0.2 * L, -0.15 * L, 0.9 * L]])
    mol = np.asarray(s["molecule"])
    first = np.concatenate([[0], np.flatnonzero(mol[1:] != mol[:-1]) + 1])
    anchor = s["pos"][first][np.cumsum(np.concatenate([[0], mol[1:] != mol[:-1]]))]
    out = dict(s)
    out["pos"] = (anchor / L) @ basis + (s["pos"] - anchor)
    out["basis"] = basis
    return out


_cache = {}


def system(name):
    if name not in _cache:
        _cache[name] = {"c130": lambda: synth.s_phahst(130), "c320": lambda: synth.s_phahst(320),
                        "t130": lambda: sheared(synth.s_phahst(130))}[name]()
    return _cache[name]


_ref = {}


def reference(name, variant):
    """phahst_reference.rd_terms of one case, computed once and shared (never modified)."""
    import phahst_reference as ph

    key = (name, variant)
    if key not in _ref:
        _ref[key] = ph.rd_terms(system(name), VARIANTS[variant])
    return _ref[key]


RD_TOL = 1e-12  # |rd_energy - reference| <= RD_TOL * sum |terms|
