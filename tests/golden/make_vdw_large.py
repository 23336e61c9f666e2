"""Writes tests/golden/vdw_large.npz: the recorded references of the large coupled-dipole cases of tests/vdw_cases.py (LARGE:
rows1023, rows1026, rows1029, big1, big2, frame), which tests/test_gpu_vdw_large.py holds the engine to and
tests/test_vdw_reference.py checks on the CPU.  Per case:

    <case>/sha256                         vdw_cases.input_hash of the inputs and the row count
    <case>/rows                           matrix rows of e_total
    <case>/<term>, <case>/abs_<term>      e_total, e_iso, lr_corr, repulsion, repulsion_lrc and the sums of |terms|: two
                                          float64 (hi, lo) whose longdouble sum is the longdouble value
    <case>/err_e_total, <case>/err_e_iso  the certified error of vdw_reference.prerotated_eigen_energy (e_iso: summed over
                                          the molecules; a block of at most 8 rows goes through the Jacobi iteration: 0)
    <case>/b_min, <case>/b_max            the extreme diagonal values of the rotated matrix of e_total

It imports nothing but the helpers of tests/ and needs no GPU:

    python tests/golden/make_vdw_large.py [case ...]

With case names it recomputes those and keeps the rest of the file.  Run time, one core of the development host (x86-64,
80-bit longdouble; the longdouble matrix products have no BLAS): rows1023 27 s, rows1026 26 s, rows1029 43 s, big1 31 s, big2 699 s,
frame 71 s (two matrices above 1024 rows) -- 15 minutes in all.
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                   # tests/: the helpers
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the package the cases take their system layout from

import numpy as np

import vdw_cases as vc
import vdw_reference as vr
from pair_reference import LD


def eigen_sum(C):
    """(e, err, info or None) of one matrix"""
    if C.shape[0] <= 8:
        return vr.eigen_energy(vr.jacobi_eigenvalues(C)), LD(0), None
    return vr.prerotated_eigen_energy(C)


def record(name):
    """the entries of one case, without the <case>/ prefix"""
    s, f = vc.large(name), vc.FLAGS
    C, idx = vr.c_matrix(s, f)
    rows = C.shape[0]
    assert rows == vc.LARGE_ROWS[name]
    et, err_t, info = eigen_sum(C)
    ei, err_i, cache = LD(0), LD(0), {}
    for t, atoms in vr.molecules(s):  # sum_eiso_vdw: the value of the first molecule of the type
        if t not in cache:
            cache[t] = eigen_sum(vr.c_matrix(s, f, atoms)[0])[:2] if vc.active_rows(s, atoms) else (LD(0), LD(0))
        ei += cache[t][0]
        err_i += cache[t][1]
    lr, lr_abs = vr.lr_corr(s, f)
    rep, rep_abs, margin = vr.repulsion(s, f)
    rl, rl_abs = vr.repulsion_lrc(s, f)
    assert margin >= 1e-9  # no Lennard-Jones pair within 1e-9 A of the cutoff
    vals = dict(e_total=et, e_iso=ei, lr_corr=lr, repulsion=rep, repulsion_lrc=rl, abs_e_total=et, abs_e_iso=ei,
                abs_lr_corr=lr_abs, abs_repulsion=rep_abs, abs_repulsion_lrc=rl_abs)
    out = {k: np.array([float(v), float(v - LD(float(v)))]) for k, v in vals.items()}
    out.update(err_e_total=np.float64(err_t), err_e_iso=np.float64(err_i), b_min=np.float64(info["b_min"]),
               b_max=np.float64(info["b_max"]), rows=np.int64(rows), sha256=np.array(vc.input_hash(s, rows)))
    print("%-9s rows %d e_total %.6f err/e %.2g e_iso %.6f err %.2g b_min/b_max %.3f off/|C| %.2g defect %.2g" % (
        name, rows, float(et), float(err_t / et), float(ei), float(err_i), float(info["b_min"] / info["b_max"]),
        float(info["off"] / info["norm"]), float(info["defect"])), flush=True)
    return out


if __name__ == "__main__":
    names = sys.argv[1:] or list(vc.LARGE)
    d = {}
    if sys.argv[1:] and os.path.exists(vc.GOLDEN_LARGE):
        with np.load(vc.GOLDEN_LARGE) as z:
            d = {k: z[k] for k in z.files}
    for name in names:
        t0 = time.time()
        for k, v in record(name).items():
            d["%s/%s" % (name, k)] = v
        print("%-9s %.0f s" % (name, time.time() - t0), flush=True)
    np.savez(vc.GOLDEN_LARGE, **d)
    print("wrote", vc.GOLDEN_LARGE, len(d), "entries")
