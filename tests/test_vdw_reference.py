"""The longdouble reference of the coupled-dipole van der Waals mode (tests/vdw_reference.py) checked against independent
arithmetic on the CPU: its Jacobi eigenvalues against LAPACK in fp64 and against mpmath at 40 digits, its pair sums against
plain double loops, and the conditions the GPU parity cases rely on (tests/vdw_cases.py); the certified reference of the large
cases (prerotated_eigen_energy) against the Jacobi iteration, and its record tests/golden/vdw_large.npz against the inputs'
hashes, fp64 LAPACK and one full regeneration."""
import math

import numpy as np
import pytest

import vdw_cases as vc
import vdw_reference as vr
from pair_reference import LD, _molecule_index, minimum_image, pbc


def test_jacobi_against_lapack_fp64():
    s, f = vc.system("box43"), vc.FLAGS
    Cm, idx = vr.c_matrix(s, f)
    assert Cm.shape[0] == 3 * len(idx) and 60 <= Cm.shape[0] <= 129
    assert (Cm == Cm.T).all()
    lam = vr.jacobi_eigenvalues(Cm)
    w = np.linalg.eigvalsh(Cm.astype(np.float64))
    assert np.abs(lam.astype(np.float64) - w).max() <= 1e-14 * abs(w).max()
    a, b = float(np.sqrt(lam).sum()), float(np.sqrt(w).sum())
    assert abs(a - b) <= 1e-15 * b
    # the trace and the Frobenius norm are invariants the iteration must keep
    assert abs(lam.sum(dtype=LD) - np.trace(Cm)) <= 1e-17 * abs(np.trace(Cm)) * Cm.shape[0]
    assert abs((lam * lam).sum(dtype=LD) - (Cm * Cm).sum(dtype=LD)) <= 1e-17 * (Cm * Cm).sum(dtype=LD) * Cm.shape[0]


@pytest.mark.parametrize("name", ["box2", "clip"])
def test_jacobi_against_mpmath(name):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    Cm, _ = vr.c_matrix(vc.system(name), vc.flags_of(name))
    n = Cm.shape[0]
    assert 0 < n <= 30
    M = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            M[i, j] = mp.mpf(float(Cm[i, j])) + mp.mpf(float(Cm[i, j] - LD(float(Cm[i, j]))))
    E = sorted(mp.eigsy(M, eigvals_only=True))
    lam = vr.jacobi_eigenvalues(Cm)
    top = max(abs(float(e)) for e in E)
    for a, b in zip(lam, E):
        hi = float(a)
        assert abs((mp.mpf(hi) + mp.mpf(float(a - LD(hi)))) - b) <= 1e-17 * top
    want = sum(mp.sqrt(e) for e in E if e > 0)
    got = np.sqrt(np.where(lam < 0, LD(0), lam)).sum(dtype=LD)
    assert abs((mp.mpf(float(got)) + mp.mpf(float(got - LD(float(got))))) - want) <= 1e-17 * want


@pytest.mark.parametrize("n", vc.SITE_COUNTS)
def test_parity_cases_are_well_conditioned(n):
    s = vc.system("box%d" % n)
    ref = vc.reference("box%d" % n)
    lam = ref["lam"]
    assert len(lam) == 3 * int((vr.site_k(s) != 0).sum()) > 0
    assert lam.min() >= vc.COND * lam.max(), (float(lam.min()), float(lam.max()))
    assert ref["rimg_margin"] >= 1e-9  # no Lennard-Jones pair within 1e-9 A of the cutoff
    if n >= 21:  # the cases hold what they say they hold
        k = vr.site_k(s)
        assert (np.asarray(s["alpha"]) == 0).any() and ((np.asarray(s["omega"]) == 0) & (np.asarray(s["alpha"]) != 0)).any()
        assert np.asarray(s["frozen"]).any() and (k[np.asarray(s["frozen"]).astype(bool)] == 0).any()
        types = set(int(t) for t in s["mol_type"])
        assert {vc.TYPE_FRAME, vc.TYPE_FIVE, vc.TYPE_ONE}.issubset(types)
        assert float(ref["e_iso"]) > 0 and float(ref["lr_corr"]) < 0 and float(ref["repulsion"]) > 0


def test_clip_case_clips():
    lam = vc.reference("clip")["lam"]
    top = lam.max()
    assert (lam < -vc.COND * top).sum() >= 1
    assert not ((lam > 0) & (lam < vc.COND * top)).any()
    # the clipped sum differs from the unclipped magnitude sum: the clip matters
    assert float(vr.eigen_energy(lam)) < float(vr.CONV * np.sqrt(np.abs(lam)).sum(dtype=LD))


def test_e_iso_is_cached_per_type_from_the_first_molecule():
    s, f = vc.system("box22"), vc.FLAGS
    cache = {}
    total = vr.e_iso(s, f, cache)
    mols = vr.molecules(s)
    assert set(cache) == set(t for t, _ in mols)
    assert total == sum((cache[t] for t, _ in mols), LD(0))
    assert cache[vc.TYPE_ONE_NOALPHA] == 0 and cache[vc.TYPE_ONE_NOOMEGA] == 0  # dimension 0: no eigenvalue
    # a one-site molecule: three times omega, whatever alpha is
    want = 3 * vr.CONV * LD(0.62)
    assert abs(cache[vc.TYPE_ONE] - want) <= 4e-16 * want  # (k = sqrt(alpha) * omega is rounded to fp64, as in the reference)
    # moving a LATER molecule of a type changes nothing; a poisoned cache entry is used as it is
    five = [k for k, (t, _) in enumerate(mols) if t == vc.TYPE_FIVE]
    t2, _, _ = vc.moved(s, five[-1], (0.1, 0.0, 0.0), rot_seed=3)
    assert vr.e_iso(t2, f, dict(cache)) == total
    poisoned = dict(cache)
    poisoned[vc.TYPE_FIVE] = LD(1)
    assert vr.e_iso(s, f, poisoned) == total - len(five) * cache[vc.TYPE_FIVE] + len(five)


def test_pair_sums_against_double_loops():
    s, f = vc.system("box22"), vc.FLAGS
    ref = vc.reference("box22")
    pos, alpha, w = s["pos"], s["alpha"], s["omega"]
    eps, sig, frz = s["epsilon"], s["sigma"], np.asarray(s["frozen"]).astype(bool)
    mol = _molecule_index(s["molecule"])
    vol, rb, rc = pbc(s["basis"], 0.0)
    lr = rep = lrc = 0.0
    for i in range(len(pos)):
        if sig[i] != 0 and eps[i] != 0 and not frz[i]:
            lrc += 16.0 / 9.0 * math.pi * eps[i] * abs(sig[i]) ** 3 * (abs(sig[i]) / rc) ** 9 / vol
        for j in range(i + 1, len(pos)):
            if frz[i] and frz[j]:
                continue
            if alpha[i] != 0 and alpha[j] != 0 and w[i] != 0 and w[j] != 0:
                cC = 1.5 * 7.63822291e-12 * w[i] * w[j] / (w[i] + w[j]) * 4.13412763705e16 * alpha[i] * alpha[j]
                lr += -4.0 / 3.0 * math.pi * cC * rc ** -3 / vol
            if eps[i] != 0 and eps[j] != 0 and sig[i] != 0 and sig[j] != 0:
                e, sg = math.sqrt(eps[i] * eps[j]), 0.5 * (sig[i] + sig[j])
                lrc += 16.0 / 9.0 * math.pi * e * sg ** 3 * (sg / rc) ** 9 / vol
                if mol[i] != mol[j]:
                    _, _, rimg, _ = minimum_image(s["basis"], rb, (pos[i] - pos[j])[None, :])
                    if rimg[0] - 1e-12 < rc:
                        rep += 4.0 * e * (sg / rimg[0]) ** 12
    assert abs(lr - float(ref["lr_corr"])) <= 1e-13 * float(ref["abs_lr_corr"])
    assert abs(rep - float(ref["repulsion"])) <= 1e-13 * float(ref["abs_repulsion"])
    assert abs(lrc - float(ref["repulsion_lrc"])) <= 1e-13 * float(ref["abs_repulsion_lrc"])
    assert ref["vdw_energy"] == ref["e_total"] - ref["e_iso"] + ref["lr_corr"]


def test_contact_reference_counts():
    f = vc.FLAGS
    assert vr.close_contacts(vc.contacts(False, False, False), f, vc.SCALE)[0] == 0
    assert vr.close_contacts(vc.contacts(True, False, False), f, vc.SCALE)[0] == 1
    assert vr.close_contacts(vc.contacts(False, True, False), f, vc.SCALE)[0] == 0
    assert vr.close_contacts(vc.contacts(False, False, True), f, vc.SCALE)[0] == 1
    n, margin = vr.close_contacts(vc.system("contacts"), f, vc.SCALE)
    assert n == 2 and 0.5e-9 < margin < 2e-9  # the two edge pairs sit 1e-9 A from the scale, on either side
    for name in ("box43", "box130"):  # liquid density: nobody is that close
        assert vr.close_contacts(vc.system(name), f, vc.SCALE)[0] == 0


# ---- the certified reference of the large cases (vdw_reference.prerotated_eigen_energy) and its record
@pytest.mark.parametrize("n", vc.SITE_COUNTS)
def test_prerotated_reference_against_jacobi(n):
    name = "box%d" % n
    Cm, _ = vr.c_matrix(vc.system(name), vc.FLAGS)
    e, err, info = vr.prerotated_eigen_energy(Cm)
    want = vc.reference(name)["e_total"]  # eigen_energy(jacobi_eigenvalues(C))
    assert abs(e - want) <= err, (float(e - want), float(err))
    assert err <= 1e-2 * vc.TOL * e
    assert info["defect"] <= 1e-15 and info["b_min"] > 0 and info["off"] <= 1e-13 * info["norm"]


def test_prerotated_reference_refuses_a_spectrum_that_reaches_zero():
    Cm, _ = vr.c_matrix(vc.system("clip"), vc.CLIP_FLAGS)
    with pytest.raises(ValueError):
        vr.prerotated_eigen_energy(Cm)


_large_matrix = {}


def _large_eigvalsh(name):
    if name not in _large_matrix:
        Cm, _ = vr.c_matrix(vc.system(name), vc.FLAGS)
        _large_matrix[name] = np.linalg.eigvalsh(Cm.astype(np.float64))
    return _large_matrix[name]


@pytest.mark.parametrize("name", vc.LARGE)
def test_large_record_belongs_to_the_inputs(name):
    rec = vc.large_reference(name)
    s = vc.system(name)
    assert rec["rows"] == vc.LARGE_ROWS[name] == vc.active_rows(s)
    assert rec["sha256"] == vc.input_hash(s, rec["rows"])
    # what the sizes are for: trips of the 1024-thread loops of vdw_sum_kernel (k < n) and vdw_reflect_kernel (1 + tid < n - 1)
    trips = {"rows1023": (1, 1), "rows1026": (2, 1), "rows1029": (2, 2), "big1": (2, 2), "big2": (3, 3), "frame": (2, 2)}[name]
    assert (-(-rec["rows"] // 1024), -(-(rec["rows"] - 2) // 1024)) == trips
    if name == "frame":
        assert 1027 <= vc.FRAME_ROWS <= 1100 and rec["rows"] <= 1150
        assert float(rec["e_iso"]) > 0.95 * float(rec["e_total"])  # vdw_energy is their small difference


@pytest.mark.parametrize("name", vc.LARGE)
def test_large_record_against_lapack_fp64(name):
    rec = vc.large_reference(name)
    w = _large_eigvalsh(name)
    assert len(w) == rec["rows"] and w.min() >= vc.COND * w.max() and rec["b_min"] >= vc.COND * rec["b_max"]
    assert abs(w.min() - rec["b_min"]) <= 1e-12 * w.max() and abs(w.max() - rec["b_max"]) <= 1e-12 * w.max()
    e64 = vr.CONV * LD(float(np.sqrt(w).sum()))
    assert abs(e64 - rec["e_total"]) <= 1e-14 * rec["e_total"], float((e64 - rec["e_total"]) / rec["e_total"])
    assert 0 < rec["err_e_total"] <= 1e-2 * vc.TOL * float(rec["e_total"])
    assert 0 <= rec["err_e_iso"] <= 1e-2 * vc.TOL * float(rec["e_iso"])


def test_large_record_regenerated():
    """the one slow test of this file: rows1023 made again by the generator, whole, and compared with the file"""
    import importlib.util
    import os

    path = os.path.join(os.path.dirname(vc.GOLDEN_LARGE), "make_vdw_large.py")
    spec = importlib.util.spec_from_file_location("make_vdw_large", path)
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    new, rec = gen.record("rows1023"), vc.large_reference("rows1023")
    assert str(new["sha256"]) == rec["sha256"] and int(new["rows"]) == rec["rows"]
    for t in vc.LARGE_TERMS + tuple("abs_" + t for t in vc.LARGE_TERMS):
        v = LD(new[t][0]) + LD(new[t][1])
        # the eigenvalue sums start from LAPACK's basis, which may differ between builds: each is within its certified
        # error of the truth; the pair sums are the same longdouble operations
        if t in ("e_total", "e_iso"):
            slack = float(new["err_" + t]) + rec["err_" + t]
        else:
            slack = 1e-17 * abs(float(rec["abs_" + t.replace("abs_", "")]))
        assert abs(v - rec[t]) <= slack, (t, float(v - rec[t]), slack)
    assert abs(float(new["b_min"]) - rec["b_min"]) <= 1e-12 * rec["b_max"]
    assert float(new["err_e_total"]) <= 2 * rec["err_e_total"]
