"""GPU tests of polarvdw, the coupled-dipole many-body van der Waals mode: the kernels of mpmc_amd/csrc/kernels_vdw.h through
mpmc_hip_set_vdw, against tests/vdw_reference.py (longdouble, Jacobi eigenvalues).

Tolerance of every term: 1e-12 * sum |terms|, the project's convention.  For e_total and e_iso the terms are the
au2invsec * halfHBAR * sqrt(lambda_i), all positive.  The worst-case backward error of Householder + bisection at n = 390
is about 390 * 2^-53 = 4e-14 of the largest eigenvalue, and the parity cases keep lambda_min >= 1e-3 lambda_max (asserted
on the reference's eigenvalues), so the square roots do not amplify it: the tolerance has 25x over the bound.
"""
import numpy as np
import pytest

import vdw_cases as vc
import vdw_reference as vr
from mpmc_amd import engine
from pair_reference import _molecule_index

pytestmark = pytest.mark.gpu
FIELDS = [f for f, _ in engine.Result._fields_]
TERMS = engine.VDW_TERMS


def _engine(s, flags, cap=None):
    e = engine.Engine(cap or len(s["charge"]))
    e.load_system(s, flags)
    return e


def _all(e, r=None):
    """result fields + the mode's terms + vdw_energy of the last call"""
    r = e.energy() if r is None else r
    return dict(r, vdw_energy=e.vdw_energy(), **e.vdw_terms())


def _fresh(s, flags):
    e = _engine(s, flags)
    out = _all(e)
    e.close()
    return out


def _check(got, ref, what):
    worst = 0.0
    for t in TERMS:
        want, tol = float(ref[t]), vc.TOL * float(ref["abs_" + t])
        err = abs(got[t] - want)
        print("%s: %-13s %.10f reference %.10f |diff| %.3g tol %.3g (%.3g of it)" % (what, t, got[t], want, err, tol,
                                                                                    err / tol if tol else 0.0))
        assert err <= tol, (what, t, got[t], want, err, tol)
        worst = max(worst, err / tol if tol else 0.0)
    tol = vc.TOL * float(ref["abs_e_total"] + ref["abs_e_iso"] + ref["abs_lr_corr"])
    assert abs(got["vdw_energy"] - float(ref["vdw_energy"])) <= tol
    tol = vc.TOL * float(ref["abs_repulsion"] + ref["abs_repulsion_lrc"])
    assert abs(got["rd_energy"] - float(ref["rd_energy"])) <= tol
    assert got["status"] == 0
    return worst


@pytest.mark.parametrize("n", vc.SITE_COUNTS)
def test_terms_against_the_reference(n):
    name = "box%d" % n
    ref = vc.reference(name)
    lam = ref["lam"]
    assert lam.min() >= vc.COND * lam.max()  # the condition the tolerance rests on
    got = _fresh(vc.system(name), vc.FLAGS)
    worst = _check(got, ref, "%s (matrix %d)" % (name, len(lam)))
    print("%s: worst term at %.3g of the tolerance" % (name, worst))


def test_negative_eigenvalues_are_clipped():
    ref = vc.reference("clip")
    lam, top = ref["lam"], ref["lam"].max()
    assert (lam < -vc.COND * top).sum() >= 1 and not ((lam > 0) & (lam < vc.COND * top)).any()
    got = _fresh(vc.system("clip"), vc.CLIP_FLAGS)
    _check(got, ref, "clip")
    unclipped = float(vr.CONV * np.sqrt(np.abs(lam)).sum())
    assert abs(got["e_total"] - unclipped) > 1e-3 * unclipped  # |lambda| instead of the clip would be far off


def test_rd_only_and_no_lrc():
    s, ref = vc.system("box43"), vc.reference("box43")
    got = _fresh(s, dict(vc.FLAGS, rd_lrc=0))
    assert got["lr_corr"] == 0.0 and got["repulsion_lrc"] == 0.0
    assert abs(got["e_total"] - float(ref["e_total"])) <= vc.TOL * float(ref["abs_e_total"])
    assert got["vdw_energy"] == (got["e_total"] - got["e_iso"]) + 0.0
    got = _fresh(s, dict(vc.FLAGS, rd_only=1))  # vdw() is not called under rd_only; Lennard-Jones is still repulsion only
    assert got["vdw_energy"] == 0.0 and got["e_total"] == 0.0 and got["e_iso"] == 0.0 and got["lr_corr"] == 0.0
    assert abs(got["repulsion"] - float(ref["repulsion"])) <= vc.TOL * float(ref["abs_repulsion"])
    assert got["energy"] == got["rd_energy"] == got["repulsion"] + got["repulsion_lrc"]


def test_two_fresh_contexts_agree_to_the_bit():
    a, b = _fresh(vc.system("box130"), vc.FLAGS), _fresh(vc.system("box130"), vc.FLAGS)
    assert a == b


def _later_molecule(s, kind):
    """index (upload order) of the LAST molecule of a type: e_iso comes from the first one"""
    mols = vr.molecules(s)
    hits = [k for k, (t, _) in enumerate(mols) if t == kind]
    assert len(hits) >= 2
    return hits[-1]


@pytest.mark.parametrize("name", ["box70", "box130"])
def test_update_atoms_leaves_the_bits_of_a_fresh_context(name):
    s = vc.system(name)
    e = _engine(s, vc.FLAGS)
    before = _all(e)
    for step, (kind, shift, rot) in enumerate([(vc.TYPE_FIVE, (0.21, -0.13, 0.08), 11), (vc.TYPE_ONE, (-0.3, 0.2, 0.1), None)]):
        s, first, pos = vc.moved(s, _later_molecule(s, kind), shift, rot)
        e.update_atoms(first, pos)
        got = _all(e)
        want = _fresh(s, vc.FLAGS)
        assert got == want, (name, step, {k: (got[k], want[k]) for k in got if got[k] != want[k]})
        assert got["e_total"] != before["e_total"] and got["repulsion"] != before["repulsion"]
        assert got["e_iso"] == before["e_iso"] and got["lr_corr"] == before["lr_corr"]
    # nothing moved: the same record again
    assert _all(e) == got
    e.close()


def test_scale_box_leaves_the_bits_of_a_fresh_context():
    s = vc.system("box70")
    e = _engine(s, vc.FLAGS)
    before = _all(e)
    mol = _molecule_index(s["molecule"])
    first = np.array([np.flatnonzero(mol == m)[0] for m in range(mol.max() + 1)])
    basis = np.asarray(s["basis"]) * 1.01
    delta = 0.01 * s["pos"][first]
    assert e.scale_box(basis, delta)
    t = dict(s, basis=basis, pos=s["pos"] + delta[mol])
    got, want = _all(e), _fresh(t, vc.FLAGS)
    # e_iso is the value the context keeps per type (vdw.c:262-320), made in the cell of the first call; a fresh context
    # makes it in the new cell, and the framework molecule's own sub-block holds minimum-image distances across the cell
    # (kept as the reference has it: its cache outlives a volume move too).  Every other term is a function of the present
    # configuration alone.
    kept = ("e_iso", "vdw_energy", "energy")
    diff = {k: (got[k], want[k]) for k in got if got[k] != want[k] and k not in kept}
    assert not diff, diff
    assert got["lr_corr"] != before["lr_corr"] and got["repulsion_lrc"] != before["repulsion_lrc"]
    assert got["e_iso"] == before["e_iso"]
    assert got["vdw_energy"] == (got["e_total"] - got["e_iso"]) + got["lr_corr"]
    e.close()


def test_energy_begin_end_is_energy():
    s = vc.system("box43")
    e = _engine(s, vc.FLAGS)
    one = _all(e)
    s2, first, pos = vc.moved(s, _later_molecule(s, vc.TYPE_FIVE), (0.1, 0.1, -0.1), 5)
    e.update_atoms(first, pos)
    e.energy_begin()
    with pytest.raises(engine.EngineError):
        e.vdw_energy()
    two = _all(e, e.energy_end())
    e.close()
    assert two == _fresh(s2, vc.FLAGS) and two != one


def test_energy_is_the_sum_of_the_published_terms():
    e = _engine(vc.system("box70"), vc.FLAGS)
    r = _all(e)
    e.close()
    assert r["vdw_energy"] == (r["e_total"] - r["e_iso"]) + r["lr_corr"]
    assert r["rd_energy"] == r["repulsion"] + r["repulsion_lrc"]
    assert r["coulombic_energy"] != 0.0 and r["polarization_energy"] != 0.0
    assert r["energy"] == ((r["rd_energy"] + r["coulombic_energy"]) + r["polarization_energy"]) + r["vdw_energy"]


def test_mode_off_again_is_a_context_that_never_had_it():
    s = vc.system("box70")
    plain = {k: v for k, v in vc.FLAGS.items() if k != "polarvdw"}
    never = _engine(s, plain)
    want, want_dip = _all(never), never.dipoles()
    e = _engine(s, vc.FLAGS)
    on, on_dip = _all(e), e.dipoles()
    # in the mode: no device-side insert (the caller uploads again)
    one = dict(pos=s["pos"][-1:] + 0.5, charge=[0.0], alpha=[1.1], epsilon=[35.0], sigma=[3.1], mass=[16.0])
    assert e.insert_molecule(**one) is None
    e.set_vdw(s, enable=False)
    off, off_dip = _all(e), e.dipoles()
    assert off == want, {k: (off[k], want[k]) for k in off if off[k] != want[k]}
    assert off["vdw_energy"] == 0.0 and all(off[t] == 0.0 for t in TERMS)
    for k in want_dip:
        assert np.array_equal(off_dip[k], want_dip[k]) and np.array_equal(on_dip[k], want_dip[k]), k
    for fld in FIELDS:  # the mode changes rd_energy and energy, nothing else
        if fld not in ("energy", "rd_energy"):
            assert on[fld] == want[fld], fld
    assert on["rd_energy"] != want["rd_energy"]
    big = engine.Engine(len(s["charge"]) + 8)
    big.load_system(s, vc.FLAGS)
    big.energy()
    assert big.insert_molecule(**one) is None
    big.set_vdw(s, enable=False)
    big.energy()
    assert big.insert_molecule(**one) is not None  # ... and after the mode it answers 0 again
    for x in (never, e, big):
        x.close()


def test_e_iso_survives_a_new_upload_while_the_mode_stays_on():
    s = vc.system("box22")
    mols = vr.molecules(s)
    first_five = [k for k, (t, _) in enumerate(mols) if t == vc.TYPE_FIVE][0]
    t, _, _ = vc.moved(s, first_five, (0.05, 0.0, 0.0), rot_seed=9)  # the first molecule of the type, turned
    e = _engine(s, vc.FLAGS)
    a = _all(e)
    e.upload(t)
    e.set_vdw(t)
    b = _all(e)
    assert b["e_iso"] == a["e_iso"] and b["e_total"] != a["e_total"]
    ref = vr.vdw_terms(t, vc.FLAGS)
    assert abs(b["e_total"] - float(ref["e_total"])) <= vc.TOL * float(ref["abs_e_total"])
    # an upload WITHOUT the call returns the context to Lennard-Jones and the values go
    e.upload(t)
    lj = _all(e)
    assert lj["vdw_energy"] == 0.0 and lj["e_iso"] == 0.0
    e.set_vdw(t)
    c = _all(e)
    fresh = _fresh(t, vc.FLAGS)
    e.close()
    assert c == fresh, {k: (c[k], fresh[k]) for k in c if c[k] != fresh[k]}


def test_refused_combinations_are_named():
    s = dict(vc.system("box22"))
    n = len(s["charge"])
    s.update(c6=np.full(n, 5.0), c8=np.full(n, 50.0), c10=np.full(n, 500.0), c9=np.full(n, 100.0))
    e = _engine(s, vc.FLAGS)
    e.set_dispersion(s, disp_expansion=1)
    with pytest.raises(engine.EngineError, match="mpmc_hip_set_dispersion"):
        e.energy()
    e.set_dispersion(s, disp_expansion=0)
    e.set_rd_crystal(2)
    with pytest.raises(engine.EngineError, match="mpmc_hip_set_rd_crystal"):
        e.energy()
    e.set_rd_crystal(0)
    e.set_axilrod_teller(s)
    with pytest.raises(engine.EngineError, match="mpmc_hip_set_axilrod_teller"):
        e.energy()
    e.set_axilrod_teller(s, enable=False)
    e.set_params(**dict(vc.FLAGS, feynman_hibbs=1, feynman_hibbs_order=2))
    with pytest.raises(engine.EngineError, match="feynman_hibbs"):
        e.energy()
    e.set_params(**vc.FLAGS)
    got = _all(e)  # and with all of them off again it is the mode's result
    e.close()
    want = _fresh(vc.system("box22"), vc.FLAGS)
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    with pytest.raises(engine.EngineError, match="negative polarizability"):
        _engine(dict(vc.system("box2"), alpha=np.array([1.0, -1.0])), vc.FLAGS)


# ---- the fixture: the first 20 molecules of the reference's sample 013 (bulk CH4, 1070 sites), its box and its keywords
def _fixture_system(tmp_path, tail):
    import os
    import shutil

    from mpmc_amd import host

    gold = os.path.join(os.path.dirname(__file__), "golden", "ch4_cdvdw")
    shutil.copy(os.path.join(gold, "init.pdb"), tmp_path / "init.pdb")
    (tmp_path / "run.in").write_text(open(os.path.join(gold, "run.in")).read() + tail)
    lib = host.load()
    p = lib.setup_system(str(tmp_path / "run.in").encode())
    assert p
    return lib, p


def _fixture_state(lib, p):
    """(system as the host layer holds it, observables, vdw state)"""
    n = lib.host_natoms(p)
    f = [np.zeros(n) for _ in range(5)]
    pos, mol, frz, w = np.zeros((n, 3)), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n)
    lib.host_get_system(p, pos.ctypes.data, *[a.ctypes.data for a in f], mol.ctypes.data, frz.ctypes.data)
    lib.host_get_omega(p, w.ctypes.data)
    basis = np.zeros(9)
    lib.host_get_basis(p, basis.ctypes.data)
    s = dict(pos=pos, charge=f[0], alpha=f[1], epsilon=f[2], sigma=f[3], mass=f[4], molecule=mol, frozen=frz, omega=w,
             mol_type=np.zeros(n, dtype=np.int32), basis=basis.reshape(3, 3))
    obs, v = np.zeros(8), np.zeros(5)
    lib.host_get_observables(p, obs.ctypes.data)
    lib.host_get_vdw(p, v.ctypes.data)
    return s, obs, v


def _check_fixture(s, obs, v, what):
    ref = vr.vdw_terms(s, dict(polar_damp=2.1304, rd_lrc=1))
    assert len(ref["lam"]) == 300 and ref["lam"].min() >= vc.COND * ref["lam"].max()
    tol = vc.TOL * float(ref["abs_e_total"] + ref["abs_e_iso"] + ref["abs_lr_corr"])
    err = abs(v[4] - float(ref["vdw_energy"]))
    print("%s: vdw_energy %.10f reference %.10f |diff| %.3g tol %.3g" % (what, v[4], float(ref["vdw_energy"]), err, tol))
    assert err <= tol
    tol = vc.TOL * float(ref["abs_repulsion"] + ref["abs_repulsion_lrc"])
    assert abs(obs[2] - float(ref["rd_energy"])) <= tol
    assert obs[0] == ((obs[2] + obs[1]) + obs[3]) + v[4]  # energy.c:194
    assert vr.close_contacts(s, {}, 1.5)[0] == 0


def test_fixture_total_energy(tmp_path):
    lib, p = _fixture_system(tmp_path, "ensemble total_energy\nnumsteps 1\n")
    e = lib.energy(p)
    s, obs, v = _fixture_state(lib, p)
    lib.free_system(p)
    assert len(s["charge"]) == 180 and (s["sigma"] == 1.0).all()  # forced by the reader
    assert v[0] == 1 and v[1] == 1 and v[2] == 1.5 and v[3] == 0 and e == obs[0] and np.isfinite(e)
    _check_fixture(s, obs, v, "total_energy")


def test_fixture_nvt_chain(tmp_path):
    lib, p = _fixture_system(tmp_path, "ensemble nvt\nnumsteps 50\npreset_seeds 2718\n")
    assert lib.host_mc_steps(p, 50) >= 0
    s, obs, v = _fixture_state(lib, p)
    lib.free_system(p)
    assert obs[6] + obs[7] == 50 and obs[6] >= 1  # some move was accepted: the final configuration is not the first
    _check_fixture(s, obs, v, "nvt, 50 steps")
