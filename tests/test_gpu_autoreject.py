"""GPU tests of the close-contact count behind cavity_autoreject_absolute: contact_tile_kernel
(mpmc_amd/csrc/kernels_vdw.h) through mpmc_hip_set_autoreject / mpmc_hip_get_close_contacts, against
vdw_reference.close_contacts.  The count is a sum of exact small integers: it is compared with ==."""
import numpy as np
import pytest

import vdw_cases as vc
import vdw_reference as vr
from mpmc_amd import engine, host

pytestmark = pytest.mark.gpu
LJ = dict(temperature=150.0)                        # Lennard-Jones + Ewald, no polarization
AR = dict(cavity_autoreject_absolute=1, cavity_autoreject_scale=vc.SCALE)


def _engine(s, flags):
    e = engine.Engine(len(s["charge"]))
    e.load_system(s, flags)
    return e


@pytest.mark.parametrize("which", [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)])
def test_counts_are_the_references(which):
    """a pair 1e-9 A inside the scale counts, one 1e-9 A outside does not, a same-molecule pair far inside is ignored, a
    frozen-frozen pair on different molecules counts"""
    s = vc.contacts(*[bool(w) for w in which])
    want, margin = vr.close_contacts(s, LJ, vc.SCALE)
    assert want == which[0] + which[2] and margin > 0.0
    e = _engine(s, dict(LJ, **AR))
    r = e.energy()
    assert e.close_contacts() == want and r["status"] == 0
    e.close()


def test_the_count_follows_moves_and_the_setting():
    s = vc.system("contacts")
    never = _engine(s, LJ)
    plain = never.energy()
    assert never.close_contacts() == 0
    never.close()
    e = _engine(s, dict(LJ, **AR))
    r = e.energy()
    assert e.close_contacts() == 2
    assert r == plain  # counting changes no other number
    # the inside pair's second molecule (upload order: five singles, then the inside pair) steps 2e-9 A outwards, and back
    first = 6
    step = 2 * vc.EDGE * np.array([0.6, 0.0, 0.8])
    for shift, want in ((step, 1), (0 * step, 2)):
        t = dict(s, pos=np.array(s["pos"]))
        t["pos"][first] += shift
        assert vr.close_contacts(t, LJ, vc.SCALE)[0] == want
        e.update_atoms(first, t["pos"][first:first + 1])
        e.energy()
        assert e.close_contacts() == want
    e.energy()
    assert e.close_contacts() == 2  # nothing moved: the same count
    # a wider and a narrower scale, on the resident configuration
    for scale in (0.5, 1.2, 1.6, 3.0):
        e.set_autoreject(scale)
        e.energy()
        assert e.close_contacts() == vr.close_contacts(s, LJ, scale)[0], scale
    e.set_autoreject(0.0)
    assert e.energy() == plain and e.close_contacts() == 0
    # the setting persists across an upload
    e.set_autoreject(vc.SCALE)
    e.upload(s)
    e.energy()
    assert e.close_contacts() == 2
    e.close()


def test_the_count_in_the_vdw_mode_and_beside_a_non_finite_solve():
    s = vc.system("contacts")
    f = dict(vc.FLAGS, **AR)
    e = _engine(s, f)
    r = e.energy()
    assert e.close_contacts() == 2 and r["status"] == 0 and np.isfinite(e.vdw_energy())
    # two molecules on one point: the repulsion is infinite (the damped tensor of the pair is exactly 0 at rimg = 0, so the
    # coupled-dipole term itself stays finite); the count is delivered beside the status bit
    t = dict(s, pos=np.array(s["pos"]))
    t["pos"][1] = t["pos"][0]
    e.update_atoms(1, t["pos"][1:2])
    r = e.energy()  # returns: a non-finite term is a status bit, not a failure
    assert r["status"] & 1 and not np.isfinite(r["rd_energy"]) and np.isfinite(e.vdw_energy())
    assert e.close_contacts() == 3 == vr.close_contacts(t, vc.FLAGS, vc.SCALE)[0]
    e.update_atoms(1, s["pos"][1:2])
    # a frequency whose square overflows: the matrix, and with it the dipole solve, is non-finite -- no loop of the solver
    # depends on its data, energy() returns, and the count is that of the configuration
    w = np.array(s["omega"])
    w[0] = 1e200
    e.set_vdw(dict(s, omega=w))
    r = e.energy()
    assert r["status"] & 1 and not np.isfinite(e.vdw_energy()) and not np.isfinite(e.vdw_terms()["e_total"])
    assert np.isfinite(r["rd_energy"]) and e.close_contacts() == 2
    # and the context goes on
    e.set_vdw(s)
    r = e.energy()
    assert e.close_contacts() == 2 and r["status"] == 0
    fresh = _engine(s, f)
    assert r == fresh.energy() and e.vdw_terms() == fresh.vdw_terms()
    fresh.close()
    e.close()


# ---- through the host layer: what energy() does on a non-zero count (energy.c:99-102, :187-194)
HOST_FLAGS = dict(vc.FLAGS, **AR)
MAXVALUE = 1.0e40
TERMS = ("rd_energy", "coulombic_energy", "polarization_energy")


def test_host_energy_returns_maxvalue_and_keeps_the_stale_terms():
    s = vc.contacts(inside=False, outside=True, frozen_pair=False)  # the outside pair: molecules 5 and 6 of the list
    h = host.HostSystem(s, HOST_FLAGS)
    e0 = h.energy()
    o0, v0 = h.observables(), h.vdw()
    assert np.isfinite(e0) and e0 == o0["energy"] and v0["count_autorejects"] == 0 and v0["vdw_energy"] != 0.0
    want = vr.vdw_terms(s, vc.FLAGS)
    assert abs(v0["vdw_energy"] - float(want["vdw_energy"])) <= vc.TOL * float(
        want["abs_e_total"] + want["abs_e_iso"] + want["abs_lr_corr"])
    step = 2 * vc.EDGE * np.array([0.6, 0.0, 0.8])
    h.displace_molecule(6, -step)  # 1e-9 A inside the scale now
    e1 = h.energy()
    o1, v1 = h.observables(), h.vdw()
    assert e1 == MAXVALUE == o1["energy"] and v1["count_autorejects"] == 1
    for t in TERMS:  # ... as the previous call left them
        assert o1[t] == o0[t], t
    assert v1["vdw_energy"] == v0["vdw_energy"]
    h.displace_molecule(6, step)
    e2 = h.energy()
    assert h.vdw()["count_autorejects"] == 1 and np.isfinite(e2)
    t = dict(s, pos=h.positions())
    fresh = host.HostSystem(t, HOST_FLAGS)
    assert fresh.energy() == e2 and fresh.observables()["rd_energy"] == h.observables()["rd_energy"]
    assert fresh.vdw()["vdw_energy"] == h.vdw()["vdw_energy"]
    fresh.close()
    h.close()


def test_host_chain_rejects_the_moves_that_make_a_contact():
    s = vc.cage()  # nobody in contact, and almost every step of an inner molecule makes one
    assert vr.close_contacts(s, vc.FLAGS, vc.SCALE)[0] == 0
    h = host.HostSystem(s, HOST_FLAGS, seed=11, move_factor=0.02, rot_factor=0.02)
    steps = 40
    h.mc_steps(steps)
    o, v = h.observables(), h.vdw()
    assert o["accept"] + o["reject"] == steps
    assert 1 <= v["count_autorejects"] <= o["reject"]
    assert np.isfinite(o["energy"]) and o["energy"] < MAXVALUE
    final = dict(s, pos=h.positions())
    assert vr.close_contacts(final, vc.FLAGS, vc.SCALE)[0] == 0  # no such move was kept
    want = vr.vdw_terms(final, vc.FLAGS)
    assert abs(v["vdw_energy"] - float(want["vdw_energy"])) <= vc.TOL * float(
        want["abs_e_total"] + want["abs_e_iso"] + want["abs_lr_corr"])
    h.close()
