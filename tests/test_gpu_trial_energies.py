"""mpmc_hip_trial_energies() (Engine.trial_energies) on the device: the energy of the resident configuration with one
molecule at K trial placements, the configuration left untouched.

Shapes: the smallest at which the kernels can go wrong -- 64, 65 and 130 background atoms (one block exactly, one atom
into the second, a third block) plus a molecule of 1, 2, 3, 5 or 16 sites at the first slots, the last slots or across
the boundary of the first 64-atom block; a frozen framework or an all-movable box; a cubic cell and the sheared cell of
tests/adversarial.py; placements with a site 5e-10 A inside and outside the cutoff and on a half-box tie; zero charges,
zero epsilons and a negative sigma in the molecule and around it; Ewald with 718 and with 61 k-vectors (neither a
multiple of 64), Wolf, rd_only; feynman_hibbs off / 2 / 4; rd_lrc on / off.

Bound: every energy within 1e-12 * sum |terms| of tests/trial_reference.py (the molecule really moved, longdouble
sums) -- the project's standing bound; the largest ratio seen is printed per case (profiles/quantum_rotation/README.md
records it).  Everything about the state of the context is held with ==."""
import numpy as np
import pytest

import trial_reference as tr
from mpmc_amd import engine, synth

pytestmark = pytest.mark.gpu

EW = dict(temperature=77.0)
CASES = {
    # name: (nbox, nsites, where, frozen framework, cell, flags)
    "b64_m5_start_ewald": (64, 5, "start", False, "cubic", dict(EW)),
    "b65_m5_straddle_fw_fh2": (65, 5, "straddle", True, "cubic", dict(EW, feynman_hibbs=1, feynman_hibbs_order=2)),
    "b130_m3_end_fw_fh4": (130, 3, "end", True, "cubic", dict(EW, feynman_hibbs=1, feynman_hibbs_order=4)),
    "b130_m16_start_sheared": (130, 16, "start", False, "sheared", dict(EW)),
    "b64_m1_end_wolf": (64, 1, "end", False, "cubic", dict(EW, wolf=1)),
    "b65_m2_start_fw_sheared_rdonly_nolrc": (65, 2, "start", True, "sheared", dict(EW, rd_only=1, rd_lrc=0)),
    "b130_m5_straddle_sheared_k3_nolrc": (130, 5, "straddle", False, "sheared", dict(EW, ewald_kmax=3, rd_lrc=0)),
    "b64_m16_end_fw_wolf": (64, 16, "end", True, "cubic", dict(EW, wolf=1)),
    "b65_m1_start_fw_fh2": (65, 1, "start", True, "cubic", dict(EW, feynman_hibbs=1, feynman_hibbs_order=2)),
    "b130_m2_straddle_fw_sheared_fh4": (130, 2, "straddle", True, "sheared", dict(EW, feynman_hibbs=1, feynman_hibbs_order=4)),
    "b65_m3_straddle_rdonly_fh2": (65, 3, "straddle", False, "cubic", dict(EW, rd_only=1, feynman_hibbs=1, feynman_hibbs_order=2)),
}
_BUILT = {}


def case(name):
    """(system, first, nsites, flags, placements, reference energies, sum |terms|): made once, shared, never changed."""
    if name not in _BUILT:
        nbox, nsites, where, fw, cell, flags = CASES[name]
        system, first = tr.build(nbox, nsites, where, fw, cell)
        xyz = tr.placements(system, flags, first, nsites)
        static = tr.static_terms(system, flags)
        ref = [tr.trial_energy(system, flags, first, p, static) for p in xyz]
        for a in list(system.values()) + [xyz]:
            a.setflags(write=False)
        _BUILT[name] = (system, first, nsites, flags, xyz, np.array([float(r[0]) for r in ref]), np.array([r[1] for r in ref]))
    return _BUILT[name]


def loaded(system, flags, **options):
    eng = engine.Engine(len(system["charge"]) + 16, device=0)
    for k, v in options.items():
        eng.set_option(k, v)
    eng.load_system(system, flags)
    return eng


def public_sequence(eng, first, xyz):
    """What a caller gets from update_atoms + energy() per placement on a context of its own."""
    return np.array([(eng.update_atoms(first, p), eng.energy()["energy"])[1] for p in xyz])


@pytest.mark.parametrize("name", sorted(CASES))
def test_batched_and_serial_against_the_reference(name):
    system, first, nsites, flags, xyz, ref, mags = case(name)
    eng, ser, pub = loaded(system, flags), loaded(system, flags, trial_batched=0), loaded(system, flags)
    try:
        e0 = eng.energy()
        assert ser.energy() == e0 and pub.energy() == e0
        got, terms = eng.trial_energies(first, xyz, terms=True)
        ratio = np.abs(got - ref) / mags
        print("%s: largest |batched - reference| / sum|terms| = %.3e" % (name, ratio.max()))
        assert (ratio <= tr.BOUND).all(), (name, ratio)
        assert abs(e0["energy"] - ref[0]) <= tr.BOUND * mags[0]  # (placement 0 is the current one)
        # the terms add up to the total, in the stated order, exactly
        base = e0["energy"] - ((terms[0, 0] + terms[0, 1]) + terms[0, 2])
        assert np.array_equal(got, base + ((terms[:, 0] + terms[:, 1]) + terms[:, 2]))
        if flags.get("rd_only"):
            assert not terms[:, 1:].any()
        if flags.get("wolf"):
            assert not terms[:, 2].any()
        # the serial path == the public sequence on a second context; the batched path within the bound of it
        serial = ser.trial_energies(first, xyz)
        assert np.array_equal(serial, public_sequence(pub, first, xyz))
        r2 = np.abs(got - serial) / mags
        print("%s: largest |batched - serial| / sum|terms| = %.3e" % (name, r2.max()))
        assert (r2 <= tr.BOUND).all(), (name, r2)
        assert eng.trial_call_count() == 1 and ser.trial_call_count() == 1
        # both contexts still hold the configuration: energy() == before
        assert eng.energy() == e0 and ser.energy() == e0
    finally:
        for e in (eng, ser, pub):
            e.close()


@pytest.mark.parametrize("name", ["b130_m5_straddle_sheared_k3_nolrc", "b65_m5_straddle_fw_fh2", "b64_m16_end_fw_wolf"])
def test_a_placement_s_bits_do_not_depend_on_the_batch(name):
    system, first, nsites, flags, _, _, _ = case(name)
    xyz = tr.random_placements(system, first, nsites, 257, seed=5)
    eng = loaded(system, flags)
    try:
        eng.energy()
        full, tfull = eng.trial_energies(first, xyz, terms=True)
        for n in (1, 63, 64, 65, 255, 256):
            e, t = eng.trial_energies(first, xyz[:n], terms=True)
            assert np.array_equal(e, full[:n]) and np.array_equal(t, tfull[:n]), n
        for k in (0, 62, 63, 64, 256):  # alone
            assert eng.trial_energies(first, xyz[k:k + 1])[0] == full[k]
        assert np.array_equal(eng.trial_energies(first, xyz[::-1]), full[::-1])  # ... nor on the position in it
        assert np.array_equal(eng.trial_energies(first, xyz), full)  # ... nor on the call
    finally:
        eng.close()


@pytest.mark.parametrize("batched", [1, 0])
def test_the_context_is_left_as_it_was(batched):
    system, first, nsites, flags, xyz, _, _ = case("b130_m5_straddle_sheared_k3_nolrc")
    a, b = loaded(system, flags, trial_batched=batched), loaded(system, flags)  # b never makes the call
    try:
        assert a.energy() == b.energy()
        a.trial_energies(first, xyz)
        assert a.energy() == b.energy()
        a.trial_energies(first, xyz)
        # a further move of the molecule, and of another atom, give the bits of the context that never called
        for f, p in ((first, xyz[2]), (first + nsites, system["pos"][first + nsites:first + nsites + 1] + 0.2), (first, xyz[3])):
            a.update_atoms(f, p)
            b.update_atoms(f, p)
            assert a.energy() == b.energy()
            a.trial_energies(first, xyz[:3])
    finally:
        a.close()
        b.close()


def _polar_system():
    system = synth.s_pol(70)
    first, k = 15, 5  # the fourth BSSP molecule
    rng = np.random.default_rng(3)
    cur = system["pos"][first:first + k]
    xyz = np.array([cur] + [cur[0] + (cur - cur[0]) @ tr._rotation(rng).T for _ in range(3)])
    return system, first, xyz


@pytest.mark.parametrize("mode", ["polarization", "disp_expansion"])
def test_polarization_and_dense_modes_take_the_serial_path(mode):
    if mode == "polarization":
        system, first, xyz = _polar_system()
        flags = dict(synth.FLAGS_POL_JACOBI)
    else:
        system = synth.s_phahst(60)
        mol = np.asarray(system["molecule"])
        movable = np.flatnonzero(np.asarray(system["frozen"]) == 0)
        first = int(movable[0])
        k = int((mol == mol[first]).sum())
        rng = np.random.default_rng(4)
        cur = system["pos"][first:first + k]
        xyz = np.array([cur] + [cur[0] + (cur - cur[0]) @ tr._rotation(rng).T for _ in range(3)])
        flags = dict(synth.FLAGS_PHAHST)
    a, pub, never = loaded(system, flags), loaded(system, flags), loaded(system, flags)
    try:
        e0 = a.energy()
        assert pub.energy() == e0 and never.energy() == e0
        d0 = a.dipoles()
        got = a.trial_energies(first, xyz)
        assert np.array_equal(got, public_sequence(pub, first, xyz))
        assert got[0] == e0["energy"]  # (the current placement)
        with pytest.raises(engine.EngineError, match="terms are the batched path's"):
            a.trial_energies(first, xyz, terms=True)
        assert a.energy() == e0
        d1, dn = a.dipoles(), never.dipoles()
        for key in d0:
            assert np.array_equal(d0[key], d1[key]) and np.array_equal(dn[key], d1[key]), key
        a.update_atoms(first, xyz[1])
        never.update_atoms(first, xyz[1])
        assert a.energy() == never.energy()
        d1, dn = a.dipoles(), never.dipoles()
        for key in d1:
            assert np.array_equal(dn[key], d1[key]), key
    finally:
        for e in (a, pub, never):
            e.close()


def test_every_refusal_is_by_name_and_changes_nothing():
    system, first, nsites, flags, xyz, _, _ = case("b65_m5_straddle_fw_fh2")
    a, b = loaded(system, flags), loaded(system, flags)
    try:
        def refused(match, *args, **kw):
            with pytest.raises(engine.EngineError, match=match):
                a.trial_energies(*args, **kw)

        stale = "needs a completed energy\\(\\) on the current configuration"
        refused(stale, first, xyz)  # an upload, no energy() yet
        e0 = a.energy()
        assert e0 == b.energy()
        refused("ntrial = 0", first, xyz[:0])
        # slot ranges that are not one whole valid, non-frozen molecule of 1 .. 16 sites
        whole = "not one whole valid, non-frozen molecule"
        refused(whole + ".*the molecule goes on", first, xyz[:, :nsites - 1])
        refused(whole + ".*the molecule starts earlier", first + 1, xyz[:, 1:])
        refused(whole + ".*more than one molecule", first, np.zeros((2, nsites + 1, 3)))
        refused(whole + ".*frozen", 0, np.zeros((2, 1, 3)))
        refused(whole + ".*outside the slots in use", len(system["charge"]) - 1, np.zeros((2, 2, 3)))
        refused(whole + ".*outside the slots in use", -1, np.zeros((2, 1, 3)))
        refused(whole + ".*site count", first, np.zeros((2, 17, 3)))
        assert a.trial_call_count() == 0
        assert a.energy() == e0
        # between energy_begin() and energy_end()
        a.energy_begin()
        refused("between energy_begin\\(\\) and energy_end\\(\\)", first, xyz)
        assert a.energy_end() == e0
        # a move, a box change, a parameter change since the last completed energy()
        a.update_atoms(first, xyz[1])
        refused(stale, first, xyz)
        b.update_atoms(first, xyz[1])
        assert a.energy() == b.energy()
        a.set_box(system["basis"])
        refused(stale, first, xyz)
        b.set_box(system["basis"])
        assert a.energy() == b.energy()
        a.set_params(**flags)
        refused(stale, first, xyz)
        b.set_params(**flags)
        assert a.energy() == b.energy()
        # setting the path option is no change of the evaluation
        a.set_option("trial_batched", 0)
        a.set_option("trial_batched", 1)
        assert len(a.trial_energies(first, xyz)) == len(xyz)
    finally:
        a.close()
        b.close()


def test_an_edit_is_refused_and_a_hole_is_skipped():
    """All-movable box: after remove_molecule the call is refused until energy() has run; then the removed atom's slot is
    a hole that the kernels skip -- the reference is the system without that atom."""
    system, first, nsites, flags, xyz, _, _ = case("b64_m5_start_ewald")
    gone = first + nsites + 7  # a single-site background molecule
    eng = loaded(system, flags)
    try:
        eng.energy()
        assert eng.remove_molecule(gone, 1)
        with pytest.raises(engine.EngineError, match="needs a completed energy"):
            eng.trial_energies(first, xyz)
        e0 = eng.energy()
        got = eng.trial_energies(first, xyz)
        keep = np.arange(len(system["charge"])) != gone
        small = {k: (v if k == "basis" else np.asarray(v)[keep]) for k, v in system.items()}
        static = tr.static_terms(small, flags)
        for t, p in enumerate(xyz):
            ref, mags = tr.trial_energy(small, flags, first, p, static)
            assert abs(got[t] - float(ref)) <= tr.BOUND * mags, t
        with pytest.raises(engine.EngineError, match="a slot holds no atom"):
            eng.trial_energies(gone, np.zeros((1, 1, 3)))
        assert eng.energy() == e0
    finally:
        eng.close()
