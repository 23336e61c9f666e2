"""CPU: the fixtures of tests/golden/reference_chains/ (tests/golden/make_reference_chains.py) -- seeded Monte Carlo inputs
and what the reference program wrote for them.  Per fixture: the host layer's reader takes the input and the binding
refuses nothing in it; the independent references of this suite reproduce the reference program's step-0 line; and the
reference's chain did what the fixture is there for (moves accepted and rejected, the volume both ways, N both ways).
The device part is tests/test_gpu_reference_chains.py.

The step-0 line, column by column, `to the printed digits`: |value - printed| <= half a unit of the sixth decimal (plus
1e-12 |value| for the reference program's own rounding):
  coulombic  oracle.energy                           (absent under rd_only / sg)
  polar      oracle.energy; for `polar_iterative off` + `polar_damp_type linear` the longdouble Cholesky solve of
             tests/test_thole_models_reference.py
  rd         oracle.energy (Lennard-Jones), phahst_reference (disp_expansion), rdforms_reference (sg, lj_buffered_14_7),
             rdc_reference (rd_crystal)
  energy     the sum of the columns -- plus, under axilrod_teller, at_reference's three-body energy, which no column of
             the file carries on its own
"""
import os
from decimal import Decimal

import numpy as np
import pytest

import reference_chain_compare as rcc
from mpmc_amd import host

HALF_UNIT = 0.5e-6


def keywords(name):
    kw = {}
    for line in open(os.path.join(rcc.CHAINS, name, "input")).read().splitlines():
        t = line.split()
        if t:
            kw[t[0]] = t[1:]
    return kw


def flags_of(kw):
    """the energy keywords of an input in the naming of the oracle and the Python references"""
    f = {}
    for k, v in kw.items():
        if k.startswith(("basis", "pqr_", "job_name", "ensemble", "preset_seeds", "numsteps", "corrtime", "move_factor",
                         "rot_factor", "energy_output", "traj_output", "dipole_output", "field_output", "wrapall",
                         "user_fugacities", "insert_probability", "pressure", "volume_")):
            continue
        if v[0] in ("on", "off"):
            f[k] = int(v[0] == "on")
        elif k == "polar_damp_type":
            f[k] = v[0]
        else:
            f[k] = float(v[0]) if "." in v[0] else int(v[0])
    return f


def read_system(name):
    """what the host layer's reader makes of the fixture (the doubles the reference program ran on), with c6 c8 c10 c9;
    also: the binding's word on the input"""
    lib = host.load()
    ptr = lib.setup_system(os.path.join(rcc.CHAINS, name, "input").encode())
    assert ptr, "setup_system refused " + name
    refusal = lib.host_unsupported(ptr)
    n = lib.host_natoms(ptr)
    f = {k: np.zeros(n) for k in ("charge", "alpha", "epsilon", "sigma", "mass", "c6", "c8", "c10", "c9")}
    pos, basis = np.zeros((n, 3)), np.zeros(9)
    mol, frz = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    lib.host_get_system(ptr, pos.ctypes.data, f["charge"].ctypes.data, f["alpha"].ctypes.data, f["epsilon"].ctypes.data,
                        f["sigma"].ctypes.data, f["mass"].ctypes.data, mol.ctypes.data, frz.ctypes.data)
    lib.host_get_dispersion(ptr, f["c6"].ctypes.data, f["c8"].ctypes.data, f["c10"].ctypes.data)
    lib.host_get_c9(ptr, f["c9"].ctypes.data)
    lib.host_get_basis(ptr, basis.ctypes.data)
    lib.free_system(ptr)
    return dict(pos=pos, molecule=mol, frozen=frz, basis=basis.reshape(3, 3), **f), refusal


def test_fixture_set_is_the_table():
    assert sorted(os.listdir(rcc.CHAINS)) == sorted(rcc.NAMES + ("README.md",))
    for name in rcc.NAMES:
        assert sorted(os.listdir(os.path.join(rcc.CHAINS, name))) == ["in.pqr", "input", "reference_energy.dat",
                                                                      "reference_restart.pqr"]
        kw = keywords(name)
        assert kw["ensemble"] == [name.split("_")[0]] and int(kw["numsteps"][0]) <= 200
        assert int(kw["numsteps"][0]) % int(kw["corrtime"][0]) == 0  # (the reference also writes the last step's line)
        want = rcc.energy_lines(os.path.join(rcc.CHAINS, name, "reference_energy.dat"))
        assert want[0] == rcc.HEADER and len(want) == 2 + int(kw["numsteps"][0]) // int(kw["corrtime"][0]) <= 202


@pytest.mark.parametrize("name", rcc.NAMES)
def test_host_layer_reads_the_input_and_refuses_nothing(name):
    s, refusal = read_system(name)
    assert refusal is None, refusal
    assert 0 < len(s["charge"]) <= 320
    # the reader's atoms are the restart file's atoms where no molecule was inserted or removed
    atoms, basis = rcc.restart_atoms(os.path.join(rcc.CHAINS, name, "reference_restart.pqr"))
    assert len(basis) == 9
    if not name.startswith("uvt"):
        assert len(atoms) == len(s["charge"]) and [a[2] == "F" for a in atoms] == [bool(f) for f in s["frozen"]]


def _close(value, printed):
    return abs(float(value) - float(printed)) <= HALF_UNIT + 1e-12 * abs(float(value))


@pytest.mark.parametrize("name", rcc.NAMES)
def test_step_0_line_is_what_the_independent_references_give(name):
    from oracle import oracle

    s, _ = read_system(name)
    f = flags_of(keywords(name))
    line = rcc.rows(rcc.energy_lines(os.path.join(rcc.CHAINS, name, "reference_energy.dat")))[0]
    got = dict(zip(rcc.COLUMNS, line))
    assert got["step"] == "0" and got["vdw"] == "0.000000"
    no_es = bool(f.get("rd_only") or f.get("sg"))
    plain_polar = f.get("polarization") and f.get("polar_iterative", 1) and f.get("polar_damp_type") == "exponential"
    o = oracle.energy(s, {k: v for k, v in f.items()
                          if k in oracle.PARAM_NAMES and (plain_polar or not k.startswith("polar"))})
    # coulombic
    if no_es:
        assert got["coulombic"] == "0.000000" and got["polar"] == "0.000000"
    else:
        assert _close(o["coulombic_energy"], got["coulombic"]), (o["coulombic_energy"], got["coulombic"])
    # polar
    if plain_polar:
        assert _close(o["polarization_energy"], got["polar"]), (o["polarization_energy"], got["polar"])
    elif f.get("polarization"):
        import exact_reference as xref
        import pair_reference as pr
        import thole_models_reference as tm

        assert not f["polar_iterative"] and f["polar_damp_type"] == "linear"
        fp = dict(temperature=f["temperature"], polarization=1, polar_damp=f["polar_damp"], polar_wolf=0)
        E = pr.sums(pr.pair_table(s, fp), s, fp)["ef_static"]
        t = tm.ModelTensor(s, f["polar_damp"], "linear")
        Ev = E[t.view].reshape(-1).astype(np.longdouble)
        upol = np.longdouble(-0.5) * (xref.solve(tm.view_matrix(t), Ev) @ Ev)
        assert _close(upol, got["polar"]), (upol, got["polar"])
    else:
        assert got["polar"] == "0.000000"
    # rd
    if f.get("disp_expansion"):
        import phahst_reference as ph

        rd = ph.rd_terms(s, f)["total"]
    elif f.get("sg") or f.get("lj_buffered_14_7"):
        import rdforms_reference as rf

        form = "sg" if f.get("sg") else "lj_buffered_14_7"
        rd = rf.rd_terms(s, f, form, "halgren_mixing" if f.get("halgren_mixing") else "lb")["total"]
    elif f.get("rd_crystal"):
        import rdc_reference as rr

        rd = rr.rd_terms(s, f, f["rd_crystal_order"])["total"]
    else:
        rd = o["rd_energy"]
    assert _close(rd, got["rd"]), (rd, got["rd"])
    # the total, and what it holds beyond the columns
    rest = Decimal(got["energy"]) - sum(Decimal(got[k]) for k in ("coulombic", "rd", "polar", "vdw"))
    if f.get("axilrod_teller"):
        import at_reference as at

        three_body = float(at.unordered(s, False).total)
        assert abs(three_body) > 1.0  # visible in the printed digits
        assert abs(three_body - float(rest)) <= 4 * HALF_UNIT, (three_body, rest)  # (four rounded columns)
    else:
        assert abs(rest) <= 3 * rcc.UNIT, rest


def _facts(name):
    r = rcc.rows(rcc.energy_lines(os.path.join(rcc.CHAINS, name, "reference_energy.dat")))
    pairs = list(zip(r, r[1:]))
    return dict(
        changed=sum(1 for a, b in pairs if a[1] != b[1]), repeated=sum(1 for a, b in pairs if a[1] == b[1]),
        v_up=sum(1 for a, b in pairs if Decimal(b[10]) > Decimal(a[10])),
        v_down=sum(1 for a, b in pairs if Decimal(b[10]) < Decimal(a[10])),
        all_kept=sum(1 for a, b in pairs if b[10] == a[10] and b[1] == a[1]),
        n_up=sum(max(Decimal(b[8]) - Decimal(a[8]), 0) for a, b in pairs),
        n_down=sum(max(Decimal(a[8]) - Decimal(b[8]), 0) for a, b in pairs),
        n_min=min(Decimal(a[8]) for a in r))


@pytest.mark.parametrize("name", rcc.NAMES)
def test_reference_chain_exercises_what_its_row_claims(name):
    k = _facts(name)
    print(name, k)
    assert k["changed"] >= 5 and k["repeated"] >= 5  # moves were accepted, and rejected
    if name.startswith("npt"):
        assert k["v_up"] >= 1 and k["v_down"] >= 1 and k["all_kept"] >= 1
    else:
        assert k["v_up"] == k["v_down"] == 0
    if name.startswith("uvt"):
        assert k["n_up"] >= 3 and k["n_down"] >= 3 and k["n_min"] >= 1
    else:
        assert k["n_up"] == k["n_down"] == 0


def _replayed(name):
    import reference_chain_replay as rp

    kw = keywords(name)
    return kw, rp.replay(kw, rcc.rows(rcc.energy_lines(os.path.join(rcc.CHAINS, name, "reference_energy.dat")))), rp


MARGIN = 1e-6  # relative: the factors are formed from energies and volumes printed to six decimals


@pytest.mark.parametrize("name", rcc.NAMES)
def test_energy_file_is_the_chain_of_its_seed(name):
    """tests/reference_chain_replay.py: the draws of the seed give every step a kind of move that fits the N and the volume
    of the file, and every accepted move's Metropolis draw lies below the acceptance factor of mc.c:37-135 formed from the
    file's own energies -- so the kinds, the draws and the factors the next test speaks of are the reference's"""
    kw, steps, rp = _replayed(name)
    counts = {}
    for s in steps:
        counts[(s["kind"], s["accepted"])] = counts.get((s["kind"], s["accepted"]), 0) + 1
        if s["accepted"]:
            assert s["u"] < rp.factor(kw, s) * (1 + MARGIN), s
    print(name, ", ".join("%s %d accepted %d rejected" % (k, counts.get((k, True), 0), counts.get((k, False), 0))
                          for k in ("displace", "volume", "insert", "remove") if (k, True) in counts or (k, False) in counts))
    # an accepted uphill move: the draw was compared with exp(-dE / T) < 1, not waved through
    assert any(s["accepted"] and s["kind"] == "displace" and s["dE"] > 0 for s in steps)


def _decided(kw, steps, rp, kind, n_shift):
    """accepted steps of a kind that the factor with its molecule count shifted would have rejected"""
    return [s["step"] for s in steps if s["accepted"] and s["kind"] == kind and s["u"] >= rp.factor(kw, s, n_shift) * (1 + MARGIN)]


def test_seeds_hold_steps_at_which_the_prefactors_decide():
    """What a chain that merely tracks the energies cannot show: steps whose acceptance hangs on the N of the factor.  A
    driver with N in place of N + 1 in the removal factor or in the volume move's log term, or with N + 1 under the
    insertion's fugacity term, rejects these steps and leaves the reference's chain there."""
    kw, steps, rp = _replayed("uvt_polar_framework")
    assert len(_decided(kw, steps, rp, "remove", -1)) >= 3
    assert len(_decided(kw, steps, rp, "insert", +1)) >= 1
    # never emptying the list: a removal drawn with one movable molecule left became a displacement
    assert any(s["drawn"] == "remove" and s["kind"] == "displace" and s["N_before"] == 1 for s in steps)
    assert min(s["N_after"] for s in steps) == 1
    kw, steps, rp = _replayed("npt_default_probability")
    assert len(_decided(kw, steps, rp, "volume", -1)) >= 1
    assert sum(1 for s in steps if s["kind"] == "volume" and not s["accepted"]) >= 1  # revert_volume_change() ran
    # npt_jacobi: |ln V'/V| <= 0.01 leaves little room for N against N + 1 in 80 steps; each of the two terms beside
    # the energy decides steps as a whole (the log term where the box grew, P dV where it shrank)
    kw, steps, rp = _replayed("npt_jacobi")
    volume = [s for s in steps if s["accepted"] and s["kind"] == "volume"]
    no_log = [s["step"] for s in volume if s["u"] >= rp.factor(kw, s, -(s["N_after"] + 1)) * (1 + MARGIN)]
    no_pv = [s["step"] for s in volume if s["u"] >= rp.factor(kw, s, 0, pv=0.0) * (1 + MARGIN)]
    print("npt_jacobi: accepted only with the log term:", no_log, "only with P dV:", no_pv)
    assert len(no_log) + len(no_pv) >= 2 and no_pv
    assert sum(1 for s in steps if s["kind"] == "volume" and not s["accepted"]) >= 1
