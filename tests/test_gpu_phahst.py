"""GPU tests of the PHAHST repulsion / dispersion term (disp_expansion): disp_tile_kernel + disp_lrc_kernel
(mpmc_amd/csrc/kernels_disp.h) through mpmc_hip_set_dispersion, against tests/phahst_reference.py.

The tolerance of rd_energy is 1e-12 * sum |terms| (the four terms of every pair and every long-range term).  The derived
rounding bound is a few ulp per term plus a log-depth sum, about 5e-15 * sum |terms|: two orders below.
tests/test_phahst_reference.py checks on the CPU, for every input used here, that the smallest beyond-cutoff pair term that
is not exactly 0 exceeds 1e3 * that tolerance -- a single dropped pair fails these tests -- and that applying a cutoff to
the pair sum moves the total by more than 1e6 * the tolerance; the first of the two is asserted again below.
"""
import os
import subprocess

import numpy as np
import pytest

import phahst_cases as pc
import phahst_reference as ph
from mpmc_amd import engine, host, synth
from oracle import oracle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10  # the project's bound on `energy` against the oracle
FIELDS = [f for f, _ in engine.Result._fields_]


def _engine(s, flags, cap=None, **options):
    e = engine.Engine(cap or len(s["charge"]))
    for k, v in options.items():
        e.set_option(k, v)
    e.load_system(s, flags)
    return e


def _fresh(s, flags):
    e = _engine(s, flags)
    r = e.energy()
    d = e.dipoles() if flags.get("polarization") and not flags.get("rd_only") else None
    e.close()
    return r, d


def _check_rd(got, ref, what):
    want, tol = float(ref["total"]), pc.RD_TOL * float(ref["abs_sum"])
    err = abs(got["rd_energy"] - want)
    print("%s: rd_energy %.12f reference %.12f |diff| %.3g tol %.3g (%.3g of it)" % (what, got["rd_energy"], want, err, tol,
                                                                                     err / tol))
    assert err <= tol, (what, got["rd_energy"], want, err, tol)
    assert got["status"] == 0


_oracle_cache = {}


def _oracle_es(name, variant):
    """coulombic + polarization energies of the case from the CPU oracle (which has no dispersion term: it is given
    epsilon = sigma = 0, and those two energies do not depend on the repulsion / dispersion term)"""
    key = (name, variant)
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle.energy(ph.without_dispersion(pc.system(name)), ph.plain_flags(pc.VARIANTS[variant]))
    return _oracle_cache[key]


@pytest.mark.parametrize("name", pc.INPUTS)
@pytest.mark.parametrize("variant", sorted(pc.VARIANTS))
def test_rd_energy_against_the_reference(name, variant):
    s, flags, ref = pc.system(name), pc.VARIANTS[variant], pc.reference(name, variant)
    tol = pc.RD_TOL * float(ref["abs_sum"])
    beyond = np.abs(ref["table"].energy[ref["table"].beyond].astype(np.float64))
    # One dropped beyond-cutoff pair would fail the comparison below.  Terms that are exactly 0 are left out of this check:
    # under damp_dispersion every pair of the dispersion-only site has b_ij = 0, x = 0, f_n = 0, so in ALL damped variants
    # (FLAGS_PHAHST included) that site contributes nothing to the pair sum -- the reference's own behaviour -- and only the
    # undamped variants ("extrapolate", "plain") exercise its dispersion; the long-range correction sees it in every variant.
    assert beyond[beyond != 0.0].min() > 1e3 * tol
    got, dip = _fresh(s, flags)
    _check_rd(got, ref, "%s/%s" % (name, variant))
    assert got["cutoff"] == ref["cutoff"] and got["volume"] == ref["volume"] and got["n_atoms"] == len(s["charge"])
    if flags.get("rd_only"):
        assert got["energy"] == got["rd_energy"] and got["coulombic_energy"] == 0.0 and got["polarization_energy"] == 0.0
        return
    want = _oracle_es(name, variant)
    total = float(ref["total"]) + want["coulombic_energy"] + want["polarization_energy"]
    assert abs(got["coulombic_energy"] - want["coulombic_energy"]) <= RTOL * max(1.0, abs(want["coulombic_energy"]))
    assert abs(got["polarization_energy"] - want["polarization_energy"]) <= RTOL * max(1.0, abs(want["polarization_energy"]))
    assert abs(got["energy"] - total) <= RTOL * max(1.0, abs(total)), (got["energy"], total)
    # the other terms do not see this one: bit for bit what the same atoms give without any repulsion / dispersion
    bare, bare_dip = _fresh(ph.without_dispersion(s), ph.plain_flags(flags))
    for f in FIELDS:
        if f not in ("energy", "rd_energy"):
            assert got[f] == bare[f], (f, got[f], bare[f])
    assert bare["rd_energy"] == 0.0
    if dip is not None:
        for k in dip:
            assert np.array_equal(dip[k], bare_dip[k]), k


def _move(s, pos, rng, movable):
    """one movable molecule displaced and turned a little: (first atom, new coordinates of its atoms)"""
    mol = np.asarray(s["molecule"])
    idx = np.flatnonzero(mol == rng.choice(movable))
    c = pos[idx].mean(axis=0)
    th = rng.uniform(-0.2, 0.2)
    rot = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
    return int(idx[0]), (pos[idx] - c) @ rot.T + c + rng.uniform(-0.15, 0.15, 3)


def test_incremental_pass_leaves_the_bits_of_a_from_scratch_pass():
    s, flags = pc.system("c320"), pc.VARIANTS["polarizable"]
    rng = np.random.default_rng(11)
    movable = np.unique(np.asarray(s["molecule"])[np.asarray(s["frozen"]) == 0])
    live, full = _engine(s, flags), _engine(s, flags, incremental_pairs=0)
    assert live.energy() == full.energy()
    cur = dict(s, pos=s["pos"].copy())
    for step in range(20):
        first, new = _move(s, cur["pos"], rng, movable)
        cur["pos"][first:first + len(new)] = new
        live.update_atoms(first, new)
        full.update_atoms(first, new)
        a, b = live.energy(), full.energy()
        c, _ = _fresh(cur, flags)
        for f in FIELDS:
            assert a[f] == c[f], ("live vs fresh", step, f, a[f], c[f])
            assert b[f] == c[f], ("incremental_pairs = 0 vs fresh", step, f, b[f], c[f])
    _check_rd(a, ph.rd_terms(cur, flags), "after 20 moves")
    # the same evaluation again, and in two halves: the same bits
    assert live.energy() == a
    live.energy_begin()
    assert live.energy_end() == a
    first, new = _move(s, cur["pos"], rng, movable)
    cur["pos"][first:first + len(new)] = new
    live.update_atoms(first, new)
    live.energy_begin()
    assert live.energy_end() == _fresh(cur, flags)[0]
    live.close()
    full.close()


@pytest.mark.parametrize("variant", ["damp_extrapolate", "polarizable"])
def test_scale_box_follows_volume_and_cutoff(variant):
    """+3 %, revert, -3 %, revert on the resident configuration: the long-range correction, the cutoff-free pair sum and
    the volume follow, bit for bit as a fresh context and within tolerance of the reference."""
    s, flags = pc.system("c320"), pc.VARIANTS[variant]
    mol = np.asarray(s["molecule"])
    ids = np.cumsum(np.concatenate([[0], mol[1:] != mol[:-1]]))
    nmol = ids[-1] + 1
    com = np.stack([s["pos"][ids == m].mean(axis=0) for m in range(nmol)])
    live = _engine(s, flags)
    live.energy()
    cur = dict(s, pos=s["pos"].copy(), basis=s["basis"].copy())
    for scale in (1.03, None, 0.97, None):
        if scale is not None:
            f = scale ** (1.0 / 3.0)
            delta, basis = com * (f - 1.0), s["basis"] * f
        else:
            delta, basis = -delta, s["basis"].copy()
        cur["pos"] = cur["pos"] + delta[ids]  # the very addition the engine does
        cur["basis"] = basis
        assert live.scale_box(basis, delta) is True
        a = live.energy()
        b, _ = _fresh(cur, flags)
        for fld in FIELDS:
            assert a[fld] == b[fld], (scale, fld, a[fld], b[fld])
        ref = ph.rd_terms(cur, flags)
        _check_rd(a, ref, "scale %s" % scale)
        assert a["volume"] == ref["volume"] and a["cutoff"] == ref["cutoff"]
    live.close()


def test_mode_switching():
    """insert / remove answer "upload again" in this mode; an upload without set_dispersion afterwards is Lennard-Jones
    again, bit for bit as on a context that never saw the PHAHST potential."""
    s, flags = pc.system("c130"), pc.VARIANTS["ewald"]
    lj, ljflags = synth.s_pol(130), dict(synth.FLAGS_POL_JACOBI)
    never = _engine(lj, ljflags, cap=192)
    want, want_dip = never.energy(), never.dipoles()
    never.close()
    e = _engine(s, flags, cap=192)
    phahst = e.energy()
    _check_rd(phahst, pc.reference("c130", "ewald"), "before the switch")
    idx = np.flatnonzero(np.asarray(s["molecule"]) == s["molecule"][-1])
    assert e.remove_molecule(int(idx[0]), len(idx)) is False
    z = np.zeros(1)
    assert e.insert_molecule(np.zeros((1, 3)), z, z, z + 3.5, z + 2.6, z + 2.0) is None
    assert e.energy() == phahst  # neither call changed anything
    e.load_system(lj, ljflags)  # upload without set_dispersion
    got = e.energy()
    assert got == want
    for k, v in e.dipoles().items():
        assert np.array_equal(v, want_dip[k]), k
    assert e.remove_molecule(125, 5) is True  # ... and device-side edits are back
    # switching the record off explicitly does the same as never sending it
    e.load_system(s, flags)
    assert e.energy() == phahst
    e.set_dispersion(s, disp_expansion=0)
    off = e.energy()
    bare, _ = _fresh(dict(s, c6=np.zeros(130), c8=np.zeros(130), c10=np.zeros(130)), ph.plain_flags(flags))
    assert off == bare
    e.close()


def test_two_contexts_side_by_side():
    a, b = _engine(pc.system("c130"), pc.VARIANTS["polarizable"]), _engine(pc.system("t130"), pc.VARIANTS["plain"])
    a.energy_begin()
    b.energy_begin()
    rb, ra = b.energy_end(), a.energy_end()
    _check_rd(ra, pc.reference("c130", "polarizable"), "context a")
    _check_rd(rb, pc.reference("t130", "plain"), "context b")
    a.close()
    b.close()


def _pqr_system(s):
    """s written as PQR text (reference column layout, c6 / c8 / c10 after omega and gwp_alpha) and read back the way the
    host layer reads it, so that both sides hold the same doubles"""
    lines, cols = [], []
    for i in range(len(s["charge"])):
        t = ["%.3f" % v for v in s["pos"][i]] + ["%.4f" % s["mass"][i], "%.5f" % (s["charge"][i] / synth.E2REDUCED),
                                                  "%.5f" % s["alpha"][i], "%.5f" % s["epsilon"][i], "%.5f" % s["sigma"][i],
                                                  "0.0", "0.0", "%.4f" % s["c6"][i], "%.4f" % s["c8"][i], "%.4f" % s["c10"][i]]
        lines.append("ATOM  %5d X    M   %s %4d   %s" % (i + 1, "F" if s["frozen"][i] else "M", s["molecule"][i], " ".join(t)))
        cols.append([float(x) for x in t])
    c = np.array(cols)
    out = dict(s, pos=c[:, 0:3].copy(), mass=c[:, 3].copy(), charge=c[:, 4] * synth.E2REDUCED, alpha=c[:, 5].copy(),
               epsilon=c[:, 6].copy(), sigma=c[:, 7].copy(), c6=c[:, 10].copy(), c8=c[:, 11].copy(), c10=c[:, 12].copy())
    return "\n".join(lines) + "\nEND\n", out


def test_driver_runs_a_phahst_input(tmp_path):
    """mpmc_hip on a PHAHST input written here (130 atoms): the rd column of its step-0 line is the engine's rd_energy of
    the same numbers, and that is the reference's."""
    text, s = _pqr_system(pc.system("c130"))
    (tmp_path / "in.pqr").write_text(text)
    L = float(s["basis"][0, 0])
    out = tmp_path / "energy.dat"
    (tmp_path / "input").write_text(
        "job_name phahst\nensemble nvt\npreset_seeds 4321\nnumsteps 4\ncorrtime 2\nmove_factor 0.01\nrot_factor 0.01\n"
        "temperature 77.0\npolarization on\npolar_damp_type exponential\npolar_damp 2.1304\npolar_iterative on\n"
        "polar_max_iter 10\nfeynman_hibbs on\nfeynman_hibbs_order 4\ndisp_expansion on\ndamp_dispersion on\n"
        "extrapolate_disp_coeffs on\nbasis1 %r 0 0\nbasis2 0 %r 0\nbasis3 0 0 %r\nhip on\npqr_input in.pqr\n"
        "energy_output %s\n" % (L, L, L, out))
    r = subprocess.run([host.EXE_PATH, str(tmp_path / "input")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = out.read_text().splitlines()
    assert lines[0].startswith("#step #energy #coulombic #rd #polar")
    t = lines[1].split()
    got, _ = _fresh(s, pc.VARIANTS["polarizable"])
    _check_rd(got, ph.rd_terms(s, pc.VARIANTS["polarizable"]), "pqr")
    assert t[0] == "0" and t[3] == "%.6f" % got["rd_energy"] and t[1] == "%.6f" % got["energy"]
    assert [l.split()[0] for l in lines[1:]] == ["0", "2", "4"]


def test_host_layer_chain_carries_the_engine_energy():
    """a short NVT chain through the C host layer in this mode: the energy it carries is a fresh context's energy of its
    final configuration"""
    s, flags = pc.system("c130"), pc.VARIANTS["polarizable"]
    h = host.HostSystem(s, flags, seed=5, move_factor=0.05, rot_factor=0.05)
    h.mc_steps(12)
    o = h.observables()
    assert o["accept"] + o["reject"] == 12
    got, _ = _fresh(dict(s, pos=h.positions()), flags)
    assert o["energy"] == got["energy"] and o["rd_energy"] == got["rd_energy"]
    h.close()


def test_lennard_jones_results_are_those_of_the_parent_commit():
    """Regression guard: an LJ + Ewald + Jacobi box of 320 atoms (no dispersion record) gives, bit for bit, the result
    fields stored in tests/golden/phahst_lj_guard.npz, which were produced by the build of the commit before this term
    existed, on the same kind of device."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "phahst_lj_guard.npz"))
    s, flags = synth.s_pol(320), dict(synth.FLAGS_POL_JACOBI)
    e = _engine(s, flags)
    first = e.energy()
    rng = np.random.default_rng(3)
    pos = s["pos"].copy()
    for k in (7, 23, 41):  # three single-molecule moves through the incremental paths
        new = pos[5 * k:5 * k + 5] + rng.uniform(-0.1, 0.1, 3)
        pos[5 * k:5 * k + 5] = new
        e.update_atoms(5 * k, new)
        last = e.energy()
    dip = e.dipoles()
    e.close()
    for f in FIELDS:
        assert first[f] == gold["first_" + f], (f, first[f], gold["first_" + f])
        assert last[f] == gold["last_" + f], (f, last[f], gold["last_" + f])
    assert np.array_equal(dip["mu"], gold["mu"]) and np.array_equal(dip["ef_static"], gold["ef_static"])
