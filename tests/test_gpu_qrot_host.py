"""`quantum_rotation on` through the host layer on the device (mpmc_amd/host/qrot.c).

The driver runs the reference's own sample (one BSS H2 at a sorption site of MOF-5, `ensemble total_energy`, l_max 7, 64
levels; tests/golden/qrot/) and its printed DEBUG_QROT lines are parsed back and held to the independent model of
tests/qrot_reference.py.

The level bound.  The model takes the 256 grid energies from Engine.trial_energies() on PYTHON-made placements, so the
two Hamiltonians differ by (a) the energies: both sets are within dE = 1e-12 * sum |terms| of the true ones
(tests/test_gpu_trial_energies.py holds that bound; sum |terms| is under-estimated here by |rd| + |es_real| + |es_recip| +
|es_self| of the configuration, which only tightens it), twice that between the two; (b) the quadrature: a matrix element
is sum_pt (pi^2 / 2) w_p w_t sin(theta_t) conj(Y_i) Y_j E_pt, so |dH_ij| <= W * 2 dE with W = sum_pt (pi^2 / 2) w_p w_t
sin(theta_t) max_i |Y_i|^2 (qrot_reference.quadrature_weight_norm), and by Weyl |dlambda| <= ||dH||_F <= dim W 2 dE;
(c) fp64 sums of 256 products against the model's longdouble sums: 64 * 256 u ||H||_F per element bound as in
tests/test_qrot_reference.py, times dim; (d) the C Jacobi against eigh: 8 (sweeps + 1) dim u ||H||_F with the 9 sweeps
its CPU tests see at dim 64 .. 81 (10 taken); (e) the print: %.6f, 5e-7 K.

A hindered-rotor `nvt` chain with spin flips is held, draw by draw, to the model: all epsilons are zero under rd_only,
so every energy is exactly 0 and the model needs no device energy -- what it checks is the order of the draws
(checkpoint, the flip, the 128 symmetry points of every level of every movable molecule, Metropolis), the acceptance
rot_partfunc * exp(0), the counters and spin_ratio.  A chain of four BSS H2 in a 20 A box on the real potential checks
that a spin-flip step leaves the configuration's observables and makes one trial-energy call per movable molecule."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import qrot_reference as qr
from mpmc_amd import engine, host, pqr, synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "qrot")
DRIVER = os.path.join(ROOT, "mpmc_amd", "host", "mpmc_hip")
U = 2.0 ** -53
LINE = re.compile(r"DEBUG_QROT: molecule #(\d+) \((\S+)\) rotational level (\d+) = (\S+) K \((\S+) cm\^-1 or (\S+) meV or "
                  r"(\S+) / B\) \*\*\* (symmetric|antisymmetric) \*\*\*")
B, L_MAX, LEVELS, NSUM, T = 85.35060622, 7, 64, 10, 50.0
BASIS = np.diag([25.669] * 3)


@pytest.mark.parametrize("site", ["MOF5+alpha.pdb", "MOF5+H2.beta.pdb", "MOF5+H2.gamma.pdb", "MOF5+H2.delta.pdb"])
def test_the_driver_on_the_sample(site, tmp_path):
    shutil.copy(os.path.join(GOLD, "MOF5+QR.inp"), tmp_path / "MOF5+QR.inp")
    shutil.copy(os.path.join(GOLD, site), tmp_path / "input.pqr")
    with open(tmp_path / "MOF5+QR.inp", "a") as f:
        f.write("preset_seeds 20121\n")
    out = subprocess.run([DRIVER, str(tmp_path / "MOF5+QR.inp")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [LINE.match(l) for l in out.stdout.splitlines() if l.startswith("DEBUG_QROT: molecule")]
    assert len(rows) == LEVELS and all(rows)
    levels = np.array([float(r.group(4)) for r in rows])
    sym = [0 if r.group(8) == "symmetric" else 1 for r in rows]
    assert [int(r.group(3)) for r in rows] == list(range(LEVELS)) and {r.group(2) for r in rows} == {"H2"}
    for r, e in zip(rows, levels):  # the other units of the line are the same number
        assert abs(float(r.group(5)) - e * 1.3806503e-23 / (100.0 * 6.626068e-34 * 2.99792458e8)) < 1e-6 + 1e-6 * abs(e)
        assert abs(float(r.group(6)) - 8.61733238e-2 * (e - levels[0])) < 2e-6 + 1e-6 * abs(e)
        assert abs(float(r.group(7)) - e / B) < 1e-6 + 1e-7 * abs(e)

    # ---- the model, on device energies of Python-made placements
    system = pqr.read_pqr(str(tmp_path / "input.pqr"), BASIS)
    flags = dict(temperature=T, rd_lrc=0)
    movable = np.flatnonzero(np.asarray(system["frozen"]) == 0)
    first, k = int(movable[0]), len(movable)
    assert k >= 2 and (np.diff(movable) == 1).all()
    mass, pos = system["mass"][first:first + k], system["pos"][first:first + k]
    com, tot = np.zeros(3), 0.0
    for s in range(k):  # update_com(): summed in site order
        tot += mass[s]
        com += mass[s] * pos[s]
    com /= tot
    eng = engine.Engine(len(system["charge"]), device=0)
    try:
        eng.load_system(system, flags)
        e0 = eng.energy()
        E = eng.trial_energies(first, qr.placements(pos, com))
    finally:
        eng.close()
    V = (np.sin(qr.THETA_C)[None, :] * E.reshape(16, 16)).T  # V[t][p] = sin(theta_t) E[p * 16 + t]
    rng = qr.new_rng(20121)
    want, wsym, pf, _ = qr.evaluate(V, L_MAX, B, LEVELS, NSUM, T, qr.PARA, rng)
    dim = (L_MAX + 1) ** 2
    dE = 1e-12 * (abs(e0["rd_energy"]) + abs(e0["es_real"]) + abs(e0["es_recip"]) + abs(e0["es_self"]))
    normH = np.linalg.norm(qr.hamiltonian(V, L_MAX, B))
    bound = (dim * qr.quadrature_weight_norm(L_MAX) * 2 * dE + dim * 64 * 256 * U * normH + 8 * 11 * dim * U * normH + 5e-7)
    worst = np.abs(levels - want).max()
    print("%s: E = %.6f K, level 0 = %.6f K, 1 - 0 = %.4f meV, largest |level - model| = %.3e K (bound %.3e K)"
          % (site, e0["energy"], levels[0], 8.61733238e-2 * (levels[1] - levels[0]), worst, bound))
    print("%s levels - level 0 (meV): %s" % (site, " ".join("%.3f" % (8.61733238e-2 * (x - levels[0])) for x in levels[:10])))
    assert worst <= bound
    # ---- symmetries and partition functions, from the same random numbers: the host layer on the same input and seed
    # (the driver prints no partition function).  A level closer than 1e3 * bound to a neighbour is exempt from the symmetry
    # comparison -- there the eigenvector, and with it the sign the reference's test reads off, is the solver's -- and the
    # count of exempt levels is printed; none of the quantum_rotation_sum levels behind the partition functions may be.
    hflags = dict(flags, quantum_rotation=1, quantum_rotation_B=B, quantum_rotation_l_max=L_MAX,
                  quantum_rotation_level_max=LEVELS, quantum_rotation_sum=NSUM)
    hs = host.HostSystem(system, hflags, seed=20121)
    try:
        hs.energy()
        hs.qrot_evaluate()
        got = hs.rotational_levels()
        assert hs.qrot_counts()["trial_calls"] == 1 and len(got) == 1 and len(got[0]["levels"]) == LEVELS
        got = got[0]
    finally:
        hs.close()
    assert np.abs(got["levels"] - levels).max() <= 5e-7 and list(got["symmetry"]) == sym  # what the driver printed
    gaps = np.minimum(np.diff(want, prepend=-np.inf), np.diff(want, append=np.inf))
    clear = gaps > 1e3 * bound
    print("%s: %d of %d levels exempt from the symmetry comparison (gap to a neighbour below %.1e K)"
          % (site, int((~clear).sum()), LEVELS, 1e3 * bound))
    assert clear[:NSUM].all() and clear.sum() >= LEVELS // 2
    assert [s for s, c in zip(sym, clear) if c] == [s for s, c in zip(wsym, clear) if c]
    tol = 2.0 * bound / T + 1e-12  # d exp(-E / T) / exp(-E / T) = dE / T
    for key, val in zip(("rot_partfunc_g", "rot_partfunc_u", "rot_partfunc"), pf):
        assert abs(got[key] - val) <= tol * max(abs(val), 1e-300), (key, got[key], val)
    assert got["nuclear_spin"] == qr.PARA


def _zero_energy_system(nmol=3):
    system = synth.s_pol(5 * nmol)
    system = dict(system)
    system["epsilon"] = np.zeros_like(system["epsilon"])
    return system


def test_hindered_rotor_chain_with_spin_flips_is_the_model_s():
    nmol, steps, seed, p_flip = 3, 40, 9191, 0.5
    l_max, level_max, nsum, barrier = 2, 9, 5, 10.0
    flags = dict(temperature=T, rd_only=1, quantum_rotation=1, quantum_rotation_hindered=1,
                 quantum_rotation_hindered_barrier=barrier, quantum_rotation_B=B, quantum_rotation_l_max=l_max,
                 quantum_rotation_level_max=level_max, quantum_rotation_sum=nsum)
    hs = host.HostSystem(_zero_energy_system(nmol), flags, seed=seed, extra=dict(spinflip_probability=p_flip))
    try:
        rng = qr.new_rng(seed)
        V = qr.hindered_grid(B, barrier)

        def evaluate_all(spins):
            return [qr.evaluate(V, l_max, B, level_max, nsum, T, s, rng) for s in spins]

        spins = [qr.PARA] * nmol
        ev = evaluate_all(spins)  # mc.c:253-256, after the first energy()
        kinds, accepted = [], []
        kind, pick = qr.movetype_draw(rng, "nvt", p_flip)
        for step in range(steps):
            assert hs.mc_steps(1) >= 0
            assert hs.lib.host_last_movetype(hs.ptr) in (2, 4)  # (what checkpoint() drew for the NEXT step)
            altered = int(np.floor(pick * nmol))
            trial = list(spins)
            if kind == "spinflip":
                trial[altered] = qr.PARA if rng.rand() < 0.5 else qr.ORTHO
                ev_trial = evaluate_all(trial)  # mc.c:304-308: every movable molecule, after the flip
                bf = ev_trial[altered][2][2]    # rot_partfunc * exp(-0 / T)
            else:
                for _ in range(10):  # translate 6 + rotate 4
                    rng.rand()
                ev_trial, bf = ev, 1.0
            ok = rng.rand() < bf
            if ok:
                spins, ev = trial, ev_trial
            kinds.append(kind)
            accepted.append(ok)
            got = hs.rotational_levels()
            c = hs.qrot_counts()
            assert [g["nuclear_spin"] for g in got] == spins, step
            assert hs.spin_ratio() == sum(sp == qr.PARA for sp in spins) / nmol, step
            assert hs.lib.host_last_movetype(hs.ptr) in (2, 4)
            assert c["accept_spinflip"] == sum(a for a, kd in zip(accepted, kinds) if kd == "spinflip")
            assert c["reject_spinflip"] == sum(not a for a, kd in zip(accepted, kinds) if kd == "spinflip")
            assert hs.observables()["accept"] == sum(accepted)
            for g, (lev, sym, pf, _) in zip(got, ev):
                assert np.abs(g["levels"] - lev).max() < 1e-9 and list(g["symmetry"]) == list(sym)
                assert abs(g["rot_partfunc"] - pf[2]) < 1e-12 and abs(g["rot_partfunc_g"] - pf[0]) < 1e-12
            kind, pick = qr.movetype_draw(rng, "nvt", p_flip)
        assert {"spinflip", "displace"} <= set(kinds) and 0 < sum(accepted) < steps
        assert c["trial_calls"] == 0  # the hindered rotor needs no energy
        assert abs(hs.lib.host_get_rand(hs.ptr) - rng.rand()) == 0.0  # the generators are still in step
    finally:
        hs.close()


def test_spin_flip_chain_on_the_real_potential_is_the_model_s():
    """Four BSS H2 in a 20 A box, nvt, spinflip_probability 0.5, 30 seeded steps, against the Python model driven by device
    energies: the model draws from its own generator in the chain's order, takes a displacement's trial energy from the
    host layer (the Metropolis factor is then its own exp(-dE / T)), and after a flip evaluates every movable molecule
    itself -- Python-made placements through Engine.trial_energies() on a context of its own, model Hamiltonian, eigh, its
    symmetry test -- for rot_partfunc.  Per step: the move type, the acceptance, the counters, every spin, spin_ratio; after
    a flip the levels; and the observables after a spin-flip step are those of the configuration (OWNED DEVIATION: the
    reference leaves the last grid orientation's behind).  One trial-energy call per movable molecule per evaluation."""
    nmol, steps, seed, p_flip = 4, 30, 515, 0.5
    l_max, level_max, nsum = 2, 9, 5
    system = dict(synth.s_pol(5 * nmol))
    system["basis"] = np.diag([20.0] * 3)
    eflags = dict(temperature=T)
    flags = dict(eflags, quantum_rotation=1, quantum_rotation_B=B, quantum_rotation_l_max=l_max,
                 quantum_rotation_level_max=level_max, quantum_rotation_sum=nsum)
    hs = host.HostSystem(system, flags, seed=seed, extra=dict(spinflip_probability=p_flip), move_factor=0.05, rot_factor=0.05)
    eng = engine.Engine(5 * nmol, device=0)
    try:
        eng.load_system(system, eflags)
        rng = qr.new_rng(seed)
        mass = np.asarray(system["mass"])

        def evaluate_all(pos, spins):
            eng.update_atoms(0, pos)
            eng.energy()
            out = []
            for m in range(nmol):
                p, w = pos[5 * m:5 * m + 5], mass[5 * m:5 * m + 5]
                com, tot = np.zeros(3), 0.0
                for k in range(5):  # update_com(): summed in site order
                    tot += w[k]
                    com += w[k] * p[k]
                com /= tot
                E = eng.trial_energies(5 * m, qr.placements(p, com))
                V = (np.sin(qr.THETA_C)[None, :] * E.reshape(16, 16)).T
                out.append(qr.evaluate(V, l_max, B, level_max, nsum, T, spins[m], rng))
            return out

        assert hs.mc_steps(0) == 0  # the first energy(), the first evaluation, the first checkpoint()
        assert hs.qrot_counts()["trial_calls"] == nmol
        spins = [qr.PARA] * nmol
        pos = hs.positions().copy()
        ev = evaluate_all(pos, spins)
        kinds, accepted = [], []
        kind, pick = qr.movetype_draw(rng, "nvt", p_flip)
        for step in range(steps):
            assert hs.next_movetype() == kind, step
            before = hs.observables()
            assert hs.mc_steps(1) >= 0
            e_trial = hs.last_energy()
            altered = int(np.floor(pick * nmol))
            trial = list(spins)
            if kind == "spinflip":
                trial[altered] = qr.PARA if rng.rand() < 0.5 else qr.ORTHO
                ev_trial = evaluate_all(pos, trial)
                assert e_trial == before["energy"]  # nothing moved
                bf = ev_trial[altered][2][2] * np.exp(-(e_trial - before["energy"]) / T)
            else:
                for _ in range(10):  # translate 6 + rotate 4
                    rng.rand()
                ev_trial = ev
                bf = np.exp(-(e_trial - before["energy"]) / T) if np.isfinite(e_trial) else 0.0
            ok = bool(rng.rand() < bf)
            kinds.append(kind)
            accepted.append(ok)
            after, c, got = hs.observables(), hs.qrot_counts(), hs.rotational_levels()
            if ok:
                spins, ev = trial, ev_trial
                if kind == "displace":
                    pos = hs.positions().copy()
                    assert after["energy"] == e_trial
            assert np.array_equal(hs.positions(), pos), step
            if not ok or kind == "spinflip":  # the observables are those of the configuration
                for key in ("energy", "coulombic_energy", "rd_energy", "polarization_energy"):
                    assert after[key] == before[key], (step, key)
            assert after["accept"] == sum(accepted) and after["reject"] == len(accepted) - sum(accepted), step
            flips = [a for a, kd in zip(accepted, kinds) if kd == "spinflip"]
            assert c["accept_spinflip"] == sum(flips) and c["reject_spinflip"] == len(flips) - sum(flips), step
            assert c["trial_calls"] == nmol * (1 + len(flips)), step
            assert [g["nuclear_spin"] for g in got] == spins, step
            assert hs.spin_ratio() == sum(sp == qr.PARA for sp in spins) / nmol, step
            if kind == "spinflip" and ok:
                for g, (lev, sym, pf, _) in zip(got, ev):
                    assert np.abs(g["levels"] - lev).max() < 1e-6 and list(g["symmetry"]) == list(sym), step
                    assert abs(g["rot_partfunc"] - pf[2]) < 1e-7, step
            kind, pick = qr.movetype_draw(rng, "nvt", p_flip)
        assert {"spinflip", "displace"} <= set(kinds) and len(flips) > 3
        print("real-potential chain: %d flips (%d accepted), %d displacements (%d accepted), spin_ratio %.2f"
              % (len(flips), sum(flips), steps - len(flips), sum(accepted) - sum(flips), hs.spin_ratio()))
    finally:
        hs.close()
        eng.close()
