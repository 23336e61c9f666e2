"""Reference and inputs for mpmc_hip_trial_energies() (Engine.trial_energies).  Helper module for the tests (a plain
import, not a conftest).

trial_energy() computes the total energy of a configuration with one molecule REALLY moved to a placement, from the
per-pair longdouble functions of tests/pair_reference.py -- Lennard-Jones (+ Feynman-Hibbs, + long-range correction),
the real-space Ewald / Wolf term, ewald_recip_energy and ewald_self_energy -- so it shares nothing with the batched
kernels (kernels_trial.h), which never move the molecule and never form the full sums.  It also returns the sum of the
magnitudes of the terms of that full-system sum: the scale of the project's standing bound, 1e-12 of it.

build() makes the small boxes of tests/test_gpu_trial_energies.py: single-site background atoms (frozen framework or
all movable) on a jittered lattice of any cell, one rigid molecule of 1 .. 16 sites somewhere in the atom order, with
zero charges, zero epsilons and a negative sigma among both.  placements() makes rigid placements of the molecule:
random rotations about its first site plus a shift, the current placement, and translations that put the first site
within 5e-10 A of the cutoff from a background atom on either side, and on a half-box tie of the minimum image."""
import numpy as np

import pair_reference as pr
from mpmc_amd import synth

LD = np.longdouble
BOUND = 1.0e-12  # of sum |terms|: the project's standing bound on an fp64 evaluation of these sums


def moved(system, first, xyz):
    s = dict(system)
    pos = np.array(system["pos"], dtype=np.float64, copy=True)
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 3)
    pos[first:first + xyz.shape[0]] = xyz
    s["pos"] = pos
    return s


def static_terms(system, params):
    """The terms no re-placement changes: (lj long-range correction, Ewald self term), longdouble."""
    lrc = pr.lj_lrc(system, params)
    ewald = not params.get("rd_only") and not params.get("wolf")
    return lrc, (pr.ewald_self_energy(system, params)[0] if ewald else LD(0))


def trial_energy(system, params, first, xyz, static=None):
    """(total energy as energy() defines it, sum |terms|) with the molecule at slots first.. moved to xyz [k, 3]."""
    s = moved(system, first, xyz)
    lrc, self_e = static if static is not None else static_terms(system, params)
    tab = pr.pair_table(s, params, keep=0.0)
    total = tab["rd"].sum() + lrc
    mags = np.abs(tab["rd"]).sum() + abs(lrc)
    if not params.get("rd_only"):
        total += tab["es"].sum() - tab["es_intra"].sum()
        mags += np.abs(tab["es"]).sum() + np.abs(tab["es_intra"]).sum()
        if not params.get("wolf"):
            U, _ = pr.ewald_recip_energy(s, params)
            total += U + self_e
            mags += abs(U) + abs(self_e)
    return total, float(mags)


SHEARED = np.array([[25.0, 0, 0], [0.3 * 25.0, 0.9 * 25.0, 0], [-0.2 * 25.0, 0.25 * 25.0, 0.85 * 25.0]])  # adversarial.CELLS


def build(nbox, nsites, where, frozen_framework, cell="cubic", seed=0):
    """(system, first): nbox single-site background atoms + one molecule of nsites sites at `where` in the atom order
    ("start": slots 0 ..; "end": the last slots; "straddle": across the boundary of the first 64-atom block)."""
    rng = np.random.default_rng(9000 + 131 * nbox + 7 * nsites + seed)
    m = int(np.ceil((nbox + 1) ** (1.0 / 3.0) - 1e-9))
    basis = np.diag([3.6 * m] * 3) if cell == "cubic" else SHEARED.copy()
    idx = rng.permutation(m ** 3)[:nbox + 1]
    ijk = np.stack([idx // (m * m), (idx // m) % m, idx % m], axis=1)
    frac = (ijk + 0.5) / m - 0.5 + rng.uniform(-0.06, 0.06, size=(nbox + 1, 3)) / m
    sites = frac @ basis
    bg, centre = sites[:nbox], sites[nbox]
    sign = np.where(np.arange(nbox) % 2 == 0, 1.0, -1.0)
    q = 0.35 * sign * synth.E2REDUCED
    eps = np.full(nbox, 45.0) + 10.0 * (np.arange(nbox) % 3)
    sig = np.full(nbox, 2.9) + 0.1 * (np.arange(nbox) % 4)
    q[3::17] = 0.0
    eps[5::19] = 0.0
    sig[7::23] *= -1.0  # attractive-only: contributes exactly 0
    mass = np.full(nbox, 20.0)
    # the molecule: sites within ~0.8 A of its centre
    off = rng.normal(size=(nsites, 3))
    off *= (0.25 + 0.55 * rng.uniform(size=(nsites, 1))) / np.linalg.norm(off, axis=1, keepdims=True)
    off[0] = 0.0
    mq = rng.uniform(-0.4, 0.4, size=nsites) * synth.E2REDUCED
    meps = rng.uniform(5.0, 30.0, size=nsites)
    msig = rng.uniform(2.2, 3.0, size=nsites)
    mmass = rng.uniform(1.0, 4.0, size=nsites)
    if nsites >= 3:
        meps[1] = msig[1] = 0.0
        mq[2] = 0.0
    if nsites >= 5:
        msig[3] *= -1.0
    first = {"start": 0, "end": nbox, "straddle": 64 - nsites // 2}[where]
    assert 0 <= first <= nbox

    def ins(a, b):
        return np.concatenate([a[:first], b, a[first:]])

    n = nbox + nsites
    mol = np.concatenate([np.arange(first), np.full(nsites, first), np.arange(first + 1, nbox + 1)])
    frozen = ins(np.full(nbox, 1 if frozen_framework else 0), np.zeros(nsites, dtype=np.int64))
    system = dict(pos=np.ascontiguousarray(ins(bg, centre + off)), charge=ins(q, mq), alpha=np.zeros(n), epsilon=ins(eps, meps),
                  sigma=ins(sig, msig), mass=ins(mass, mmass), molecule=mol.astype(np.int32), frozen=frozen.astype(np.int32),
                  basis=basis)
    return system, first


def _rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def random_placements(system, first, nsites, count, seed=1):
    rng = np.random.default_rng(seed)
    cur = system["pos"][first:first + nsites]
    out = np.empty((count, nsites, 3))
    for t in range(count):
        out[t] = cur[0] + (cur - cur[0]) @ _rotation(rng).T + rng.uniform(-0.4, 0.4, size=3)
    return out


def edge_placements(system, params, first, nsites):
    """Translations of the molecule that put its first site at rc - 5e-10, rc + 5e-10 from a background atom (along a
    direction whose own image is the minimum image), and half a lattice vector (+ a small offset across it) away from
    one: a fractional component of the displacement on 0.5."""
    basis = np.asarray(system["basis"], dtype=np.float64)
    _, _, rc = pr.pbc(basis, params.get("pbc_cutoff", 0.0))
    cur = system["pos"][first:first + nsites]
    j = 0 if first > 0 else nsites  # a background atom
    pj = system["pos"][j]
    # a direction along which a displacement of length rc keeps every fractional component well below 0.5: it is its own image
    u = np.array([0.48, 0.62, 0.62]) if np.count_nonzero(basis - np.diag(np.diag(basis))) == 0 else \
        np.array([0.21, 0.23, 0.19]) @ basis
    u = u / np.linalg.norm(u)
    out = []
    for d in (rc - 5e-10, rc + 5e-10):
        out.append(cur + ((pj + d * u) - cur[0]))
    tie = 0.5 * basis[0] + 0.31 * basis[1] / np.linalg.norm(basis[1]) + 0.17 * basis[2] / np.linalg.norm(basis[2])
    out.append(cur + ((pj + tie) - cur[0]))
    return np.array(out)


def placements(system, params, first, nsites, nrandom=4, seed=1):
    cur = system["pos"][first:first + nsites]
    return np.concatenate([cur[None], random_placements(system, first, nsites, nrandom, seed),
                           edge_placements(system, params, first, nsites)])
