"""Synthetic periodic boxes: S-LJ(N), S-ES(N), S-POL(N), S-PHAHST(N) for disp_expansion and S-AT(N) for
axilrod_teller.

Deterministic (seeded) inputs of the shapes BASELINE.json names, used by bench.py and the
parity tests.  Units as the reference reads them: Angstrom, K, charges already multiplied by
E2REDUCED (reference src/io/read_pqr.c:249).
"""
import numpy as np

E2REDUCED = 408.7816

# BSSP H2, parameters from the reference's sample_configs_gpu/cuda_pol.small/small.initial.pdb:1-5
# (site, offset along the molecular axis, mass, charge/e, alpha, epsilon, sigma)
BSSP_SITES = [
    ("H2G", 0.0, 0.0, -0.7464, 0.69380, 12.76532, 3.15528),
    ("H2E", 0.371, 1.008, 0.3732, 0.00044, 0.0, 0.0),
    ("H2E", -0.371, 1.008, 0.3732, 0.00044, 0.0, 0.0),
    ("H2N", 0.363, 0.0, 0.0, 0.0, 2.16726, 2.37031),
    ("H2N", -0.363, 0.0, 0.0, 0.0, 2.16726, 2.37031),
]


def _lattice(nmol, spacing, jitter, rng):
    m = int(np.ceil(nmol ** (1.0 / 3.0) - 1e-9))
    L = spacing * m
    idx = np.arange(m ** 3)
    ijk = np.stack([idx // (m * m), (idx // m) % m, idx % m], axis=1)[:nmol]
    com = (ijk + 0.5) * spacing - 0.5 * L
    com = com + rng.uniform(-jitter, jitter, size=com.shape)
    return com, L


def _random_axes(n, rng):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _finish(pos, q, alpha, eps, sig, mass, mol, frozen, L):
    return dict(
        pos=np.ascontiguousarray(pos, dtype=np.float64),
        charge=np.asarray(q, dtype=np.float64) * E2REDUCED,
        alpha=np.asarray(alpha, dtype=np.float64),
        epsilon=np.asarray(eps, dtype=np.float64),
        sigma=np.asarray(sig, dtype=np.float64),
        mass=np.asarray(mass, dtype=np.float64),
        molecule=np.asarray(mol, dtype=np.int32),
        frozen=np.asarray(frozen, dtype=np.int32),
        basis=np.diag([L, L, L]).astype(np.float64),
    )


def s_lj(n, seed=None):
    """N single-site LJ atoms (eps 120 K, sigma 3.4 A) on a jittered cubic lattice, spacing 3.8 A."""
    rng = np.random.default_rng(1234 + n if seed is None else seed)
    com, L = _lattice(n, 3.8, 0.3, rng)
    z = np.zeros(n)
    return _finish(com, z, z, np.full(n, 120.0), np.full(n, 3.4), np.full(n, 39.948), np.arange(1, n + 1), z, L)


def s_es(n, seed=None):
    """N/2 rigid dimers (bond 1.0 A, q = +-0.4 e, LJ on site 1), spacing 3.8 A."""
    rng = np.random.default_rng(2234 + n if seed is None else seed)
    nmol = n // 2
    com, L = _lattice(nmol, 3.8, 0.3, rng)
    ax = _random_axes(nmol, rng)
    pos = np.empty((2 * nmol, 3))
    pos[0::2] = com + 0.5 * ax
    pos[1::2] = com - 0.5 * ax
    q = np.tile([0.4, -0.4], nmol)
    eps = np.tile([120.0, 0.0], nmol)
    sig = np.tile([3.4, 0.0], nmol)
    mass = np.tile([20.0, 20.0], nmol)
    mol = np.repeat(np.arange(1, nmol + 1), 2)
    z = np.zeros(2 * nmol)
    return _finish(pos, q, z, eps, sig, mass, mol, z, L)


def s_pol(n, seed=None, spacing=3.6):
    """floor(N/5) five-site BSSP H2 molecules (+ N mod 5 single LJ sites so that the atom count is
    exactly N), COMs on a jittered cubic lattice (spacing 3.6 A), random orientations."""
    rng = np.random.default_rng(3234 + n if seed is None else seed)
    nmol = n // 5
    extra = n - 5 * nmol
    com, L = _lattice(nmol + extra, spacing, 0.3, rng)
    ax = _random_axes(nmol, rng)
    pos, q, alpha, eps, sig, mass, mol = [], [], [], [], [], [], []
    for m in range(nmol):
        for (_, off, ms, qq, al, ep, sg) in BSSP_SITES:
            pos.append(com[m] + off * ax[m])
            q.append(qq)
            alpha.append(al)
            eps.append(ep)
            sig.append(sg)
            mass.append(ms)
            mol.append(m + 1)
    for e in range(extra):
        pos.append(com[nmol + e])
        q.append(0.0)
        alpha.append(0.0)
        eps.append(10.22)
        sig.append(2.556)
        mass.append(4.0026)
        mol.append(nmol + e + 1)
    return _finish(np.array(pos), q, alpha, eps, sig, mass, mol, np.zeros(n), L)


# A three-site PHAHST sorbate in the style of the reference group's H2 models (exponent b in 1/A in the epsilon column,
# range rho in A in the sigma column, C6 / C8 / C10 in atomic units): a centre with repulsion, dispersion and a charge, a
# dispersion-only site (epsilon = sigma = 0) and a charge-only site.  Round numbers of the right magnitude, not a
# published parameter set.
# (site, offset along the molecular axis, mass, charge/e, alpha, b, rho, c6, c8, c10)
PHAHST_SITES = [
    ("H2G", 0.0, 2.016, -0.7464, 0.69380, 3.5, 2.6, 9.0, 160.0, 4000.0),
    ("H2N", 0.363, 0.0, 0.0, 0.0, 0.0, 0.0, 1.5, 20.0, 300.0),
    ("H2E", -0.371, 0.0, 0.7464, 0.00044, 0.0, 0.0, 0.0, 0.0, 0.0),
]
# a frozen framework atom: repulsion, dispersion, charge and polarizability
PHAHST_FRAMEWORK = (12.011, 0.1, 1.2, 3.2, 3.1, 25.0, 600.0, 18000.0)


def s_phahst(n, seed=None, spacing=3.6):
    """s_pol's geometry for the PHAHST potential: the first third of the lattice sites (rounded down) holds single frozen
    framework atoms (charges alternate in sign), the rest of the atoms are three-site sorbate molecules, plus single movable
    centre sites so that the atom count is exactly N.  Carries c6, c8, c10 (atomic units) next to the usual arrays."""
    rng = np.random.default_rng(4234 + n if seed is None else seed)
    nfr = n // 3
    nmol = (n - nfr) // 3
    extra = n - nfr - 3 * nmol
    com, L = _lattice(nfr + nmol + extra, spacing, 0.3, rng)
    com = com[rng.permutation(len(com))]  # framework and sorbate interleaved in space
    ax = _random_axes(nmol, rng)
    rows, pos = [], []
    ms, qq, al, b, rho, c6, c8, c10 = PHAHST_FRAMEWORK
    for f in range(nfr):
        pos.append(com[f])
        rows.append((qq if f % 2 == 0 else -qq, al, b, rho, ms, f + 1, 1, c6, c8, c10))
    if nfr % 2:  # keep the cell neutral
        rows[-1] = (0.0,) + rows[-1][1:]
    for m in range(nmol):
        for (_, off, ms, qq, al, b, rho, c6, c8, c10) in PHAHST_SITES:
            pos.append(com[nfr + m] + off * ax[m])
            rows.append((qq, al, b, rho, ms, nfr + m + 1, 0, c6, c8, c10))
    _, _, ms, _, al, b, rho, c6, c8, c10 = PHAHST_SITES[0]
    for e in range(extra):
        pos.append(com[nfr + nmol + e])
        rows.append((0.0, al, b, rho, ms, nfr + nmol + e + 1, 0, c6, c8, c10))
    r = np.array(rows, dtype=np.float64)
    out = _finish(np.array(pos), r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5], r[:, 6], L)
    out.update(c6=r[:, 7].copy(), c8=r[:, 8].copy(), c10=r[:, 9].copy())
    return out


# Sites of the three-body box (Angstrom^3, K, Angstrom, atomic units): an argon-like atom, the two sites of a rigid
# nitrogen-like dimer and a carbon-like framework atom.  Magnitudes of the published values, not a parameter set.
# (mass, charge/e, alpha, epsilon, sigma, c6, c9)
AT_ATOM = (39.948, 0.0, 1.6411, 119.8, 3.405, 64.3, 518.3)
AT_DIMER = ((14.0067, 0.2, 0.80, 36.0, 3.31, 24.0, 100.0), (14.0067, -0.2, 0.80, 36.0, 3.31, 24.0, 100.0))
AT_DIMER_BOND = 1.10
AT_FRAMEWORK = (12.011, 0.0, 1.20, 50.0, 3.40, 40.0, 250.0)


def s_at(n, seed=None, spacing=3.8):
    """A box for the Axilrod-Teller term (axilrod_teller): the first third of the atoms (rounded down) is ONE frozen
    multi-atom framework molecule on a slab of the lattice; then (n - n/3) / 4 rigid two-site sorbates with both sites
    active -- preceded by one single atom when that makes a dimer sit on atoms 127 / 128, across a 64-atom block
    boundary --; the rest are single argon-like atoms, of which every 7th has polarizability 0 and every 5th has a
    polarizability but c9 = 0.  Carries c6 and c9 (atomic units) next to the usual arrays."""
    rng = np.random.default_rng(5234 + n if seed is None else seed)
    nfr = n // 3
    ndim = (n - nfr) // 4
    lead = 1 if nfr % 2 == 0 else 0  # dimers then start on an odd atom index: one of them straddles every block boundary
    nsingle = n - nfr - 2 * ndim
    com, L = _lattice(nfr + ndim + nsingle, spacing, 0.3, rng)
    rest = nfr + rng.permutation(ndim + nsingle)  # sorbate sites in random order; the framework keeps its slab
    ax = _random_axes(ndim, rng)
    rows, pos = [], []

    def add(p, site, mol, frozen, alpha=None, c9=None):
        ms, qq, al, ep, sg, c6, c9_ = site
        pos.append(p)
        rows.append((qq, al if alpha is None else alpha, ep, sg, ms, mol, frozen, c6, c9_ if c9 is None else c9))

    for f in range(nfr):
        add(com[f], AT_FRAMEWORK, 1, 1)
    site, mol = 0, 2
    singles = 0

    def single():
        nonlocal site, mol, singles
        kind = singles % 7 == 3, singles % 5 == 2
        add(com[rest[site]], AT_ATOM, mol, 0, alpha=0.0 if kind[0] else None, c9=0.0 if (kind[1] and not kind[0]) else None)
        site, mol, singles = site + 1, mol + 1, singles + 1

    for _ in range(lead):
        single()
    for m in range(ndim):
        c = com[rest[site]]
        add(c + 0.5 * AT_DIMER_BOND * ax[m], AT_DIMER[0], mol, 0)
        add(c - 0.5 * AT_DIMER_BOND * ax[m], AT_DIMER[1], mol, 0)
        site, mol = site + 1, mol + 1
    for _ in range(nsingle - lead):
        single()
    r = np.array(rows, dtype=np.float64)
    out = _finish(np.array(pos), r[:, 0], r[:, 1], r[:, 2], r[:, 3], r[:, 4], r[:, 5], r[:, 6], L)
    out.update(c6=r[:, 7].copy(), c9=r[:, 8].copy())
    return out


# flag sets (reference config keywords) used with the synthetic polarizable boxes
FLAGS_POL_JACOBI = dict(temperature=77.0, polarization=1, polar_damp=2.1304, polar_max_iter=10,
                        feynman_hibbs=1, feynman_hibbs_order=4)
FLAGS_POL_PRODUCTION = dict(temperature=77.0, polarization=1, polar_damp=2.1304, polar_wolf=1,
                            polar_wolf_alpha=0.13, polar_gs_ranked=1, polar_palmo=1, polar_gamma=1.03,
                            polar_max_iter=4)
# the polarizable set with the PHAHST repulsion / dispersion (Tang-Toennies damping, C10 extrapolated, default mixing)
FLAGS_PHAHST = dict(FLAGS_POL_JACOBI, disp_expansion=1, damp_dispersion=1, extrapolate_disp_coeffs=1, schmidt_mixing=0)
FLAGS_LJ = dict(temperature=100.0, rd_only=1)
# Lennard-Jones + Ewald with the three-body term (per-atom c9 as read; add midzuno_kihara_approx=1 for 3/4 alpha c6)
FLAGS_AT = dict(temperature=100.0, axilrod_teller=1)
FLAGS_ES = dict(temperature=100.0)
