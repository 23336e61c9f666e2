"""Molecules, placements and flag sets of the dimer tests (tests/test_dimer_reference.py, tests/test_gpu_dimer.py): small
rigid molecules of 1 .. 16 sites with zero-charge, zero-epsilon and non-polarizable sites mixed in, and the five-site N2
model.  Sites of one molecule lie inside a sphere of 1.6 A, at least 0.6 A apart; placements keep the centres 5.5 A or more
apart, so sites of different molecules are never closer than 2.3 A (the tests never place two sites on each other)."""
import numpy as np

E2REDUCED = 408.7816  # e -> sqrt(K A), read_pqr.c:249
DAMP = 2.1304


def n2():
    """the five-site N2 of the reference's 014-n2_virial_coef sample: a zero-mass centre and zero-parameter sites included"""
    return dict(pos=np.array([[0.0, 0.0, 0.0], [0.549, 0.0, 0.0], [-0.549, 0.0, 0.0], [0.653, 0.0, 0.0], [-0.653, 0.0, 0.0]]),
                charge=np.array([1.04742, -0.47103, -0.47103, -0.05268, -0.05268]) * E2REDUCED,
                alpha=np.array([1.1, 0.3, 0.3, 0.0, 0.0]), epsilon=np.array([17.60293, 0.0, 0.0, 18.12618, 18.12618]),
                sigma=np.array([3.44522, 0.0, 0.0, 3.30426, 3.30426]), mass=np.array([0.0, 14.0067, 14.0067, 0.0, 0.0]))


def molecule(n, seed, polarizable=True, phahst=False):
    """n sites, reproducible; every third site has charge 0, every fourth epsilon 0 (and sigma 0 on every eighth), every
    fifth polarizability 0 (all of them with polarizable=False)."""
    rng = np.random.default_rng(1000 + 37 * n + seed)
    pos = []
    while len(pos) < n:
        p = rng.uniform(-1.6, 1.6, 3)
        if np.linalg.norm(p) <= 1.6 and all(np.linalg.norm(p - q) >= 0.6 for q in pos):
            pos.append(p)
    k = np.arange(n)
    m = dict(pos=np.array(pos) + rng.uniform(-3.0, 3.0, 3),  # (the entry takes the centre of mass out)
             charge=np.where(k % 3 == 1, 0.0, rng.uniform(-0.5, 0.5, n)) * E2REDUCED,
             alpha=np.where((k % 5 == 2) | (not polarizable), 0.0, rng.uniform(0.03, 0.15, n)),
             epsilon=np.where(k % 4 == 3, 0.0, rng.uniform(5.0, 40.0, n)),
             sigma=np.where(k % 8 == 7, 0.0, rng.uniform(2.4, 3.4, n)),
             mass=np.where(k % 6 == 5, 0.0, rng.uniform(1.0, 16.0, n)))
    if n == 1:
        m["mass"] = np.array([4.0026])
    if phahst:  # epsilon = the exponent b (1/A), sigma = the range rho (A), c6 / c8 / c10 in atomic units
        # (a site without repulsion has no dispersion either: two such sites would mix to b = 0 / 0, which the reference
        #  follows into NaN)
        null = (k % 4 == 3) | (k % 7 == 6)
        m["epsilon"] = np.where(k % 4 == 3, 0.0, rng.uniform(2.5, 4.0, n))
        m["sigma"] = np.where(k % 8 == 7, 0.0, rng.uniform(1.8, 2.6, n))
        m["c6"] = np.where(null, 0.0, rng.uniform(4.0, 30.0, n))
        m["c8"] = np.where(null, 0.0, rng.uniform(80.0, 600.0, n))
        m["c10"] = np.where(null, 0.0, rng.uniform(2000.0, 20000.0, n))
    return m


def placements(n, seed=0, rmin=5.5, rmax=7.0):
    rng = np.random.default_rng(77 + seed)
    conf = rng.uniform(0.0, 2.0 * np.pi, (n, 7))
    conf[:, 0] = rng.uniform(rmin, rmax, n)
    conf[:, 2] *= 0.5
    conf[:, 5] *= 0.5
    return conf


SHAPES = [(1, 1), (1, 16), (16, 1), (5, 5), (15, 16), (16, 16)]
SOLVERS = {
    "jacobi4": dict(polar_damp=DAMP, polar_max_iter=4),
    "gs3": dict(polar_damp=DAMP, polar_gs=1, polar_max_iter=3),
    "ranked_palmo5": dict(polar_damp=DAMP, polar_gs_ranked=1, polar_palmo=1, polar_max_iter=5),
    "precision": dict(polar_damp=DAMP, polar_gs=1, polar_precision=1e-6, polar_max_iter=0),
    "jacobi_precision_gamma": dict(polar_damp=DAMP, polar_precision=1e-5, polar_max_iter=0, polar_gamma=1.03),
}
MODELS = {
    "linear": dict(polar_damp=DAMP, polar_damp_type="linear", polar_gs_ranked=1, polar_palmo=1, polar_max_iter=4),
    "off": dict(polar_damp=0.0, polar_damp_type="off", polar_max_iter=4),
}
RD = {
    "lb": dict(rd_only=1),
    "waldmanhagler": dict(rd_only=1, waldmanhagler=1),
    "halgren_mixing": dict(rd_only=1, halgren_mixing=1),
    "c6_mixing": dict(rd_only=1, c6_mixing=1),
}
PHAHST = {
    "damped_extrapolated": dict(disp_expansion=1, damp_dispersion=1, extrapolate_disp_coeffs=1, **SOLVERS["ranked_palmo5"]),
    "schmidt": dict(disp_expansion=1, damp_dispersion=1, schmidt_mixing=1, rd_only=1),
    "plain": dict(disp_expansion=1, rd_only=1),
}
