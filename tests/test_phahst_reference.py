"""CPU checks of tests/phahst_reference.py itself, the yardstick of the PHAHST GPU tests (tests/test_gpu_phahst.py)."""
import math

import numpy as np
import pytest

import phahst_cases as pc
import phahst_reference as ph

C6_K = 0.021958709 / (3.166811429 * 0.000001)  # 1 Hartree Bohr^6 in K A^6 (pairs.c:185)


def test_damping_goes_to_one_and_is_exactly_zero_below_the_clamp():
    """f_n(x) = 1 - exp(-x) sum_{k<=n} x^k / k! ~ x^(n+1) / (n+1)! for small x: 1e-9 is reached at x = 0.18 (n = 6),
    0.43 (n = 8), 0.74 (n = 10); below that the reference returns exactly 0 (disp_expansion.c:173-176)."""
    for n in (6, 8, 10):
        big, kept = ph.tt_damping(n, np.array([100.0, 200.0]))
        assert kept.all() and np.all(np.abs(big - 1) < 1e-15)
        xs = np.array([0.0, 0.01, 0.1])
        small, kept = ph.tt_damping(n, xs)
        assert not kept.any() and np.all(small == 0) and np.all(ph.tt_damping64(n, xs) == 0.0)
        # just above the clamp the value is of the size of the leading term x^(n+1) / (n+1)!
        x = {6: 0.25, 8: 0.6, 10: 1.0}[n]
        f, kept = ph.tt_damping(n, np.array([x]))
        lead = x ** (n + 1) / math.factorial(n + 1)
        assert kept[0] and 1e-9 < float(f[0]) < lead and float(f[0]) > 0.3 * lead
        # monotone in x and between 0 and 1
        g, _ = ph.tt_damping(n, np.linspace(1.0, 40.0, 200))
        assert np.all(np.diff(g.astype(float)) >= 0) and 0 < float(g[0]) and float(g[-1]) <= 1
    # NaN (b_ij = 0 / 0) is "not > 1e-9": exactly 0
    assert ph.tt_damping64(6, np.array([np.nan]))[0] == 0.0


def _two_atoms(**kw):
    s = dict(pos=np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]]), epsilon=np.array([1.0, 1.0]), sigma=np.array([1.0, 3.0]),
             c6=np.array([1.0, 1.0]), c8=np.zeros(2), c10=np.zeros(2), molecule=np.array([1, 2]), frozen=np.zeros(2),
             basis=np.diag([20.0, 20.0, 20.0]), charge=np.zeros(2))
    s.update(kw)
    return s


def test_two_atoms_by_hand():
    """Two atoms 2 A apart in a 20 A cube (cutoff 10 A, volume 8000 A^3), b_1 = b_2 = 1 / A, rho = 1 and 3 A, c6 = 1 a.u.
    each, no c8 / c10:
        b_12 = 2 * 1 * 1 / (1 + 1) = 1,  rho_12 = 2,  c6_12 = sqrt(1 * 1) * 0.021958709 / 3.166811429e-6 = 6934.012... K A^6
        repulsion = 315.7750382111558 * exp(-1 * (2 - 2)) = 315.7750382111558 K
        undamped:  E = 315.7750382111558 - c6_12 / 2^6
        damped:    x = b_12 r = 2,  f6 = 1 - e^-2 (1 + 2 + 2 + 4/3 + 2/3 + 4/15 + 4/45) = 1 - e^-2 * 331/45 = 0.004533...
                   E = 315.7750382111558 - f6 * c6_12 / 64
        long-range correction (rd_lrc): pair  -4 pi c6_12 / (3 * 10^3) / 8000
                                        self  2 * (-4 pi * 1 / (3 * 10^3) / 8000)   <- c6 = 1, the atomic-unit value
    """
    assert abs(C6_K - 6934.012) < 1e-3
    und = ph.rd_terms(_two_atoms(), dict(rd_lrc=0))
    assert float(und["total"]) == pytest.approx(315.7750382111558 - C6_K / 64.0, rel=1e-15)
    f6 = 1.0 - math.exp(-2.0) * 331.0 / 45.0
    assert abs(f6 - 0.004533) < 1e-6
    dmp = ph.rd_terms(_two_atoms(), dict(rd_lrc=0, damp_dispersion=1))
    # (f6 itself carries the cancellation of 1 - 0.9955 in fp64: 1e-13 relative; the helper evaluates it in longdouble)
    assert float(dmp["total"]) == pytest.approx(315.7750382111558 - f6 * C6_K / 64.0, rel=1e-13)
    lrc = ph.rd_terms(_two_atoms(), dict(damp_dispersion=1))
    pair = -4.0 * math.pi * C6_K / 3000.0 / 8000.0
    self_ = 2.0 * (-4.0 * math.pi * 1.0 / 3000.0 / 8000.0)
    assert float(lrc["lrc_pair"]) == pytest.approx(pair, rel=1e-15)
    assert float(lrc["lrc_self"]) == pytest.approx(self_, rel=1e-15)
    assert float(lrc["total"]) == pytest.approx(float(dmp["total"]) + pair + self_, rel=1e-15)
    assert float(lrc["abs_sum"]) == pytest.approx(315.7750382111558 + f6 * C6_K / 64.0 + abs(pair) + abs(self_), rel=1e-13)
    row = und["table"][0]
    assert (row.i, row.j, row.rimg) == (0, 1, 2.0) and not row.beyond


def test_lrc_self_part_uses_unconverted_coefficients():
    """disp_expansion_lrc_self() reads atom->c6 / c8 / c10, which are still in atomic units (disp_expansion.c:19-38): the
    self part is ~6934 times smaller than a converted one would be.  Extrapolation applies to c10 there too."""
    s = _two_atoms(c8=np.array([10.0, 10.0]), c10=np.array([100.0, 100.0]))
    rc, vol = 10.0, 8000.0
    one = -4.0 * math.pi * (1.0 / (3 * rc ** 3) + 10.0 / (5 * rc ** 5) + 100.0 / (7 * rc ** 7)) / vol
    assert float(ph.rd_terms(s, {})["lrc_self"]) == pytest.approx(2 * one, rel=1e-15)
    ext = -4.0 * math.pi * (1.0 / (3 * rc ** 3) + 10.0 / (5 * rc ** 5) + (49.0 / 40.0 * 100.0) / (7 * rc ** 7)) / vol
    assert float(ph.rd_terms(s, dict(extrapolate_disp_coeffs=1))["lrc_self"]) == pytest.approx(2 * ext, rel=1e-15)
    converted = -4.0 * math.pi * (C6_K / (3 * rc ** 3)) / vol
    assert abs(float(ph.rd_terms(_two_atoms(), {})["lrc_self"])) < 1e-3 * abs(2 * converted)
    # frozen atoms have no self part, and a frozen-frozen pair no pair part; same-molecule pairs DO have a pair part
    assert float(ph.rd_terms(_two_atoms(frozen=np.ones(2)), {})["total"]) == 0.0
    same = ph.rd_terms(_two_atoms(molecule=np.array([1, 1])), {})
    assert float(same["pair_sum"]) == 0.0 and float(same["lrc_pair"]) == pytest.approx(-4.0 * math.pi * C6_K / 3000.0 / vol, rel=1e-15)


def test_exclusion_rule_and_literal_mixing():
    """rd-excluded only if a zero epsilon / sigma comes WITH six zero coefficients (pairs.c:68); b_ij = 0 / 0 = NaN is
    "!= 0" for the repulsion test, and a NaN damping factor is clamped to 0."""
    # a dispersion-only atom against a full one: not excluded; b_12 = 0 so no repulsion; undamped dispersion only
    s = _two_atoms(epsilon=np.array([1.0, 0.0]), sigma=np.array([1.0, 0.0]))
    r = ph.rd_terms(s, dict(rd_lrc=0))
    assert len(r["table"]) == 1 and float(r["total"]) == pytest.approx(-C6_K / 64.0, rel=1e-15)
    # ... damped: x = 0, f6 = 1 - 1 = 0, clamped: the pair contributes exactly 0
    assert float(ph.rd_terms(s, dict(rd_lrc=0, damp_dispersion=1))["total"]) == 0.0
    # no coefficients at all on either atom and a zero epsilon: excluded (no table row)
    s0 = _two_atoms(epsilon=np.array([1.0, 0.0]), c6=np.zeros(2))
    assert len(ph.rd_terms(s0, dict(rd_lrc=0))["table"]) == 0
    # both exponents 0 and a non-zero range: b_12 = NaN, rho_12 = 2: the repulsion is evaluated and is NaN
    sn = _two_atoms(epsilon=np.zeros(2))
    assert math.isnan(float(ph.rd_terms(sn, dict(rd_lrc=0))["total"]))
    # Schmidt mixing: b_12 = (1 + 3) * 1 * 3 / (1 + 9) = 1.2 instead of 2 * 1 * 3 / 4 = 1.5
    sm = _two_atoms(epsilon=np.array([1.0, 3.0]), c6=np.zeros(2), c8=np.array([1.0, 1.0]))
    rep = lambda b: 315.7750382111558 * math.exp(-b * (2.0 - 2.0))
    c8 = 0.0061490647 / (3.166811429 * 0.000001)
    assert float(ph.rd_terms(sm, dict(rd_lrc=0, schmidt_mixing=1))["total"]) == pytest.approx(rep(1.2) - c8 / 256.0, rel=1e-15)
    # extrapolation: c10_12 = 0 when c6_12 is 0, else 49/40 c8_12^2 / c6_12
    assert float(ph.rd_terms(sm, dict(rd_lrc=0, extrapolate_disp_coeffs=1))["total"]) == pytest.approx(rep(1.5) - c8 / 256.0, rel=1e-15)
    sx = _two_atoms(c8=np.array([1.0, 1.0]))
    want = 315.7750382111558 - C6_K / 64.0 - c8 / 256.0 - (49.0 / 40.0 * c8 * c8 / C6_K) / 1024.0
    assert float(ph.rd_terms(sx, dict(rd_lrc=0, extrapolate_disp_coeffs=1))["total"]) == pytest.approx(want, rel=1e-15)


@pytest.mark.parametrize("name", pc.INPUTS)
@pytest.mark.parametrize("variant", sorted(pc.VARIANTS))
def test_gpu_cases_tell_the_two_readings_apart(name, variant):
    """The inputs of tests/test_gpu_phahst.py against its tolerance tol = 1e-12 * sum |terms|:
      * applying the Lennard-Jones cutoff to the pair sum moves the total by more than 1e6 * tol, so the GPU test
        distinguishes "every pair" from "pairs within the cutoff";
      * the smallest beyond-cutoff pair term that is not exactly 0 exceeds 1e3 * tol, so ONE dropped pair fails it (a pair
        whose term is exactly 0 -- a damped pair with b_ij = 0 -- cannot change any sum);
      * a sizeable share of the pairs lies beyond the cutoff."""
    ref = pc.reference(name, variant)
    tol = pc.RD_TOL * float(ref["abs_sum"])
    t = ref["table"]
    assert t.beyond.sum() > 0.25 * len(t)
    cut = ph.rd_terms(pc.system(name), pc.VARIANTS[variant], pair_cutoff=True)
    assert abs(float(cut["total"] - ref["total"])) > 1e6 * tol
    e = np.abs(t.energy[t.beyond].astype(np.float64))
    # (exactly-zero terms are the damped pairs of the dispersion-only site, b_ij = 0: in every damped variant that site adds
    #  nothing to the pair sum, and only "extrapolate" and "plain" exercise its dispersion)
    assert e[e != 0.0].min() > 1e3 * tol
    if not pc.VARIANTS[variant].get("damp_dispersion"):
        s = pc.system(name)
        only, disp = (s["epsilon"] == 0) & (s["c6"] != 0), s["c6"] != 0
        hit = (only[t.i] & disp[t.j]) | (only[t.j] & disp[t.i])  # (against a site without coefficients the mixed ones are 0)
        assert hit.any() and (np.abs(t.energy[hit].astype(np.float64)) > 0).all()
    assert math.isfinite(float(ref["total"]))


def test_synthetic_box_has_the_three_kinds_of_site():
    s = pc.system("c320")
    eps, c6, q, frz = s["epsilon"], s["c6"], s["charge"], s["frozen"].astype(bool)
    assert len(eps) == 320 and frz.sum() == 106
    assert ((eps != 0) & (c6 != 0) & (q != 0) & ~frz).any()  # repulsion + dispersion + charge
    assert ((eps == 0) & (c6 != 0) & ~frz).any()             # dispersion only
    assert ((eps == 0) & (c6 == 0) & (q != 0) & ~frz).any()  # charge only
    assert abs(q.sum()) < 1e-9
    from mpmc_amd import synth
    assert synth.FLAGS_PHAHST == dict(synth.FLAGS_POL_JACOBI, disp_expansion=1, damp_dispersion=1,
                                      extrapolate_disp_coeffs=1, schmidt_mixing=0)
