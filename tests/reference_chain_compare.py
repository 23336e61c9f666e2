"""The comparison of a driver run with what the reference program wrote for the same seeded input (a plain helper module,
shared by tests/test_gpu_reference_chains.py, tests/test_gpu_cavity_host.py and, for the reading, by
tests/test_reference_chains.py).

An energy file is the reference's `energy_output`: a header and one line of twelve `%f` columns per corrtime.  The printed
strings are compared as decimals, so a bound of one unit of the last digit is exact and not a matter of how a double
rounds 1e-6:

  step, N                           identical strings: every move, molecule, insertion and removal fell as in the reference
  kinetic, kin_temp, core_temp      identical strings (constants of the run)
  volume                            within one unit of the last printed digit, 1e-6 A^3
  energy, coulombic, rd, polar, vdw |got - want| <= 1e-6 + 1e-10 |want|: one unit of the `%f` both programs print, and
                                    the per-term device-vs-oracle tolerance of tests/test_gpu_parity.py
  spin_ratio                        not compared (the host layer holds no nuclear spin states and prints 0)

A restart file is the reference's `pqr_restart`: ATOM lines with `%8.3f` coordinates (BOX marker atoms aside) and the box
as REMARK BOX BASIS lines with 14 decimals.
"""
import os
from decimal import Decimal

COLUMNS = ["step", "energy", "coulombic", "rd", "polar", "vdw", "kinetic", "kin_temp", "N", "spin_ratio", "volume", "core_temp"]
HEADER = " ".join("#" + c for c in COLUMNS)
ENERGY_COLUMNS = (1, 2, 3, 4, 5)
IDENTICAL = (0, 8, 6, 7, 11)
VOLUME = 10
UNIT = Decimal("0.000001")
RELATIVE = Decimal("1e-10")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHAINS = os.path.join(GOLDEN, "reference_chains")
# the table of the fixtures: DESIGN.md section 14
NAMES = ("nvt_jacobi", "nvt_production", "nvt_ewald_fh_sheared", "npt_jacobi", "npt_default_probability",
         "uvt_polar_framework", "uvt_phahst", "nvt_sg_fh", "uvt_buffered_14_7_halgren", "nvt_axilrod_teller",
         "nvt_rd_crystal", "nvt_exact_linear")


def energy_lines(path):
    return open(path).read().splitlines()


def rows(lines):
    """the data lines as lists of strings"""
    return [line.split() for line in lines[1:]]


def compare_energy(got, want):
    """got, want: the lines of two energy files.  Returns the worst |got - want| over the energy columns (a Decimal);
    raises AssertionError naming the first differing line and column, with the previous line of both files."""
    assert got[0] == want[0] == HEADER, (got[0], want[0])
    assert len(got) == len(want), "the driver wrote %d lines, the reference %d" % (len(got), len(want))
    worst = Decimal(0)
    prev = ("", "")
    for k in range(1, len(want)):
        g, w = got[k].split(), want[k].split()
        assert len(g) == len(w) == len(COLUMNS), (k, got[k], want[k])

        def fail(col, what):
            raise AssertionError(
                "line %d (step %s), column #%s: %s: driver %s, reference %s\n  previous line, driver:    %s\n"
                "  previous line, reference: %s\n  this line, driver:        %s\n  this line, reference:     %s" % (
                    k + 1, w[0], COLUMNS[col], what, g[col], w[col], prev[0], prev[1], got[k], want[k]))

        for col in IDENTICAL:
            if g[col] != w[col]:
                fail(col, "not the same string")
        if abs(Decimal(g[VOLUME]) - Decimal(w[VOLUME])) > UNIT:
            fail(VOLUME, "more than one unit of the last digit apart")
        for col in ENERGY_COLUMNS:
            d = abs(Decimal(g[col]) - Decimal(w[col]))
            if not d <= UNIT + RELATIVE * abs(Decimal(w[col])):  # (a nan compares false)
                fail(col, "|difference| %s above 1e-6 + 1e-10 |reference|" % d)
            worst = max(worst, d)
        prev = (got[k], want[k])
    return worst


def restart_atoms(path):
    """(atoms, basis) of a restart file: per ATOM line that is no BOX marker its (atom type, molecule type, F|M, molecule
    number, x, y, z) as strings; the nine strings of the REMARK BOX BASIS lines"""
    atoms, basis = [], []
    for line in open(path):
        t = line.split()
        if not t:
            continue
        if t[0] == "ATOM" and t[3] != "BOX":
            atoms.append((t[2], t[3], t[4], t[5], t[6], t[7], t[8]))
        elif t[:3] == ["REMARK", "BOX", "BASIS[%d]" % (len(basis) // 3)]:
            basis += t[4:7]
    return atoms, basis


def compare_restart(got_path, want_path):
    """Same number of atoms; per atom the same site and molecule type, frozen flag and molecule number (the list order
    after every insertion and removal), coordinates within one unit of the reference's last printed digit; the box within
    one unit of its last printed digit.  Returns the worst coordinate difference (a Decimal)."""
    got, gb = restart_atoms(got_path)
    want, wb = restart_atoms(want_path)
    assert len(got) == len(want), "the driver's restart file has %d atoms, the reference's %d" % (len(got), len(want))
    worst = Decimal(0)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g[:4] == w[:4], "atom %d: driver %s, reference %s" % (k + 1, g, w)
        for p in range(4, 7):
            digits = len(w[p].split(".")[1])
            d = abs(Decimal(g[p]) - Decimal(w[p]))
            assert d <= Decimal(1).scaleb(-digits), "atom %d, coordinate %d: driver %s, reference %s" % (k + 1, p - 4, g, w)
            worst = max(worst, d)
    assert len(gb) == len(wb) == 9, (gb, wb)
    for g, w in zip(gb, wb):
        assert abs(Decimal(g) - Decimal(w)) <= Decimal(1).scaleb(-len(w.split(".")[1])), ("box", gb, wb)
    return worst
