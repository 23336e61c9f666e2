"""`mpmc_hip` on the `ensemble surf` fixtures of tests/golden/surf/: the driver prints the reference program's lines as
identical strings.  A value may instead differ by one unit of its last printed digit, but only where the longdouble model
from the pristine frame (tests/surf_fixtures.py) rounds to the DRIVER's string -- so that it is the reference program's
cumulative rotation that moved the digit -- and at most 1 value in 50 over the whole fixture set may take that exit."""
import os
import subprocess

import pytest

import surf_fixtures as sf

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "mpmc_amd", "host", "mpmc_hip")


def is_row(line):
    t = line.split()
    try:
        [float(x) for x in t]
    except ValueError:
        return False
    return len(t) >= 2


@pytest.fixture(scope="module")
def tally():
    t = dict(exits=0, total=0, cases=0)
    yield t
    if t["cases"] == len(sf.names()):  # (the whole set ran: the cap is over the set)
        assert t["exits"] * 50 <= t["total"], t


@pytest.mark.parametrize("name", sf.names())
def test_driver_prints_the_reference_lines(name, tally):
    res = subprocess.run([DRIVER, os.path.join(sf.GOLD, name, "input")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    got = [l.strip() for l in res.stdout.splitlines() if is_row(l)]
    want = sf.reference_lines(name)
    exits, total = sf.compare_lines(want, got)  # (fails on anything further apart than one unit of the last digit)
    if exits:
        model = sf.model_lines(name)
        for lw, lg, lm in zip(want, got, model):
            for w, g, m in zip(lw.split(), lg.split(), lm.split()):
                assert w == g or g == m, (name, "reference", lw, "driver", lg, "model", lm)
    tally["exits"] += exits
    tally["total"] += total
    tally["cases"] += 1
    print("SURF %s: %d of %d values one digit from the reference's" % (name, exits, total))
    assert tally["exits"] * 50 <= max(tally["total"], 133), tally


def test_preserve_mode_prints_five_columns_and_the_angles():
    res = subprocess.run([DRIVER, os.path.join(sf.GOLD, "n2_preserve_decomp", "input")], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=120)
    rows = [l.split() for l in res.stdout.splitlines() if is_row(l)]
    assert rows and all(len(r) == 5 and r[4] == "0.00000" for r in rows)
    res = subprocess.run([DRIVER, os.path.join(sf.GOLD, "n2_preserve_rotation", "input")], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=120)
    assert "SURFACE: Setting preserve angles (radians) for molecule 2: 1.100000 0.400000 2.000000" in res.stdout
