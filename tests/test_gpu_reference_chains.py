"""GPU: the mpmc_hip driver on the inputs of tests/golden/reference_chains/ against what the reference program wrote for
them -- the same seeds, so the same draws: every line of the energy file (tests/reference_chain_compare.py has the
rules) and the restart file after the last step.  One step taken another way -- another move or molecule drawn, a draw
consumed in another order, an acceptance factor with another prefactor, a cutoff left behind by the box, a list edited in
another place -- leaves the reference's chain for good, and the message names the first line that differs: with
`corrtime 1` the step of the first decision that fell differently.  tests/test_reference_chains.py ties the same fixtures
to the independent references on the CPU."""
import os
import shutil
import subprocess

import pytest

import reference_chain_compare as rcc
from mpmc_amd import host

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", rcc.NAMES)
def test_driver_walks_the_reference_chain(tmp_path, name):
    src = os.path.join(rcc.CHAINS, name)
    for f in ("input", "in.pqr"):
        shutil.copy(os.path.join(src, f), tmp_path / f)
    r = subprocess.run([host.EXE_PATH, "input"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    worst = rcc.compare_energy(rcc.energy_lines(tmp_path / "energy.dat"),
                               rcc.energy_lines(os.path.join(src, "reference_energy.dat")))
    print("%s: largest deviation from the reference's printed energies: %s K" % (name, worst))
    moved = rcc.compare_restart(tmp_path / "restart.pqr", os.path.join(src, "reference_restart.pqr"))
    print("%s: largest deviation from the reference's restart coordinates: %s A" % (name, moved))
    # pqr_output numbers the molecules as the restart file does: in list order, so that a reader keeps an inserted
    # molecule apart from the neighbour it was copied from
    ids = [line.split()[5] for line in open(tmp_path / "out.pqr") if line.startswith("ATOM")]
    assert ids == [a[3] for a in rcc.restart_atoms(tmp_path / "restart.pqr")[0]]
