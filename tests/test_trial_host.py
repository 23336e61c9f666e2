"""mpmc_hip_trial_energies(): what can be checked without a device -- the entry is declared, exported and bound, and the
reference and the inputs of tests/test_gpu_trial_energies.py are what that file says they are."""
import os
import re

import numpy as np

import pair_reference as pr
import trial_reference as tr
from mpmc_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entry_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "mpmc_hip.h")).read()
    assert re.search(r"int mpmc_hip_trial_energies\(mpmc_hip_ctx \*ctx, int first_slot, int count, int ntrial, const double "
                     r"\*xyz, double \*energy,\s+double \*terms\);", src)
    lib = engine.load()
    for name in ("mpmc_hip_trial_energies", "mpmc_hip_trial_call_count"):
        assert hasattr(lib, name) and name in engine.EXPORTS
    assert callable(engine.Engine.trial_energies) and callable(engine.Engine.trial_call_count)
    assert '"trial_batched"' in open(os.path.join(ROOT, "mpmc_amd", "csrc", "engine.hip")).read()


def test_the_reference_of_the_current_placement_is_the_system_s_energy():
    system, first = tr.build(65, 5, "straddle", True)
    flags = dict(temperature=77.0, feynman_hibbs=1, feynman_hibbs_order=2)
    e, mags = tr.trial_energy(system, flags, first, system["pos"][first:first + 5])
    tab = pr.pair_table(system, flags)
    want = (tab["rd"].sum() + pr.lj_lrc(system, flags) + tab["es"].sum() - tab["es_intra"].sum()
            + pr.ewald_recip_energy(system, flags)[0] + pr.ewald_self_energy(system, flags)[0])
    assert e == want and mags >= abs(float(e))


def test_the_inputs_are_what_they_claim():
    for cell in ("cubic", "sheared"):
        for where, nsites in (("start", 1), ("end", 16), ("straddle", 5)):
            system, first = tr.build(130, nsites, where, True, cell)
            mol, frozen = system["molecule"], system["frozen"]
            assert (mol[first:first + nsites] == mol[first]).all() and (mol == mol[first]).sum() == nsites
            assert not frozen[first:first + nsites].any() and frozen.sum() == 130
            assert first == {"start": 0, "end": 130, "straddle": 62}[where]
            assert (system["charge"] == 0).any() and (system["epsilon"] == 0).any() and (system["sigma"] < 0).any()
            flags = dict(temperature=77.0)
            xyz = tr.placements(system, flags, first, nsites)
            cur = system["pos"][first:first + nsites]
            for p in xyz:  # rigid: the same site-site distances
                assert np.allclose(np.linalg.norm(p[:, None] - p[None], axis=2), np.linalg.norm(cur[:, None] - cur[None], axis=2),
                                   rtol=0, atol=1e-12)
            _, rb, rc = pr.pbc(system["basis"])
            j = 0 if first > 0 else nsites
            d = xyz[-3:, 0] - system["pos"][j]
            _, _, rimg, _ = pr.minimum_image(system["basis"], rb, d)
            assert -1e-9 < rimg[0] - rc < 0 < rimg[1] - rc < 1e-9  # either side of every cutoff comparison
            frac = d[2] @ rb  # f_p = sum_q rb[q][p] d_q
            assert abs(frac[0] - 0.5) < 1e-12  # a half-box tie
