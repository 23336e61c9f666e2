"""Grand-canonical chains through the C host layer in the dense energy modes: insertions and removals reach the device as
ONE mpmc_hip_edit_molecules call per change of N (sync_walk() in mpmc_amd/host/energy_hip.c) instead of a full upload.

As tests/test_gpu_host.py::test_uvt_incremental_edits_match_full_reuploads: one chain runs with edits, the same seed runs
with incremental_amatrix = 0 -- the engine then answers "upload again" to every edit, which is what every chain in these
modes did before the entry existed.  Same decisions, same atom counts, energies equal to 1e-10 (that test's number; the two
arms keep different atom orders), the final configuration against the modes' independent references, and
host_get_sync_counts() says which arm edited and which uploaded.

CHAINS: seed, fugacity (the `pressure` keyword) and insert_probability were chosen on the RE-UPLOADING arm -- the one that
does not run the code under test -- as the first of a small scan in which that arm sees at least 3 distinct N, 3 accepted
insertions and 3 accepted removals within the steps below; the conditions are asserted for both arms.
"""
import numpy as np
import pytest

import at_reference as ar
import phahst_reference as ph
import rdc_reference as rr
import rdforms_reference as rf
import test_gpu_at as t_at
import test_gpu_phahst as t_phahst
import test_gpu_rd_crystal as t_rdc
import test_gpu_rdforms as t_rdf
from mpmc_amd import host, synth

pytestmark = pytest.mark.gpu


def _phahst(n=160):
    return synth.s_phahst(n, spacing=4.5)


def _phahst_c9(n=160):
    s = _phahst(n)
    return dict(s, c9=8.0 * s["c6"])


def _pol(n=160):
    return synth.s_pol(n, spacing=4.5)


POLAR4 = dict(synth.FLAGS_PHAHST, polar_max_iter=4, rd_lrc=1)
MODES = {
    "phahst": (_phahst, POLAR4),
    "phahst_at": (_phahst_c9, dict(POLAR4, axilrod_teller=1)),
    "dreiding": (_pol, dict(temperature=77.0, rd_lrc=1, dreiding=1)),
    "rd_crystal": (_pol, dict(temperature=77.0, rd_only=1, rd_lrc=1, rd_crystal=1, rd_crystal_order=2)),
}
# mode -> (seed, pressure, insert_probability, steps)
CHAINS = {
    "phahst": (33, 300.0, 0.7, 120),
    "phahst_at": (33, 300.0, 0.7, 120),
    "dreiding": (33, 300.0, 0.7, 120),
    "rd_crystal": (33, 300.0, 0.7, 120),
}


def chain(mode, seed, pressure, insert_probability, steps, incremental):
    """One uvt chain, a step at a time.  Returns (the HostSystem, [(accepted, natoms, energy)] per step)."""
    make, flags = MODES[mode]
    h = host.HostSystem(make(), flags, seed=seed, move_factor=0.05, rot_factor=0.05,
                        extra={"ensemble": "uvt", "insert_probability": insert_probability, "pressure": pressure})
    h.energy()  # creates the context
    h.set_option("incremental_amatrix", incremental)  # 0: the engine asks for re-uploads instead of edits
    trace = []
    for _ in range(steps):
        acc = h.mc_steps(1)
        trace.append((acc, h.natoms(), h.observables()["energy"]))
    return h, trace


def census(trace, n0):
    """(distinct N, accepted insertions, accepted removals) of a trace that started from n0 atoms"""
    ns, ins, rem, n = {n0}, 0, 0, n0
    for acc, natoms, _ in trace:
        ns.add(natoms)
        if acc and natoms > n:
            ins += 1
        if acc and natoms < n:
            rem += 1
        n = natoms
    return len(ns), ins, rem


def _final_system(h, basis, flags):
    s = h.system(basis)
    n = h.natoms()
    if flags.get("disp_expansion"):
        c = {k: np.zeros(n) for k in ("c6", "c8", "c10")}
        h.lib.host_get_dispersion(h.ptr, c["c6"].ctypes.data, c["c8"].ctypes.data, c["c10"].ctypes.data)
        s.update(c)
    if flags.get("axilrod_teller"):
        c9 = np.zeros(n)
        h.lib.host_get_c9(h.ptr, c9.ctypes.data)
        s["c9"] = c9
    return s


def _against_references(h, mode, flags, basis):
    e = h.energy()  # the device may still hold a rejected trial: evaluate the configuration the chain kept
    o = h.observables()
    assert e == o["energy"]
    s = _final_system(h, basis, flags)
    got = dict(rd_energy=o["rd_energy"], status=0, cutoff=o["cutoff"], volume=o["volume"])
    what = "%s, final configuration of %d atoms" % (mode, h.natoms())
    if flags.get("disp_expansion"):
        t_phahst._check_rd(got, ph.rd_terms(s, flags), what)
    elif flags.get("rd_crystal"):
        t_rdc._check_rd(got, dict(rr.rd_terms(s, flags, 2), order=2), what)
    else:
        t_rdf._check_rd(got, rf.rd_terms(s, flags, "dreiding", "lb"), what)
    if flags.get("axilrod_teller"):
        t_at._check(h.three_body_energy(), ar.unordered(s, False), what)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_uvt_chain_edits_instead_of_uploading(mode):
    make, flags = MODES[mode]
    seed, pressure, insert_probability, steps = CHAINS[mode]
    n0 = len(make()["charge"])
    # one chain after the other: the host layer has ONE Mersenne twister per process, like the reference
    (edits, t_edit), (uploads, t_up) = [chain(mode, seed, pressure, insert_probability, steps, k) for k in (1, 0)]
    for name, t in (("editing", t_edit), ("re-uploading", t_up)):
        ns, ins, rem = census(t, n0)
        print("%s, %s arm: %d distinct N, %d accepted insertions, %d accepted removals" % (mode, name, ns, ins, rem))
        assert ns >= 3 and ins >= 3 and rem >= 3, (name, ns, ins, rem)
    for k, (a, b) in enumerate(zip(t_edit, t_up)):
        assert a[0] == b[0] and a[1] == b[1], (k, a, b)
        assert abs(a[2] - b[2]) <= 1e-10 * max(1.0, abs(b[2])), (k, a, b)
    changes = sum(1 for k in range(steps) if t_edit[k][1] != (t_edit[k - 1][1] if k else n0))
    ce, cu = edits.sync_counts(), uploads.sync_counts()
    print("%s: N changed %d times; editing arm %s; re-uploading arm %s" % (mode, changes, ce, cu))
    assert ce["full_uploads"] == 1 and ce["molecules_edited"] >= changes and ce["edit_calls"] >= 1
    assert cu["edit_calls"] == 0 and cu["molecules_edited"] == 0 and cu["full_uploads"] > changes
    basis = make()["basis"]
    for h in (edits, uploads):
        _against_references(h, mode, flags, basis)
        h.close()
