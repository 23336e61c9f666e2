"""CPU-only checks of mpmc_hip_edit_molecules: the entry is declared and exported, mpmc_hip_molecule has the layout of its
ctypes mirror, tests/edit_model.py predicts the slots of every script the GPU tests run, and the host layer forms the
effective c9 with the arithmetic of engine.effective_c9."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import dense_edit_cases as dc
from mpmc_amd import engine, host, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "mpmc_hip.h")


def test_the_header_declares_the_entry_and_the_library_exports_it():
    src = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    assert re.search(r"\bint\s+mpmc_hip_edit_molecules\s*\(\s*mpmc_hip_ctx\s*\*", src)
    assert re.search(r"#define\s+MPMC_HIP_ABI_VERSION\s+1\b", src)
    lib = engine.load()
    assert hasattr(lib, "mpmc_hip_edit_molecules") and "mpmc_hip_edit_molecules" in engine.EXPORTS
    assert lib.mpmc_hip_abi_version() == 1
    # a null context is an error, not a crash
    assert lib.mpmc_hip_edit_molecules(None, 0, None, None, 0, None, None) < 0
    assert b"edit_molecules" in lib.mpmc_hip_last_error()
    # the old entries are still there, and the header says what they cannot carry
    assert hasattr(lib, "mpmc_hip_insert_molecule") and hasattr(lib, "mpmc_hip_remove_molecule")
    assert "cannot carry the per-atom data of the dense energy modes" in " ".join(open(HDR).read().replace("*", " ").split())


def test_the_molecule_record_matches_its_ctypes_mirror(tmp_path):
    fields = [f for f, _ in engine.Molecule._fields_]
    assert fields == ["count", "frozen", "x", "y", "z", "charge", "polarizability", "epsilon", "sigma", "mass", "c6", "c8",
                      "c10", "c9"]
    prog = tmp_path / "layout.c"
    prog.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpmc_hip.h"\n'
                    'int main(void){printf("%zu %zu %zu %zu %zu\\n", sizeof(mpmc_hip_molecule),'
                    ' offsetof(mpmc_hip_molecule, frozen), offsetof(mpmc_hip_molecule, x), offsetof(mpmc_hip_molecule, c6),'
                    ' offsetof(mpmc_hip_molecule, c9));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    M = engine.Molecule
    assert got == [C.sizeof(M), M.frozen.offset, M.x.offset, M.c6.offset, M.c9.offset]


@pytest.mark.parametrize("mode,script", dc.CASES, ids=["%s-%s" % c for c in dc.CASES])
@pytest.mark.parametrize("each", [False, True], ids=["at_end", "per_edit"])
def test_the_model_predicts_the_slots_of_every_script(mode, script, each):
    """the scripts assert the slots they are written for (60 .. 64 across the block edge, the hole that is taken, the
    molecule that is appended, npad 128 -> 256); run on the model alone they must hold, and leave a consistent layout"""
    n, fn = dc.SCRIPTS[script]
    sim = dc.Sim(mode, n)
    assert sim.model.slot_count == n and sim.model.grids()[0] == 128 * ((n + 127) // 128)
    fn(sim, sim.evaluate if each else (lambda: None))
    sim.evaluate()
    sim.model.check_invariants()
    s = sim.live_system()
    assert len(s["charge"]) == sim.model.n_atoms
    for k in dc.EXTRA:
        assert (k in s) == (k in dc.system(mode, n))
    # a hole keeps none of the modes' per-atom data
    for k in dc.EXTRA:
        assert not sim.extra[k][sim.model.hole_slots()].any()


def test_the_scripts_cover_the_shapes_they_name():
    sim = dc.Sim("phahst_lrc", 60)
    dc.edge(sim, lambda: None)
    first, count = sim.model.molecules[sim.mol_at(60)]
    assert (first, count) == (60, 5) and first // 64 != (first + count - 1) // 64
    sim = dc.Sim("lj_at", 130)
    dc.last_block(sim, lambda: None)
    assert sim.model.slot_count == 130 and list(sim.model.hole_slots()[-2:]) == [128, 129]
    sim = dc.Sim("rd_crystal", 130)
    dc.eight(sim, lambda: None)
    assert len(sim.model.molecules) == 26
    sim = dc.Sim("phahst_at", 70)
    before = int(sim.model.frozen.sum())
    dc.frozen(sim, lambda: None)
    assert int(sim.model.frozen.sum()) == before + 5 and before > 0


def test_the_host_layer_forms_the_effective_c9_as_the_binding_does():
    lib = host.load()
    s = synth.s_at(130)
    s = dict(s, alpha=np.concatenate([s["alpha"][:-3], [0.0, 1e-3, 7.25]]))
    for mk in (0, 1):
        want = engine.effective_c9(s, bool(mk))
        got = np.array([lib.host_effective_c9(mk, float(a), float(c6), float(c9))
                        for a, c6, c9 in zip(s["alpha"], s["c6"], s["c9"])])
        assert np.array_equal(got, want), mk
    assert not np.array_equal(engine.effective_c9(s, True), engine.effective_c9(s, False))


def test_the_sync_counters_are_exported_and_start_at_zero():
    lib = host.load()
    assert hasattr(lib, "host_get_sync_counts")
    h = host.HostSystem(synth.s_phahst(60), dict(synth.FLAGS_PHAHST))
    assert h.sync_counts() == dict(full_uploads=0, edit_calls=0, molecules_edited=0)
    h.close()
