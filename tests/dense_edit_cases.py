"""Modes, molecules and edit scripts of the mpmc_hip_edit_molecules tests (a plain helper module, no conftest).

A script is a function of a `Sim`: tests/edit_model.py's Model -- which predicts the slots of the new entry exactly as it
predicts those of insert_molecule / remove_molecule, the slot rules being the same -- together with the per-atom arrays of
the dense modes (c6, c8, c10, c9), which the model does not know.  tests/test_dense_edits_host.py runs every script on a
Sim alone (no device) and checks the slots the scripts are written for; tests/test_gpu_dense_edits.py runs them on a
`Live`, a Sim that carries out each operation on an engine as well and compares what the engine answers with what the
model says.

The shapes are the smallest at which the path can go wrong: 60 atoms (one block, an appended molecule crosses the block
edge at 64), 126 (an appended molecule takes npad from 128 to 256: every partial layout moves), 130 (three blocks, the
last with two atoms).
"""
import itertools

import numpy as np

import edit_model
import rdforms_cases as rfc
from mpmc_amd import engine, synth

EXTRA = ("c6", "c8", "c10", "c9")
MODE_KEYS = frozenset(engine.DISP_NAMES + engine.AT_NAMES + engine.RDC_NAMES + engine.RDFORM_NAMES)
MAX_MOLECULES = 8  # removals / insertions per call
CAP_EXTRA = 160     # head-room of every context: no script fills it


def _phahst_c9(n):
    s = synth.s_phahst(n)
    return dict(s, c9=8.0 * s["c6"])  # a three-body coefficient of the magnitude of synth.s_at's (c6 64, c9 518)


def _pol_frozen(n):
    """synth.s_pol with its first two molecules frozen: frozen-frozen pairs to exclude from the sums and the corrections"""
    s = synth.s_pol(n)
    frozen = s["frozen"].copy()
    frozen[:10] = 1
    return dict(s, frozen=frozen)


# name -> (system of n atoms, flags)
MODES = {
    "phahst": (synth.s_phahst, dict(synth.FLAGS_PHAHST, rd_lrc=0)),
    "phahst_lrc": (synth.s_phahst, dict(synth.FLAGS_PHAHST, rd_lrc=1)),
    "phahst_at": (_phahst_c9, dict(synth.FLAGS_PHAHST, rd_lrc=1, axilrod_teller=1)),
    "lj_at": (synth.s_at, dict(synth.FLAGS_AT, rd_lrc=1)),
    "rd_crystal": (_pol_frozen, dict(temperature=77.0, rd_only=1, rd_lrc=1, rd_crystal=1, rd_crystal_order=2)),
    "lj_wh_fh4": (_pol_frozen, dict(rfc.FH4, rd_only=1, waldmanhagler=1)),
    "sg": (_pol_frozen, dict(rfc.BASE, rd_only=1, sg=1)),
    "dreiding": (_pol_frozen, dict(rfc.BASE, rd_only=1, dreiding=1)),
    "lj_buffered_14_7": (_pol_frozen, dict(rfc.BASE, rd_only=1, lj_buffered_14_7=1)),
}

_systems = {}


def system(mode, n):
    """built once, never modified"""
    if (mode, n) not in _systems:
        _systems[mode, n] = MODES[mode][0](n)
    return _systems[mode, n]


def flags(mode):
    return MODES[mode][1]


# the 26 neighbours of the origin on a 0.45 A grid, nearest first: where the atoms a molecule is grown by go
_GRID = 0.45 * np.array(sorted((p for p in itertools.product((-1, 0, 1), repeat=3) if any(p)),
                               key=lambda p: (sum(x * x for x in p), p)), dtype=np.float64)


def grown(mol, count, centre):
    """A molecule of `count` atoms made from `mol` (a dict as Sim.molecule() gives): its own atoms in their own geometry,
    then copies of its first atom without charge and polarizability on a 0.45 A grid around that atom (pairs on one
    molecule are in no pair sum), all moved so that the first atom sits at `centre`.  (Only `mol`'s own sites are
    polarizable: close polarizable sites on one molecule would make the dipole iteration diverge, which is not what these
    tests are about.)"""
    k0 = len(mol["charge"])
    out = {}
    take = [i if i < k0 else 0 for i in range(count)]
    for key in edit_model.FIELDS + EXTRA:
        out[key] = np.array([mol[key][i] for i in take], dtype=np.float64)
    for i in range(k0, count):
        out["charge"][i] = 0.0
        out["alpha"][i] = 0.0
    pos = np.array([mol["pos"][i] - mol["pos"][0] if i < k0 else _GRID[i - k0] for i in range(count)])
    out["pos"] = pos + np.asarray(centre, dtype=np.float64)
    out["frozen"] = 0
    return out


class Sim:
    """edit_model.Model + the dense modes' per-atom arrays, driven by molecule ids"""

    def __init__(self, mode, n):
        s, f = system(mode, n), flags(mode)
        self.mode, self.flags, self.start = mode, f, s
        self.cap = len(s["charge"]) + CAP_EXTRA
        self.model = edit_model.Model(s, {k: v for k, v in f.items() if k not in MODE_KEYS}, self.cap)
        self.extra = {k: np.zeros(self.cap) for k in EXTRA}
        for k in EXTRA:
            if k in s:
                self.extra[k][:len(s[k])] = s[k]
        self.spacing = float(s["basis"][0][0]) / round(float(s["basis"][0][0]) / 3.7)
        self.model.energy()  # (a context takes edits once it has been evaluated)

    # ---- what the scripts read
    def movable(self):
        """ids of the molecules a script may remove, in slot order"""
        m = self.model
        return [k for k, (first, count) in sorted(m.molecules.items(), key=lambda kv: kv[1][0])
                if not m.frozen[first] and count <= edit_model.MAX_EDIT]

    def molecule(self, mol):
        m = self.model
        first, count = m.molecules[mol]
        sl = slice(first, first + count)
        out = {k: m.prop[k][sl].copy() for k in edit_model.FIELDS}
        out.update({k: self.extra[k][sl].copy() for k in EXTRA})
        out.update(pos=m.pos[sl].copy(), frozen=int(m.frozen[first]))
        return out

    def gap(self, mol):
        """a point of the lattice's body centres next to molecule `mol`: 3.1 A from the nearest lattice sites"""
        first, _ = self.model.molecules[mol]
        return self.model.pos[first] + 0.5 * self.spacing

    def mol_at(self, slot):
        return int(self.model.mol[slot])

    # ---- operations
    def edit(self, remove=(), insert=()):
        """remove: molecule ids; insert: molecule dicts.  Returns the inserted molecules' first slots, or None when the
        entry answers "upload again" (nothing has changed then)."""
        m = self.model
        ranges = [m.molecules[k] for k in remove]
        if (len(ranges) > MAX_MOLECULES or len(insert) > MAX_MOLECULES
                or any(len(d["charge"]) > edit_model.MAX_EDIT for d in insert) or not m.edits_supported()):
            return self._apply(ranges, insert, None)
        for first, count in ranges:
            assert m.remove(first, count)
            for k in EXTRA:
                self.extra[k][first:first + count] = 0.0
        firsts = []
        for d in insert:
            first = m.insert(d["pos"], *[d[k] for k in edit_model.FIELDS], frozen=d.get("frozen", 0))
            assert first is not None
            for k in EXTRA:
                self.extra[k][first:first + len(d["charge"])] = d[k]
            firsts.append(first)
        m.check_invariants()
        return self._apply(ranges, insert, firsts)

    def _apply(self, ranges, insert, firsts):
        return firsts

    def move(self, mol, shift):
        first, count = self.model.molecules[mol]
        pos = self.model.pos[first:first + count] + np.asarray(shift, dtype=np.float64)
        self.model.update_atoms(first, pos)
        return first, pos

    def scale_box(self, factor):
        """False: after an edit the engine asks for an upload instead (the slots are no longer those of the upload)"""
        return False

    def evaluate(self):
        self.model.energy()

    def unchanged(self):
        """the call before this one answered None: the next energy() is the previous one"""

    def live_system(self):
        s, slots = self.model.live_system()
        for k in EXTRA:
            if k in self.start:
                s[k] = self.extra[k][slots].copy()
        return s


# ---- the scripts.  each(): "evaluate here when the run evaluates after every edit"
def edge(sim, each):
    """60 atoms; a 5-atom molecule lands in slots 60 .. 64, across the block edge at 64"""
    a = sim.movable()[3]
    got = sim.edit(insert=[grown(sim.molecule(a), 5, sim.gap(a))])
    assert got == [60], got


def grow(sim, each):
    """126 atoms; 5 more take npad from 128 to 256; then the molecule leaves again and the grid stays"""
    a = sim.movable()[5]
    got = sim.edit(insert=[grown(sim.molecule(a), 5, sim.gap(a))])
    assert got == [126] and sim.model.grids()[0] == 256, got
    each()
    assert sim.edit(remove=[sim.mol_at(126)]) == []
    assert sim.model.grids()[0] == 256 and sim.model.holes == [(126, 5)]


def hole(sim, each):
    """a middle molecule leaves; one of its size takes the hole; one of another size is appended"""
    mv = sim.movable()
    a = mv[len(mv) // 2]
    first, count = sim.model.molecules[a]
    mol, n = sim.molecule(a), sim.model.slot_count
    assert sim.edit(remove=[a]) == []
    each()
    assert sim.edit(insert=[grown(mol, count, sim.gap(mv[2]))]) == [first]
    each()
    assert sim.edit(insert=[grown(mol, count + 1, sim.gap(mv[4]))]) == [n]


def last_block(sim, each):
    """130 atoms; every atom of the last block leaves: a block of holes only"""
    m = sim.model
    gone = [k for k, (first, count) in m.molecules.items() if first + count > 128]
    assert sim.edit(remove=sorted(gone, key=lambda k: m.molecules[k][0])) == []
    assert not m.valid[128:].any() and m.slot_count == 130


def eight(sim, each):
    """8 removals and 8 insertions in one call; then 9 + 0 and 0 + 9, which answer None and change nothing"""
    mv = sim.movable()
    mols = [sim.molecule(k) for k in mv[:8]]
    new = [grown(mols[k], len(mols[k]["charge"]) + (k % 2), sim.gap(mv[8 + k])) for k in range(8)]
    got = sim.edit(remove=mv[:8], insert=new)
    assert got is not None and len(got) == 8
    each()
    mv = sim.movable()
    assert sim.edit(remove=mv[:9]) is None
    sim.unchanged()
    assert sim.edit(insert=[grown(mols[0], 3, sim.gap(mv[k])) for k in range(9)]) is None
    sim.unchanged()


def sixteen(sim, each):
    """a 16-atom molecule; then a 17-atom one, which answers None and changes nothing"""
    a = sim.movable()[1]
    n = sim.model.slot_count
    assert sim.edit(insert=[grown(sim.molecule(a), 16, sim.gap(a))]) == [n]
    each()
    assert sim.edit(insert=[grown(sim.molecule(a), 17, sim.gap(sim.movable()[2]))]) is None
    sim.unchanged()


def frozen(sim, each):
    """a frozen molecule enters a system that holds frozen ones: frozen-frozen pairs stay out of the sum and the correction"""
    assert sim.model.frozen[:sim.model.slot_count].any()
    a = sim.movable()[2]
    n = sim.model.slot_count
    assert sim.edit(insert=[dict(grown(sim.molecule(a), 5, sim.gap(a)), frozen=1)]) == [n]


def move_and_edit(sim, each):
    """an update_atoms of another molecule and an edit before ONE energy()"""
    mv = sim.movable()
    sim.move(mv[1], [0.15, -0.1, 0.05])
    mol, n = sim.molecule(mv[6]), sim.model.slot_count
    assert sim.edit(remove=[mv[6]], insert=[grown(mol, len(mol["charge"]) + 2, sim.gap(mv[9]))]) == [n]
    sim.move(mv[3], [-0.1, 0.1, 0.1])


def then_scale_box(sim, each):
    """an edit, then scale_box (which asks for an upload after an edit and changes nothing), then energy()"""
    mv = sim.movable()
    sim.edit(remove=[mv[2]], insert=[grown(sim.molecule(mv[4]), 4, sim.gap(mv[7]))])
    assert sim.scale_box(1.02) is False


SCRIPTS = {  # name -> (atoms, script)
    "edge": (60, edge),
    "grow": (126, grow),
    "hole": (130, hole),
    "last_block": (130, last_block),
    "eight": (130, eight),
    "sixteen": (60, sixteen),
    "frozen": (70, frozen),
    "move_and_edit": (130, move_and_edit),
    "then_scale_box": (126, then_scale_box),
}
# every script in the modes that have a long-range correction or a three-body term to keep in step; the scripts that move
# the layout in all modes
FULL_MODES = ("phahst_lrc", "phahst_at", "lj_at", "rd_crystal", "lj_wh_fh4")
CASES = [(m, s) for m in MODES for s in SCRIPTS if m in FULL_MODES or s in ("edge", "grow", "hole")]
