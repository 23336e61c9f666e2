"""A plain-Python model of the bookkeeping behind mpmc_hip_insert_molecule / mpmc_hip_remove_molecule /
mpmc_hip_set_sweep_order, written from the text of include/mpmc_hip.h ("Grand-canonical moves ... without a re-upload")
and from what the engine documents about itself.  Helper module for the tests (a plain import, not a conftest).

What the model holds:

* SLOTS.  The engine keeps its own atom order.  An inserted molecule takes a hole left by a removed molecule of exactly
  the same size -- the most recently opened one first -- or new slots at the end; a removed molecule leaves a hole.
  slot_count only grows.  Per-atom downloads span slot_count slots, holes reading as zeros.
* WHAT IS REFUSED ("upload again", None / False here): more than 16 atoms, a full context, a context that has not been
  evaluated since its upload, one that has seen more than 256 edited or moved atoms since its last energy() (the engine
  then recomputes everything and keeps no list to patch), and the modes that keep data an edit does not patch:
  pair_coefficients = 0, incremental_amatrix / incremental_pairs = 0, Gauss-Seidel with persistent_gs = 0, the exact
  dipoles, disp_expansion, axilrod_teller, rd_crystal, polarvdw.
* THE VIEW (the compacted list of polarizable sites the solver works on).  In the order-free solver modes a view slot
  stays with its atom slot: it becomes a hole of the view when the atom leaves or when the slot is reused by a site with
  alpha = 0, is filled again when a polarizable site arrives, and a polarizable site in an atom slot that never had one is
  appended.  In the Gauss-Seidel modes the view is the list the caller states (set_sweep_order), and energy() refuses
  until it has been stated after an edit.
* THE CALLER'S ORDER of the molecules (the reference's molecule list): an inserted molecule goes in front of the one it
  was copied from (`before`), or to the end.

live_system() and the index maps are what pair_reference.pair_table(), polar_reference.Tensor and oracle.energy()
consume: compacted arrays in slot order or in the caller's order, with the slots they came from.
"""
import numpy as np

MAX_EDIT = 16  # atoms per insert / remove
MAX_LISTED = 256  # edited or moved atoms between two energy() calls that are still patched one by one
FIELDS = ("charge", "alpha", "epsilon", "sigma", "mass")
DIRTYING_OPTIONS = ("pair_coefficients", "incremental_amatrix", "incremental_pairs")  # setting one asks for a full pass


class NeedsOrder(RuntimeError):
    """energy() in a Gauss-Seidel mode after an edit, before set_sweep_order()"""


def runs(ids):
    """[(first, count)] of the contiguous runs of equal id"""
    ids = np.asarray(ids)
    cut = np.flatnonzero(ids[1:] != ids[:-1]) + 1
    first = np.concatenate([[0], cut])
    last = np.concatenate([cut, [len(ids)]])
    return [(int(a), int(b - a)) for a, b in zip(first, last)]


class Model:
    def __init__(self, system, params, max_atoms, options=None):
        n = len(system["charge"])
        assert n <= max_atoms
        self.params, self.options = dict(params), dict(options or {})
        self.basis = np.array(system["basis"], dtype=np.float64)
        self.max_atoms = int(max_atoms)
        self.pos = np.zeros((max_atoms, 3))
        self.pos[:n] = system["pos"]
        self.prop = {k: np.zeros(max_atoms) for k in FIELDS}
        for k in FIELDS:
            self.prop[k][:n] = system[k]
        self.frozen = np.zeros(max_atoms, dtype=np.int32)
        self.frozen[:n] = system["frozen"]
        self.valid = np.zeros(max_atoms, dtype=bool)
        self.valid[:n] = True
        self.mol = np.full(max_atoms, -1, dtype=np.int64)  # molecule id per slot, -1 in a hole
        self.molecules = {}  # id -> (first slot, count)
        self.caller_order = []  # molecule ids in the caller's order
        for m, (first, count) in enumerate(runs(system["molecule"])):
            self.mol[first:first + count] = m
            self.molecules[m] = (first, count)
            self.caller_order.append(m)
        self.next_mol = len(self.molecules)
        self.slot_count = n
        self.holes = []  # (first, count), in the order they were opened
        self.view = [int(a) for a in np.flatnonzero(self.prop["alpha"][:n] != 0.0)]  # view slot -> atom slot
        self.view_of = {a: k for k, a in enumerate(self.view)}  # atom slot -> view slot
        self.order_stale = False
        self.listed = 0
        self.full_pass = True  # an upload: nothing to patch until the first energy()

    # ---- modes ------------------------------------------------------------------------------------------------------
    def _polar(self):
        return bool(self.params.get("polarization")) and not self.params.get("rd_only")

    def _exact(self):
        return self._polar() and "polar_iterative" in self.params and not self.params["polar_iterative"]

    def _gauss_seidel(self):
        p = self.params
        return self._polar() and bool(p.get("polar_gs") or p.get("polar_gs_ranked"))

    def order_mode(self):
        """Gauss-Seidel on the chain kernel: the view is the caller's list"""
        return (self._gauss_seidel() and not self.params.get("polar_zodid") and not self._exact()
                and self.options.get("pair_coefficients", 1) != 0 and self.options.get("persistent_gs", 1) != 0)

    def edits_supported(self):
        o, p = self.options, self.params
        if self.full_pass:
            return False
        if not o.get("pair_coefficients", 1) or not o.get("incremental_amatrix", 1) or not o.get("incremental_pairs", 1):
            return False
        if p.get("disp_expansion") or p.get("axilrod_teller") or p.get("rd_crystal") or p.get("polarvdw") or p.get("cdvdw"):
            return False
        if self._exact():
            return False
        if self._gauss_seidel() and not self.order_mode():
            return False
        return True

    def set_option(self, name, value):
        self.options[name] = int(value)
        if name in DIRTYING_OPTIONS:
            self.full_pass = True

    # ---- operations -------------------------------------------------------------------------------------------------
    def _note(self, count):
        self.listed += count
        if self.listed > MAX_LISTED:
            self.full_pass = True

    def update_atoms(self, first, pos):
        pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
        assert 0 <= first and first + len(pos) <= self.slot_count
        self.pos[first:first + len(pos)] = pos  # (a hole keeps coordinates too: they count for nothing)
        if not self.full_pass:
            if self.listed + len(pos) > MAX_LISTED:
                self.full_pass = True
            else:
                self.listed += len(pos)

    def find_slot(self, count):
        """where an insert of `count` atoms goes: (first, index of the hole or None); None when the context is full"""
        for h in range(len(self.holes) - 1, -1, -1):
            if self.holes[h][1] == count:
                return self.holes[h][0], h
        if self.slot_count + count > self.max_atoms:
            return None
        return self.slot_count, None

    def insert(self, pos, charge, alpha, epsilon, sigma, mass, frozen=False, before=None):
        """-> first slot, or None = upload again.  before: id of the molecule it goes in front of in the caller's order"""
        pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
        count = len(pos)
        assert count > 0
        if count > MAX_EDIT or not self.edits_supported():
            return None
        where = self.find_slot(count)
        if where is None:
            return None
        first, hole = where
        if hole is not None:
            del self.holes[hole]
        else:
            self.slot_count += count
        sl = slice(first, first + count)
        self.pos[sl] = pos
        for k, v in zip(FIELDS, (charge, alpha, epsilon, sigma, mass)):
            self.prop[k][sl] = np.asarray(v, dtype=np.float64)
        self.frozen[sl] = int(bool(frozen))
        self.valid[sl] = True
        m = self.next_mol
        self.next_mol += 1
        self.mol[sl] = m
        self.molecules[m] = (first, count)
        if before is None:
            self.caller_order.append(m)
        else:
            self.caller_order.insert(self.caller_order.index(before), m)
        if self.order_mode():
            self.order_stale = True
        else:
            for a in range(first, first + count):
                if self.prop["alpha"][a] != 0.0 and a not in self.view_of:
                    self.view_of[a] = len(self.view)
                    self.view.append(a)
        self._note(count)
        return first

    def remove(self, first, count):
        """-> True, or False = upload again"""
        assert 0 <= first and count > 0 and first + count <= self.slot_count
        assert self.valid[first:first + count].all(), "slot holds no atom"
        if count > MAX_EDIT or not self.edits_supported():
            return False
        m = int(self.mol[first])
        assert self.molecules[m] == (first, count), "not one whole molecule"
        sl = slice(first, first + count)
        self.valid[sl] = False
        self.mol[sl] = -1
        for k in FIELDS:
            if k != "mass":
                self.prop[k][sl] = 0.0
        self.frozen[sl] = 0
        del self.molecules[m]
        self.caller_order.remove(m)
        self.holes.append((first, count))
        if self.order_mode():
            self.order_stale = True
        self._note(count)
        return True

    def sweep_order(self):
        """what a caller passes to set_sweep_order(): the slots of the polarizable atoms in the caller's order"""
        return [int(a) for a in self.live_slots("caller") if self.prop["alpha"][a] != 0.0]

    def set_sweep_order(self, slots):
        if not self.order_mode():
            return
        slots = [int(a) for a in slots]
        assert sorted(slots) == sorted(int(a) for a in np.flatnonzero(self.valid & (self.prop["alpha"] != 0.0)))
        self.view = slots
        self.view_of = {a: k for k, a in enumerate(slots)}
        self.order_stale = False

    def energy(self):
        """-> n_atoms of the result"""
        if self.order_stale and self.order_mode():
            raise NeedsOrder()
        self.listed = 0
        self.full_pass = False
        return self.n_atoms

    # ---- what the references consume --------------------------------------------------------------------------------
    @property
    def n_atoms(self):
        return int(self.valid.sum())

    def live_slots(self, order="slot"):
        if order == "slot":
            return np.flatnonzero(self.valid)
        assert order == "caller"
        out = []
        for m in self.caller_order:
            first, count = self.molecules[m]
            out.extend(range(first, first + count))
        return np.asarray(out, dtype=np.int64)

    def hole_slots(self):
        return np.flatnonzero(~self.valid[:self.slot_count])

    def live_system(self, order="slot"):
        """(system dict of the live atoms, the slot of each of its atoms)"""
        slots = self.live_slots(order)
        s = {k: self.prop[k][slots].copy() for k in FIELDS}
        s["pos"] = self.pos[slots].copy()
        s["molecule"] = (self.mol[slots] + 1).astype(np.int32)
        s["frozen"] = self.frozen[slots].copy()
        s["basis"] = self.basis.copy()
        return s, slots

    def view_live(self):
        """per view slot: does it hold a polarizable site now"""
        return np.array([bool(self.valid[a]) and self.prop["alpha"][a] != 0.0 for a in self.view], dtype=bool)

    def live_view_count(self):
        return int(self.view_live().sum())

    def grids(self):
        """(npad, nvpad): the atom and view tile grids, on 128 boundaries"""
        up = lambda n: 128 * ((n + 127) // 128)
        return up(self.slot_count), max(128, up(len(self.view)))

    def check_invariants(self):
        n = self.slot_count
        assert n <= self.max_atoms and not self.valid[n:].any()
        seen = np.zeros(n, dtype=np.int64)
        for m, (first, count) in self.molecules.items():
            assert first >= 0 and first + count <= n
            seen[first:first + count] += 1
            assert (self.mol[first:first + count] == m).all() and self.valid[first:first + count].all()
        hole = np.zeros(n, dtype=np.int64)
        for first, count in self.holes:
            assert first >= 0 and first + count <= n
            hole[first:first + count] += 1
        assert seen.max(initial=0) <= 1, "a slot is in two molecules"
        assert np.array_equal(seen + hole, np.ones(n, dtype=np.int64)), "holes and live slots do not partition the slots"
        assert np.array_equal(seen.astype(bool), self.valid[:n])
        assert sorted(self.caller_order) == sorted(self.molecules)
        assert len(set(self.view)) == len(self.view)
        for k, a in enumerate(self.view):  # view <-> slot maps are inverse to each other
            assert self.view_of[a] == k and 0 <= a < n
        assert len(self.view_of) == len(self.view)
        if not self.order_stale:
            pol = set(int(a) for a in np.flatnonzero(self.valid & (self.prop["alpha"] != 0.0)))
            assert pol <= set(self.view)
            if self.order_mode():
                assert pol == set(self.view)
