"""CPU tests of the edit harness (tests/edit_model.py, tests/edit_cases.py), which tests/test_gpu_edits.py turns on the
engine: the model's invariants on every scenario, the comparison of every comparison point pinned WITHOUT a GPU (the
oracle's results are fed through it in the engine's place: pair_reference.sums() agrees with the oracle at the
existing RTOL, and polar_reference.solve() on the oracle's static field holds the oracle's vectors inside its bound), the
cap on the bound, and -- the point of a harness -- that deliberately wrong "engine" output fails and names the slot or pair.
"""
import numpy as np
import pytest

import edit_cases as ec
import edit_model as em
import polar_reference as pref
from oracle import oracle

ALL = sorted(ec.SCENARIOS)
REFUSED = ["excluded " + k for k in sorted(ec.EXCLUDED)]


def scatter(script, point, want):
    """the oracle's result on the live atoms, in the shape the engine returns it: vectors over slot_count slots, holes
    zero; (rank_metric by slot, the order as slots)"""
    snap = point["snap"]
    slots = snap["slots"]
    r = dict(want, n_atoms=len(slots))
    if not ec.polarizable(script):
        return r, None, None
    d = {k: np.zeros((snap["slot_count"], 3)) for k in ec.VECTORS}
    for k in ec.VECTORS:
        d[k][slots] = want[k]
    rank = np.zeros(snap["slot_count"])
    rank[slots] = want["rank_metric"]
    return r, d, (rank, slots[want["ranked_array"]])


# ---------------------------------------------------------------------------------------------
# 1. the model
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL + REFUSED + ["deferred"])
def test_model_invariants_hold_after_every_operation(name):
    """Script checks them after every insert and remove while it records; here: the recorded script replays on a fresh
    model to the same return values, and the snapshots are consistent with it"""
    s = ec.scenario(name)
    m = em.Model(s.system, s.params, s.max_atoms, s.options)
    for op in s.ops:
        if op["op"] == "insert":
            assert m.insert(op["pos"], *[op["props"][f] for f in em.FIELDS], frozen=op["frozen"]) == op["expect"]
        elif op["op"] == "remove":
            assert m.remove(op["first"], op["count"]) == op["expect"]
        elif op["op"] == "move":
            m.update_atoms(op["first"], op["pos"])
        elif op["op"] == "order":
            assert sorted(op["slots"]) == sorted(np.flatnonzero(m.valid & (m.prop["alpha"] != 0.0)))
            m.set_sweep_order(op["slots"])
        elif op["op"] == "energy":
            if op["n_atoms"] is None:
                with pytest.raises(em.NeedsOrder):
                    m.energy()
            else:
                assert m.energy() == op["n_atoms"]
                if op["label"] is not None:
                    snap = op["snap"]
                    assert sorted(np.r_[snap["slots"], snap["holes"]]) == list(range(m.slot_count))
                    assert np.array_equal(np.sort(snap["slots"]), m.live_slots())
        if op["op"] in ("insert", "remove"):
            assert m.slot_count == op["slot_count"]
        m.check_invariants()
        inv = {a: k for k, a in enumerate(m.view)}  # view <-> slot maps are inverse to each other
        assert inv == m.view_of and all(m.view[k] == a for a, k in m.view_of.items())


def test_holes_are_reused_most_recent_first_by_exact_size():
    s = ec.scenario("slots")
    inserts = [op for op in s.ops if op["op"] == "insert"]
    assert [op["expect"] for op in inserts[:3]] == [75, 121, 40]
    assert inserts[3]["expect"] == 123 and len(inserts[3]["pos"]) == 2  # no hole of two atoms: appended
    assert [op["expect"] for op in inserts if len(op["pos"]) == 17] == [None]
    full = [op for op in inserts if op["slot_count"] == 136 and op["expect"] is None and len(op["pos"]) == 1]
    assert len(full) == 1
    assert inserts[-1]["expect"] == 10  # a hole that fits is still taken in a full context


def test_edges_of_the_scenarios_are_where_they_claim():
    grid = lambda name: [p["snap"]["grids"] for p in ec.scenario(name).comparison_points()]
    assert [g[0] for g in grid("tiles128")] == [128, 256, 256]
    assert [g[1] for g in grid("view_steps")] == [128, 128, 256, 256, 256]
    assert [(p["snap"]["view"], p["snap"]["live_view"]) for p in ec.scenario("view_steps").comparison_points()] == \
        [(127, 127), (128, 128), (129, 129), (129, 128), (129, 127)]
    assert [(p["snap"]["view"], p["snap"]["live_view"]) for p in ec.scenario("view_holes").comparison_points()] == \
        [(129, 129), (129, 65), (129, 64), (129, 63)]
    for nv in (65, 129):
        for flags in ("production", "gs3"):
            pts = ec.scenario("gs_%s_%d" % (flags, nv)).comparison_points()
            assert [p["snap"]["live_view"] for p in pts] == [nv, nv - 1, nv, nv]
    assert ec.scenario("view_alpha").comparison_points()[-1]["snap"]["live_view"] == 0
    burst = ec.scenario("burst")
    edited = sum(len(op["pos"]) if op["op"] == "insert" else op["count"] for op in burst.ops[1:53])
    assert edited == 260 > em.MAX_LISTED
    d = ec.scenario("deferred")
    assert len(d.model.view) >= 1345 and d.model.live_view_count() == 1345
    for name in ALL:
        assert len(ec.scenario(name).comparison_points()) <= 20


@pytest.mark.parametrize("name", REFUSED)
def test_excluded_modes_are_predicted_to_refuse(name):
    s = ec.scenario(name)
    assert [op["expect"] for op in s.ops if op["op"] in ("insert", "remove")] == [None, False]


# ---------------------------------------------------------------------------------------------
# 2. the harness, pinned on the oracle; the cap on the bound
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_comparison_holds_the_oracle_at_every_point(name):
    """check_point() with the oracle's output in the engine's place: rd_energy / es_real / ef_static of
    pair_reference.sums() against it at RTOL / FIELD_TOL, es_recip and es_self inside their derived bounds, the vectors
    inside polar_reference's bound, the ranking through the slot map -- and, inside check_point, the bound itself at most
    1e-11 max|mu| on every scenario but the one beyond 2048 A."""
    s = ec.scenario(name)
    for point in s.comparison_points():
        want = ec.references(s, point)["oracle"]
        r, d, ranking = scatter(s, point, want)
        ec.check_point(s, point, r, d, ranking=ranking, who="oracle", zero_outside=False)


def test_the_far_scenario_is_the_only_one_outside_the_cap():
    assert [n for n in ALL if not ec.scenario(n).capped] == ["far"]
    assert np.abs(ec.scenario("far").comparison_points()[1]["snap"]["system"]["pos"]).max() > 2048.0


# ---------------------------------------------------------------------------------------------
# 3. breakage is named
# ---------------------------------------------------------------------------------------------
def _with_stale_atom(script, point, which):
    """the oracle on the live atoms plus ONE atom removed before this point (as a molecule of its own): a hole that still
    contributes.  Returns (its slot, the result on the live atoms)"""
    stale, _, extra = ec.stale_table(script, point)
    gone = point["snap"]["gone"]
    n = len(point["snap"]["system"]["charge"])
    keep = np.r_[0:n, extra[which]]
    sys2 = {k: (v if k == "basis" else v[keep]) for k, v in stale.items()}
    want = oracle.energy(sys2, script.params, want_vectors=ec.polarizable(script))
    for k in ec.VECTORS + ("rank_metric",):
        if k in want:
            want[k] = want[k][:n]
    want["ranked_array"] = np.arange(n, dtype=np.int32)
    return gone[which]["slot"], want


@pytest.mark.parametrize("name,label,which", [("pair_ewald_fh0", "remove", 0), ("order", "move, remove, insert", 0)])
def test_a_removed_atom_that_still_contributes_is_named(name, label, which):
    s = ec.scenario(name)
    point = next(p for p in s.comparison_points() if p["label"] == label)
    slot, want = _with_stale_atom(s, point, which)  # the H2G site: charge, Lennard-Jones and a polarizability
    r, d, ranking = scatter(s, point, want)
    with pytest.raises(AssertionError) as e:
        ec.check_point(s, point, r, d, ranking=ranking, who="broken", zero_outside=False)
    msg = str(e.value)
    print(msg)
    lines = msg.split("\n")
    for key in ("rd_energy", "es_real"):
        k = next(i for i, l in enumerate(lines) if (" %s: " % key) in l)
        assert ("removed slot %d still contributing" % slot) in lines[k + 1], lines[k:k + 3]
    if ec.polarizable(s):
        k = next(i for i, l in enumerate(lines) if "ef_static against" in l)
        assert ("removed slot %d still contributing its field" % slot) in lines[k + 1], lines[k:k + 3]


def test_a_single_stale_pair_is_named():
    """one tile entry left behind: rd_energy off by exactly one pair term of a removed atom"""
    s = ec.scenario("pair_ewald_fh0")
    point = s.comparison_points()[2]
    _, t, extra = ec.stale_table(s, point)
    n = len(point["snap"]["system"]["charge"])
    rows = np.flatnonzero((t["j"] == extra[0]) & (t["i"] < n) & (t["rd"] != 0))
    row = rows[np.argmax(np.abs(t["rd"][rows]))]
    want = dict(ec.references(s, point)["oracle"])
    want["rd_energy"] += float(t["rd"][row])
    want["energy"] += float(t["rd"][row])
    r, d, ranking = scatter(s, point, want)
    with pytest.raises(AssertionError) as e:
        ec.check_point(s, point, r, d, who="broken", zero_outside=False)
    msg = str(e.value)
    print(msg)
    assert "pair (%d, removed slot %d)" % (t["i"][row], point["snap"]["gone"][0]["slot"]) in msg and "extra" in msg


def test_a_reused_slot_that_keeps_its_old_polarizability_is_named():
    s = ec.scenario("view_alpha")
    point = s.comparison_points()[1]  # slots 20 and 22 were polarizable and hold alpha = 0 now
    snap = point["snap"]
    a = int(np.flatnonzero(snap["slots"] == 20)[0])
    assert snap["system"]["alpha"][a] == 0.0
    sys2 = dict(snap["system"], alpha=snap["system"]["alpha"].copy())
    sys2["alpha"][a] = s.system["alpha"][20]  # what the view slot held before
    want = oracle.energy(sys2, s.params, want_vectors=True)
    r, d, ranking = scatter(s, point, want)
    with pytest.raises(AssertionError) as e:
        ec.check_point(s, point, r, d, who="broken")
    msg = str(e.value)
    print(msg)
    assert "alpha = 0" in msg and "slots [20]" in msg and "not polarizable" in msg


def test_a_dipole_outside_the_bound_is_named_with_its_slot():
    s = ec.scenario("view_holes")
    point = s.comparison_points()[2]
    want = dict(ec.references(s, point)["oracle"])
    t = ec.references(s, point)["tensor"]
    a = int(t.view[40])
    want["mu"] = want["mu"].copy()
    want["mu"][a] *= 1.0 + 1e-9
    r, d, ranking = scatter(s, point, want)
    with pytest.raises(AssertionError) as e:
        ec.check_point(s, point, r, d, who="broken", zero_outside=False)
    msg = str(e.value)
    print(msg)
    assert "atom %d component" % a in msg and "[atom %d is slot %d]" % (a, point["snap"]["slots"][a]) in msg


class OldestHoleFirst(em.Model):
    """a context that reuses the OLDEST hole of the size"""

    def find_slot(self, count):
        for h, (first, c) in enumerate(self.holes):
            if c == count:
                return first, h
        return super().find_slot(count)


class StandIn:
    """play()'s engine interface on a model; energy() is the oracle's"""

    def __init__(self, script, model):
        self.s, self.m = script, model

    def insert_molecule(self, pos, *props, frozen=False):
        return self.m.insert(pos, *props, frozen=frozen)

    def remove_molecule(self, first, count):
        return self.m.remove(first, count)

    def update_atoms(self, first, pos):
        self.m.update_atoms(first, pos)

    def set_sweep_order(self, slots):
        self.m.set_sweep_order(slots)

    def slot_count(self):
        return self.m.slot_count

    def energy(self):
        n = self.m.energy()
        return dict(oracle.energy(self.m.live_system()[0], self.s.params), n_atoms=n)

    def dipoles(self):
        return {k: np.zeros((self.m.slot_count, 3)) for k in ec.VECTORS}


def test_a_hole_reused_in_the_wrong_order_is_caught_at_the_call():
    s = ec.scenario("slots")
    good = StandIn(s, em.Model(s.system, s.params, s.max_atoms))
    ec.play(s, good)  # the stand-in itself replays clean
    bad = StandIn(s, OldestHoleFirst(s.system, s.params, s.max_atoms))
    with pytest.raises(AssertionError, match="insert returned 10, the model predicts 75"):
        ec.play(s, bad)
