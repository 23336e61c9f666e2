"""Scenarios for the grand-canonical edit path (mpmc_hip_insert_molecule / remove_molecule / set_sweep_order on a live
context), shared by tests/test_edit_model.py (CPU: model invariants, the harness against the oracle) and
tests/test_gpu_edits.py (the engine against the model and the longdouble references).

A scenario is a Script: the list of operations, recorded while they are played on tests/edit_model.py's Model, with the
model's predicted return value next to each and, at every comparison point, a snapshot of the live atoms (the system dict
the references consume, and the slot of each of its atoms).  Inserted molecules are copies of live ones -- where the alpha
pattern changes, a permutation of the source's -- placed at least MIN_DIST from every live atom (asserted here, on the
CPU: no scenario is a close-contact case).  Sizes are the smallest at which the edge exists (the 64 / 128 boundaries of the
atom and view tile grids, the 16-atom and 256-atom limits, a full context).

The second half is the harness both test modules share: play() replays a Script on an engine (or a stand-in) and checks
every return value against the model's prediction; check_point() holds one evaluation to the references and, where it
fails, names the slot, site or pair (a removed atom that still contributes included: explain_stale()).
"""
import functools

import numpy as np

import adversarial as adv
import edit_model as em
import pair_reference as pr
import polar_cases as pc
import polar_reference as pref
import vdw_cases
from mpmc_amd import synth
from oracle import oracle
from test_gpu_parity import RTOL, check_energies, rel  # (plain helpers: importing them needs no device)
from test_gpu_screen_edges import FIELD_TOL

MIN_DIST = 2.5
GS3 = dict(pc.BASE, polar_max_iter=3, polar_gs=1)
ES = dict(temperature=100.0)


def min_image_distance(basis, placed, p):
    """smallest distance (27 images of the reduced displacement) between the points p[m,3] and placed[k,3]"""
    if not len(placed) or not len(p):
        return np.inf
    d = np.asarray(placed)[None, :, :] - np.asarray(p)[:, None, :]
    f = d @ np.linalg.inv(basis)
    d = (f - np.rint(f)) @ basis
    sh = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)], dtype=np.float64) @ basis
    return float(np.sqrt(((d[:, :, None, :] + sh[None, None, :, :]) ** 2).sum(-1)).min())


def _rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


class Script:
    def __init__(self, name, system, params, max_atoms, options=None, seed=0, capped=True):
        self.name, self.system, self.params, self.max_atoms = name, system, dict(params), int(max_atoms)
        self.options = dict(options or {})
        self.model = em.Model(system, params, max_atoms, self.options)
        self.rng = np.random.default_rng([len(name), seed] + [ord(c) for c in name])
        self.ops = []
        self.points = []  # indices into ops of the comparison points
        self.capped = capped  # the polar bound stays below 1e-11 max|mu| (not with coordinates beyond 2048 A)
        self.gone = []  # atoms removed since the last comparison point, as they were: what a stale contribution looks like

    # ---- recording --------------------------------------------------------------------------------------------------
    def _live_pos(self):
        return self.model.pos[self.model.live_slots()]

    def spot(self, rel, shift=None):
        """a rigid copy of the site offsets rel[m,3] (about their centroid), rotated at random and put where every site is
        MIN_DIST + 0.05 from every live atom"""
        m = self.model
        live = self._live_pos()
        basis = m.basis
        for _ in range(4000):
            c = self.rng.uniform(0.0, 1.0, 3) @ basis - 0.5 * basis.sum(axis=0)
            p = rel @ _rotation(self.rng).T + c
            if min_image_distance(basis, live, p) >= MIN_DIST + 0.05:
                return p if shift is None else p + np.asarray(shift) @ basis
        raise RuntimeError("%s: no room for another molecule" % self.name)

    def insert(self, src, alpha=None, frozen=False, sites=None, pos=None, before="source", shift=None, copies=1):
        """a copy of the live molecule whose first slot is `src` (of its sites `sites`; `copies` > 1 strings copies together,
        for the calls that are refused by their size); alpha: a replacement pattern (a permutation of the source's)"""
        m = self.model
        mol = int(m.mol[src])
        first, count = m.molecules[mol]
        sl = np.arange(first, first + count)[slice(None) if sites is None else list(sites)]
        sl = np.tile(sl, copies)[:em.MAX_EDIT + 1] if copies > 1 else sl
        rel = m.pos[sl] - m.pos[sl].mean(axis=0)
        if pos is None:
            pos = self.spot(rel, shift) if copies == 1 else m.pos[sl] + 0.5 * m.basis.sum(axis=0)
        props = {k: m.prop[k][sl].copy() for k in em.FIELDS}
        if alpha is not None:
            assert sorted(alpha) == sorted(props["alpha"]), "alpha patterns are permutations of the source's"
            props["alpha"] = np.asarray(alpha, dtype=np.float64)
        live = self._live_pos()
        expect = m.insert(pos, *[props[k] for k in em.FIELDS], frozen=frozen, before=mol if before == "source" else before)
        if expect is not None:
            assert min_image_distance(m.basis, live, pos - (0 if shift is None else np.asarray(shift) @ m.basis)) >= MIN_DIST
        self.ops.append(dict(op="insert", pos=np.array(pos), props=props, frozen=bool(frozen), expect=expect,
                             slot_count=m.slot_count))
        m.check_invariants()
        return expect

    def remove(self, first, count=None):
        m = self.model
        if count is None:
            count = m.molecules[int(m.mol[first])][1]
        was = [dict(slot=a, pos=m.pos[a].copy(), frozen=int(m.frozen[a]), **{k: float(m.prop[k][a]) for k in em.FIELDS})
               for a in range(first, first + count)]
        expect = m.remove(first, count)
        if expect:
            self.gone += was
        self.ops.append(dict(op="remove", first=int(first), count=int(count), expect=expect, slot_count=m.slot_count))
        m.check_invariants()
        return expect

    def move(self, first, count, delta=(0.11, -0.07, 0.05), pos=None):
        m = self.model
        pos = m.pos[first:first + count] + np.asarray(delta) if pos is None else np.asarray(pos, dtype=np.float64)
        m.update_atoms(first, pos)
        self.ops.append(dict(op="move", first=int(first), pos=np.array(pos)))

    def order(self):
        slots = self.model.sweep_order()
        self.model.set_sweep_order(slots)
        self.ops.append(dict(op="order", slots=slots))

    def option(self, name, value):
        self.model.set_option(name, value)
        self.ops.append(dict(op="option", name=name, value=int(value)))

    def energy(self, label=None, same_as_previous=False, dipoles=None):
        """label: a comparison point (snapshot taken); same_as_previous: every result bit equals the previous energy()'s;
        dipoles: read the vectors here (default: at comparison points)"""
        m = self.model
        op = dict(op="energy", label=label, same=bool(same_as_previous))
        try:
            op["n_atoms"] = m.energy()
        except em.NeedsOrder:
            op["n_atoms"] = None  # the engine refuses by name
            self.ops.append(op)
            return
        op["dipoles"] = (label is not None) if dipoles is None else bool(dipoles)
        if label is not None:
            order = "caller" if m.order_mode() else "slot"
            s, slots = m.live_system(order)
            op["snap"] = dict(system=s, slots=slots, holes=m.hole_slots(), slot_count=m.slot_count, grids=m.grids(),
                              view=len(m.view), live_view=m.live_view_count(), key=(self.name, len(self.points)),
                              gone=self.gone)
            self.gone = []
            self.points.append(len(self.ops))
        self.ops.append(op)

    def comparison_points(self):
        return [self.ops[k] for k in self.points]

    # ---- helpers for the builders -----------------------------------------------------------------------------------
    def molecules(self, count=None, sites=None):
        """first slots of the live molecules (of `count` atoms, with `sites` polarizable sites), in slot order"""
        m = self.model
        out = []
        for first, c in sorted(m.molecules.values()):
            if count is not None and c != count:
                continue
            if sites is not None and int(np.count_nonzero(m.prop["alpha"][first:first + c])) != sites:
                continue
            out.append(first)
        return out


def polarizable(s):
    return bool(s.params.get("polarization")) and not s.params.get("rd_only")


# ---------------------------------------------------------------------------------------------------------------------
# the references at one comparison point, computed once per process and shared by every test that needs them
# ---------------------------------------------------------------------------------------------------------------------
_REF = {}


def references(script, point):
    """dict(oracle, table, sums, tensor) of a comparison point (an op of Script.comparison_points())"""
    key = point["snap"]["key"]
    if key not in _REF:
        s, p = point["snap"]["system"], script.params
        pol = polarizable(script)
        table = pr.pair_table(s, p)
        _REF[key] = dict(oracle=oracle.energy(s, p, want_vectors=pol), table=table, sums=pr.sums(table, s, p),
                         tensor=pref.Tensor(s, p["polar_damp"]) if pol else None)
    return _REF[key]


# ---------------------------------------------------------------------------------------------------------------------
# the scenarios
# ---------------------------------------------------------------------------------------------------------------------
def sized(n, nv, seed=0):
    """s_pol(n) with exactly nv polarizable sites (the alpha := 0 trick of polar_cases.sized)"""
    s = dict(synth.s_pol(n))
    alpha = s["alpha"].copy()
    pol = np.flatnonzero(alpha != 0.0)
    alpha[np.random.default_rng([7000 + nv, n, seed]).choice(pol, size=len(pol) - nv, replace=False)] = 0.0
    s["alpha"] = alpha
    return s


def slots_scenario():
    """S-POL(123) in a context of 136: holes of 5 and 1 reused most recent first, a 2-atom insert appended, the context
    filled to its last slot, refusals by a full context and by size -- each leaving the next energy() bit-identical."""
    s = Script("slots", synth.s_pol(123), pc.JACOBI4, 136)
    s.energy("upload")
    for first in (10, 120, 40, 121, 75):  # holes, in this order: (10,5) (120,1) (40,5) (121,1) (75,5)
        assert s.remove(first)
    assert s.insert(20) == 75 and s.insert(122) == 121 and s.insert(20) == 40  # not the lowest, not the oldest: the newest
    s.energy("most recent hole first")
    assert s.insert(0, sites=(3, 4)) == 123  # two atoms: no hole of that size, appended
    assert s.insert(122) == 120
    s.energy("2 atoms appended")
    for k in range(11):  # single sites to the last slot; the 5-atom hole (10,5) stays open
        assert s.insert(122) == 125 + k
    assert s.model.slot_count == 136
    s.energy("full to the last slot")
    assert s.insert(122) is None  # full: no hole of one atom
    s.energy(same_as_previous=True, dipoles=True)
    assert s.insert(0, copies=4) is None  # 17 atoms
    assert s.remove(15, 17) is False
    s.energy(same_as_previous=True, dipoles=True)
    assert s.insert(20) == 10  # ... while a molecule that fits the open hole still enters
    s.energy("hole filled in a full context")
    return s


def _vdw_small():
    return vdw_cases.box(22)


EXCLUDED = {  # name -> (system, params, options set before the first energy())
    "pair_coefficients=0": (lambda: synth.s_pol(60), pc.JACOBI4, dict(pair_coefficients=0)),
    "persistent_gs=0": (lambda: synth.s_pol(60), GS3, dict(persistent_gs=0)),
    "incremental_amatrix=0": (lambda: synth.s_pol(60), pc.JACOBI4, dict(incremental_amatrix=0)),
    "incremental_pairs=0": (lambda: synth.s_pol(60), pc.JACOBI4, dict(incremental_pairs=0)),
    "exact dipoles": (lambda: synth.s_pol(60), dict(pc.BASE, polar_iterative=0), {}),
    "disp_expansion": (lambda: synth.s_phahst(60), synth.FLAGS_PHAHST, {}),
    "axilrod_teller": (lambda: synth.s_at(60), synth.FLAGS_AT, {}),
    "rd_crystal": (lambda: synth.s_lj(60), dict(synth.FLAGS_LJ, rd_crystal=1, rd_crystal_order=2), {}),
    "polarvdw": (_vdw_small, vdw_cases.FLAGS, {}),
}


def excluded_scenario(name):
    make, params, options = EXCLUDED[name]
    system = make()
    s = Script("excluded " + name, system, params, len(system["charge"]) + 16, options)
    s.energy()
    first = s.molecules()[1]
    assert s.insert(first) is None and s.remove(first) is False
    s.energy(same_as_previous=True, dipoles=polarizable(s))
    return s


def tiles128_scenario():
    """128 live atoms: one insert takes the atom tile grid from 128 to 256 slots, the remove leaves it there"""
    s = Script("tiles128", synth.s_pol(128), pc.JACOBI4, 320)
    s.energy("128 atoms")
    assert s.model.grids()[0] == 128
    assert s.insert(30) == 128 and s.model.grids()[0] == 256
    s.energy("npad 128 -> 256")
    assert s.remove(128)
    s.energy("removed again")
    return s


def tiles192_scenario():
    """192 slots: every slot of block 1 (64..127) a hole, molecules that straddle its edges included; then the last
    block; then one molecule left alive in the whole context"""
    s = Script("tiles192", synth.s_pol(192), pc.JACOBI4, 256)
    s.energy("192 atoms")
    for first in [f for f in s.molecules() if 60 <= f <= 125]:  # 60..64 and 125..129 straddle
        assert s.remove(first)
    assert not s.model.valid[64:128].any() and s.model.valid[59] and s.model.valid[130]
    s.energy("block 1 all holes")
    for first in [f for f in s.molecules() if f >= 130]:
        assert s.remove(first)
    assert not s.model.valid[64:192].any()
    s.energy("last block all holes")
    for first in [f for f in s.molecules() if f != 25]:
        assert s.remove(first)
    assert s.model.n_atoms == 5
    s.energy("one molecule alive")
    return s


def view_steps_scenario():
    """view slots 127 -> 128 -> 129 by inserts of molecules with one polarizable site (the view grid goes from 128 to 256
    at 129) and live sites back to 127 by removes, the view keeping its 129 slots"""
    s = Script("view_steps", sized(320, 127), pc.JACOBI4, 384)
    s.energy("view 127")
    src = s.molecules(5, sites=1)[3]
    a = s.insert(src)
    assert len(s.model.view) == 128 and s.model.grids()[1] == 128
    s.energy("view 128")
    b = s.insert(src)
    assert len(s.model.view) == 129 and s.model.grids()[1] == 256
    s.energy("view 129: nvpad 128 -> 256")
    assert s.remove(b)
    s.energy("live 128 of 129")
    assert s.remove(a)
    assert s.model.live_view_count() == 127 and len(s.model.view) == 129
    s.energy("live 127 of 129")
    return s


def view_holes_scenario():
    """live sites 65 / 64 / 63 inside a view of 129 slots: holes fill most of the view's blocks"""
    s = Script("view_holes", sized(320, 129), pc.JACOBI4, 320)
    s.energy("view 129")
    rng = np.random.default_rng(5)
    while s.model.live_view_count() > 65:
        spare = s.model.live_view_count() - 65
        firsts = next(f for f in (s.molecules(5, sites=k) for k in (3, 2, 1) if k <= spare) if f)  # fewest edits
        assert s.remove(firsts[int(rng.integers(len(firsts)))])
    for want in (65, 64, 63):
        if s.model.live_view_count() > want:
            assert s.remove(s.molecules(5, sites=1)[2])
        assert s.model.live_view_count() == want and len(s.model.view) == 129
        s.energy("live %d of 129" % want)
    return s


def view_alpha_scenario():
    """an atom slot that was polarizable and is reused by a site with alpha = 0, and the reverse (which appends a view
    slot); then every polarizable molecule removed"""
    s = Script("view_alpha", synth.s_pol(63), pc.JACOBI4, 80)
    s.energy("upload")
    a = s.model.prop["alpha"][0:5].copy()  # (H2G, H2E, H2E, 0, 0)
    nview = len(s.model.view)
    assert s.remove(20)
    assert s.insert(30, alpha=[0.0, a[1], 0.0, a[0], a[2]]) == 20  # slots 20, 22: polarizable -> 0; 23, 24: 0 -> polarizable
    assert len(s.model.view) == nview + 2 and s.model.live_view_count() == nview
    s.energy("alpha pattern permuted in a reused hole")
    assert s.remove(20)
    assert s.insert(30) == 20  # and the upload's pattern again: 23, 24 keep their view slots as holes
    assert len(s.model.view) == nview + 2 and s.model.live_view_count() == nview
    s.energy("pattern restored")
    for first in s.molecules(5):
        assert s.remove(first)
    assert s.model.live_view_count() == 0 and s.model.n_atoms == 3
    s.energy("no polarizable site left")
    return s


def gauss_seidel_scenario(nv, flags):
    """live sites nv after a remove, after an insert in front of its source, and after both; energy() refuses in between"""
    params = pc.PRODUCTION if flags == "production" else GS3
    s = Script("gs %s %d" % (flags, nv), sized(320, nv), params, 384)
    s.energy("upload")
    one = s.molecules(5, sites=1)
    assert s.remove(one[1])
    s.energy()  # refused: no order stated
    s.order()
    s.energy("remove: live %d" % (nv - 1))
    assert s.insert(one[4]) == one[1]
    s.energy()
    s.order()
    s.energy("insert in front of its source: live %d" % nv)
    assert s.remove(one[6])
    assert s.insert(one[2]) == one[6]
    s.order()
    s.energy("remove and insert: live %d" % nv)
    return s


def variant_scenario(variant):
    """one insert and one remove under every pair / field kernel variant, on 160 atoms"""
    s = Script("pair " + variant, synth.s_pol(160), adv.VARIANTS[variant], 192)
    s.energy("upload")
    assert s.insert(50) == 160
    s.energy("insert")
    assert s.remove(100)
    s.energy("remove")
    return s


def ewald_scenario(kmax):
    """S-ES dimers (rd_lrc on): es_self and es_recip follow inserts into holes and appended ones"""
    s = Script("ewald kmax %d" % kmax, synth.s_es(126), dict(ES, ewald_kmax=kmax, rd_lrc=1), 160)
    s.energy("upload")
    assert s.remove(62) and s.remove(64)  # across the 64-atom block of the structure factors
    s.energy("two dimers removed")
    assert s.insert(10) == 64 and s.insert(20) == 62 and s.insert(30) == 126
    s.energy("three inserted: 128 atoms")
    return s


def frozen_scenario(variant):
    """a frozen framework (the first 12 molecules) and one insert with frozen = True: frozen-frozen pairs stay excluded"""
    base = dict(synth.s_pol(160))
    base["frozen"] = base["frozen"].copy()
    base["frozen"][:60] = 1
    s = Script("frozen " + variant, base, adv.VARIANTS[variant], 192)
    s.energy("upload")
    assert s.insert(10, frozen=True) == 160
    s.energy("frozen insert")
    assert s.insert(100) == 165
    s.energy("movable insert")
    return s


def order_scenario():
    """update_atoms(m), remove(m), an insert into that hole elsewhere -- all before one energy()"""
    s = Script("order", synth.s_pol(160), pc.JACOBI4, 192)
    s.energy("upload")
    s.move(35, 5)
    assert s.remove(35)
    assert s.insert(90) == 35
    s.energy("move, remove, insert")
    return s


def burst_scenario(each):
    """260 edited atoms between two energy() calls (the engine gives up its list past 256 and recomputes everything),
    against the same edits with energy() after each one"""
    s = Script("burst each" if each else "burst", synth.s_pol(160), pc.JACOBI4, 192, seed=1)
    s.rng = np.random.default_rng(77)  # (both forms draw the same placements)
    s.energy("upload")
    firsts = s.molecules(5)[:26]
    for f in firsts:
        assert s.remove(f)
        if each:
            s.energy()
    for k, f in enumerate(reversed(firsts)):
        assert s.insert(150) == f
        if each and k < 25:
            s.energy()
    assert each or s.model.full_pass
    s.energy("after 260 edited atoms")
    if not each:
        assert s.remove(150) is True  # (the list is empty again after the call)
        s.energy("one more remove")
    return s


def far_scenario():
    """an insert 200 cells away (|x| > 2048 A): the pair screen switches to fp64"""
    s = Script("far", synth.s_pol(160), pc.JACOBI4, 192, capped=False)
    s.energy("upload")
    assert s.insert(50, shift=(200.0, 0.0, 0.0)) == 160
    assert np.abs(s.model.pos[160:165]).max() > 2048.0
    s.energy("insert beyond 2048 A")
    assert s.remove(160)
    s.energy("removed again")
    return s


def hole_update_scenario(touch):
    """update_atoms addressed to a hole slot: accepted, and no bit of any result changes, then or after the slot is
    reused (touch = False: the same script without that call)"""
    s = Script("hole update" if touch else "hole untouched", synth.s_pol(160), pc.JACOBI4, 192, seed=2)
    s.rng = np.random.default_rng(78)
    s.energy("upload")
    assert s.remove(45)
    s.energy("removed")
    if touch:
        s.move(45, 5, delta=(0.9, -1.3, 0.4))
    s.energy("hole moved", same_as_previous=touch)
    assert s.insert(80) == 45
    s.energy("hole reused")
    return s


def walk_scenario(seed, flags):
    """about 60 operations drawn from {move, insert, remove, energy, dipoles} on S-POL(160) in a context of 224"""
    params = pc.PRODUCTION if flags == "production" else pc.JACOBI4
    s = Script("walk %s %d" % (flags, seed), synth.s_pol(160), params, 224, seed=seed)
    rng = np.random.default_rng(seed)
    s.energy("upload")
    points, edited = 1, False
    for step in range(60):
        kind = rng.choice(["move", "insert", "remove", "energy", "dipoles"], p=[0.25, 0.25, 0.2, 0.2, 0.1])
        live = s.molecules()
        if kind == "move":
            first = live[int(rng.integers(len(live)))]
            count = s.model.molecules[int(s.model.mol[first])][1]
            s.move(first, count, delta=rng.uniform(-0.05, 0.05, 3))
        elif kind == "insert":
            first = live[int(rng.integers(len(live)))]
            edited = s.insert(first) is not None or edited
        elif kind == "remove" and len(live) > 8:
            edited = s.remove(live[int(rng.integers(len(live)))]) or edited
        elif kind in ("energy", "dipoles"):
            if edited and s.model.order_mode():
                s.order()
            edited = False
            compare = kind == "dipoles" or points < 12
            if compare and points < 19:
                points += 1
                s.energy("step %d" % step)
            else:
                s.energy()
    if edited and s.model.order_mode():
        s.order()
    s.energy("end of the walk")
    return s


def deferred_scenario():
    """The one large case: fixed-count Jacobi on a view of 1345 slots, whose sweeps past ceil(n / 2) are deferred.  The
    upload is the committed case nv1345 with molecule 100 missing and one extra molecule at the end; the extra one
    leaves, molecule 100 enters the hole it left: the live set is exactly nv1345's atoms in another slot arrangement, so
    the cached polar_cases.tensor("nv1345") serves through the permutation Script.permutation."""
    full = pc.system("nv1345")
    n = len(full["charge"])
    gone = np.arange(500, 505)  # molecule 100: (H2G, H2E, H2E, 0, 0) with whatever alpha sized() left it
    src = np.arange(700, 705)
    keep = np.r_[0:500, 505:n]
    rel = full["pos"][src] - full["pos"][src].mean(axis=0)
    helper = Script("deferred placement", full, pc.JACOBI4, n + 5)
    extra = helper.spot(rel)
    up = {k: (v if k == "basis" else np.concatenate([v[keep], v[src]])) for k, v in full.items()}
    up["pos"] = np.concatenate([full["pos"][keep], extra])
    up["molecule"] = np.concatenate([full["molecule"][keep], [full["molecule"].max() + 1] * 5]).astype(np.int32)
    nsites = int(np.count_nonzero(full["alpha"][gone])) - int(np.count_nonzero(full["alpha"][src]))
    assert int(np.count_nonzero(up["alpha"])) == 1345 - nsites
    s = Script("deferred", up, pc.JACOBI4, n, options=dict(timing=2))
    s.energy()
    assert s.remove(n - 5)
    m = s.model
    first = m.insert(full["pos"][gone], *[full[k][gone] for k in em.FIELDS], frozen=False)
    assert first == n - 5
    s.ops.append(dict(op="insert", pos=full["pos"][gone].copy(), props={k: full[k][gone].copy() for k in em.FIELDS},
                      frozen=False, expect=first, slot_count=m.slot_count))
    assert len(m.view) >= 1345 and m.live_view_count() == 1345
    s.permutation = np.r_[0:500, n - 5:n, 500:n - 5]  # slot of every atom of nv1345
    assert np.array_equal(m.pos[s.permutation], full["pos"]) and np.array_equal(m.prop["alpha"][s.permutation], full["alpha"])
    return s


def restore_scenario(flags):
    """a remove and an insert that give the upload's slot layout (and order) back: every bit equals a fresh engine's"""
    params = pc.PRODUCTION if flags == "production" else pc.JACOBI4
    s = Script("restore " + flags, synth.s_pol(160), params, 192)
    s.energy("upload")
    m = s.model
    pos, nxt = m.pos[70:75].copy(), int(m.mol[75])
    assert s.remove(70)
    if m.order_mode():
        s.order()
    s.energy("removed")
    assert s.insert(40, pos=pos, before=nxt) == 70  # (every molecule of S-POL carries the same properties)
    if m.order_mode():
        s.order()
    s.energy("restored")
    assert np.array_equal(m.pos[:160], s.system["pos"]) and list(m.live_slots("caller")) == list(range(160))
    return s


SCENARIOS = {
    "restore_jacobi": lambda: restore_scenario("jacobi"),
    "restore_production": lambda: restore_scenario("production"),
    "slots": slots_scenario,
    "tiles128": tiles128_scenario,
    "tiles192": tiles192_scenario,
    "view_steps": view_steps_scenario,
    "view_holes": view_holes_scenario,
    "view_alpha": view_alpha_scenario,
    "order": order_scenario,
    "burst": lambda: burst_scenario(False),
    "burst_each": lambda: burst_scenario(True),
    "far": far_scenario,
    "hole_update": lambda: hole_update_scenario(True),
    "hole_untouched": lambda: hole_update_scenario(False),
    "ewald_kmax1": lambda: ewald_scenario(1),
    "ewald_kmax7": lambda: ewald_scenario(7),
    "frozen_ewald_fh0": lambda: frozen_scenario("ewald_fh0"),
    "frozen_field_bare": lambda: frozen_scenario("field_bare"),
    "walk_jacobi": lambda: walk_scenario(11, "jacobi"),
    "walk_production": lambda: walk_scenario(12, "production"),
}
for _nv in (65, 129):
    for _flags in ("production", "gs3"):
        SCENARIOS["gs_%s_%d" % (_flags, _nv)] = functools.partial(gauss_seidel_scenario, _nv, _flags)
for _v in sorted(adv.VARIANTS):
    SCENARIOS["pair_" + _v] = functools.partial(variant_scenario, _v)
JACOBI_FORMS = ("view_steps", "view_holes", "view_alpha")  # run in the three forms of the Jacobi solve


@functools.lru_cache(maxsize=None)
def scenario(name):
    if name.startswith("excluded "):
        return excluded_scenario(name[len("excluded "):])
    if name == "deferred":
        return deferred_scenario()
    return SCENARIOS[name]()


# ---------------------------------------------------------------------------------------------------------------------
# the harness: replaying a Script on an engine, and one comparison point against model and references
# ---------------------------------------------------------------------------------------------------------------------
VECTORS = ("mu", "ef_static", "ef_induced", "ef_induced_change")
LD = pref.LD


def keys_of(params):
    return ("mu", "ef_induced") + (("ef_induced_change",) if params.get("polar_palmo") else ())


def same_bits(a, b, what):
    """two (record, vectors) of play(): every result field and every vector"""
    for k, v in a[0].items():
        assert v == b[0][k], (what, k, v, b[0][k])
    assert (a[1] is None) == (b[1] is None), what
    if a[1] is not None:
        for k in VECTORS:
            assert np.array_equal(a[1][k], b[1][k]), (what, k)


def stale_table(script, point):
    """the pair table of the live atoms PLUS the atoms removed since the last comparison point (each a molecule of its
    own, appended), and the appended atoms' slots: what a hole that still contributes would add"""
    snap = point["snap"]
    s = {k: (v if k == "basis" else np.array(v)) for k, v in snap["system"].items()}
    gone = snap["gone"]
    if not gone:
        return None, None, []
    n = len(s["charge"])
    s["pos"] = np.concatenate([s["pos"], [g["pos"] for g in gone]])
    for k in em.FIELDS:
        s[k] = np.concatenate([s[k], [g[k] for g in gone]])
    s["frozen"] = np.concatenate([s["frozen"], [g["frozen"] for g in gone]]).astype(np.int32)
    s["molecule"] = np.concatenate([s["molecule"], s["molecule"].max() + 1 + np.arange(len(gone))]).astype(np.int32)
    return s, pr.pair_table(s, script.params), [n + k for k in range(len(gone))]


def explain_stale(script, point, channel, diff):
    """Which REMOVED atom, if it still contributed with all its pairs to the live atoms, explains got - want = diff on an
    energy channel ('rd' / 'es'); lines name its slot."""
    s, t, extra = stale_table(script, point)
    lines = []
    n = len(point["snap"]["system"]["charge"])
    for a, g in zip(extra, point["snap"]["gone"]):
        rows = np.flatnonzero(((t["i"] == a) & (t["j"] < n)) | ((t["j"] == a) & (t["i"] < n)))
        v = float(t[channel][rows].sum() - (t["es_intra"][rows].sum() if channel == "es" else 0))
        if v != 0.0:
            lines.append((abs(diff - v), "removed slot %d still contributing (%d pairs, %.6e) would leave a residual of %.3e"
                          % (g["slot"], len(rows), v, abs(diff - v))))
    lines.sort(key=lambda x: x[0])
    out = [l for _, l in lines[:3]]
    if lines:  # and its single pairs, by the per-pair explanation (the appended atoms' rows only)
        rows = np.flatnonzero((t["i"] >= n) ^ (t["j"] >= n))
        slot_of = {a: g["slot"] for a, g in zip(extra, point["snap"]["gone"])}
        for line in pr.explain_energy(t, channel, diff, rows, top=2):
            for a, sl in slot_of.items():
                line = line.replace(", %d)" % a, ", removed slot %d)" % sl)
            out.append(line)
    return out


def explain_stale_field(script, point, err):
    """the same for ef_static: err[n,3] = got - want on the live atoms"""
    s, t, extra = stale_table(script, point)
    n = len(point["snap"]["system"]["charge"])
    lines = []
    for a, g in zip(extra, point["snap"]["gone"]):
        f = np.zeros((n, 3))
        rows = np.flatnonzero((t["j"] == a) & (t["i"] < n))  # (appended atoms are the higher index of their pairs)
        np.add.at(f, t["i"][rows], np.asarray(t["field_i"][rows], dtype=np.float64))
        if f.any():
            res = float(np.abs(err - f).max())
            lines.append((res, "removed slot %d still contributing its field would leave %.3e of %.3e" % (
                g["slot"], res, float(np.abs(err).max()))))
    lines.sort(key=lambda x: x[0])
    return [l for _, l in lines[:3]]


def check_point(script, point, r, d, ranking=None, who="engine", zero_outside=True, path=""):
    """One evaluation (record r; vectors d in SLOT space, slot_count rows, or None) at a comparison point against the
    model (n_atoms, exact zeros in the holes) and the references.  Prints an EDITREF line; raises with the slot, site
    or pair that explains a difference."""
    snap, p = point["snap"], script.params
    s, slots = snap["system"], snap["slots"]
    what = "%s | %s | %s" % (script.name, point["label"], path or who)
    ref = references(script, point)
    want, sums, table = ref["oracle"], ref["sums"], ref["table"]
    assert r["n_atoms"] == point["n_atoms"] == len(slots), (what, r["n_atoms"], point["n_atoms"])
    pol = polarizable(script)
    ratios, msgs = {}, []
    for key, chan in (("rd_energy", "rd"), ("es_real", "es")):
        for name, w in (("per-pair reference", sums[key]), ("oracle", want[key])):
            ratios[key] = max(ratios.get(key, 0.0), rel(r[key], w) / RTOL)
            if not rel(r[key], w) < RTOL:
                msgs.append("%s %s: %s %.17g, %s %.17g, difference %.6e" % (what, key, who, r[key], name, w, r[key] - w))
                msgs += ["    " + m for m in explain_stale(script, point, chan, r[key] - float(sums[key]))]
                msgs += ["    " + m for m in pr.explain_energy(table, chan, r[key] - float(sums[key]))[:3]]
    try:
        check_energies(r, want)
    except AssertionError as e:
        msgs.append("%s check_energies against the oracle: %s" % (what, e))
    if not p.get("rd_only") and not p.get("wolf"):
        u, du = pr.ewald_recip_energy(s, p)
        diff = abs(float(LD(r["es_recip"]) - u))
        ratios["es_recip"] = diff / du if du else 0.0
        if not diff <= du:
            msgs.append("%s es_recip %.17g, reference %.17g, difference %.3e, bound %.3e" % (what, r["es_recip"], float(u), diff, du))
        us, nterms = pr.ewald_self_energy(s, p)
        if not abs(float(LD(r["es_self"]) - us)) <= 2 * nterms * np.spacing(abs(float(us))):
            msgs.append("%s es_self %.17g, reference %.17g" % (what, r["es_self"], float(us)))
    if pol:
        assert d is not None, what
        for k in VECTORS:
            assert d[k].shape == (snap["slot_count"], 3), (what, k, d[k].shape)
            if zero_outside:
                bad = snap["holes"][np.abs(d[k][snap["holes"]]).max(axis=1) != 0.0] if len(snap["holes"]) else []
                if len(bad):
                    msgs.append("%s %s is not zero in the hole slots %s" % (what, k, list(bad[:8])))
        got = {k: d[k][slots] for k in VECTORS}
        for name, w in (("per-pair reference", sums["ef_static"]), ("oracle", want["ef_static"])):
            scale = float(np.abs(w).max())
            err = float(np.abs(got["ef_static"] - w).max()) if len(slots) else 0.0
            ratios["ef_static"] = max(ratios.get("ef_static", 0.0), err / (FIELD_TOL * scale) if scale else 0.0)
            if not err <= FIELD_TOL * scale:
                msgs.append("%s ef_static against the %s: max error %.6e, allowed %.6e" % (what, name, err, FIELD_TOL * scale))
                msgs += ["    " + m for m in explain_stale_field(script, point, got["ef_static"] - sums["ef_static"])]
                msgs += ["    " + m.replace("atom ", "live atom ") for m in pr.explain_field(table, got["ef_static"], sums["ef_static"], top=3)]
        t = ref["tensor"]
        res = pref.solve(t, s, p, got["ef_static"])
        if zero_outside:
            off = np.flatnonzero(np.asarray(s["alpha"]) == 0.0)
            bad = off[np.abs(got["mu"][off]).max(axis=1) != 0.0] if len(off) else []
            if len(bad):
                msgs.append("%s: a dipole on sites with alpha = 0 -- a view slot that kept its polarizability? slots %s" % (
                    what, [int(slots[a]) for a in bad[:8]]))
                msgs += ["    slot %d = " % int(slots[a]) + l for a in bad[:2] for l in pref.explain(t, s, res, got["mu"], "mu", top=1)]
        if not msgs:
            try:
                ratios.update(pref.check(t, s, res, got, keys_of(p), what=what, zero_outside=zero_outside))
            except AssertionError as e:
                lines = str(e).split("\n")
                for k, line in enumerate(lines):  # explain() speaks of the compacted atoms: add their slots
                    if line.strip().startswith("atom "):
                        a = int(line.split()[1])
                        lines[k] = line + " [atom %d is slot %d]" % (a, int(slots[a]))
                msgs.append("\n".join(lines))
            if not p.get("polar_palmo") and zero_outside and d["ef_induced_change"].any():
                msgs.append("%s ef_induced_change is not zero without polar_palmo" % what)
            if (r["polar_iterations"], r["iter_success"]) != (res["polar_iterations"], res["iter_success"]):
                msgs.append("%s polar_iterations / iter_success %r, reference %r" % (
                    what, (r["polar_iterations"], r["iter_success"]), (res["polar_iterations"], res["iter_success"])))
            try:
                ratios["U_pol"] = pref.check_energy(res, r["polarization_energy"], what=what)
            except AssertionError as e:
                msgs.append(str(e))
            if p.get("polar_gs_ranked") and ranking is not None:
                rank, order = ranking
                if not np.array_equal(np.asarray(rank)[slots], res["rank_metric"]):
                    msgs.append("%s rank_metric differs from the reference's" % what)
                is_pol = np.zeros(snap["slot_count"], bool)
                is_pol[slots[t.view]] = True
                got_order = [int(a) for a in order if 0 <= a < snap["slot_count"] and is_pol[a]]
                want_order = [int(slots[a]) for a in res["ranked_array"] if s["alpha"][a] != 0.0]
                if got_order != want_order:
                    k = next(i for i, (x, y) in enumerate(zip(got_order, want_order)) if x != y)
                    msgs.append("%s the ranked order of the polarizable sites differs from the reference's at position %d: "
                                "slot %d, reference slot %d" % (what, k, got_order[k], want_order[k]))
        if script.capped and t.nv:
            cap = 1e-11 * float(np.abs(res["mu"]).max())
            assert float(res["mu_err"].max()) <= cap, (what, "the reference's own bound exceeds the cap", float(res["mu_err"].max()), cap)
    print("EDITREF %s | n %d slots %d view %d live %d | %s" % (
        what, len(slots), snap["slot_count"], snap["view"], snap["live_view"],
        " ".join("%s %.3g" % kv for kv in sorted(ratios.items()))))
    assert not msgs, "\n".join(msgs)
    return ratios


def play(script, eng, refusal=Exception, check=None, each=False):
    """Replay a Script on an engine (mpmc_amd.engine.Engine with a slot_count() method, or a stand-in): every return value,
    slot_count() and n_atoms against the model's prediction.  check(point, r, d) runs at the comparison points.  each:
    an extra energy() after every insert / remove / move (not in Gauss-Seidel modes, which need the order first).
    Returns {label: (record, vectors or None)} of the comparison points."""
    pol = polarizable(script)
    out, prev = {}, None
    for k, op in enumerate(script.ops):
        kind, what = op["op"], "%s op %d %s" % (script.name, k, op["op"])
        if kind == "insert":
            got = eng.insert_molecule(op["pos"], *[op["props"][f] for f in em.FIELDS], frozen=op["frozen"])
            assert got == op["expect"], "%s returned %r, the model predicts %r" % (what, got, op["expect"])
        elif kind == "remove":
            got = eng.remove_molecule(op["first"], op["count"])
            assert bool(got) == op["expect"], "%s(%d, %d) returned %r, the model predicts %r" % (
                what, op["first"], op["count"], got, op["expect"])
        elif kind == "move":
            eng.update_atoms(op["first"], op["pos"])
        elif kind == "order":
            eng.set_sweep_order(op["slots"])
        elif kind == "option":
            eng.set_option(op["name"], op["value"])
        if kind in ("insert", "remove"):
            assert eng.slot_count() == op["slot_count"], (what, eng.slot_count(), op["slot_count"])
        if kind != "energy":
            if each and kind in ("insert", "remove", "move"):
                eng.energy()
            continue
        if op["n_atoms"] is None:
            try:
                eng.energy()
            except refusal as e:
                assert "set_sweep_order" in str(e), (what, str(e))
            else:
                raise AssertionError("%s: energy() ran without the sweep order of the edited configuration" % what)
            continue
        r = eng.energy()
        assert r["n_atoms"] == op["n_atoms"], (what, r["n_atoms"], op["n_atoms"])
        d = eng.dipoles() if (pol and op["dipoles"]) else None
        if op["same"]:
            assert prev is not None
            for key, v in prev[0].items():
                assert r[key] == v, (what, "a refused or ignored call changed", key, v, r[key])
            if d is not None and prev[1] is not None:
                for key in VECTORS:
                    assert np.array_equal(d[key], prev[1][key]), (what, "a refused or ignored call changed", key)
        prev = (r, d if d is not None else (prev[1] if op["same"] and prev else None))
        if op["label"] is not None:
            if check is not None:
                check(op, r, d)
            out[op["label"]] = (r, d)
    return out
