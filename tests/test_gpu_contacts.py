"""GPU tests of the close-contact count (cavity_autoreject_absolute) beyond one tile: contact_tile_kernel
(mpmc_amd/csrc/kernels_vdw.h) on the pair kernel's grid and dirty-block selection, the fold of its channel of the tile
partials inside publish_result_kernel and by reduce_rows_kernel on the side stream, and the two publishers, at 63 .. 130 and
2050 atoms (tests/contact_cases.py; tests/test_contact_cases.py proves those inputs on the CPU).

Every comparison is ==: the count against the fp64-decision / longdouble reference (vdw_reference.close_contacts), against
the closed form C(n, 2) - sum C(m_k, 2) at a scale of 1e3 A, against a fresh context or a full pass; every other number
against the same run with the count off, because counting changes no other number.  No tolerance is introduced.  A case
enters only if it is decisive (min |rimg - scale| over the different-molecule pairs well above the fp64 rounding of a
minimum image in a 20 .. 45 A box, ~1e-14 A): asserted next to each reference.
"""
import numpy as np
import pytest

import contact_cases as cc
import edit_model
import rdforms_cases as rf
import tile_pass_cases as tp
import vdw_cases as vc
import vdw_reference as vr
from mpmc_amd import engine, host, synth
from pair_reference import kvector_list

pytestmark = pytest.mark.gpu
FIELDS = [f for f, _ in engine.Result._fields_]
CONDITION = 1e-12  # decisive: min |rimg - scale| above this (every configuration evaluated here has 1e-9: cc.MARGIN)


def _ar(scale):
    return dict(cavity_autoreject_absolute=1, cavity_autoreject_scale=scale) if scale else {}


def _engine(s, flags, scale=0.0, cap=None, **options):
    e = engine.Engine(len(s["charge"]) if cap is None else cap)
    for k, v in options.items():
        e.set_option(k, v)
    e.load_system(s, dict(flags, **_ar(scale)))
    if flags.get("polar_gs") or flags.get("polar_gs_ranked"):
        e.set_option("gs_lags", 2)  # (pinned as tests/test_gpu_npt.py does: the lag count depends on a context's history)
    return e


def _bits(a, b):
    return a == b or (a != a and b != b)


def _same(got, want, what, skip=("close_contacts",)):
    """every field of two records, bit for bit"""
    assert sorted(got) == sorted(want), what
    diff = {k: (got[k], want[k]) for k in want if k not in skip and not _bits(got[k], want[k])}
    assert not diff, (what, diff)


def _want(s, scale, key=None, flags=cc.FLAGS, floor=cc.MARGIN):
    count, margin = cc.reference(s, scale, key, flags)
    assert margin > CONDITION and margin >= floor, (key, scale, margin)
    return count


def _explain(s, flags, scale, what):
    """for the assertion message: the tiles the reference counts pairs in"""
    return what, "reference tiles", vr.contact_tiles(vr.contact_table(s, flags, scale))


# ---- from scratch
@pytest.mark.parametrize("n,cell", cc.CASES, ids=cc.CASE_IDS)
def test_from_scratch(n, cell):
    """the count of an upload at every size and cell == the reference == the designed pairs; at a scale of 1e3 A == the
    closed form (a lost or doubled tile, a padding lane taken for an atom); every Result field == the count off"""
    c = cc.case(n, cell)
    s, f = c["system"], c["flags"]
    want = _want(s, cc.SCALE, c["name"])
    assert want == c["count"]
    off = _engine(s, f)
    plain = off.energy()
    assert off.close_contacts() == 0
    off.close()
    e = _engine(s, f, cc.SCALE)
    r = e.energy()
    got = e.close_contacts()
    print(c["name"], "count", got, "reference", want)
    assert got == want, _explain(s, f, cc.SCALE, (c["name"], got, want))
    assert r == plain and r["status"] == 0 and r["n_atoms"] == n
    e.set_autoreject(cc.BIG_SCALE)
    assert e.energy() == plain
    assert e.close_contacts() == cc.closed_form(s["molecule"]) == _want(s, cc.BIG_SCALE, c["name"])
    if (n, cell) == (130, "sheared"):  # above half the shortest box width: only the minimum image decides
        e.set_autoreject(cc.WIDE_SCALE)
        assert e.energy() == plain
        assert e.close_contacts() == _want(s, cc.WIDE_SCALE, c["name"])
    e.set_autoreject(cc.SCALE)
    assert e.energy() == plain and e.close_contacts() == want
    e.close()


def test_exact_ties():
    """A cubic cell of edge 16 and coordinates that are multiples of 1 / 8: the pair displaced by (1.125, 0, 1.5), inside the
    cell and across the x face, has rimg == 1.875 == scale and must NOT count (<); with scale one ulp up it must.

    Why the device arithmetic is exact here (minimum_image, device_common.h, compiled without FMA contraction): the
    reciprocal basis is diag(1 / 16) exactly (1 / 4096 * 256); a displacement component d is a multiple of 1 / 8 below 16,
    so d / 16 is exact and so are the two zero products added to it; rint() gives 0 or +-1; 16 * 1 and d - 16 are exact;
    the squares 1.265625 and 2.25 and their sum 3.515625 = 1.875^2 are exact in binary, and sqrt of an exact square is
    exact.  fp64 on the device, fp64 and longdouble on the CPU give the same 1.875 (tests/test_contact_cases.py)."""
    s = cc.ties()
    up = float(np.nextafter(cc.TIE_SCALE, 2.0))
    assert vr.close_contacts(s, cc.FLAGS, cc.TIE_SCALE) == (0, 0.0) and vr.close_contacts(s, cc.FLAGS, up)[0] == 2
    e = _engine(s, cc.FLAGS, cc.TIE_SCALE)
    e.energy()
    assert e.close_contacts() == 0
    e.set_autoreject(up)
    e.energy()
    assert e.close_contacts() == 2
    e.close()


# ---- incremental passes
@pytest.mark.parametrize("n,cell", [(130, "cubic"), (130, "sheared"), (cc.LARGE, "cubic")])
def test_incremental_passes(n, cell):
    """One evaluation after moves that dirty three or more 64-atom blocks, highest first (contact_cases.contact_moves: the
    same evaluation breaks and makes contacts with a lower block, a higher block and another dirty block): the count ==
    the reference == a context with incremental_pairs 0 == a fresh context.  Then the move is rejected (everything put
    back), then energy() with nothing moved, then more moved atoms than the MoveList holds."""
    c = cc.case(n, cell)
    s, f = c["system"], c["flags"]
    mv = cc.contact_moves(c)
    cur = tp.moved(s, mv)
    want0, want1 = _want(s, cc.SCALE, c["name"]), _want(cur, cc.SCALE, c["name"] + "/moved")
    assert want0 != want1
    live, full, off = _engine(s, f, cc.SCALE), _engine(s, f, cc.SCALE, incremental_pairs=0), _engine(s, f)
    ctx = (live, full, off)
    first = live.energy()
    assert full.energy() == first and off.energy() == first and live.close_contacts() == full.close_contacts() == want0

    def step(moves, state, want, what):
        for e in ctx:
            for at, new in moves:
                e.update_atoms(at, new)
        r = live.energy()
        got = live.close_contacts()
        print(c["name"], what, "count", got, "reference", want)
        assert got == want, _explain(state, f, cc.SCALE, (what, got, want))
        assert full.energy() == r and full.close_contacts() == want, what
        assert off.energy() == r and off.close_contacts() == 0, what  # counting changes no other number
        fresh = _engine(state, f, cc.SCALE)
        assert fresh.energy() == r and fresh.close_contacts() == want, what
        fresh.close()
        return r

    r1 = step(mv, cur, want1, "moved")
    assert r1["energy"] != first["energy"]
    back = [(at, s["pos"][at:at + len(new)]) for at, new in mv]
    assert step(back, s, want0, "rejected") == first
    assert step([], s, want0, "nothing moved") == first
    many = cc.too_many_moves(c)
    assert sum(len(new) for _, new in many) > tp.MAX_MOVED
    cur2 = tp.moved(s, many)
    want2 = _want(cur2, cc.SCALE, c["name"] + "/many")
    assert want2 != want0
    step(many, cur2, want2, "more moves than the list holds")
    for e in ctx:
        e.close()


# ---- every route from the tile partials to the host
POL = dict(temperature=150.0, polarization=1, polar_damp=2.1304, polar_max_iter=4)
NOT_FUSED_KMAX = {130: 7, cc.LARGE: 11}
# name -> (flags, options, begin / end?)
ROUTES = {
    "lj": (dict(temperature=150.0, rd_only=1), {}, False),          # two launches, the fold in the publish kernel
    "ewald_fused": (dict(cc.FLAGS, ewald_kmax=3), {}, False),      # the reciprocal slice rides in the pair launch
    "ewald_not_fused": (None, {}, False),                          # more k-vector chunks than tiles per side
    "wolf": (dict(cc.FLAGS, wolf=1), {}, False),
    "jacobi_sweeps": (POL, dict(resident_jacobi=0), False),        # side stream: reduce_rows_kernel, publish_side_kernel
    "jacobi_resident": (POL, dict(resident_jacobi=1), False),
    "jacobi_sweeps_1": (dict(POL, polar_max_iter=1), dict(resident_jacobi=0), False),
    "jacobi_resident_1": (dict(POL, polar_max_iter=1), dict(resident_jacobi=1), False),
    "gauss_seidel_production": (dict(synth.FLAGS_POL_PRODUCTION), {}, False),  # the join instead of the side record
    "exact": (dict(POL, polar_iterative=0), {}, False),
    "begin_end": (POL, {}, True),
    "begin_end_lj_ewald": (dict(cc.FLAGS), {}, True),
    "step_graph": (POL, dict(step_graph=1), False),                # the plan must decline; results unchanged
    # every atom polarizable (2050 sites, 33 coefficient tiles: more tile pairs than the device has CUs), untimed calls:
    # the last sweeps are deferred and the main record goes out behind the finish of sweep 2, the side record beside it
    "jacobi_deferred": (POL, dict(resident_jacobi=0, timing=0), False),
}
RESIDENT_ROUTES = ("jacobi_resident", "jacobi_resident_1", "begin_end", "step_graph")
ROUTE_CELLS = [(n, r) for n in (130, cc.LARGE) for r in sorted(ROUTES) if r != "jacobi_deferred" or n == cc.LARGE]


def _route(s, mv, flags, options, scale, begin_end):
    e = _engine(s, flags, scale, **options)
    out = []
    for moves in ([], mv):
        for at, new in moves:
            e.update_atoms(at, new)
        if begin_end:
            e.energy_begin()
            r = e.energy_end()
        else:
            r = e.energy()
        out.append((r, e.close_contacts(), e.timings()))
    e.close()
    return out


@pytest.mark.parametrize("n,route", ROUTE_CELLS, ids=["%d-%s" % c for c in ROUTE_CELLS])
def test_routes(n, route):
    """The count after the upload and after a move that changes it == the reference, and every other field == the same
    run with the count off, on every arrangement of launches that carries the tile partials to the host.  (2050 atoms: 1156
    partial rows, a second trip of the 1024-thread row loop of both reducers; a few dozen polarizable sites keep the
    solve short -- except on the deferred route, which needs a view of more tile pairs than the device has CUs and makes
    every atom polarizable.  The contexts of a route live one after the other: the resident solver wants the device alone.)
    That the route is the one its name says is asserted where the engine shows it: resident_calls and resident_fallbacks,
    pending_sweeps, graph_steps.  Whether the reciprocal slice rode in the pair launch is not shown by any getter; the two
    Ewald routes assert the rule of launch_pair_kernel (k-vector chunks against tiles per side) on their own numbers."""
    c = cc.case(n, "cubic")
    flags, options, begin_end = ROUTES[route]
    s = c["system"]
    ntile = (128 * ((n + 127) // 128)) // 64
    if route == "ewald_not_fused":
        flags = dict(cc.FLAGS, ewald_kmax=NOT_FUSED_KMAX[n])
        assert (len(kvector_list(flags["ewald_kmax"])) + 63) // 64 > ntile
    if route == "ewald_fused":
        assert (len(kvector_list(3)) + 63) // 64 <= ntile
    if route == "jacobi_deferred":
        s = cc.all_polarizable(s)
        assert int((s["alpha"] != 0).sum()) == n
    elif flags.get("polarization"):
        s = cc.polarizable(s, 40 if n > 1000 else None)
        nv = int((s["alpha"] != 0).sum())
        assert nv == 40 if n > 1000 else 64 < nv < 128  # (130 atoms: a view of two blocks)
    mv = cc.contact_moves(c)
    wants = (_want(c["system"], cc.SCALE, c["name"]), _want(tp.moved(c["system"], mv), cc.SCALE, c["name"] + "/moved"))
    assert wants[0] != wants[1]
    off = _route(s, mv, flags, {k: v for k, v in options.items() if k != "step_graph"}, 0.0, begin_end)
    on = _route(s, mv, flags, options, cc.SCALE, begin_end)
    for k, what in enumerate(("upload", "moved")):
        (r, count, t), (r0, count0, _) = on[k], off[k]
        print(n, route, what, "count", count, "reference", wants[k],
              {x: t[x] for x in ("resident_calls", "resident_fallbacks", "sweep_count", "graph_steps", "pending_sweeps")})
        assert count == wants[k] and count0 == 0, (route, what, count, wants[k])
        _same(r, r0, (route, what))
        assert r["status"] == 0
        assert t["graph_steps"] == 0
        if route.startswith("jacobi_sweeps") or route == "jacobi_deferred":
            assert t["resident_calls"] == 0
        if route in RESIDENT_ROUTES:  # the one-launch plan ran in both calls, and did not quietly fall back
            assert t["resident_calls"] == k + 1 and t["resident_fallbacks"] == 0, t
        if route == "jacobi_deferred":  # sweeps 3 and 4 are still to be launched: the record went out behind sweep 2
            assert t["pending_sweeps"] > 0 and r["polar_iterations"] == 4, t
        else:
            assert t["pending_sweeps"] == 0, t
    assert on[1][0]["energy"] != on[0][0]["energy"]


# ---- dense modes: the smallest committed case of each, with designed contacts added
DENSE_SCALE = 2.6
DENSE = {  # name -> (system and flags, seed of contact_cases.with_contacts)
    "disp_expansion": (lambda: tp.CASES["phahst-c320-polarizable"]()[:2], 5),
    "rd_crystal": (lambda: tp.CASES["rdc-t150-fh4"]()[:2], 5),
    "axilrod_teller": (lambda: tp.CASES["at-n320-lj"]()[:2], 4),
    "sg": (lambda: (rf.system("t130", "sg", "lb"), rf.flags("t130", rf.BASE, "sg", "lb")), 5),
    "polarvdw": (lambda: (vc.system("box130"), vc.FLAGS), 4),
}


@pytest.mark.parametrize("mode", sorted(DENSE))
def test_dense_modes(mode):
    """the count beside every dense term, from scratch and after the multi-block move: == the reference, and the mode's
    own term (with every other field and getter) == the count off"""
    make, seed = DENSE[mode]
    s0, f = make()
    s = cc.with_contacts(s0, DENSE_SCALE, seed=seed)
    mv = tp.moves(s)
    cur = tp.moved(s, mv)
    wants = (_want(s, DENSE_SCALE, flags=f), _want(cur, DENSE_SCALE, flags=f))
    assert wants[0] >= 2
    snaps = []
    for scale in (0.0, DENSE_SCALE):
        e = _engine(s, f, scale)
        a = tp.snapshot(e)
        for at, new in mv:
            e.update_atoms(at, new)
        b = tp.snapshot(e)
        e.close()
        snaps.append((a, b))
    for k, what in enumerate(("upload", "moved")):
        off, on = snaps[0][k], snaps[1][k]
        print(mode, what, "count", on["close_contacts"], "reference", wants[k])
        assert on["close_contacts"] == wants[k] and off["close_contacts"] == 0
        _same(on, off, (mode, what))
    term = {"axilrod_teller": "three_body", "polarvdw": "vdw_energy"}.get(mode, "rd_energy")
    assert snaps[1][0][term] != 0.0 and snaps[1][1][term] != snaps[1][0][term]


# ---- box events against the reference, and the setting itself
def _scaled(s, factor):
    """(basis, one displacement per molecule, the system) of a volume move by the linear factor: molecules move rigidly
    with their first atom"""
    mol, first = tp._per_molecule(s)
    delta = (factor - 1.0) * s["pos"][first]
    basis = np.asarray(s["basis"]) * factor
    return basis, delta, dict(s, basis=basis, pos=s["pos"] + delta[mol])


def test_scale_box_brings_pairs_inside_and_outside():
    """a linear factor of 1 - 2e-9 brings every twin (scale + 1e-9 A apart) to scale - 2e-9 A; 1 + 2e-9 takes every designed
    contact out: the count of the live context == the reference on the scaled system, in both directions and back"""
    c = cc.case(130, "cubic")
    s, f = c["system"], c["flags"]
    e = _engine(s, f, cc.SCALE)
    e.energy()
    assert e.close_contacts() == c["count"]
    twins = sum(1 for d in c["designed"] if not d[2])
    seen = []
    for factor in (1.0 - 2e-9, 1.0 + 2e-9):
        basis, delta, t = _scaled(s, factor)
        want = _want(t, cc.SCALE)
        assert e.scale_box(basis, delta) is True
        r = e.energy()
        got = e.close_contacts()
        print("scale_box", factor, "count", got, "reference", want)
        assert got == want, _explain(t, f, cc.SCALE, (factor, got, want))
        fresh = _engine(t, f, cc.SCALE)
        assert fresh.energy() == r and fresh.close_contacts() == want
        fresh.close()
        seen.append(got)
        basis, delta, back = _scaled(t, 1.0 / factor)  # and back (to the rounding of the factor: decisive all the same)
        assert e.scale_box(basis, delta) is True
        e.energy()
        assert e.close_contacts() == _want(back, cc.SCALE) == c["count"]
        s = back
    assert seen[0] >= c["count"] + twins - 2 and seen[1] <= 2  # (a pair on a molecule across a border moves with its first atom)
    e.close()


def test_the_scale_through_zero_and_back_on_a_live_context():
    c = cc.case(130, "cubic")
    s, f = c["system"], c["flags"]
    mv = cc.contact_moves(c)
    cur = tp.moved(s, mv)
    off = _engine(s, f)
    e = _engine(s, f, cc.SCALE)
    assert e.energy() == off.energy() and e.close_contacts() == c["count"]
    e.set_autoreject(0.0)
    for x in (e, off):
        for at, new in mv[:2]:
            x.update_atoms(at, new)
    assert e.energy() == off.energy() and e.close_contacts() == 0  # the moves were evaluated with the count off
    for x in (e, off):
        for at, new in mv[2:]:
            x.update_atoms(at, new)
    e.set_autoreject(cc.SCALE)
    assert e.energy() == off.energy()
    assert e.close_contacts() == _want(cur, cc.SCALE, c["name"] + "/moved")
    e.set_autoreject(cc.BIG_SCALE)
    e.energy()
    assert e.close_contacts() == cc.closed_form(s["molecule"])
    e.set_autoreject(0.0)
    assert e.energy() == off.energy() and e.close_contacts() == 0
    for x in (e, off):
        x.close()


# ---- edits
EDIT_SCALE = 2.6
EDIT_FLAGS = {
    "lj_ewald": dict(synth.FLAGS_ES),
    "disp_expansion": dict(synth.FLAGS_ES, disp_expansion=1, damp_dispersion=1, extrapolate_disp_coeffs=1),
}
DISP = ("c6", "c8", "c10")


def _edit_system(n, mode):
    """synth.s_pol(n): every molecule movable.  Under disp_expansion epsilon / sigma become the exponent and the range of the
    repulsion and every site with one gets dispersion coefficients.  Molecule 6 is moved into contact with atom 2."""
    s = synth.s_pol(n)
    if mode == "disp_expansion":
        on = s["epsilon"] != 0.0
        s = dict(s, epsilon=np.where(on, 3.5, 0.0), sigma=np.where(on, 2.6, 0.0), c6=np.where(on, 9.0, 0.0),
                 c8=np.where(on, 160.0, 0.0), c10=np.where(on, 4000.0, 0.0))
    pos = np.array(s["pos"])
    pos[30:35] += pos[2] + (EDIT_SCALE - cc.EDGE) * cc.E1 - pos[30]
    return dict(s, pos=pos)


def x_mol(mol, at):
    """the molecule dict `mol` with its first atom at `at`"""
    return dict(mol, pos=mol["pos"] + (np.asarray(at) - mol["pos"][0]))


class _Edits:
    """an engine and tests/edit_model.py's Model side by side; check() after every step"""

    def __init__(self, n, mode):
        self.s, self.f = _edit_system(n, mode), EDIT_FLAGS[mode]
        self.disp = mode == "disp_expansion"
        self.cap = n + 96
        self.model = edit_model.Model(self.s, {k: v for k, v in self.f.items() if k not in engine.DISP_NAMES}, self.cap)
        self.extra = {k: np.zeros(self.cap) for k in DISP}
        if self.disp:
            for k in DISP:
                self.extra[k][:n] = self.s[k]
        self.e = _engine(self.s, self.f, EDIT_SCALE, cap=self.cap)
        self.what = "%s/%d" % (mode, n)
        self.counts = []
        self.check("upload")

    def molecule(self, first, count):
        """the molecule in [first, first + count) as edit_molecules takes one"""
        m = self.model
        sl = slice(first, first + count)
        d = {k: m.prop[k][sl].copy() for k in edit_model.FIELDS}
        if self.disp:
            d.update({k: self.extra[k][sl].copy() for k in DISP})
        d["pos"] = m.pos[sl].copy()
        return d

    def edit(self, remove=(), insert=()):
        m = self.model
        for first, count in remove:
            assert m.remove(first, count)
            for k in DISP:
                self.extra[k][first:first + count] = 0.0
        want = []
        for d in insert:
            first = m.insert(d["pos"], *[d[k] for k in edit_model.FIELDS])
            assert first is not None
            if self.disp:
                for k in DISP:
                    self.extra[k][first:first + len(d["charge"])] = d[k]
            want.append(first)
        m.check_invariants()
        got = self.e.edit_molecules(list(remove), list(insert))
        assert got == want, (self.what, got, want)
        return want

    def check(self, what):
        m, e = self.model, self.e
        r = e.energy()
        m.energy()
        got = e.close_contacts()
        live, slots = m.live_system()
        want = _want(live, EDIT_SCALE, flags=self.f)
        print(self.what, what, "slots", m.slot_count, "atoms", m.n_atoms, "count", got, "reference", want)
        assert got == want and r["n_atoms"] == m.n_atoms and r["status"] == 0, (self.what, what, got, want)
        ids, present = m.mol[:m.slot_count], m.valid[:m.slot_count]
        e.set_autoreject(cc.BIG_SCALE)
        assert e.energy() == r
        assert e.close_contacts() == cc.closed_form(ids, present), (self.what, what, "closed form")  # no hole counts
        e.set_autoreject(EDIT_SCALE)
        assert e.energy() == r and e.close_contacts() == want, (self.what, what, "a full pass")
        self.counts.append(want)
        return want


@pytest.mark.parametrize("mode", sorted(EDIT_FLAGS))
@pytest.mark.parametrize("n", [65, 130])
def test_edits(n, mode):
    """With the count on: a molecule in contact leaves (the hole must not count); one enters the hole in contact with a
    block-0 atom, and again out of contact; molecules are appended until the tile grid has grown (65 atoms: 13 five-site
    molecules in two calls take the slots from 65 to 130, two blocks to three and the padded grid from 128 to 256), the
    first of them in contact with a block-0 atom; eight molecules leave and eight enter in one call.  After every step the
    count == the reference on the model's slots == a full pass, and at 1e3 A == the closed form."""
    x = _Edits(n, mode)
    m = x.model
    spacing = float(x.s["basis"][0][0]) / round(float(x.s["basis"][0][0]) / 3.6)
    gap = lambda first: m.pos[first] + 0.5 * spacing  # a body centre of the lattice: 3.1 A from the nearest sites
    mol = x.molecule(30, 5)
    x.edit(remove=[(30, 5)])
    x.check("the molecule in contact left")
    assert x.counts[-1] < x.counts[-2]
    assert x.edit(insert=[x_mol(mol, m.pos[7] + (EDIT_SCALE - cc.EDGE) * cc.E1)]) == [30]
    x.check("into the hole, in contact with atom 7")
    assert x.counts[-1] > x.counts[-2]
    x.edit(remove=[(30, 5)])
    x.check("and out again")
    assert x.edit(insert=[x_mol(mol, m.pos[7] + (EDIT_SCALE + cc.EDGE) * cc.E1)]) == [30]
    x.check("into the hole, 1e-9 A outside the scale")
    blocks = lambda: (m.slot_count + 63) // 64
    start, grids = m.slot_count, m.grids()[0]
    firsts = [5 * k for k in range(1, 14)]
    new = [x_mol(mol, m.pos[12] + (EDIT_SCALE - cc.EDGE) * cc.E1)] + [x_mol(mol, gap(a)) for a in firsts[1:]]
    if n == 65:
        assert x.edit(insert=new[:8]) == [start + 5 * k for k in range(8)]
        x.check("eight appended, the first in contact with atom 12")
        assert x.edit(insert=new[8:]) == [start + 40 + 5 * k for k in range(5)]
        x.check("five more: three blocks")
        assert blocks() == 3 and (grids, m.grids()[0]) == (128, 256)
    else:
        assert x.edit(insert=new[:2]) == [start, start + 5]
        x.check("two appended, the first in contact with atom 12")
    gone = [(a, 5) for a in (start, 10, 15, 20, 35, 40, 45, 50)]  # the appended one in contact among them
    back = [x_mol(mol, m.pos[17 if k == 0 else 3] + (EDIT_SCALE - cc.EDGE if k == 0 else 4.1 + 0.2 * k) * cc.E1) if k < 2
            else x_mol(mol, gap(a) + 0.3) for k, (a, _) in enumerate(gone)]
    assert len(x.edit(remove=gone, insert=back)) == 8
    x.check("eight out and eight in, in one call")
    x.e.close()


# ---- trial placements
@pytest.mark.parametrize("path", ["batched", "serial", "polarizable"])
def test_trial_placements_leave_the_count(path):
    """trial_energies() with placements that WOULD be in contact: close_contacts() is still that of the resident
    configuration, and energy() afterwards gives the same count and the same record"""
    c = cc.case(130, "cubic")
    s = c["system"]
    f = POL if path == "polarizable" else c["flags"]
    want = _want(s, cc.SCALE, c["name"])
    mol, frozen = np.asarray(s["molecule"]), np.asarray(s["frozen"])
    designed = set(c["plan"]["designed_atoms"])
    first = next(a for a in range(64, 130) if a not in designed and not frozen[a] and (mol == mol[a]).sum() == 3
                 and mol[a - 1] != mol[a])
    shape = s["pos"][first:first + 3] - s["pos"][first]
    targets = [s["pos"][a] + d * cc.E1 for a in (0, 70, 129) for d in (cc.SCALE - cc.EDGE, 0.8)]
    xyz = np.array([t + shape for t in targets])
    for t in xyz:  # each placement would change the count
        assert vr.close_contacts(dict(s, pos=np.concatenate([s["pos"][:first], t, s["pos"][first + 3:]])), f, cc.SCALE)[0] > want
    e = _engine(s, f, cc.SCALE, cap=130 + 16, **({"trial_batched": 0} if path == "serial" else {}))
    r = e.energy()
    assert e.close_contacts() == want
    energies = e.trial_energies(first, xyz)
    assert len(energies) == len(xyz) and e.trial_call_count() == 1
    assert e.close_contacts() == want
    assert e.energy() == r and e.close_contacts() == want
    e.update_atoms(first, xyz[0])  # and the placement for real
    e.energy()
    assert e.close_contacts() == _want(dict(s, pos=np.concatenate([s["pos"][:first], xyz[0], s["pos"][first + 3:]])), cc.SCALE)
    e.close()


# ---- through the host layer: seeded chains with cavity_autoreject_absolute on the 130-atom box
HOST_SCALE = 1.4  # no pair of the 130-atom box is in contact at the start: the designed pairs are 0.1 A outside
HOST_STEPS = 60
NPT = dict(seed=11, move_factor=0.05, extra={"ensemble": "npt", "pressure": "200.0", "volume_probability": "0.3",
                                              "volume_change_factor": "0.02"})
UVT = dict(seed=11, move_factor=0.05, extra={"ensemble": "uvt", "pressure": "300.0", "insert_probability": "0.5"})


def _host_chain(spec, reupload):
    """One chain, a step at a time: (HostSystem, [per step: accept, reject, accept_volume, reject_volume, natoms,
    count_autorejects, then every other observable the host layer returns: energy, volume, rd_energy, coulombic_energy,
    polarization_energy, cutoff, N, polar_iterations], the reference's count on the configuration every step KEPT).  reupload: the arm
    that uploads the whole configuration again at every volume step (npt: no volume notes) or change of N (uvt:
    incremental_amatrix 0, as tests/test_gpu_dense_edits_host.py does)."""
    c = cc.case(130, "cubic")
    s = c["system"]
    f = dict(c["flags"], cavity_autoreject_absolute=1, cavity_autoreject_scale=HOST_SCALE)
    assert _want(s, HOST_SCALE, c["name"], floor=0.05) == 0
    h = host.HostSystem(s, f, seed=spec["seed"], move_factor=spec["move_factor"], rot_factor=spec["move_factor"],
                        extra=spec["extra"])
    npt = spec["extra"]["ensemble"] == "npt"
    if npt:
        h.set_volume_notes(not reupload)
    h.energy()  # creates the context
    if not npt:
        h.set_option("incremental_amatrix", 0 if reupload else 1)
    trace, kept = [], []
    for _ in range(HOST_STEPS):
        h.mc_steps(1)
        o, v = h.observables(), h.vdw()
        trace.append((o["accept"], o["reject"], o["accept_volume"], o["reject_volume"], h.natoms(), v["count_autorejects"],
                      o["energy"], o["volume"], o["rd_energy"], o["coulombic_energy"], o["polarization_energy"], o["cutoff"],
                      o["N"], o["polar_iterations"]))
        cur = dict(s, pos=h.positions(), basis=h.basis()) if npt else h.system(h.basis())
        kept.append(vr.close_contacts(cur, f, HOST_SCALE)[0])
    return h, trace, kept


def _autoreject_steps_are_rejections(trace):
    prev = (0, 0, 0, 0, None, 0)
    for t in trace:
        if t[5] != prev[5]:
            assert t[5] == prev[5] + 1 and t[0] == prev[0] and t[1] == prev[1] + 1, (prev, t)
        prev = t


def test_host_npt_chain_with_autoreject():
    """ensemble npt, 60 steps on the 130-atom box, cavity_autoreject_scale 1.4.  Seed 11, move_factor = rot_factor = 0.05,
    pressure 200 atm, volume_change_factor 0.02 were chosen on the MI355X (on the re-uploading arm) so that every branch
    occurs; seen there: 33 moves accepted and 27 rejected, of which volume moves 7 accepted and 9 rejected; 12 autorejects.

    The chain on a live context (volume notes) == the arm that uploads the configuration again at every volume step: every
    observable of every step, count_autorejects, the final positions and basis.  A step that counts an autoreject is a
    rejected step; the reference counts no contact in any configuration the chain kept, the final one included.  (The
    host layer does not expose a step's trial configuration, so the reference cannot be asked which trials were in
    contact: a contact the device missed shows here as a kept configuration with a contact, one it invented does not --
    the engine-level tests above are what holds that.)"""
    live, t_live, kept_live = _host_chain(NPT, False)
    cur = (live.positions(), live.basis())
    o, v = live.observables(), live.vdw()
    print("npt + autoreject: accept %d reject %d, volume moves accepted %d rejected %d, autorejects %d" %
          (o["accept"], o["reject"], o["accept_volume"], o["reject_volume"], v["count_autorejects"]))
    live.close()
    up, t_up, kept_up = _host_chain(NPT, True)
    assert t_live == t_up
    assert np.array_equal(up.positions(), cur[0]) and np.array_equal(up.basis(), cur[1])
    up.close()
    assert o["accept"] + o["reject"] == HOST_STEPS
    assert v["count_autorejects"] >= 1 and o["accept_volume"] >= 1
    _autoreject_steps_are_rejections(t_live)
    assert not any(kept_live) and not any(kept_up)
    assert np.isfinite(o["energy"]) and o["energy"] < 1.0e40


def test_host_uvt_chain_with_autoreject():
    """ensemble uvt, 60 steps on the 130-atom box, cavity_autoreject_scale 1.4.  Seed 11, move_factor = rot_factor = 0.05,
    fugacity (`pressure`) 300, insert_probability 0.5 were chosen on the MI355X (on the re-uploading arm); seen there: 44
    moves accepted and 16 rejected, 11 accepted insertions and 10 accepted removals (130 -> 124 atoms), 10 autorejects.

    The editing arm against the arm that uploads again at every change of N: accept, reject, N and count_autorejects of
    every step ==, and the final positions == as sets of rows.  (The two arms keep different atom orders, so their energies
    differ in rounding and are not compared here; tests/test_gpu_dense_edits_host.py holds them to its 1e-10.)  A step
    that counts an autoreject is a rejected step; the reference counts no contact in any configuration either arm kept."""
    edits, t_edit, kept_edit = _host_chain(UVT, False)
    pos = edits.positions()
    o, v = edits.observables(), edits.vdw()
    ce = edits.sync_counts()
    edits.close()
    up, t_up, kept_up = _host_chain(UVT, True)
    cu = up.sync_counts()
    ns = [130] + [t[4] for t in t_edit]
    ins = sum(1 for a, b in zip(ns, ns[1:]) if b > a)
    rem = sum(1 for a, b in zip(ns, ns[1:]) if b < a)
    print("uvt + autoreject: accept %d reject %d, insertions %d removals %d, N %d, autorejects %d; editing arm %s, "
          "re-uploading arm %s" % (o["accept"], o["reject"], ins, rem, ns[-1], v["count_autorejects"], ce, cu))
    assert [t[:6] for t in t_edit] == [t[:6] for t in t_up]
    assert sorted(map(tuple, pos)) == sorted(map(tuple, up.positions()))
    up.close()
    assert v["count_autorejects"] >= 1 and ins >= 1 and rem >= 1
    # (which arm edited and which uploaded; the option call behind the first energy() costs the editing arm one upload)
    assert ce["edit_calls"] >= ins + rem and cu["edit_calls"] == 0 and cu["full_uploads"] > ins + rem >= ce["full_uploads"]
    _autoreject_steps_are_rejections(t_edit)
    assert not any(kept_edit) and not any(kept_up)
