"""Inputs of tests/test_gpu_tile_passes.py and tests/golden/make_dense_terms_guard.py: the smallest committed case of each
dense-term mode, a move of several molecules whose 64-atom blocks arrive at the engine in DESCENDING order, and the
sequence of evaluations both files record; and the modes and events of the test that pins what drops which cached sum
(EVENT_MODES, EVENTS).

Why descending.  A step of the existing incremental tests moves one molecule: one dirty block, or two in ascending order.
The rule "the tile of two dirty blocks belongs to the earlier entry of the list" (kernels_tile.h, owned_tile) decides
something only when a later entry has a lower block index than an earlier one: then the mutual tile must be computed
once, by the earlier entry, although the later one holds its row.
"""
import numpy as np

import at_cases as ac
import phahst_cases as pc
import rdc_cases as rc
import rdforms_cases as rf
import vdw_cases as vc
from mpmc_amd import synth
from mpmc_amd.engine import DISP_NAMES
from pair_reference import _molecule_index

MAX_MOVED = 32  # kMaxMoves: the moves ride in the MoveList of the pair kernel's launch
RDC_ORDER = 2


def _at_phahst(s):
    """tests/test_gpu_at.py's "phahst" variant: epsilon / sigma become the exponent b and the range rho"""
    on = s["epsilon"] != 0.0
    return dict(s, epsilon=np.where(on, 3.2, 0.0), sigma=np.where(on, 2.9, 0.0), c8=20.0 * s["c6"], c10=500.0 * s["c6"])


# name -> (system, flags, mode)
CASES = {
    "phahst-c320-polarizable": lambda: (pc.system("c320"), pc.VARIANTS["polarizable"], "phahst"),
    "phahst-c320-damp_extrapolate": lambda: (pc.system("c320"), pc.VARIANTS["damp_extrapolate"], "phahst"),
    "rdc-t150-fh4": lambda: (rc.system("t150"), rc.flags("fh4", RDC_ORDER), "rdc"),
    "rdc-t150-lrc": lambda: (rc.system("t150"), rc.flags("lrc", RDC_ORDER), "rdc"),
    "at-n320-lj": lambda: (ac.case("n320"), dict(synth.FLAGS_AT), "at"),
    "at-n320-phahst": lambda: (_at_phahst(ac.case("n320")), dict(synth.FLAGS_PHAHST, axilrod_teller=1), "at"),
}
# the three the multi-block test runs on (the guard records all six)
TEST_CASES = ("phahst-c320-polarizable", "rdc-t150-fh4", "at-n320-lj")
EDIT_CASE = "lj-s_pol320"  # plain Lennard-Jones + Ewald + rd_lrc: remove_molecule / insert_molecule (lj_lrc_kernel's pass)


def moves(s, seed=23):
    """[(first atom, new coordinates)], one non-frozen molecule per 64-atom block that has one, highest block first; where
    non-frozen molecules lie across a block border, the first of them stands for the block its first atom is in."""
    mol, frozen = np.asarray(s["molecule"]), np.asarray(s["frozen"])
    rng = np.random.default_rng(seed)
    mols = [np.flatnonzero(mol == m) for m in np.unique(mol[frozen == 0])]
    for idx in mols:
        assert np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx))) and not frozen[idx].any()
    if "active" in s:  # axilrod_teller cases: molecules with a site that carries the term first
        mols.sort(key=lambda idx: not np.isin(idx, s["active"]).any())
    straddlers = [idx for idx in mols if idx[0] // 64 != idx[-1] // 64]
    pick = {}  # block of the first atom -> atom indices of the molecule
    for idx in straddlers[:1] + mols:
        pick.setdefault(idx[0] // 64, idx)
    out = []
    for b in sorted(pick, reverse=True):
        idx = pick[b]
        c = s["pos"][idx].mean(axis=0)
        th = rng.uniform(-0.2, 0.2)
        rot = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]])
        out.append((int(idx[0]), (s["pos"][idx] - c) @ rot.T + c + rng.uniform(-0.15, 0.15, 3)))
    assert sum(len(new) for _, new in out) <= MAX_MOVED
    return out


def moved(s, mv):
    pos = s["pos"].copy()
    for first, new in mv:
        pos[first:first + len(new)] = new
    return dict(s, pos=pos)


def _record(e, mode):
    r = dict(e.energy())
    if mode == "at":
        r["three_body"] = e.three_body_energy()
    return r


def run_case(engine, name, **options):
    """(first evaluation, evaluation after the multi-block move) of a new context; each a dict of the Result fields, plus
    three_body in the axilrod_teller cases"""
    s, flags, mode = CASES[name]()
    e = engine.Engine(len(s["charge"]))
    for k, v in options.items():
        e.set_option(k, v)
    e.load_system(s, flags)
    first = _record(e, mode)
    for at, new in moves(s):
        e.update_atoms(at, new)
    after = _record(e, mode)
    e.close()
    return first, after


def run_edit_case(engine):
    """(first evaluation, after remove_molecule of molecule 26 -- which lies across the border of blocks 1 and 2 --, after
    insert_molecule puts it back) on synth.s_pol(320) without polarization"""
    s, flags = synth.s_pol(320), dict(synth.FLAGS_ES)
    assert flags.get("rd_lrc", 1) and not flags.get("polarization")
    idx = np.flatnonzero(np.asarray(s["molecule"]) == 26)
    assert idx[0] // 64 != idx[-1] // 64
    e = engine.Engine(320)
    e.load_system(s, flags)
    out = [dict(e.energy())]
    assert e.remove_molecule(int(idx[0]), len(idx)) is True
    out.append(dict(e.energy()))
    assert e.insert_molecule(s["pos"][idx], s["charge"][idx], s["alpha"][idx], s["epsilon"][idx], s["sigma"][idx],
                             s["mass"][idx]) == int(idx[0])
    out.append(dict(e.energy()))
    e.close()
    return out


# ---- What drops which cached sum, pinned from outside: a live context that went through an event
# against a fresh one on the final state.  One entry per mode that owns rd_energy, plus Axilrod-Teller: the smallest
# committed case of each (2 to 5 blocks of 64 atoms: full and incremental passes differ).
#   term          the field the mode's own term shows in
#   leave / back  leave the mode and come back to it, on a live context (plain Lennard-Jones leaves by entering rd_crystal)
#   fh4           the mode's existing tests run feynman_hibbs order 4
#   lrc           rd_lrc changes something in the mode (the sg form has no long-range correction: kernels_rdforms.h)
def _event_mode(system, flags, term, leave, back, fh4=False, lrc=True):
    return dict(system=system, flags=dict(flags), term=term, leave=leave, back=back, fh4=fh4, lrc=lrc)


def _rd_form_mode(form, mixing, base):
    return _event_mode(rf.system("t130", form, mixing), rf.flags("t130", base, form, mixing), "rd_energy",
                       lambda e, s, f: e.set_rd_form("off"), lambda e, s, f: e.set_rd_form(form, mixing), fh4=form == "lj",
                       lrc=form == "lj")


EVENT_MODES = {
    "lj": lambda: _event_mode(synth.s_pol(320), synth.FLAGS_ES, "rd_energy", lambda e, s, f: e.set_rd_crystal(RDC_ORDER),
                              lambda e, s, f: e.set_rd_crystal(0), fh4=True),
    "phahst": lambda: _event_mode(pc.system("c320"), pc.VARIANTS["polarizable"], "rd_energy",
                                  lambda e, s, f: e.set_dispersion(s),
                                  lambda e, s, f: e.set_dispersion(s, **{k: f[k] for k in DISP_NAMES if k in f})),
    "rd_crystal": lambda: _event_mode(rc.system("t150"), rc.flags("lrc", RDC_ORDER), "rd_energy",
                                      lambda e, s, f: e.set_rd_crystal(0), lambda e, s, f: e.set_rd_crystal(RDC_ORDER),
                                      fh4=True),
    "lj-waldmanhagler": lambda: _rd_form_mode("lj", "waldmanhagler", rf.POLAR),
    "sg": lambda: _rd_form_mode("sg", "lb", rf.BASE),
    "polarvdw": lambda: _event_mode(vc.system("box70"), vc.FLAGS, "vdw_energy", lambda e, s, f: e.set_vdw(s, enable=False),
                                    lambda e, s, f: e.set_vdw(s)),
    "axilrod_teller": lambda: _event_mode(ac.case("n320"), synth.FLAGS_AT, "three_body",
                                          lambda e, s, f: e.set_axilrod_teller(s, enable=False),
                                          lambda e, s, f: e.set_axilrod_teller(s)),
}
# the lj and phahst modes once more with the close-contact count on (cavity_autoreject_absolute; the count rides in the pair
# kernel's tile partials): every event then also holds close_contacts to a fresh context.  At 3.0 A the reference counts
# 203 pairs in synth.s_pol(320) and 30 in phahst_cases' c320.
AUTOREJECT = dict(cavity_autoreject_absolute=1, cavity_autoreject_scale=3.0)
AUTOREJECT_MODES = {"lj+autoreject": "lj", "phahst+autoreject": "phahst"}


def _with_autoreject(base):
    def make():
        m = EVENT_MODES[base]()
        return dict(m, flags=dict(m["flags"], **AUTOREJECT))
    return make


for _name, _base in AUTOREJECT_MODES.items():
    EVENT_MODES[_name] = _with_autoreject(_base)


def snapshot(e):
    """every Result field of an energy() and every mode's getters behind it (zeros outside their mode)"""
    return dict(e.energy(), three_body=e.three_body_energy(), vdw_energy=e.vdw_energy(), close_contacts=e.close_contacts(),
                **e.vdw_terms())


def _per_molecule(s):
    """(molecule index of every atom in upload order, first atom of every molecule)"""
    mol = _molecule_index(s["molecule"])
    return mol, np.array([np.flatnonzero(mol == m)[0] for m in range(mol.max() + 1)])


# An event: (live context, mode entry, system, flags, snapshot before) -> (system, flags of the final state, the snapshot
# that must differ from `before` or None for the one behind the event, the fields it must differ in).
def _ev_rd_lrc(e, m, s, f, before):
    f2 = dict(f, rd_lrc=0 if f.get("rd_lrc", 1) else 1)
    e.set_params(**f2)
    return s, f2, None, ("rd_energy",) if m["lrc"] else ()


def _ev_fh4(e, m, s, f, before):
    f2 = dict(f, feynman_hibbs=1, feynman_hibbs_order=4)
    e.set_params(**f2)
    return s, f2, None, ("rd_energy",)


def _ev_set_box(e, m, s, f, before):
    f2 = dict(f, pbc_cutoff=0.95 * before["cutoff"])
    e.set_box(s["basis"], f2["pbc_cutoff"])
    return s, f2, None, ("cutoff", "rd_energy")


def _ev_scale_box(e, m, s, f, before):
    mol, first = _per_molecule(s)
    basis, delta = np.asarray(s["basis"]) * 1.01, 0.01 * s["pos"][first]
    assert e.scale_box(basis, delta, f.get("pbc_cutoff", 0.0))
    return dict(s, basis=basis, pos=s["pos"] + delta[mol]), f, None, ("volume", "rd_energy")


def _ev_load_system(e, m, s, f, before):
    mol, first = _per_molecule(s)
    shift = np.random.default_rng(5).uniform(-0.05, 0.05, (len(first), 3))
    s2 = dict(s, pos=s["pos"] + shift[mol], epsilon=1.02 * s["epsilon"], sigma=1.01 * s["sigma"])
    e.load_system(s2, f)
    return s2, f, None, ("rd_energy", m["term"])


def _ev_full_passes(e, m, s, f, before):
    e.set_option("incremental_pairs", 0)
    mv = moves(s, seed=31)[:1]
    e.update_atoms(*mv[0])
    return moved(s, mv), f, None, ("energy",)


def _ev_leave_and_back(e, m, s, f, before):
    m["leave"](e, s, f)
    outside = snapshot(e)
    assert outside["status"] == 0
    m["back"](e, s, f)
    return s, f, outside, (m["term"],)


EVENTS = {
    "rd_lrc": _ev_rd_lrc,
    "fh4": _ev_fh4,
    "set_box": _ev_set_box,
    "scale_box": _ev_scale_box,
    "load_system": _ev_load_system,
    "full_passes": _ev_full_passes,
    "leave_and_back": _ev_leave_and_back,
}
FH4_MODES = ("lj", "rd_crystal", "lj-waldmanhagler", "lj+autoreject")  # (polarvdw refuses feynman_hibbs)
EVENT_CELLS = [(mode, ev) for mode in EVENT_MODES for ev in EVENTS if ev != "fh4" or mode in FH4_MODES]


# Further inputs of leave_and_back only: from one mode that owns rd_energy straight into another and back, where the cells
# above leave a mode only towards plain Lennard-Jones.  rd_crystal and set_rd_form are context settings, so nothing is
# uploaded in between; the state outside is the other mode's (status 0, another rd_energy), and both cases span 3 blocks.
def _crystal_to_form(e, s, f):
    e.set_rd_crystal(0)
    e.set_rd_form("lj", "lb")


def _form_to_crystal(e, s, f):
    e.set_rd_form("off")
    e.set_rd_crystal(RDC_ORDER)


def _crystal_to_lj_wh(e, s, f):
    e.set_rd_crystal(0)
    e.set_rd_form("lj", "waldmanhagler")


MODE_TO_MODE = {
    "rd_crystal>lj-lb": lambda: _event_mode(rc.system("t150"), rc.flags("lrc", RDC_ORDER), "rd_energy", _crystal_to_form,
                                            _form_to_crystal),
    "lj-waldmanhagler>rd_crystal": lambda: dict(_rd_form_mode("lj", "waldmanhagler", rf.POLAR), leave=_form_to_crystal,
                                                back=_crystal_to_lj_wh),
}
EVENT_MODES.update(MODE_TO_MODE)
EVENT_CELLS += [(mode, "leave_and_back") for mode in MODE_TO_MODE]
# polarvdw keeps e_iso per molecule type for as long as the mode stays on, through a box change and an upload (vdw.c:262-320;
# tests/test_gpu_vdw.py::test_scale_box_leaves_the_bits_of_a_fresh_context): behind these events it is the value from before,
# not the one a fresh context makes, and so are the two sums it enters
E_ISO_KEPT_BY = ("set_box", "scale_box", "load_system")
E_ISO_FIELDS = ("e_iso", "vdw_energy", "energy")


def guard_entries(engine):
    """{key: value} of everything tests/golden/dense_terms_guard.npz holds"""
    d = {}
    for name in CASES:
        for tag, r in zip(("first", "moved"), run_case(engine, name)):
            for k, v in r.items():
                d["%s:%s:%s" % (name, tag, k)] = v
    for tag, r in zip(("first", "removed", "inserted"), run_edit_case(engine)):
        for k, v in r.items():
            d["%s:%s:%s" % (EDIT_CASE, tag, k)] = v
    return d
