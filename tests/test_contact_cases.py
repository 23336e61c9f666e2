"""The inputs of the close-contact tests (tests/contact_cases.py) proved on the CPU: the reference counts exactly the
designed pairs, every case is decisive, the exact ties are exact in fp64 and in longdouble, the closed form holds, the
moves dirty at least three 64-atom blocks in descending order and change the count, and vdw_reference.explain() names the
tile of a deliberately altered input."""
import numpy as np
import pytest

import contact_cases as cc
import edit_model
import tile_pass_cases as tp
import vdw_reference as vr
from pair_reference import LD, minimum_image, pbc

CONDITION = 1e-12  # a case is decisive when min |rimg - scale| is above this; the cases are built with 1e-9


def _counted(table):
    return {(int(i), int(j)) for i, j, k in zip(table["i"], table["j"], table["counted"]) if k}


@pytest.mark.parametrize("n,cell", cc.CASES, ids=cc.CASE_IDS)
def test_the_designed_pairs_are_what_the_reference_counts(n, cell):
    c = cc.case(n, cell)
    s = c["system"]
    assert len(s["charge"]) == n
    count, margin = cc.reference(s, cc.SCALE, c["name"])
    table = vr.contact_table(s, c["flags"], cc.SCALE)
    designed = {(i, j) for i, j, counted, _ in c["designed"] if counted}
    twins = {(i, j) for i, j, counted, _ in c["designed"] if not counted}
    print(c["name"], "count", count, "margin", margin, "pairs within 1e-6 of the scale", cc.near(s, cc.SCALE))
    assert count == c["count"] == len(designed) == int(table["counted"].sum())
    assert _counted(table) == designed and not (twins & designed)
    assert margin > CONDITION and margin >= cc.MARGIN
    # the twins are the pairs just outside: as many pairs within 1e-6 of the scale as were designed
    assert cc.near(s, cc.SCALE) == len(designed) + len(twins)
    # the table's longdouble distances say the same as the fp64 decision, pair by pair
    assert ((table["rimg"] < LD(cc.SCALE)) == table["counted"]).all()


@pytest.mark.parametrize("n,cell", cc.CASES, ids=cc.CASE_IDS)
def test_the_designed_pairs_sit_where_the_plan_says(n, cell):
    c = cc.case(n, cell)
    s, p = c["system"], c["plan"]
    mol, frozen = np.asarray(s["molecule"]), np.asarray(s["frozen"]).astype(bool)
    sizes = set(np.unique(mol, return_counts=True)[1].tolist())
    assert sizes == {1, 2, 3, 5}
    pairs = {(i, j): name for i, j, counted, name in c["designed"] if counted}
    on_diag = {j % 64 for (i, j) in pairs if i // 64 == j // 64}
    want = {7, 8, 31, 56} | ({63} if n in (64, 128, cc.LARGE) else set())
    assert want <= on_diag, (want, on_diag)
    assert (n - 2, n - 1) in pairs or n in (65, 129)  # the last two real atoms (one tile) where both can be placed
    if n >= 65:
        assert any(i // 64 == 0 and j == 64 and (i % 64) // 8 == 7 for i, j in pairs)  # jj = 0; the row atom in slice 7
        assert any(j // 64 == i // 64 + 1 for i, j in pairs)
        border = [(first, k, frz) for first, k, frz in p["straddlers"]]
        for first, k, frz in border:
            assert first // 64 != (first + k - 1) // 64 and len(set(mol[first:first + k])) == 1
            assert frozen[first:first + k].all() == frz and frozen[first:first + k].any() == frz
            d = np.linalg.norm(s["pos"][first + 1] - s["pos"][first])
            assert abs(d - 0.7) < 1e-12  # two sites of one molecule 0.7 A apart across the border: ignored
    if n >= 129:
        assert any(i // 64 == 0 and j // 64 == (n - 1) // 64 for i, j in pairs)  # the tile of the first and the last block
        assert {frz for _, _, frz in p["straddlers"]} == {True, False}
    assert any(frozen[i] and frozen[j] for i, j in pairs) and any(frozen[i] != frozen[j] for i, j in pairs)
    # a pair across a cell face on each axis: its minimum image is not the stored displacement
    _, rb, _ = pbc(s["basis"])
    for axis in range(3):
        (i, j), = [(i, j) for (i, j), name in pairs.items() if name == "across face %d" % axis]
        image, r, rimg, _ = minimum_image(s["basis"], rb, s["pos"][i] - s["pos"][j])
        assert image[axis] != 0 and r > 10 * rimg


def test_exact_ties():
    """rimg == scale exactly, in fp64 and in longdouble, inside the cell and across a face: the pair does not count (<);
    one ulp more of scale and it does"""
    s = cc.ties()
    _, rb, _ = pbc(s["basis"])
    assert (np.asarray(rb) == np.diag([0.0625] * 3)).all()  # 1 / 16 exactly
    assert (s["pos"] * 8 == np.rint(s["pos"] * 8)).all()
    up = np.nextafter(cc.TIE_SCALE, 2.0)
    for i, j in ((0, 1), (2, 3)):
        d = s["pos"][i] - s["pos"][j]
        image, _, rimg, dimg = minimum_image(s["basis"], rb, d)
        assert rimg == cc.TIE_SCALE and sorted(np.abs(dimg)) == [0.0, 1.125, 1.5]
        assert (image != 0).any() == (i == 2)
    t = vr.contact_table(s, cc.FLAGS, cc.TIE_SCALE)
    tie = [k for k in range(len(t["i"])) if (t["i"][k], t["j"][k]) in ((0, 1), (2, 3))]
    assert len(tie) == 2 and all(t["rimg"][k] == LD(cc.TIE_SCALE) and not t["counted"][k] for k in tie)
    assert vr.close_contacts(s, cc.FLAGS, cc.TIE_SCALE) == (0, 0.0)
    assert vr.close_contacts(s, cc.FLAGS, up)[0] == 2
    assert _counted(vr.contact_table(s, cc.FLAGS, up)) == {(0, 1), (2, 3)}


@pytest.mark.parametrize("n,cell", cc.CASES, ids=cc.CASE_IDS)
def test_closed_form(n, cell):
    s = cc.case(n, cell)["system"]
    count, margin = cc.reference(s, cc.BIG_SCALE, cc.case(n, cell)["name"])
    assert count == cc.closed_form(s["molecule"]) and margin > 900.0
    # and before and after removals, on the slots of the edit model
    if n <= 130:
        model = edit_model.Model(s, cc.FLAGS, n + 16)
        model.energy()
        movable = [(first, k) for first, k in edit_model.runs(s["molecule"]) if not s["frozen"][first]]
        for first, k in movable[3:12:4]:
            assert model.remove(first, k)
        live, slots = model.live_system()
        assert len(slots) < n
        assert cc.reference(live, cc.BIG_SCALE)[0] == cc.closed_form(model.mol[:model.slot_count], model.valid[:model.slot_count])


def test_a_scale_above_half_the_shortest_box_width():
    s = cc.case(130, "sheared")["system"]
    _, _, half = pbc(s["basis"])
    scale = cc.WIDE_SCALE
    assert half < scale < 2 * half
    count, margin = cc.reference(s, scale, "sheared130")
    print("half width", half, "scale", scale, "count", count, "margin", margin)
    assert margin > CONDITION and margin >= cc.MARGIN
    assert cc.case(130, "sheared")["count"] < count < cc.closed_form(s["molecule"])


@pytest.mark.parametrize("n,cell", [(130, "cubic"), (130, "sheared"), (cc.LARGE, "cubic")])
def test_moves_dirty_three_blocks_in_descending_order_and_change_the_count(n, cell):
    c = cc.case(n, cell)
    s = c["system"]
    frozen = np.asarray(s["frozen"])
    if n < 1000:
        blocks = [first // 64 for first, _ in tp.moves(s)]
        assert len(set(blocks)) >= 3 and blocks == sorted(blocks, reverse=True)
    mv = cc.contact_moves(c)
    blocks = [first // 64 for first, _ in mv]
    touched = {a // 64 for first, new in mv for a in range(first, first + len(new))}
    assert len(touched) >= 3 and blocks == sorted(blocks, reverse=True) and blocks != sorted(blocks)
    assert 3 <= len(touched) <= 16 and sum(len(new) for _, new in mv) <= tp.MAX_MOVED
    for first, new in mv:
        assert not frozen[first:first + len(new)].any()
    t = tp.moved(s, mv)
    count, margin = cc.reference(t, cc.SCALE)
    before, after = vr.contact_table(s, c["flags"], cc.SCALE), vr.contact_table(t, c["flags"], cc.SCALE)
    made, broken = _counted(after) - _counted(before), _counted(before) - _counted(after)
    print(c["name"], "blocks", blocks, "count", c["count"], "->", count, "made", sorted(made), "broken", sorted(broken))
    assert margin > CONDITION and margin >= cc.MARGIN and count != c["count"] and made and broken
    moved_atoms = {a for first, new in mv for a in range(first, first + len(new))}
    dirty = touched

    def partner_blocks(pairs):
        out = set()
        for i, j in pairs:
            m, o = (i, j) if i in moved_atoms else (j, i)
            out.add(("lower" if o // 64 < m // 64 else "higher" if o // 64 > m // 64 else "same",
                     "dirty" if o // 64 in dirty and o // 64 != m // 64 else "clean"))
        return out

    kinds = partner_blocks(made | broken)
    assert {k for k, _ in kinds} >= {"lower", "higher"} and (("lower", "dirty") in kinds or ("higher", "dirty") in kinds)
    # more moves than the MoveList holds
    many = cc.too_many_moves(c)
    assert sum(len(new) for _, new in many) > tp.MAX_MOVED
    count2, margin2 = cc.reference(tp.moved(s, many), cc.SCALE)
    assert margin2 > CONDITION and margin2 >= cc.MARGIN and count2 != c["count"]


def test_explain_names_the_tile():
    c = cc.case(130, "cubic")
    s, f = c["system"], c["flags"]
    want = vr.contact_table(s, f, cc.SCALE)
    assert vr.explain(want, want) == ["the two tables count the same pairs (%d)" % c["count"]]
    # (1) a pair moved across the scale: the partner of the "first and last block" anchor, 2e-9 A outwards
    (i, j), = [(i, j) for i, j, counted, name in c["designed"] if counted and name == "first and last block"]
    pos = np.array(s["pos"])
    pos[i] += 2 * cc.EDGE * cc.E1
    got = vr.contact_table(dict(s, pos=pos), f, cc.SCALE)
    lines = vr.explain(got, want)
    assert lines[0] == "tile (%d, %d): -1 (0 extra, 1 missing)" % (i // 64, j // 64) and len(lines) == 2, lines
    assert "missing pair (%d, %d)" % (i, j) in lines[1]
    # (2) a hole counted: the reference without the atom (a removed one-site molecule) against the table that keeps it
    present = np.ones(130, dtype=bool)
    present[j] = False
    hole = vr.contact_table(s, f, cc.SCALE, present=present)
    lines = vr.explain(want, hole)
    assert lines[0].startswith("tile (%d, %d): +" % (i // 64, j // 64)) and "extra pair (%d, %d)" % (i, j) in "\n".join(lines)
    assert {ln.split(":")[0] for ln in lines if ln.startswith("tile")} == \
        {"tile (%d, %d)" % (min(a, b) // 64, max(a, b) // 64) for a, b in _counted(want) if j in (a, b)}
    # (3) a same-molecule pair counted: the two border sites 0.7 A apart, given different molecule ids
    first = c["plan"]["straddlers"][0][0]
    mol = np.array(s["molecule"])
    mol[first + 1:] += 1
    got = vr.contact_table(dict(s, molecule=mol), f, cc.SCALE)
    lines = vr.explain(got, want)
    assert lines[0] == "tile (0, 1): +1 (1 extra, 0 missing)" and "extra pair (63, 64)" in lines[1], lines
