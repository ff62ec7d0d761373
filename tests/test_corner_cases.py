"""CPU only: the directed corner-stream cases of tests/corner_cases.py hold what they claim, shown from the oracle and the model alone.

* model_streams (the bitmaps in, the rule restated) equals the oracle's fitting_quad_smooth streams on every case, all seven passes; a mismatch
  here is about the model and is settled before any GPU test is trusted;
* the claims of every group, from the census: byte values and same-byte relations (a), neighbour placements of every pair of passes and across
  bytes, swizzle blocks and workgroups (b), run shapes and the counts on both sides of the LDS cap (c), edges (d), the batch triples (e);
* every deliberate defect of the model is seen by the case named in CAUGHT_BY;
* the model's colours per pass are what tests/graddec_cases.py::model_decode pops for the same bitmaps.
"""
import numpy as np
import pytest

from oracle.pyoracle import PASSES
from tests import corner_cases as cc
from tests import graddec_cases as gd

# defect -> the case that sees it (the smallest that does)
CAUGHT_BY = {"corner_order": "p0_64x64", "later_pass_wins": "mosaic_72x40", "larger_bit_wins": "p0_64x64", "row_major": "small_72x40", "no_clamp": "p0_64x64",
             "no_plus127": "p0_64x64", "no_round6": "p0_64x64", "left_across_wrap": "p0_64x64", "upright_owns_tl": "bytes_p0_0"}


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle_built):
    pass


def _bitmaps(name):
    return [bm for _, bm, _ in cc.case(name)["run"]]


# ---- the two references agree ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_model_equals_oracle(name):
    c, m = cc.case(name), cc.model(name)
    for p in range(7):
        want = c["run"][p][2]
        assert m["streams"][p].size == want.size and np.array_equal(m["streams"][p], want), (name, cc.story(name, p, want))
    assert int((m["ordinal"] >= 0).sum()) == sum(s.size for s in m["streams"]) // 3
    assert np.array_equal(m["owner"], cc.census(name)["owner"]), name          # first toucher by sequence == minimum of the keys


@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_images_follow_the_stated_rule(name):
    c = cc.case(name)
    assert c["w"] % 8 == 0 and c["h"] % 8 == 0 and c["planes"].min() >= 0 and c["planes"].max() <= 255
    equal = total = 0
    for _, _, rgb in c["run"]:
        t = rgb.reshape(-1, 3)
        if len(t) > 1:
            equal += int((t[1:] == t[:-1]).all(axis=1).sum()); total += len(t) - 1
    assert equal * 50 <= total, (name, equal, total)                           # a colour at the wrong offset changes bytes


@pytest.mark.parametrize("name", cc.ALL_NAMES)
def test_colour_counts_are_what_the_decode_model_pops(name):
    c, m = cc.case(name), cc.model(name)
    chunks = [(sx, sy, bm, np.zeros(0, np.uint8)) for (sx, sy), bm in zip(PASSES, _bitmaps(name))]
    dec = gd.model_decode({"w": c["w"], "h": c["h"], "remap": 0, "chunks": chunks}, render=False)
    assert dec["consumed"] == [s.size for s in m["streams"]], name
    assert not dec["skipped"]


# ---- a. byte values ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", range(7))
def test_every_byte_value_of_every_pass(p):
    names = [n for n, a in cc.BYTES_CASES.items() if a[0] == p]
    values, combos, rel = set(), set(), set()
    for n in names:
        cs = cc.census(n)
        values |= cs["byte_values"][p]
        for r in cs["groups"][p]:
            combos |= r["combos"]; rel |= r["relations"]
        assert np.array_equal(cc.case(n)["run"][p][1], np.asarray(cc.BYTES_CASES[n][3], dtype=np.uint8)), (n, "the bitmap is not the one asked for")
    assert values == set(range(256)), (p, sorted(set(range(256)) - values))
    two_rows = (64 >> PASSES[p][0]) == 4
    if two_rows:
        assert p in (0, 1)
        # every relation alone, all four together, none; and the two places where the byte wraps: bit k - 1 at column 0, bit k - 3 at column 3
        assert {()} | {(n,) for n in cc.RELATIONS} | {cc.RELATIONS} <= combos, (p, combos)
        assert ("wrapLeft", 4, 0) in rel and ("wrapUpRight", 7, 3) in rel, (p, rel)
        assert {k for n, k, col in rel if n == "left"} == {1, 2, 3, 5, 6, 7} and {k for n, k, col in rel if n == "upRight"} == {4, 5, 6}
    else:
        assert combos == {(), ("left",)} and {k for n, k, col in rel if n == "left"} == set(range(1, 8)), (p, combos)
        assert not any(n.startswith("wrap") for n, _, _ in rel)                # a byte is one row of a block: column 0 is bit 0


# ---- b. ownership across passes and boundaries ---------------------------------------------------------------------------------------------------
MOSAICS = ("mosaic_256_a", "mosaic_256_b", "mosaic_256_c")
PAIR_CASES = MOSAICS + cc.ORIGIN_NAMES


def _q_first_possible(p, q, w=256, h=256):
    return next(cc.q_first_witnesses(p, q, w, h), None) is not None


def test_every_pair_of_passes_in_every_placement():
    pairs = set().union(*[cc.census(n)["pairs"] for n in PAIR_CASES])
    for n in MOSAICS:
        assert all(c > 0 for c in cc.census(n)["counts"]), (n, "a pass is empty")
    for p in range(7):
        for q in range(p + 1, 7):
            have = {where for a, b, where, _ in pairs if (a, b) == (p, q)}
            assert have == set(cc.PLACEMENTS), (p, q, "missing", set(cc.PLACEMENTS) - have)
            q_first = any(first for a, b, _, first in pairs if (a, b) == (p, q))
            assert q_first == _q_first_possible(p, q), (p, q, q_first)        # where the geometry allows it, the later pass's tile has the smaller index
    for n in MOSAICS:
        lost = [sum(r["lost_earlier"] for r in g) for g in cc.census(n)["groups"]]
        assert lost[0] == 0 and all(v > 0 for v in lost[1:]), (n, lost)


@pytest.mark.parametrize("name,p", [("full_p6_512x512", 6), ("full_p4_512x1024", 4)])
def test_neighbours_across_bytes_blocks_and_workgroups(name, p):
    cs = cc.census(name)
    within = {(where, sep) for a, b, where, sep in cs["pairs"] if a == b == p}
    for sep in ("byte", "block", "group"):
        assert {("above", sep), ("below", sep), ("diagonal", sep)} <= within, (name, sep, within)
    assert {("left", "block"), ("right", "block")} <= within                   # a byte is a whole row of its block: left and right leave the block
    g = cs["groups"][p]
    assert len(g) == 2 and all(r["lost_byte"] and r["lost_block"] for r in g) and g[1]["lost_far"] > 0 and g[0]["lost_group"] > 0, name
    assert g[1]["offset"] == 3 * g[0]["tot"]


# ---- c. runs -------------------------------------------------------------------------------------------------------------------------------------
def test_run_shapes():
    seen, empties = set(), 0
    for name, tots in cc.RUN_TOTS.items():
        g = cc.census(name)["groups"][6]
        assert tuple(r["tot"] for r in g) == tots, (name, [r["tot"] for r in g])
        for k, r in enumerate(g):
            assert r["offset"] == 3 * sum(tots[:k])
            seen.add((r["offset"] % 4, r["tot"]))
            empties += int(r["tot"] == 0 and 0 < k < len(g) - 1 and g[k - 1]["tot"] > 0 and g[k + 1]["tot"] > 0)
    assert empties == len(cc.RUN_TOTS)                                          # an empty workgroup between two others
    assert {(o, t) for o in range(4) for t in (1, 2, 3, 4)} <= seen, seen      # every run offset mod 4 with every length 1..4
    # what that means for the copy-out of a run that starts at byte `off` of an aligned stream: head bytes, whole words, tail bytes
    shapes = set()
    for off, tot in seen:
        n = 3 * tot
        head = min(n, (4 - off) & 3)
        shapes.add((off, head, (n - head) >> 2, (n - head) & 3))
    for off in range(4):
        mine = {s for s in shapes if s[0] == off}
        assert {s[3] for s in mine} >= {1, 2, 3}, (off, mine)                   # tails of 1, 2 and 3 bytes
        assert any(s[2] == 1 for s in mine), (off, mine)                        # exactly one whole word
    assert (1, 3, 0, 0) in shapes and (2, 2, 1, 0) in shapes                    # a run that ends with its head; head + exactly one word
    assert {0, 1, 2} <= {t for _, t in seen}


def test_both_sides_of_the_lds_cap():
    # the cases are built around the kernel's constant: a change of kCap, or of which side 8192 itself falls on, is noticed here (both paths write
    # the same bytes, so no comparison of outputs can notice the latter)
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "yaik_amd", "csrc", "yk_corners.hip")).read()
    assert [int(v) for v in re.findall(r"constexpr uint32_t kCap = (\d+);", src)] == [cc.KCAP]
    assert len(re.findall(r"const bool viaLds = tot <= kCap;", src)) == 1
    assert cc.KCAP == 8192
    q, c1, c2 = cc.census("quarter_512x256"), cc.census("checker_512x256"), cc.census("checker_512x512")
    assert q["counts"] == [0] * 6 + [2048] and [r["tot"] for r in q["groups"][6]] == [8192] and cc.case("quarter_512x256")["run"][6][2].size == 24576
    assert c1["counts"] == [0] * 6 + [4096] and [r["tot"] for r in c1["groups"][6]] == [8383] and cc.case("checker_512x256")["run"][6][2].size == 25149
    g = c2["groups"][6]
    assert [r["tot"] for r in g] == [8383, 8256] and g[1]["offset"] == 25149 and min(r["tot"] for r in g) > cc.KCAP
    assert [r["tot"] for r in cc.census("full_p6_512x512")["groups"][6]] == [8385, 8256]


# ---- d. edges --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mosaic_200x136", "clean_200x136", "mosaic_72x40", "small_72x40"])
def test_edges_and_odd_sizes(name):
    c, m, cs = cc.case(name), cc.model(name), cc.census(name)
    w, h = c["w"], c["h"]
    assert w % 16 == 8 and h % 16 == 8 and w % 64 and h % 64
    assert sum(r["clamped"] for g in cs["groups"] for r in g) > 0
    own = m["owner"] != cc.NONE
    assert own[:, -1].sum() > 2 and own[-1, :].sum() > 2, (name, "the last lattice column and row are owned")
    # a clamped read differs from the cell origin it would be confused with
    for ly, lx in np.argwhere(own):
        if 4 * ly == h or 4 * lx == w:
            assert cc._colour(c["planes"], w, h, ly, lx, None) != cc._colour(c["planes"], w, h, ly, lx, "no_clamp"), (name, lx, ly)
    for p, (sx, sy) in enumerate(PASSES):                                      # the last swizzle block is partial; bits outside the image are never set
        g = gd.geo(sx, sy, w, h)
        assert g["xbb"] * g["big_x"] > w and g["ybb"] * g["big_y"] > h
        for bit, tx, ty in gd.set_tiles(sx, sy, w, c["run"][p][1]):
            assert ((tx + 1) << sx) <= w and ((ty + 1) << sy) <= h


def test_image_corners_empty_image_and_the_half_word():
    for name in ("clean_200x136", "mosaic_72x40", "p0_64x64"):
        assert all(k != cc.NONE for k in cc.census(name)["corner_points"]), name
    for name in ("plugged_72x40", "plugged_200x136", "plugged_512x256"):
        c = cc.case(name)
        assert all(cnt == 0 and not bm.any() and rgb.size == 0 for cnt, bm, rgb in c["run"]), name
    c = cc.case("p0_64x64")
    assert c["run"][0][1].size == 2 and c["run"][0][0] == 16 and c["run"][0][2].size == 75        # half of the pass's only bitmap word is padding
    c = cc.case("p0_192x64")
    assert c["run"][0][1].size == 6 and 0 < c["run"][0][0] < 48 and c["run"][0][1][4:].any()      # one and a half words


# ---- e. batches ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bname", sorted(cc.BATCHES))
def test_batch_triples(bname):
    cases = [cc.case(n) for n in cc.BATCHES[bname]]
    assert len({c["planes"].shape for c in cases}) == 1
    dense, empty, sparse = (sum(rgb.size for _, _, rgb in c["run"]) for c in cases)
    assert empty == 0 and 0 < sparse < dense, (bname, dense, empty, sparse)
    for a in range(3):
        for b in range(a + 1, 3):
            assert any(not np.array_equal(x[1], y[1]) for x, y in zip(cases[a]["run"], cases[b]["run"]))
    assert cc.BATCHES["b512x256"][0] == "checker_512x256"                      # the direct-store path in the batch kernel
    assert [cc.case(n)["planes"].shape for n in cc.STALE] == [(3, 256, 512)] * 3


# ---- every defect is seen ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("defect", cc.DEFECTS)
def test_defect_is_seen(defect):
    name = CAUGHT_BY[defect]
    c = cc.case(name)
    bad = cc.model_streams(_bitmaps(name), c["planes"], c["w"], c["h"], defect)
    differ = [p for p in range(7) if not np.array_equal(bad["streams"][p], c["run"][p][2])]
    print(f"defect {defect}: seen by case {name}, passes {differ}")
    assert differ, (defect, name)


def test_defect_table_is_complete():
    assert set(CAUGHT_BY) == set(cc.DEFECTS) and set(CAUGHT_BY.values()) <= set(cc.ALL_NAMES)
