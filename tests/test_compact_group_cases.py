"""The directed inputs for the grouped compact sweep (tests/compact_group_cases.py) hold what they claim, shown from the oracle and the numpy
model of the six variants alone: no GPU.  tests/test_gpu_compact_groups.py rests on this file."""
import re

import numpy as np
import pytest

from tests import compact_group_cases as q
from tests import gradfit_cases as gc


@pytest.fixture(scope="module")
def cases(oracle_built):
    return {n: q.case(n) for n in q.NAMES}


def _strips(cases):
    return [(c, col, s) for c in cases.values() for col, s in c["strips"]]


def test_every_strip_holds_its_counts_and_tiles(cases):
    """own = the cells of the first pass's viable tiles (a compact pass); spec = the cells of the second pass's tiles under the coverage BEFORE
    the first; the oracle accepts exactly the tiles the strip names, in both passes; model and oracle agree on every viable tile"""
    for c, col, s in _strips(cases):
        cs = c["census"]
        pa, pb = q.PAIRS[s.k]
        assert cs["stray"] == [] and not [k for k, r in cs["tiles"].items() if bool(r["survivors"]) != r["accepted"]], s.name
        assert cs["paths"].get((pa, 0, col)) == ("compact", s.own), (s.name, cs["paths"].get((pa, 0, col)))
        assert q.spec_cells(c, pa, col, pa) == s.own and q.spec_cells(c, pb, col, pa) == s.spec, (s.name, q.spec_cells(c, pb, col, pa))
        assert s.spec >= 1 and c["rf"] == s.rf
        assert q.accepted(c, pa, col) == s.accept_a, (s.name, "first pass", q.accepted(c, pa, col))
        assert q.accepted(c, pb, col) == s.accept_b, (s.name, "second pass", q.accepted(c, pb, col))
        # what the second pass really finds is never more than the speculative count, and less exactly when the first pass covered an origin
        real = cs["paths"].get((pb, 0, col), ("", 0))[1]
        assert real <= s.spec and (real < s.spec) == bool(s.accept_a and q.spec_cells(c, pb, col, pb) < s.spec), s.name


def test_counts_on_both_sides_of_the_fit(cases):
    """the count strips: all plugs (nothing accepted), every listed (own, spec) of every pair, sums of 16 and of 17 / 18"""
    seen = {k: set() for k in range(3)}
    for c, col, s in _strips(cases):
        if s.name.startswith("count") and c["rf"] == 3:
            assert not s.accept_a and not s.accept_b
            seen[s.k].add((s.own, s.spec))
    assert q.GROUP_MAX_CELLS == 16 == gc.COMPACT_MAX_CELLS
    for k in range(3):
        assert seen[k] == set(q.COUNTS[k])
        sums = {a + b for a, b in seen[k]}
        assert 16 in sums and min(x for x in sums if x > 16) <= 18, (k, sums)
    assert {(8, 8), (4, 12)} <= seen[0] and {(8, 8), (4, 12), (12, 4), (14, 2), (2, 14)} <= seen[1] and {(8, 8), (8, 9), (4, 12), (2, 14), (2, 15)} <= seen[2]
    # why the other counts of the list do not exist: a first-pass tile of 8x8 (4x8) is two whole tiles of 8x4 (4x4)
    for k in (0, 2):
        (ax, ay), (bx, by) = q._cells(q.PAIRS[k][0]), q._cells(q.PAIRS[k][1])
        assert ax % bx == 0 and ay % by == 0


def test_scenarios(cases):
    have = set()
    for c, col, s in _strips(cases):
        cs = c["census"]
        pa, pb = q.PAIRS[s.k]
        (ax, ay), (bx, by) = q._cells(pa), q._cells(pb)
        fits = s.own + s.spec <= q.GROUP_MAX_CELLS
        kind = re.match("[a-zA-Z]+", s.name).group(0)
        if s.more.get("stage") == "A1":          # the first pass loses ALL its tiles in stage 1, a tile of the second is only decided in stage 2 (accepted)
            assert fits and not s.accept_a and s.accept_b
            for (p, ty, tx), r in cs["tiles"].items():
                if p == pa and ty * ay < 4 and tx * ax // 16 == col:
                    assert q.stage1_lost(c, pa, ty * ay, tx * ax), s.name
            assert all(not q.stage1_lost(c, pb, cy, 16 * col + cx) for cy, cx in s.accept_b)
        if s.more.get("stage") == "B1":          # the reverse
            assert fits and s.accept_a and not s.accept_b
            for (p, ty, tx), r in cs["tiles"].items():
                if p == pb and ty * by < 4 and tx * bx // 16 == col:
                    assert q.stage1_lost(c, pb, ty * by, tx * bx), s.name
            assert all(not q.stage1_lost(c, pa, cy, 16 * col + cx) for cy, cx in s.accept_a)
        for cy, cx in s.more.get("covered_b", ()):   # a second-pass tile the model accepts, under an accepted first-pass tile: not in the bitmap
            assert fits
            TX, TY = gc.SHAPES[pb]
            x, y = 4 * (16 * col + cx), 4 * cy
            ok = gc.variants(c["planes"][:, y: y + TY, x: x + TX], gc.tile_corners(c["planes"], x, y, TX, TY), TX, TY, c["rf"])
            assert any(v[0] for v in ok.values()), (s.name, "would not be accepted anyway")
            assert (cy, cx) not in q.accepted(c, pb, col) and q.covered_before(c, pb)[cy, 16 * col + cx] and not q.covered_before(c, pa)[cy, 16 * col + cx]
        if "overlap" in s.more:                   # accepted tiles of the two passes share a cell, the second one's origin is free
            assert fits
            (acy, acx), (bcy, bcx) = s.more["overlap"]
            A = {(acy + j, acx + i) for j in range(ay) for i in range(ax)}
            B = {(bcy + j, bcx + i) for j in range(by) for i in range(bx)}
            assert A & B and (bcy, bcx) not in A and (acy, acx) in s.accept_a and (bcy, bcx) in s.accept_b
        for cy, cx in s.more.get("shared", ()):   # one origin lane, a viable tile in each pass, different fates
            assert fits
            ra, rb = cs["tiles"][(pa, cy // ay, (16 * col + cx) // ax)], cs["tiles"][(pb, cy // by, (16 * col + cx) // bx)]
            assert cy % ay == 0 and cx % ax == 0 and not ra["accepted"] and rb["accepted"] and ra["survivors"] != rb["survivors"]
        if s.more.get("edge"):
            w = c["planes"].shape[2]
            assert fits and w % 16 == 8 and w in (72, 136) and col == w // 64
            (cy, cx), = s.accept_a
            assert 4 * (16 * col + cx + ax) == w                          # the accepted tile ends on the image's edge: its far corners are clamped reads
        have.add((s.k, kind, c["rf"], fits))
    for k in range(3):
        for kind in ("onlyA", "onlyB", "both", "covers", "shared"):
            assert (k, kind, 3, True) in have, (k, kind)
        assert any(h[0] == k and h[2] == 0 for h in have) and any(h[0] == k and h[2] == 64 for h in have)
    assert (1, "overlap", 3, True) in have and (1, "edge", 3, True) in have
    assert {c["planes"].shape[2] for c, _, s in _strips(cases) if s.more.get("edge")} == {72, 136}


def test_batches(cases):
    for names in q.BATCHES:
        frames = [q.case(n) for n in names]
        assert len({f["planes"].shape for f in frames}) == 1 and len({f["planes"].tobytes() for f in frames}) == 3
