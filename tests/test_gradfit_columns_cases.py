"""The column-by-column gradient-fit inputs (tests/gradfit_columns_cases.py) are what they claim to be, shown from the reference alone: no GPU.

tests/test_gpu_gradfit_columns.py rests on this file, as tests/test_gpu_gradfit_directed.py rests on tests/test_gradfit_cases.py: the oracle's
accept / reject decisions and the numpy model of the six tests say that in every case the named variant is the tile's sole survivor, or that
the named pixel is the only one at which it fails.  A failure here is a fault of the generator, not of a kernel."""
from collections import Counter

import numpy as np
import pytest

from tests import gradfit_cases as gc
from tests import gradfit_columns_cases as kc

V, SHAPES = gc.VARIANTS, gc.SHAPES


@pytest.fixture(scope="module")
def cases(oracle_built):
    return {n: kc.case(n) for n in kc.ALL_NAMES}


def test_every_request_is_held_or_listed(cases):
    """the requests are the full product; what no image holds is listed by name, and that is pixel (0, 0) of the tile, the corner TL, only"""
    reqs, corner = kc.all_requests()
    combos = sum(len(gc.paths_of(p)) for p in range(7)) * len(kc.KINDS)
    # 15 (shape, path): 13 with a first and a last cell, the two of 4x4 with one cell; x 3 kinds x 16 pixels x 2 signs x 2 outcomes
    assert combos == 45 and len(reqs) + len(corner) == (13 * 2 + 2 * 1) * 3 * 16 * 2 * 2
    held = Counter(t["request"] for c in cases.values() for t in c["targets"] if t["group"] == "K")
    assert set(held) == {r[0] for r in reqs} and set(held.values()) == {1}
    assert set(kc.UNREALISED) == set(corner) == set(kc.CORNER_REQUESTS), sorted(set(kc.UNREALISED) - set(corner))
    assert all("/first-cell/col0/row0/" in n for n in kc.UNREALISED) and len(corner) == 45 * 4
    assert not set(held) & set(kc.UNREALISED)


def test_requests_cover_every_position(cases):
    """per (shape, path, kind) and outcome: every (cell, column, row, sign) but the corner; the kinds sit in the streams they name"""
    got = Counter()
    for c in cases.values():
        for t in c["targets"]:
            if t["group"] != "K":
                continue
            TX, TY = SHAPES[t["p"]]
            ch, dx, dy, sign = t["decide"]
            assert (t["kind"] == "A") == (t["variant"] < 4) and (t["kind"] == "A" or (ch == 2) == (t["kind"] == "P4"))
            first, last = (dx < 4 and dy < 4), (dx >= TX - 4 and dy >= TY - 4)
            assert first or last
            for cell in (["first"] if first else []) + (["last"] if last else []):
                got[(t["p"], t["path"], t["kind"], t["expect"], cell, dx % 4, dy % 4, sign)] += 1
    for p in range(7):
        for path in gc.paths_of(p):
            for kind in kc.KINDS:
                for e in ("sole", "reject"):
                    for cell in ("first", "last"):
                        for col in range(4):
                            for row in range(4):
                                for sign in (1, -1):
                                    if (col, row) == (0, 0) and (cell == "first" or SHAPES[p] == (4, 4)):   # the corner TL (4x4: its one cell)
                                        continue
                                    assert got[(p, path, kind, e, cell, col, row, sign)] >= 1, (SHAPES[p], path, kind, e, cell, col, row, sign)


@pytest.mark.parametrize("name", kc.ALL_NAMES)
def test_model_agrees_with_the_oracle(cases, name):
    cs = cases[name]["census"]
    assert cs["stray"] == []
    bad = [(k, r["survivors"], r["accepted"]) for k, r in cs["tiles"].items() if bool(r["survivors"]) != r["accepted"]]
    assert not bad, bad[:4]
    assert len(cs["tiles"]) > 0 and cases[name]["planes"].min() >= 0 and cases[name]["planes"].max() <= 255


@pytest.mark.parametrize("name", kc.ALL_NAMES)
def test_targets_hold_what_they_claim(cases, name):
    """the target is viable in its pass on the path it names; at rf the named variant is its sole survivor and the oracle accepts it; at rf + 1
    no variant survives, the oracle rejects it, the named pixel is the only one at which the named variant fails, and one step back it survives"""
    c = cases[name]
    cs, rf = c["census"], c["rf"]
    assert c["targets"]
    for t in c["targets"]:
        key = gc.target_tile(t)
        what = (name, t["request"])
        TX, TY = SHAPES[t["p"]]
        x, y = 4 * t["cx"], 4 * t["cy"]
        assert key in cs["tiles"], what + ("not viable in its pass",)
        rec = cs["tiles"][key]
        assert rec["path"] == t["path"], what + (rec["path"],)
        cur = c["planes"][:, y: y + TY, x: x + TX].astype(np.int64)
        corners = gc.tile_corners(c["planes"], x, y, TX, TY)
        ch, dx, dy, sign = t["decide"]
        ok, first, nf = gc._variants_many(cur[None], corners[None], TX, TY, rf)
        off = int(cur[ch, dy, dx] - gc._blends(corners[None], TX, TY)[0][t["variant"], ch, dy, dx])
        if t["expect"] == "sole":
            assert rec["survivors"] == (V[t["variant"]],) and rec["accepted"], what + (rec["survivors"],)
            assert off == sign * rf, what
        else:
            assert rec["survivors"] == () and not rec["accepted"], what + (rec["survivors"],)
            assert off == sign * (rf + 1) and nf[0, t["variant"]] == 1 and first[0, t["variant"]] == (dy * TX + dx) * 3 + ch, what
            cur[ch, dy, dx] -= sign
            assert gc._variants_many(cur[None], corners[None], TX, TY, rf)[0][0].tolist() == [i == t["variant"] for i in range(6)], what


def test_width_72(cases):
    """8x8 targets in the last tile column inside a 72-wide image: right corners clamped to column 71 (TR is the tile's own pixel), stream 4
    deciding in columns 1 and 2 of the last cell column, accepted and rejected"""
    c = cases["kw72"]
    assert c["planes"].shape == (3,) + kc.W72[::-1] and kc.W72[0] == 72
    seen = set()
    for t in c["targets"]:
        ch, dx, dy, sign = t["decide"]
        x, y = 4 * t["cx"], 4 * t["cy"]
        assert t["p"] == 3 and x == 64 and x + 8 == 72 and ch == 2 and t["variant"] >= 4 and 4 <= dx < 8
        corners = gc.tile_corners(c["planes"], x, y, 8, 8)
        assert np.array_equal(corners[1], c["planes"][:, y, 71]) and np.array_equal(corners[3], c["planes"][:, y + 8, 71])
        seen.add((dx % 4, t["expect"]))
    assert seen == {(1, "sole"), (1, "reject"), (2, "sole"), (2, "reject")}


def test_batches_hold_three_different_frames_of_one_shape(cases):
    used = set()
    for names in kc.BATCHES:
        frames = [kc.case(n) for n in names]
        assert len(names) == 3 and len({f["planes"].shape for f in frames}) == 1 and len({f["rf"] for f in frames}) == 1
        assert len({f["planes"].tobytes() for f in frames}) == 3
        used |= set(names)
    assert used >= set(kc.ALL_NAMES)
