"""CPU side of the batch-window decode's test cases (tests/batch_window_cases.py): the batches and window sets are the named ones, the origins of
a set differ pairwise across the frames, every window of every frame meets the condition of window_cases.condition_failures on the oracle -- on
the frame's own image and on the second batch's that the not-written test decodes under the same windows -- the scan-block set really crosses the
1024-tile boundary, and the empty frames are empty."""
import numpy as np
import pytest

from tests import batch_window_cases as BC
from tests import window_cases as WC


def test_batches_and_sets_are_the_named_ones():
    assert BC.BATCHES == [(520, 264, "mixed", 4), (136, 264, "mixed", 3), (8, 8, "smooth", 2)]
    for w, h, _, n in BC.BATCHES:
        sets = {name: (size, origins) for name, size, origins in BC.window_sets(w, h)}
        assert sets["whole"] == ((w, h), [(0, 0)] * n)
        if (w, h) == (8, 8):
            assert list(sets) == ["whole"]                                   # one tile: the whole image is the only window
            continue
        assert set(sets) == {"whole", "tile", "row", "column", "four_blocks"} | ({"scan_block"} if (w, h) == (520, 264) else set())
        assert sets["tile"][0] == (8, 8) and sets["row"][0] == (w, 8) and sets["column"][0] == (8, h)
        assert len({y for _, y in sets["row"][1]}) == n and len({x for x, _ in sets["column"][1]}) == n
        (ww, wh), origins = sets["four_blocks"]
        assert all(x0 // 64 != (x0 + ww - 1) // 64 and y0 // 64 != (y0 + wh - 1) // 64 for x0, y0 in origins)
        for name, ((ww, wh), origins) in sets.items():
            assert len(origins) == n
            for x0, y0 in origins:
                assert not (x0 | y0 | ww | wh) & 7 and ww >= 8 and wh >= 8 and x0 >= 0 and y0 >= 0 and x0 + ww <= w and y0 + wh <= h, (name, x0, y0)


@pytest.mark.parametrize("w,h,kind,n,name,size,origins", BC.all_batch_sets(), ids=lambda v: str(v) if isinstance(v, (str, int)) else "")
def test_origins_of_a_set_differ_pairwise(w, h, kind, n, name, size, origins):
    if name in BC.SAME_ORIGIN:
        assert size == (w, h) and set(origins) == {(0, 0)}                  # the whole image has one origin
    else:
        assert len(set(origins)) == n


def test_scan_block_set_spans_the_1024_tile_boundary():
    w, h = 520, 264
    (ww, wh), origins = BC.WINDOW_SETS[(w, h)]["scan_block"]
    assert (origins[0] + (ww, wh)) == WC.SCAN_BLOCK_WINDOW
    tiles_w = w // 8
    for x0, y0 in origins:
        rows = [(ty * tiles_w + x0 // 8, ty * tiles_w + (x0 + ww) // 8 - 1) for ty in range(y0 // 8, (y0 + wh) // 8)]
        assert rows[0][0] < 1024 <= rows[-1][1]                              # tiles of scan block 0 and of scan block 1
    # ... and in frame 1 a tile row of the window itself crosses it
    x0, y0 = origins[1]
    assert any(ty * tiles_w + x0 // 8 < 1024 <= ty * tiles_w + (x0 + ww) // 8 - 1 for ty in range(y0 // 8, (y0 + wh) // 8))


@pytest.mark.parametrize("w,h,kind,n", [b for b in BC.BATCHES if b[2] == "mixed"])
def test_every_window_of_every_frame_meets_the_condition(oracle_built, w, h, kind, n):
    checked = 0
    for second in (False, True):
        refs = BC.batch_references(w, h, kind, n, second)
        for name, size, origins in BC.window_sets(w, h):
            for f, (x0, y0) in enumerate(origins):
                kinds = WC.tile_kinds(refs[f].tile4, w, h)
                assert WC.condition_failures(kinds, (x0, y0) + size) == [], (name, f, second)
                checked += size[0] * size[1] > 64
    assert checked >= 2 * n * 4


@pytest.mark.parametrize("w,h,kind,n", BC.BATCHES)
def test_frames_differ_and_the_second_batch_differs_in_every_block(oracle_built, w, h, kind, n):
    a, b = BC.batch_references(w, h, kind, n), BC.batch_references(w, h, kind, n, second=True)
    for f in range(n):
        assert a[f].rgb.shape == (h, w, 3)
        for g in range(f):
            assert not np.array_equal(a[f].rgb, a[g].rgb)                    # a frame decoded from another frame's streams shows
        ta, tb = WC.tiles_of(a[f].planes, w, h), WC.tiles_of(b[f].planes, w, h)
        diff = (ta != tb).any(axis=(0, 3))
        assert all(diff[by:by + 8, bx:bx + 8].any() for by in range(0, h // 8, 8) for bx in range(0, w // 8, 8)), f
    name, size, origins = BC.window_sets(w, h)[-1]
    assert BC.crops(a, size, origins).shape == (n, size[1], size[0], 3)


def test_empty_frames_are_empty_on_the_oracle(oracle_built):
    w, h, frames = BC.EMPTY_BATCH
    size, origins = BC.EMPTY_WINDOWS
    assert len(origins) == len(frames) == len(set(origins))
    for (kind, f), (x0, y0) in zip(frames, origins):
        ref = BC.reference(w, h, kind, f)
        counts = [cnt for _, _, cnt, _, _ in ref.passes]
        if kind == "noise":
            assert not any(counts) and ref.typ.size and ref.pix.size        # no gradient tile: every tile is the 1-D chunk's
        elif kind == "flat":
            assert any(counts) and ref.typ.size == 0 and ref.pix.size == 0  # no 1-D bytes: gradient tiles cover the image
        else:
            assert any(counts) and ref.typ.size
            assert WC.condition_failures(WC.tile_kinds(ref.tile4, w, h), (x0, y0) + size) == []
        assert x0 + size[0] <= w and y0 + size[1] <= h
