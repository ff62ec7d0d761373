"""CPU side of the window decode's test cases (tests/window_cases.py): the images and windows are valid, the windows of the "mixed" images meet
the condition that makes a wrong stream offset visible (tiles with all, no and some quadrants marked inside the window and before it), the window
across the 1-D scan-block boundary really crosses it, and the expected pixels are the crop of the oracle's whole decode."""
import numpy as np
import pytest

from tests import window_cases as WC


def test_cases_and_windows_are_the_named_ones():
    assert WC.CASES == [(136, 264, "mixed"), (520, 264, "mixed"), (264, 136, "photo"), (8, 8, "smooth")]
    for w, h, _ in WC.CASES:
        wins = WC.windows(w, h)
        assert len(set(wins)) == len(wins)
        assert (0, 0, w, h) in wins and (0, 0, 8, 8) in wins and (w - 8, h - 8, 8, 8) in wins
        for x0, y0, ww, wh in wins:
            assert not (x0 | y0 | ww | wh) & 7 and ww >= 8 and wh >= 8 and x0 >= 0 and y0 >= 0 and x0 + ww <= w and y0 + wh <= h
        if (w, h) != (8, 8):
            assert any(ww == w and wh == 8 for _, _, ww, wh in wins) and any(ww == 8 and wh == h for _, _, ww, wh in wins)
            # a window with tiles of four different 64-blocks
            assert any(x0 // 64 != (x0 + ww - 1) // 64 and y0 // 64 != (y0 + wh - 1) // 64 and ww <= 24 and wh <= 24 for x0, y0, ww, wh in wins)
    assert WC.windows(8, 8) == [(0, 0, 8, 8)]
    assert WC.SCAN_BLOCK_WINDOW in WC.windows(520, 264)


def test_scan_block_window_spans_the_1024_tile_boundary():
    w, h = 520, 264
    x0, y0, ww, wh = WC.SCAN_BLOCK_WINDOW
    tiles_w = w // 8
    assert tiles_w * (h // 8) == 2145                                       # three scan blocks of 1024 tiles
    rows = {ty: ((ty * tiles_w + x0 // 8), (ty * tiles_w + (x0 + ww) // 8 - 1)) for ty in range(y0 // 8, (y0 + wh) // 8)}
    assert rows[15] == (999, 1022)
    assert all(last < 1024 for ty, (_, last) in rows.items() if ty <= 15) and all(first >= 1024 for ty, (first, _) in rows.items() if ty >= 16)
    assert sorted(rows) == [14, 15, 16, 17, 18]
    # a round of 64 window tiles (24 per row) therefore holds tiles of both blocks: what the whole-image kernel's scalar base loads cannot serve
    assert ww // 8 == 24 and 64 > 2 * 24


@pytest.mark.parametrize("w,h,kind", [c for c in WC.CASES if c[2] == "mixed"])
def test_windows_of_mixed_images_meet_the_condition(oracle_built, w, h, kind):
    ref = WC.reference(w, h, kind)
    kinds = WC.tile_kinds(ref.tile4, w, h)
    assert kinds.shape == (h // 8, w // 8)
    checked = 0
    for win in WC.windows(w, h):
        assert WC.condition_failures(kinds, win) == [], (win,)
        checked += win[2] * win[3] > 64
    assert checked >= 4
    # the condition itself: a window of unmarked tiles only is reported, so is one whose predecessors are all of one kind
    assert WC.condition_failures(np.zeros_like(kinds), (8, 8, 16, 16))
    one = np.zeros_like(kinds); one[1:3, 1:3] = [[4, 0], [2, 0]]
    assert WC.condition_failures(one, (8, 8, 16, 16)) == ["no tile with all quadrants marked before the window", "no tile with partly quadrants marked before the window"]
    assert WC.condition_failures(one, (0, 0, 24, 24)) == []


@pytest.mark.parametrize("w,h,kind", WC.CASES)
def test_expected_pixels_are_the_crop_of_the_oracles_whole_decode(oracle_built, w, h, kind):
    from oracle.pyoracle import image_builder
    ref = WC.reference(w, h, kind)
    whole = image_builder(ref.planes, w, h, w * 3).reshape(h, w, 3)
    assert np.array_equal(whole, ref.rgb)
    for win in WC.windows(w, h):
        x0, y0, ww, wh = win
        crop = ref.crop(win)
        assert crop.shape == (wh, ww, 3) and np.array_equal(crop, whole[y0:y0 + wh, x0:x0 + ww])
    # the second image of the work-is-skipped test differs from the first in every 64-block, so a block that was not rendered shows
    if (w, h) == (520, 264):
        other = WC.reference(w, h, kind, second=True)
        a, b = WC.tiles_of(ref.planes, w, h), WC.tiles_of(other.planes, w, h)
        diff = (a != b).any(axis=(0, 3))
        assert all(diff[by:by + 8, bx:bx + 8].any() for by in range(0, h // 8, 8) for bx in range(0, w // 8, 8))


def test_outside_rounded_is_the_complement_of_the_window_in_whole_blocks():
    out = WC.outside_rounded(520, 264, (192, 112, 192, 40))
    assert out.shape == (33, 65)
    assert not out[8:24, 24:48].any() and out[:8].all() and out[24:].all() and out[:, :24].all() and out[:, 48:].all()
    assert not WC.outside_rounded(520, 264, (0, 0, 520, 264)).any()
    edge = WC.outside_rounded(520, 264, (512, 256, 8, 8))                  # clipped to the image: the partial last blocks
    assert not edge[32:, 64:].any() and edge.sum() == 33 * 65 - 1
