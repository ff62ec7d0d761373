"""CPU side of the pixel-window decode's test cases (tests/window_px_cases.py): the windows are what the module claims -- inside the image, unique,
every residue of origin and size modulo 8 covered, the named covers equal to the named windows of tests/window_cases.py -- the origin sets of the
multi-window and batch calls hold the origins they are meant to hold, and the expected pixels are the crop of the oracle's whole decode."""
import numpy as np
import pytest

from tests import batch_window_cases as BW
from tests import window_cases as WC
from tests import window_px_cases as PX


def test_windows_are_the_named_ones():
    for w, h, _ in WC.CASES:
        wins = PX.windows(w, h)
        assert len(set(wins)) == len(wins)
        for x0, y0, ww, wh in wins:
            assert x0 >= 0 and y0 >= 0 and ww >= 1 and wh >= 1 and x0 + ww <= w and y0 + wh <= h, (w, h, x0, y0, ww, wh)
        assert (0, 0, w, h) in wins and (1, 1, w - 2, h - 2) in wins and (0, 0, 1, 1) in wins and (w - 1, h - 1, 1, 1) in wins and (3, 5, 1, 1) in wins
        if (w, h) == (8, 8):
            assert wins == [(0, 0, 8, 8), (1, 1, 6, 6), (0, 0, 1, 1), (7, 7, 1, 1), (3, 5, 1, 1), (5, 0, 1, 8), (0, 6, 8, 1)]
            continue
        for named in ((7, 7, 2, 2), (9, 10, 5, 4), (w - 3, 0, 1, h), (0, h - 2, w, 1), (w - 13, h - 11, 13, 11), (61, 59, 7, 9)):
            assert named in wins, (w, h, named)
        # every residue of x0, y0, ww and wh modulo 8
        res = [win for win in wins if win in PX.RESIDUES]
        assert len(res) == 8
        for k in range(4):
            assert {win[k] & 7 for win in res} == set(range(8)), k
        # (61, 59, 7, 9) has pixels of four 64-blocks; (7, 7, 2, 2) of four tiles; (9, 10, 5, 4) lies inside one tile
        assert 61 // 64 != 67 // 64 and 59 // 64 != 67 // 64 and (9 // 8, 10 // 8) == (13 // 8, 13 // 8)


def test_named_covers_are_the_named_aligned_windows():
    assert PX.cover(PX.SCAN_BLOCK_PX) == WC.SCAN_BLOCK_WINDOW and PX.SCAN_BLOCK_PX in PX.windows(520, 264)
    mixed = [(w, h) for w, h, kind in WC.CASES if kind == "mixed"]
    assert sorted(PX.STRADDLE_PX) == sorted(mixed) == sorted(WC.STRADDLE)
    for shape in mixed:
        assert PX.cover(PX.STRADDLE_PX[shape]) == WC.STRADDLE[shape] and PX.STRADDLE_PX[shape] in PX.windows(*shape)
    # the cover is minimal and 8-aligned; the shared cover has one size for every origin, contains the window and stays inside the image
    for w, h, _ in WC.CASES:
        for win in PX.windows(w, h):
            x0, y0, ww, wh = win
            cx, cy, cw, ch = PX.cover(win)
            assert not (cx | cy | cw | ch) & 7 and 0 <= x0 - cx < 8 and 0 <= y0 - cy < 8 and 0 <= cx + cw - x0 - ww < 8 and 0 <= cy + ch - y0 - wh < 8
            assert cx + cw <= w and cy + ch <= h
            sx, sy, sw, sh = PX.shared_cover(win, w, h)
            assert not (sx | sy | sw | sh) & 7 and 0 <= sx <= x0 and 0 <= sy <= y0 and x0 + ww <= sx + sw <= w and y0 + wh <= sy + sh <= h
            assert (sw, sh) == PX.shared_cover((0, 0, ww, wh), w, h)[2:] and sw - ww < 16 and sh - wh < 16


@pytest.mark.parametrize("w,h", [(w, h) for w, h, _ in WC.CASES] + [(w, h) for w, h, _, _ in BW.BATCHES])
def test_origin_sets_hold_the_named_origins(w, h):
    sets = PX.origin_sets(w, h)
    sizes = [s for s, _ in sets]
    assert (w, h) in sizes and (1, 1) in sizes
    if (w, h) != (8, 8):
        assert sizes == [(13, 11), (100, 37), (1, 1), (w, h)]
    for (ww, wh), origins in sets:
        assert len(set(origins)) == len(origins)
        assert all(PX.inside((x0, y0, ww, wh), w, h) for x0, y0 in origins)
        assert (0, 0) in origins and (w - ww, h - wh) in origins
        if (ww, wh) in ((13, 11), (100, 37)):
            # at the far corner the shared cover is pulled back: the window starts more than 7 pixels into it
            sx, sy, _, _ = PX.shared_cover((w - ww, h - wh, ww, wh), w, h)
            assert w - ww - sx > 7 and h - wh - sy > 7
            # two origins overlap, and the residues are mixed
            assert any(abs(a[0] - b[0]) < ww and abs(a[1] - b[1]) < wh for i, a in enumerate(origins) for b in origins[i + 1:])
            assert len({x0 & 7 for x0, _ in origins}) >= 4 and len({y0 & 7 for _, y0 in origins}) >= 4
    for n in (2, 3, 4):
        for (ww, wh), origins in PX.origin_sets(w, h, n):
            assert len(origins) == n
            if (ww, wh) != (w, h):
                assert len(set(origins)) == n and (0, 0) in origins and (w - ww, h - wh) in origins


def test_touched_blocks_counts_each_block_once():
    assert PX.touched_blocks(520, 264, [(0, 0)], 1, 1) == 1
    assert PX.touched_blocks(520, 264, [(61, 59)], 7, 9) == 4
    assert PX.touched_blocks(520, 264, [(61, 59), (63, 63)], 7, 9) == 4
    assert PX.touched_blocks(520, 264, [(0, 0)], 520, 264) == 45
    assert PX.touched_blocks(520, 264, [(64, 64)], 64, 64) == 1 and PX.touched_blocks(520, 264, [(64, 64)], 65, 64) == 2


@pytest.mark.parametrize("w,h,kind", WC.CASES)
def test_expected_pixels_are_the_crop_of_the_oracles_whole_decode(oracle_built, w, h, kind):
    from oracle.pyoracle import image_builder
    ref = WC.reference(w, h, kind)
    whole = image_builder(ref.planes, w, h, w * 3).reshape(h, w, 3)
    assert np.array_equal(whole, ref.rgb)
    for win in PX.windows(w, h):
        x0, y0, ww, wh = win
        crop = ref.crop(win)
        assert crop.shape == (wh, ww, 3) and np.array_equal(crop, whole[y0:y0 + wh, x0:x0 + ww])
        # an off-by-one clip shows: the crop differs from its neighbours one pixel to either side (where they exist and the window is not a constant)
        if ww > 8 and wh > 8 and x0 + ww < w and y0 + wh < h:
            assert not np.array_equal(crop, whole[y0 + 1:y0 + 1 + wh, x0 + 1:x0 + 1 + ww]), win
