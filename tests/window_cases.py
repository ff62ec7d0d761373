"""Shared pieces of the window-decode tests (yk_decode_set_window): the images, the windows of every image, the oracle's whole decode
that every window is a crop of, and the condition the windows have to meet so that a window decode can go wrong in every stream at once.

The condition (checked on the CPU by tests/test_decode_window_cases.py from the oracle's tile4x4Mask): for every "mixed" image and every window
larger than one tile, the window holds an 8x8 tile with all four quadrants marked by gradient tiles, one with none marked and one partly marked;
and unless the window starts at tile 0, a tile of each of these three kinds precedes the window's first tile in raster order, so that the type
stream, the pixel stream and the scan offsets are all non-zero where the window starts.

Recorded moves (the window (56, 56, 16, 16), one tile of each of four 64-blocks, misses the condition on both "mixed" images: its four tiles are
three unmarked ones and a fully marked one, none partly marked; STRADDLE holds what replaces it):
  136 x 264: none of the three 16 x 16 windows round a corner of four 64-blocks holds all three kinds.  (56, 56, 24, 16): the same origin, one
             tile wider; it still has tiles of four 64-blocks.
  520 x 264: (248, 184, 16, 16), the 16 x 16 window round a corner of four 64-blocks nearest to (56, 56) that meets the condition.
The tile row and tile column are the ones through the middle of the image (y = (h / 16) * 8, x = (w / 16) * 8); they and every other named
window meet the condition as they stand."""
import functools

import numpy as np

from tests.images import edge_image
from tests.ragged import cell_marks, oracle_streams, source

# (w, h, kind): both sides 8 (mod 16) with partial right and bottom 64-blocks; 65 x 33 = 2145 tiles = three 1-D scan blocks; a photo; one tile
CASES = [(136, 264, "mixed"), (520, 264, "mixed"), (264, 136, "photo"), (8, 8, "smooth")]
# tile row 15 of 520 x 264 holds tiles 975..1039: this window's row 15 covers tiles 999..1022 and its rows 16..18 lie in scan block 1
SCAN_BLOCK_WINDOW = (192, 112, 192, 40)
# the window that straddles four 64-blocks, per image (see "Recorded moves" above); other images of at least 72 x 72 take (56, 56, 16, 16)
STRADDLE = {(136, 264): (56, 56, 24, 16), (520, 264): (248, 184, 16, 16)}


def windows(w: int, h: int) -> list:
    """the windows (x0, y0, ww, wh) of a w x h image, without repeats"""
    out = [(0, 0, w, h), (0, 0, 8, 8), (w - 8, h - 8, 8, 8)]
    if w >= 72 and h >= 72:
        out.append(STRADDLE.get((w, h), (56, 56, 16, 16)))             # tiles of four 64-blocks
    out.append((0, (h // 16) * 8, w, 8))                               # a tile row
    out.append(((w // 16) * 8, 0, 8, h))                               # a tile column
    if (w, h) == (520, 264):
        out.append(SCAN_BLOCK_WINDOW)
    seen, uniq = set(), []
    for win in out:
        if win not in seen:
            seen.add(win)
            uniq.append(win)
    return uniq


def all_case_windows() -> list:
    return [(w, h, kind, win) for w, h, kind in CASES for win in windows(w, h)]


def second_source(w: int, h: int, kind: str) -> np.ndarray:
    """image B of the work-is-skipped test: the same kind from another seed"""
    return edge_image(w, h, kind, 3, seed=w * 7 + h + 1001)


class Reference:
    """The oracle's streams and whole decode of one image: passes, typ, pix, tile4 (after the gradient passes: what the 1-D chunk reads), planes
    (8x8-tiled, after the 1-D chunk) and rgb [h, w, 3]."""

    def __init__(self, planes: np.ndarray):
        from oracle.pyoracle import OracleDecoder, detile
        self.h, self.w = planes.shape[1:]
        self.passes, self.typ, self.pix = oracle_streams(planes)
        od = OracleDecoder(self.w, self.h)
        for sx, sy, cnt, bm, rgb in self.passes:
            if cnt:
                od.gradient(sx, sy, bm, rgb)
        self.tile4 = od.tile4x4().copy()
        od.split_masks()
        od.decode_1d(self.typ, self.pix)
        self.planes = od.planes().copy()
        self.rgb = np.stack([detile(self.planes[c], self.w, self.h) for c in range(3)], axis=-1)
        self.planes.setflags(write=False); self.rgb.setflags(write=False); self.tile4.setflags(write=False)

    def crop(self, win) -> np.ndarray:
        x0, y0, ww, wh = win
        return self.rgb[y0:y0 + wh, x0:x0 + ww]


@functools.lru_cache(maxsize=None)
def reference(w: int, h: int, kind: str, second: bool = False) -> Reference:
    """computed once per image and shared by the tests of a session (needs the oracle built: the oracle_built fixture)"""
    return Reference(second_source(w, h, kind) if second else source(w, h, kind))


def tile_kinds(tile4: np.ndarray, w: int, h: int) -> np.ndarray:
    """[h / 8, w / 8]: the number of quadrants of every 8x8 tile that tile4x4Mask marks (0 = none, 4 = all)"""
    m = cell_marks(tile4, w, h)[:, : w // 4]
    return m.reshape(h // 8, 2, w // 8, 2).sum(axis=(1, 3))


def condition_failures(kinds: np.ndarray, win) -> list:
    """what the condition of the module docstring misses for window `win` of an image with the tile kinds `kinds` (empty: it holds)"""
    x0, y0, ww, wh = win
    tx0, ty0, tw, th = x0 // 8, y0 // 8, ww // 8, wh // 8
    if tw * th <= 1:
        return []
    names = {"all": lambda k: k == 4, "none": lambda k: k == 0, "partly": lambda k: (k > 0) & (k < 4)}
    inside = kinds[ty0:ty0 + th, tx0:tx0 + tw]
    before = kinds.ravel()[: ty0 * kinds.shape[1] + tx0]
    out = [f"no tile with {n} quadrants marked inside" for n, f in names.items() if not f(inside).any()]
    if tx0 or ty0:
        out += [f"no tile with {n} quadrants marked before the window" for n, f in names.items() if not f(before).any()]
    return out


def outside_rounded(w: int, h: int, win) -> np.ndarray:
    """[h / 8, w / 8] bool: the 8x8 tiles outside the window rounded out to multiples of 64 (the tiles a window decode may not write)"""
    x0, y0, ww, wh = win
    bx0, by0, bx1, by1 = (x0 // 64) * 8, (y0 // 64) * 8, -(-(x0 + ww) // 64) * 8, -(-(y0 + wh) // 64) * 8
    out = np.ones((h // 8, w // 8), dtype=bool)
    out[by0:by1, bx0:bx1] = False
    return out


def tiles_of(planes_tiled: np.ndarray, w: int, h: int) -> np.ndarray:
    """[3, h / 8, w / 8, 64] view of the 8x8-tiled planes"""
    return planes_tiled.reshape(3, h // 8, w // 8, 64)
