"""Shared pieces of the batch-window decode tests (yk_decode_set_batch_windows): the batches, the window sets of every batch and the
oracle's whole decode of every frame, which every window is a crop of.

A batch is N frames of one shape, frame f built by the generators of tests/window_cases.py from its own seed (frame 0 is window_cases' own image,
so its oracle decode is shared with those tests).  A window set is one window size with one origin per frame.  The origins of a set differ pairwise
across the frames, so that a kernel reading the rectangle table with the wrong frame index decodes a rectangle the test does not expect; the one
exception is the whole image, which has a single origin.  On the 8 x 8 batch the whole image is also the only window there is.

The condition is that of window_cases.condition_failures, for every frame and every window larger than one tile, on the frame's image AND on the
image of the second batch (other seeds) that the not-written test decodes under the same windows: tiles with all, none and some quadrants marked
inside the window and, unless the window starts at tile 0, before its first tile.  tests/test_decode_batch_window_cases.py checks it on the CPU.

Recorded moves (what a set would be if every origin met the condition as it stood):
  tile column: the columns through x = 8 .. 32 miss the condition for every frame (no tile of each kind before them), and so do those through
               x = 40 .. 88 for the last frame of either shape; the last frames take x = 504 and x = 96, the others window_cases' middle column
               (x = 256, x = 64) and columns that meet the condition as they stand.
  four 64-blocks, 520 x 264: 16 x 16 round the corner (64, 64) misses the condition as in window_cases; frame 0 keeps window_cases' (248, 184), the
               other frames take the nearest corners that meet it: (248, 56) for frame 1 only, (312, 120), (376, 56).
  four 64-blocks, 136 x 264: window_cases' 24 x 16 at (56, 56) is the only origin of that size that meets the condition, and 16 x 16 has none: one
               origin cannot serve three frames.  32 x 32 is the smallest square with three: round (64, 64), (64, 128) and (64, 192).
  scan block:  (192, 112) is window_cases.SCAN_BLOCK_WINDOW (row 15 ends at tile 1022, the next row starts in scan block 1); (328, 104) has tile
               row 15 itself cross the boundary (tiles 1016 .. 1039); (0, 120) and (256, 96) start in block 0 and end in block 1.  All meet the
               condition as they stand."""
import functools

import numpy as np

from tests import window_cases as WC
from tests.images import edge_image

# (w, h, kind, frames): 65 x 33 = 2145 tiles = three 1-D scan blocks; both sides 8 (mod 16) with partial right and bottom 64-blocks; one tile
BATCHES = [(520, 264, "mixed", 4), (136, 264, "mixed", 3), (8, 8, "smooth", 2)]

# (w, h) -> {name: ((ww, wh), [origin of frame 0, 1, ...])}
WINDOW_SETS = {
    (520, 264): {
        "whole": ((520, 264), [(0, 0)] * 4),
        "tile": ((8, 8), [(0, 0), (512, 256), (256, 128), (64, 192)]),
        "row": ((520, 8), [(0, 128), (0, 56), (0, 192), (0, 256)]),
        "column": ((8, 264), [(256, 0), (64, 0), (0, 0), (504, 0)]),
        "four_blocks": ((16, 16), [(248, 184), (248, 56), (312, 120), (376, 56)]),
        "scan_block": ((192, 40), [(192, 112), (328, 104), (0, 120), (256, 96)]),
    },
    (136, 264): {
        "whole": ((136, 264), [(0, 0)] * 3),
        "tile": ((8, 8), [(0, 0), (128, 256), (64, 128)]),
        "row": ((136, 8), [(0, 128), (0, 64), (0, 248)]),
        "column": ((8, 264), [(64, 0), (128, 0), (96, 0)]),
        "four_blocks": ((32, 32), [(56, 56), (56, 120), (56, 184)]),
    },
    (8, 8): {"whole": ((8, 8), [(0, 0)] * 2)},
}
# the sets whose origins cannot differ (the whole image has one origin)
SAME_ORIGIN = {"whole"}

# frames without a gradient tile ("noise": no pass accepts a tile) and without 1-D bytes ("flat": gradient tiles cover everything) between ordinary
# ones; the windows are those of the "four_blocks" set of 136 x 264 and a fourth over the partial blocks of the bottom right corner.  (An empty
# frame has tiles of one kind only: the condition is asked of the ordinary frames.)
EMPTY_BATCH = (136, 264, [("mixed", 0), ("noise", 1), ("flat", 2), ("mixed", 3)])
EMPTY_WINDOWS = ((32, 32), [(56, 56), (56, 120), (56, 184), (104, 232)])


def frame_seed(w: int, h: int, f: int, second: bool = False) -> int:
    """frame 0 has the seed of window_cases.source (second: of window_cases.second_source)"""
    return w * 7 + h + 31 * f + (1001 if second else 0)


@functools.lru_cache(maxsize=None)
def reference(w: int, h: int, kind: str, f: int, second: bool = False) -> WC.Reference:
    """the oracle's streams and whole decode of frame f of a batch, computed once per session (needs the oracle built)"""
    if f == 0:
        return WC.reference(w, h, kind, second)
    return WC.Reference(edge_image(w, h, kind, 3, seed=frame_seed(w, h, f, second)))


def batch_references(w: int, h: int, kind: str, n: int, second: bool = False) -> list:
    return [reference(w, h, kind, f, second) for f in range(n)]


def window_sets(w: int, h: int) -> list:
    """[(name, (ww, wh), origins)] of a batch shape"""
    return [(name, size, list(origins)) for name, (size, origins) in WINDOW_SETS[(w, h)].items()]


def all_batch_sets() -> list:
    return [(w, h, kind, n, name, size, origins) for w, h, kind, n in BATCHES for name, size, origins in window_sets(w, h)]


def crops(refs: list, size, origins) -> np.ndarray:
    """[N, wh, ww, 3]: frame f's whole decode cut to its window"""
    ww, wh = size
    return np.stack([r.rgb[y0:y0 + wh, x0:x0 + ww] for r, (x0, y0) in zip(refs, origins)])
