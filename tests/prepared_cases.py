"""Case data of the prepared-image tests (yk_decode_prepare_device / yk_decode_render_windows_device), beside tests/window_cases.py:
the extra window, the eight windows of the one-call test, and the block list of a render call restated in numpy."""
import numpy as np

from tests import window_cases as WC

# The 64-block of 520 x 264 whose tile row 15 holds tiles 1023 and 1024 (tile row 15 is tiles 975..1039; the block's tiles there are 1023..1030):
# one 64-tile round of the block-list 1-D launch has lanes in two scan blocks.  It holds a fully marked, an unmarked and a partly marked tile
# (the condition of window_cases.py; tests/test_decode_prepared_layout.py checks that on the CPU).
SCAN_BLOCK_BLOCK = (384, 64, 64, 64)
EXTRA = {(520, 264): [SCAN_BLOCK_BLOCK]}

# 520 x 264, windows of 64 x 40: a duplicate pair, two that share 64-blocks with (0, 0), one that reaches into the partial right block column
# (x 512..519), one into the partial bottom block row (y 256..263), the corner that does both, and a second duplicate
K8_SIZE = (64, 40)
K8_ORIGINS = [(0, 0), (0, 0), (32, 24), (456, 8), (200, 224), (192, 112), (456, 224), (192, 112)]


def case_windows(w: int, h: int) -> list:
    """the windows of window_cases.py for this image, then the extra ones"""
    return WC.windows(w, h) + EXTRA.get((w, h), [])


def block_mask(w: int, h: int, origins, ww: int, wh: int) -> np.ndarray:
    """[ceil(h / 64), ceil(w / 64)] bool: the 64x64 blocks the union of the windows touches"""
    m = np.zeros(((h + 63) // 64, (w + 63) // 64), dtype=bool)
    for x0, y0 in origins:
        m[y0 // 64:(y0 + wh - 1) // 64 + 1, x0 // 64:(x0 + ww - 1) // 64 + 1] = True
    return m


def new_blocks(w: int, h: int, origins, ww: int, wh: int, done) -> np.ndarray:
    """the ids (by * ceil(w / 64) + bx, ascending) of the blocks a render call with these windows lists when the ids in `done` are rendered already"""
    m = block_mask(w, h, origins, ww, wh).ravel()
    m[np.asarray(sorted(done), dtype=np.int64)] = False
    return np.flatnonzero(m)


def tiles_in_blocks(w: int, h: int, mask: np.ndarray) -> np.ndarray:
    """[h / 8, w / 8] bool: the 8x8 tiles inside the 64x64 blocks of `mask` (clipped to the image)"""
    return np.kron(mask, np.ones((8, 8), dtype=bool))[: h // 8, : w // 8]
