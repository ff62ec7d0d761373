"""The frames of the batch 6-bit 'ALPM' tests (test infrastructure, numpy only): every alpha class on shapes from one 16 x 16 tile upwards, the mode
ProcessAlpha(false) gives each, and the numpy model of the alpha stage's bounds.  tests/test_alpha6_batch_layout.py confirms the modes and the
coverage conditions on the CPU; tests/test_gpu_alpha6_batch.py runs the same frames on the GPU."""
import numpy as np

from tests import alpha_ref as R
from tests.test_alpha_6bit_mask import tile_keep, tile_mask

# 16 x 16: one tile; 72 x 40: sides 8 mod 16 (clipped edge tiles); 1040 x 40: 65 tile columns, the band kernel's 64-lane carry; 80 x 48: sides that
# are multiples of 16 with room for a rejected tile, the one kind of shape where kept tiles can span the image next to a box with a hole
SHAPES = [(16, 16), (72, 40), (1040, 40), (80, 48)]
COUNTS = [1, 2, 7, 33]
# kind -> the mode of ProcessAlpha(false), None = no chunk.  "ring": a box of kept tiles with a rejected tile inside (needs 3 tile columns);
# "holed": kept tiles spanning the image (no 'MIPM', every pixel selected); "low13": values 1..3 only (kept tiles, empty value box);
# "offbox": a box that starts at x = 4 mod 16 and at an odd row
KIND_MODE = {"ring": 3, "holed": 3, "L": 3, "narrow1": 3, "narrow2": 3, "narrow3": 3, "scatter": 3, "binary": 1, "all255": None, "empty": None,
             "low13": None, "offbox": 3}
KINDS = list(KIND_MODE)


def _fill(rng, a, ys, xs, lo=0, hi=256):
    v = a[ys, xs]
    a[ys, xs] = rng.integers(lo, hi, v.shape)


def alpha_of(rng, h, w, kind):
    a = np.zeros((h, w), np.int32)
    mth, mtw = (h + 15) // 16, (w + 15) // 16
    if kind == "ring":                                 # every tile of the box kept but one; the last tile row stays empty: a 'MIPM' chunk
        rows = h if mth == 1 else 16 * (mth - 1)
        _fill(rng, a, slice(0, rows), slice(0, w), 1)
        a[0, 0] = a[rows - 1, w - 1] = a[0, w - 1] = a[rows - 1, 0] = 200
        if mtw >= 3:
            a[0:16, 16 * (mtw // 2):16 * (mtw // 2) + 16] = 0
    elif kind == "holed":
        _fill(rng, a, slice(0, h), slice(0, w))
        if mtw >= 3 and mth >= 3:
            a[16:32, 16:32] = 0
        a[0, 0] = a[0, w - 1] = a[h - 1, 0] = a[h - 1, w - 1] = 9
    elif kind == "L":
        _fill(rng, a, slice(3, h), slice(5, 22))
        _fill(rng, a, slice(max(h - 19, 0), h - 1), slice(5, w - 1))
        a[3, 5] = 131
    elif kind.startswith("narrow"):                    # content 1..3 samples wide before the rounding to 4
        width = int(kind[-1])
        x = int(rng.integers(0, w - width))
        _fill(rng, a, slice(4, h - 4), slice(x, x + width), 4, 255)
    elif kind == "scatter":
        for _ in range(6):
            y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
            a[y:y + int(rng.integers(1, 30)), x:x + int(rng.integers(1, 30))] = rng.integers(0, 256)
        a[int(rng.integers(0, h)), int(rng.integers(0, w))] = 77
    elif kind == "binary":
        v = a[2:h - 5, 7:w - 9]
        a[2:h - 5, 7:w - 9] = 255 * rng.integers(0, 2, v.shape)
        a[2, 7] = 255
    elif kind == "all255":
        a[:] = 255
    elif kind == "low13":
        _fill(rng, a, slice(1, h - 1), slice(2, w - 2), 1, 4)
    elif kind == "offbox":
        x0 = 20 if w >= 40 else 4
        _fill(rng, a, slice(5, h - 3), slice(x0, w - 6), 0, 255)
        a[5, x0] = a[h - 4, w - 7] = 200
    elif kind != "empty":
        raise ValueError(kind)
    return a


def kinds_of(w, h, n, first=None):
    """the kinds of a batch, a rotation of KINDS: a batch of two or more starts with "ring" and "holed"; a batch of one takes a kind per shape"""
    if first is None:
        first = 0 if n > 1 else SHAPES.index((w, h)) % 2
    return [KINDS[(first + f) % len(KINDS)] for f in range(n)]


def rgb(h, w, f):
    y, x = np.mgrid[0:h, 0:w]
    return np.stack([((x * (p + 1) + y * 2 + 17 * p + 5 * f) & 255).astype(np.int32) for p in range(3)])


def frames_of(w, h, n, seed=0, first=None):
    """(kinds, frames [n, 4, h, w] int32)"""
    rng = np.random.default_rng(6600 + seed * 1000 + w * 7 + h * 3 + n)
    kinds = kinds_of(w, h, n, first)
    return kinds, np.stack([np.concatenate([rgb(h, w, f), alpha_of(rng, h, w, k)[None]]) for f, k in enumerate(kinds)])


def model_bounds(alpha):
    """the bounds of the GPU alpha stage: the box of the kept 16 x 16 tiles (no tile kept: the empty box yk_alpha_finish reports)"""
    ys, xs = np.nonzero(tile_keep(alpha))
    if ys.size == 0:
        return np.array([9999999, 9999999, -1, -1], np.int32)
    return np.array([xs.min() * 16, ys.min() * 16, xs.max() * 16 + 16, ys.max() * 16 + 16], np.int32)


def want(alpha, bounds, force8bit):
    """ProcessAlpha(force8bit) restated, with the tile rule's mask on `bounds`"""
    return R.encode(alpha, bounds, tile_mask(alpha, bounds), bool(force8bit))


def spans_image(alpha):
    """the kept tiles span the image: no 'MIPM' chunk, every pixel selected (only shapes whose sides are multiples of 16 can: the alpha stage's
    box ends on a tile edge)"""
    h, w = alpha.shape
    return tuple(model_bounds(alpha)) == (0, 0, w, h)


def has_rejected_tile_in_box(alpha):
    """a 'MIPM' chunk whose box holds a rejected tile"""
    keep = tile_keep(alpha)
    ys, xs = np.nonzero(keep)
    return ys.size > 0 and not spans_image(alpha) and not keep[ys.min():ys.max() + 1, xs.min():xs.max() + 1].all()
