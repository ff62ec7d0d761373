"""The reference of the resampled outputs (include/yaik_hip.h) in numpy int64, on the oracle's whole decode; norm_ref makes the float
elements of its bytes.  Per axis (x shown):
    step = sw * 65536 // ow;  off = (step >> 1) - 32768;  pos(i) = clip(off + i * step, 0, (sw - 1) << 16)
    ix = pos >> 16;  fx = (pos >> 8) & 255;  ix1 = min(ix + 1, sw - 1)
    v = ((a (256 - fx) + b fx) (256 - fy) + (c (256 - fx) + d fx) fy + 32768) >> 16
Mirror flips the OUTPUT.  Every comparison made with these is exact.

`variant` names one mistake a kernel can make (VARIANTS); tests/test_decode_resample_cases.py checks that each of them changes the output of every
rectangle set the GPU tests use wherever it can, so that a kernel making it cannot pass.

The rectangle sets of the GPU tests live here too: per batch of tests/batch_window_cases.py two sets of one rectangle per frame.  Between them they
hold a 1 x 1 rectangle (an interior pixel of its tile, so that a clamp to the cover differs from a clamp to the rectangle), the whole frame next to
it (a one-tile cover beside the largest: the grid is the largest frame's), a rectangle cut on all four sides at odd offsets, one inside the partial
bottom-right 64-block, a 3 x 2 rectangle, and three whose covers take the origins of the scan_block window set (tile rows that cross a 1-D scan
block boundary)."""
import numpy as np

from tests import norm_ref as NR

RS_MAX = 16384
VARIANTS = ("no_round", "round_fx", "no_half", "clamp_image", "clamp_cover", "mirror_source")
SIZES = [(13, 11), (56, 40), (7, 3), (1, 1)]
FLAGS = [True, False, True, True]

# (w, h) -> {name: [rectangle of frame 0, 1, ...]}
RECT_SETS = {
    (520, 264): {
        "mixed_a": [(259, 131, 1, 1), (0, 0, 520, 264), (3, 5, 301, 97), (513, 257, 6, 5)],
        "mixed_b": [(329, 105, 190, 37), (193, 113, 189, 38), (2, 121, 3, 2), (257, 97, 191, 39)],
    },
    (136, 264): {
        "mixed_a": [(67, 131, 1, 1), (0, 0, 136, 264), (3, 5, 101, 97)],
        "mixed_b": [(129, 257, 6, 5), (61, 59, 3, 2), (9, 250, 120, 13)],
    },
    (8, 8): {
        "mixed_a": [(3, 4, 1, 1), (0, 0, 8, 8)],
        "mixed_b": [(1, 2, 3, 2), (2, 1, 5, 6)],
    },
}


def rect_sets(w, h):
    return [(name, list(rects)) for name, rects in RECT_SETS[(w, h)].items()]


def cover(rect):
    """(x0, y0, x1, y1) of the smallest 8-aligned rectangle that contains rect = (x0, y0, sw, sh)"""
    x0, y0, sw, sh = rect
    return x0 & ~7, y0 & ~7, (x0 + sw + 7) & ~7, (y0 + sh + 7) & ~7


def axis(n_src, n_out):
    step = (int(n_src) * 65536) // int(n_out)
    return step, (step >> 1) - 32768


def taps(n_src, n_out, variant=None, lo=0, hi=None):
    """(i0, i1, f) int64 arrays of n_out entries; lo / hi: where a wrong clamp would stop instead (indices relative to the rectangle)"""
    step, off = axis(n_src, n_out)
    if variant == "no_half":
        off = 0
    first, last = 0, n_src - 1
    if variant in ("clamp_image", "clamp_cover"):
        first, last = lo, hi
    pos = np.clip(off + np.arange(n_out, dtype=np.int64) * step, first << 16, last << 16)
    i0 = pos >> 16
    f = (pos >> 8) & 255
    if variant == "round_fx":
        f = ((pos & 0xFFFF) + 128) >> 8
    return i0, np.minimum(i0 + 1, last), f


def resample(whole, rect, size, mirror=False, variant=None, bound=None):
    """uint8 [oh, ow, C]: rect = (x0, y0, sw, sh) of whole [h, w, C] resampled to size = (ow, oh).  bound = (x0, y0, x1, y1) is what the clamp
    variants clamp to (the image or the cover)"""
    x0, y0, sw, sh = rect
    ow, oh = size
    h, w = whole.shape[:2]
    src = whole.astype(np.int64)
    if variant == "mirror_source":
        src = src.copy()
        src[y0:y0 + sh, x0:x0 + sw] = src[y0:y0 + sh, x0:x0 + sw][:, ::-1]
    bx0, by0, bx1, by1 = bound if bound is not None else (0, 0, w, h)
    ix, ix1, fx = taps(sw, ow, variant, bx0 - x0, bx1 - 1 - x0)
    iy, iy1, fy = taps(sh, oh, variant, by0 - y0, by1 - 1 - y0)
    X0, X1, Y0, Y1 = x0 + ix, x0 + ix1, y0 + iy, y0 + iy1
    fx = fx[None, :, None]
    fy = fy[:, None, None]
    a, b, c, d = src[Y0][:, X0], src[Y0][:, X1], src[Y1][:, X0], src[Y1][:, X1]
    top = a * (256 - fx) + b * fx
    bot = c * (256 - fx) + d * fx
    acc = top * (256 - fy) + bot * fy + (0 if variant == "no_round" else 32768)
    assert int(acc.max()) < 2 ** 31
    v = (acc >> 16).astype(np.uint8)
    if mirror and variant != "mirror_source":
        v = v[:, ::-1]
    return np.ascontiguousarray(v)


def resample_ref(whole, rect, size, dtype=None, scale=1.0, bias=0.0, mirror=False):
    """what the library writes for one frame: uint8 [oh, ow, C] (dtype None), or the bit patterns of the normalised elements"""
    v = resample(whole, rect, size, mirror)
    return v if dtype is None else NR.norm_ref(v, dtype, scale, bias)


def batch_ref(wholes, rects, size, dtype=None, scale=1.0, bias=0.0, flags=None):
    return np.stack([resample_ref(wh, r, size, dtype, scale, bias, bool(flags[f]) if flags is not None else False) for f, (wh, r) in enumerate(zip(wholes, rects))])
