"""Rectangles for the resampled outputs: the checks every layer makes before a library call, and the sampling rule of a random resized crop.

rect_table(rects, n, w, h)          n rectangles (x0, y0, sw, sh) as contiguous int32 [n, 4], checked against the library's rule (yk_rs_rect_ok)
output_size(size)                   (ow, oh) checked the same way
random_resized_crop_rects(n, w, h)  n rectangles by torchvision's RandomResizedCrop rule, seeded, numpy only
"""
from __future__ import annotations

import math

import numpy as np

RS_MAX = 16384                                     # YK_RS_MAX of yaik_amd/csrc/yk_resample.h: the largest rectangle side and output side


def output_size(size):
    """(ow, oh) of a resampled output from size=(ow, oh): two ints in 1..16384; raises before any library call"""
    if isinstance(size, (str, bytes)) or not hasattr(size, "__len__") or len(size) != 2:
        raise TypeError(f"size must be (ow, oh); got {size!r}")
    ow, oh = size
    for v in (ow, oh):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"size must be two ints; got {size!r}")
    if not (1 <= int(ow) <= RS_MAX and 1 <= int(oh) <= RS_MAX):
        raise ValueError(f"the output size must be 1..{RS_MAX} on both sides; got {size!r}")
    return int(ow), int(oh)


def rect_table(rects, n: int, w: int, h: int) -> np.ndarray:
    """n source rectangles (x0, y0, sw, sh) as contiguous int32 [n, 4]: an integer array [n, 4] or a sequence of n 4-tuples of ints, each with
    x0, y0 >= 0, 1 <= sw, sh <= 16384, x0 + sw <= w, y0 + sh <= h (no alignment); raises before any library call"""
    if isinstance(rects, np.ndarray):
        if rects.ndim != 2 or rects.shape[1] != 4 or not np.issubdtype(rects.dtype, np.integer):
            raise TypeError(f"rectangles must be an integer array [N, 4]; got {rects.dtype} {rects.shape}")
        rows = rects.tolist()
    else:
        if isinstance(rects, (str, bytes)) or not hasattr(rects, "__len__"):
            raise TypeError(f"rectangles must be a sequence of (x0, y0, sw, sh); got {rects!r}")
        rows = []
        for r in rects:
            if isinstance(r, (str, bytes)) or not hasattr(r, "__len__") or len(r) != 4:
                raise TypeError(f"a rectangle must be (x0, y0, sw, sh); got {r!r}")
            for v in r:
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                    raise TypeError(f"a rectangle must be four ints; got {r!r}")
            rows.append([int(v) for v in r])
    if len(rows) != n:
        raise ValueError(f"{len(rows)} rectangles for {n} frames")
    for x0, y0, sw, sh in rows:
        if x0 < 0 or y0 < 0 or sw < 1 or sh < 1 or sw > RS_MAX or sh > RS_MAX or x0 + sw > w or y0 + sh > h:
            raise ValueError(f"rectangle ({x0}, {y0}, {sw}, {sh}) must have x0, y0 >= 0, 1 <= sw, sh <= {RS_MAX} and lie inside the {w} x {h} image")
    return np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(n, 4))


def random_resized_crop_rects(n: int, w: int, h: int, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), seed=0) -> np.ndarray:
    """n source rectangles (x0, y0, sw, sh), int32 [n, 4], for frames of w x h by the sampling rule of torchvision's RandomResizedCrop: up to ten
    tries of an area fraction uniform in `scale` and an aspect ratio sw / sh log-uniform in `ratio`, sides rounded to the nearest integer, the
    first try that fits the image placed uniformly; after ten misses the centre crop of the whole image clamped to `ratio`.  A side above 16384
    (the library's limit) counts as a miss and is clamped in the fallback.  numpy only; the same seed gives the same rectangles.  Every rectangle
    is valid for HipTileDecoder.set_batch_rects on frames of w x h."""
    if n < 1 or w < 1 or h < 1:
        raise ValueError("n, w, h must be positive")
    if not (0 < scale[0] <= scale[1]) or not (0 < ratio[0] <= ratio[1]):
        raise ValueError("scale and ratio must be positive (min, max) pairs")
    rng = np.random.default_rng(seed)
    area = float(w) * float(h)
    lr = (math.log(ratio[0]), math.log(ratio[1]))
    out = np.empty((n, 4), np.int32)
    for f in range(n):
        for _ in range(10):
            target = area * rng.uniform(scale[0], scale[1])
            ar = math.exp(rng.uniform(lr[0], lr[1]))
            sw, sh = int(round(math.sqrt(target * ar))), int(round(math.sqrt(target / ar)))
            if 0 < sw <= min(w, RS_MAX) and 0 < sh <= min(h, RS_MAX):
                y0 = int(rng.integers(0, h - sh + 1))
                x0 = int(rng.integers(0, w - sw + 1))
                break
        else:
            in_ratio = w / h
            if in_ratio < ratio[0]:
                sw = w
                sh = int(round(sw / ratio[0]))
            elif in_ratio > ratio[1]:
                sh = h
                sw = int(round(sh * ratio[1]))
            else:
                sw, sh = w, h
            sw, sh = max(1, min(sw, w, RS_MAX)), max(1, min(sh, h, RS_MAX))
            x0, y0 = (w - sw) // 2, (h - sh) // 2
        out[f] = (x0, y0, sw, sh)
    return out
