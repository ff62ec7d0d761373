"""numpy restatement of the 'MIPM' bit rule (yk_alpha_bitmap / yk_alpha_bitmaps_batch, EncoderContext.cpp:1317-1327) and frames whose alpha
planes exercise it (test infrastructure)."""
from __future__ import annotations

import numpy as np

# every frame of a batch carries another kind: a box with rejected tiles inside it, kept tiles spanning the image (no chunk), all zero, one kept
# tile in the last row and column, only a part tile kept (the last tile where the shape has none), all 255
KINDS = ["box_holes", "span", "zero", "last_tile", "part_tile", "all255"]


def keep_flags(alpha: np.ndarray) -> np.ndarray:
    """[mtH, mtW] bool: a 16x16 tile (part tiles at the edges included) is kept when one of its samples is not 0"""
    h, w = alpha.shape
    mth, mtw = (h + 15) // 16, (w + 15) // 16
    pad = np.zeros((mth * 16, mtw * 16), dtype=bool)
    pad[:h, :w] = np.asarray(alpha) != 0
    return pad.reshape(mth, 16, mtw, 16).any(axis=(1, 3))


def mip_bits(keep: np.ndarray, bounds, w: int, h: int):
    """(has_chunk, tile_bbox, bits) from the keep flags and the box of kept tiles in pixels {x0, y0, x1, y1}"""
    b = [int(v) for v in bounds]
    tb = np.array([b[0] >> 4, b[1] >> 4, (b[2] >> 4) - (b[0] >> 4), (b[3] >> 4) - (b[1] >> 4)], np.int32)
    whole = b == [0, 0, w, h]
    if whole or b[2] < b[0]:
        return not whole, tb, np.zeros(0, np.uint8)
    bx0, by0, tw, th = (int(v) for v in tb)
    sub = np.zeros((th, tw), np.uint8)
    ys, xs = min(th, keep.shape[0] - by0), min(tw, keep.shape[1] - bx0)
    sub[:ys, :xs] = keep[by0:by0 + ys, bx0:bx0 + xs]
    return True, tb, np.packbits(sub.ravel(), bitorder="little")          # bit y * tw + x, LSB first


def alpha_plane(rng, h: int, w: int, kind: str) -> np.ndarray:
    """one u8 alpha plane of the named kind"""
    mth, mtw = (h + 15) // 16, (w + 15) // 16
    keep = np.zeros((mth, mtw), bool)
    if kind == "all255":
        return np.full((h, w), 255, np.uint8)
    if kind == "box_holes":
        x0, y0 = int(rng.integers(0, max(mtw - 2, 1))), int(rng.integers(0, max(mth - 2, 1)))
        x1, y1 = int(rng.integers(x0, mtw)), int(rng.integers(y0, mth))
        if (x0, y0, x1, y1) == (0, 0, mtw - 1, mth - 1) and mtw > 1:
            x0 = 1                                                            # not the whole image
        keep[y0:y1 + 1, x0:x1 + 1] = rng.integers(0, 3, (y1 - y0 + 1, x1 - x0 + 1)) == 0
        keep[y0, x0] = keep[y1, x1] = True
    elif kind == "span":
        keep[:] = rng.integers(0, 2, keep.shape) == 0
        keep[0, 0] = keep[mth - 1, mtw - 1] = True
    elif kind == "last_tile":
        keep[mth - 1, mtw - 1] = True
    elif kind == "part_tile":
        if w & 15:
            keep[0, mtw - 1] = True
        elif h & 15:
            keep[mth - 1, 0] = True
        else:
            keep[mth - 1, mtw - 1] = True
    elif kind != "zero":
        raise ValueError(kind)
    a = np.zeros((mth * 16, mtw * 16), np.uint8)
    for my, mx in zip(*np.nonzero(keep)):                                     # one sample of the tile that lies inside the image
        yy = int(rng.integers(my * 16, min(my * 16 + 16, h)))
        xx = int(rng.integers(mx * 16, min(mx * 16 + 16, w)))
        a[yy, xx] = int(rng.integers(1, 256))
    return a[:h, :w].copy()


def frames_u8(w: int, h: int, n: int, first: int = 0, seed: int = 0, channels: int = 4) -> np.ndarray:
    """[n, h, w, channels] u8: frame f carries kind KINDS[(first + f) % 6] in its alpha channel"""
    rng = np.random.default_rng(seed * 1000 + w * 7 + h * 3 + n)
    y, x = np.mgrid[0:h, 0:w]
    out = np.empty((n, h, w, channels), np.uint8)
    for f in range(n):
        for p in range(3):
            out[f, ..., p] = (x * (p + 1) + y * 2 + 17 * p + 5 * f) & 255
        if channels == 4:
            out[f, ..., 3] = alpha_plane(rng, h, w, KINDS[(first + f) % len(KINDS)])
    return out
