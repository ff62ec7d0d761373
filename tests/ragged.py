"""Shared pieces of the ragged-size decode tests: images whose width and/or height is 8 (mod 16), the oracle's streams for them, and the
tile4x4Mask arithmetic (byte (cx >> 2) + (cy >> 1) * stride4, bit ((cx >> 1) & 1) * 4 + (cy & 1) * 2 + (cx & 1) for 4x4 cell (cx, cy))."""
import numpy as np

from oracle.pyoracle import PASSES, OracleEncoder, palette_remap
from tests.images import edge_image

# (w, h, kind): w and/or h = 8 (mod 16)
SHAPES = [(8, 8, "smooth"), (24, 40, "mixed"), (200, 72, "photo"), (136, 264, "mixed"), (1920, 1080, "photo"), (1080, 1920, "smooth")]
LARGE = [(8184, 8200, "smooth"), (32760, 72, "smooth")]


def source(w: int, h: int, kind: str, n_planes: int = 3) -> np.ndarray:
    return edge_image(w, h, kind, n_planes, seed=w * 7 + h)


def oracle_streams(planes: np.ndarray, mip: bool = False):
    """[(sx, sy, count, bitmap, corner stream after PaletteFullRangeRemapping)] for the seven passes, the 1-D type and pixel streams"""
    enc = OracleEncoder(planes)
    if mip:
        enc.mip_prefilter()
    passes = []
    for sx, sy in PASSES:
        cnt, bm, rgb = enc.fitting_quad_smooth(sx, sy)
        passes.append((sx, sy, cnt, bm, palette_remap(rgb, 250)))
    for p in range(3):
        enc.dynamic_tile_compressor(p)
    pix, typ = enc.streams_1d()
    return passes, typ, pix


def cell_marks(tile4: np.ndarray, w: int, h: int) -> np.ndarray:
    """[h / 4, 4 * stride4] bool: the tile4x4Mask bit of every 4x4 cell the mask has room for (columns past w / 4 lie outside the image)"""
    stride4 = (w + 15) >> 4
    cy, cx = np.mgrid[0:h // 4, 0:stride4 * 4]
    byte = tile4[(cx >> 2) + (cy >> 1) * stride4]
    return ((byte >> ((((cx >> 1) & 1) << 2) | ((cy & 1) << 1) | (cx & 1))) & 1).astype(bool)


def stream_lengths_1d(tile4: np.ndarray, w: int, h: int, planes: int = 3):
    """what Decompress1D consumes over the w/8 x h/8 tiles with a shared mask: 3 type bytes per tile with an unmarked quadrant, 16 pixel
    bytes per unmarked quadrant, per plane"""
    m = cell_marks(tile4, w, h)[:, : w // 4]
    q = m.reshape(h // 8, 2, w // 8, 2)                       # [tile row, cell row in tile, tile column, cell column in tile]
    unmarked = (~q).sum(axis=(1, 3))
    return planes * 3 * int((unmarked > 0).sum()), planes * 16 * int(unmarked.sum())


def psnr(rec: np.ndarray, src: np.ndarray) -> float:
    mse = float(np.mean((rec.astype(np.int64) - src.astype(np.int64)) ** 2))
    return 99.0 if mse == 0 else 10 * np.log10(255.0 ** 2 / mse)
