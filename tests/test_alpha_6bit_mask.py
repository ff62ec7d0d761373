"""The mask of the 6-bit 'ALPM' encoder (ProcessAlpha(force8Bit = false)), on the CPU.

The GPU encoder selects samples by the reference's per-pixel mipmapMask as MipPrefilter leaves it, derived from the kept 16x16 tiles alone:
every pixel of a kept tile, or every pixel when the kept tiles span the image (no 'MIPM' chunk).  tile_mask() states that rule in numpy; the
tests pin it against the oracle's MipPrefilter and against the masks captured from the reference (tests/golden/alpha_analog_6bit_*.npz)."""
import os

import numpy as np
import pytest

from tests import alpha_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SIX_BIT = ["alpha_analog_6bit_mask.npz", "alpha_analog_6bit_fullmask.npz"]


def tile_keep(alpha: np.ndarray) -> np.ndarray:
    """[ceil(h/16), ceil(w/16)] bool: the tile holds a non-zero sample (edge tiles clipped to the image)."""
    a = np.asarray(alpha)
    h, w = a.shape
    mth, mtw = (h + 15) // 16, (w + 15) // 16
    pad = np.zeros((mth * 16, mtw * 16), dtype=bool)
    pad[:h, :w] = a != 0
    return pad.reshape(mth, 16, mtw, 16).any(axis=(1, 3))


def tile_mask(alpha: np.ndarray, bounds) -> np.ndarray:
    """The per-pixel mipmapMask (uint8 0 / 1) of an alpha plane whose MipPrefilter bounds are `bounds`."""
    h, w = np.asarray(alpha).shape
    if tuple(int(v) for v in bounds) == (0, 0, w, h):          # no 'MIPM' chunk: the mask is set to 255 again (:1401)
        return np.ones((h, w), np.uint8)
    return np.kron(tile_keep(alpha), np.ones((16, 16), bool))[:h, :w].astype(np.uint8)


def shape_alpha(rng, n: int, kind: str) -> np.ndarray:
    """n x n alpha planes whose kept tiles leave rejected tiles inside the box (ring, L) or span the image with a hole (no 'MIPM')."""
    a = np.zeros((n, n), np.int32)
    if kind == "ring":
        t0 = int(rng.integers(0, n // 16 - 2))
        t1 = int(rng.integers(t0 + 3, n // 16 + 1))
        a[t0 * 16:t1 * 16, t0 * 16:t1 * 16] = rng.integers(1, 256, ((t1 - t0) * 16,) * 2)
        a[t0 * 16 + 16:t1 * 16 - 16, t0 * 16 + 16:t1 * 16 - 16] = 0
    elif kind == "L":
        y0, x0 = int(rng.integers(0, n // 2)), int(rng.integers(0, n // 2))
        a[y0:n, x0:x0 + 20] = rng.integers(0, 256, (n - y0, 20))
        a[n - 24:n - 3, x0:n - 5] = rng.integers(0, 256, (21, n - 5 - x0))
    elif kind == "holed":                                       # every edge tile kept, one tile empty: bounds = image, no chunk
        a[:] = rng.integers(0, 256, (n, n))
        ty, tx = int(rng.integers(0, n // 16)), int(rng.integers(0, n // 16))
        a[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = 0
        a[0, 0] = a[0, n - 1] = a[n - 1, 0] = a[n - 1, n - 1] = 200
    return a


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("kind", ["ring", "L", "holed"])
def test_tile_mask_matches_oracle_mip_prefilter(oracle_built, seed, kind):
    rng = np.random.default_rng(300 + seed)
    n = (64, 128, 256)[seed % 3]
    a = shape_alpha(rng, n, kind)
    planes = np.stack([np.zeros((n, n), np.int32)] * 3 + [a])
    o = oracle_built.OracleEncoder(planes)
    mp = o.mip_prefilter()
    if kind == "holed":
        assert not mp["has_chunk"]
    np.testing.assert_array_equal(tile_mask(a, mp["bounds"]), (o.state("mipmapMask") != 0).astype(np.uint8))


@pytest.mark.parametrize("name", SIX_BIT)
def test_tile_mask_reproduces_the_captured_encode(name):
    """The reference's mask inside its bounds is the tile rule, and the 6-bit encode with the tile rule is the captured chunk.  (Outside
    the bounds the reference's recursion on a non-square image leaves parts of the mask it never visits at 255.)"""
    z = dict(np.load(os.path.join(GOLDEN, name)))
    x0, y0, x1, y1 = (int(v) for v in z["bounds"])
    mask = tile_mask(z["alpha"], z["bounds"])
    np.testing.assert_array_equal(mask[y0:y1, x0:x1], z["mipmask"][y0:y1, x0:x1] != 0)
    e = R.encode(z["alpha"], z["bounds"], mask, False)
    hd = z["header"]
    assert e["mode"] == hd[7] == R.IS_6_BIT_USEMIPMAPMASK_INVERSE and tuple(e["bbox"]) == tuple(int(v) for v in hd[:4])
    np.testing.assert_array_equal(e["payload"], z["payload"])


def test_selected_count_is_whole_groups():
    """bL and bR are rounded to 4 and tile edges are multiples of 16, so every selected run is whole 4-sample groups: the payload is always
    whole 3-byte groups, and pack6's partial last group never occurs on this path."""
    rng = np.random.default_rng(9)
    for _ in range(50):
        h, w = int(rng.integers(1, 12)) * 8, int(rng.integers(1, 12)) * 8
        a = np.zeros((h, w), np.int32)
        y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
        a[y:y + int(rng.integers(1, 20)), x:x + int(rng.integers(1, 20))] = rng.integers(0, 256)
        a[y, x] = 100
        keep = tile_keep(a)
        ys, xs = np.nonzero(keep)
        bounds = (xs.min() * 16, ys.min() * 16, xs.max() * 16 + 16, ys.max() * 16 + 16)
        e = R.encode(a, bounds, tile_mask(a, bounds), False)
        if e is not None and e["mode"] == R.IS_6_BIT_USEMIPMAPMASK_INVERSE:
            assert len(e["payload"]) % 3 == 0
