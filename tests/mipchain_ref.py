"""Shared pieces of the mip chain tests (yk_decode_output_mipchain_device and its kin): the rule, the images and the condition the
images have to meet so that a wrong reduction cannot hide.

The rule: a w x h image has levels 0 .. top, top = floor(log2(min(w, h))); level k has (w >> k) x (h >> k) pixels, s = 1 << k,
out_k[Y][X][c] = (sum of the s x s box of the whole decode at (s X, s Y) + s s / 2) >> (2 k), straight from level 0 in integers (mip_reduce).  From
level 4 on the columns and rows that fill no whole box are ignored.  The images are those of tests/window_cases.py plus 256 x 128 "mixed" (whole
64 x 64 blocks only), with the oracle's whole decode as level 0, and the alpha planes of tests/scaled_ref.py.

The condition (checked on the CPU by tests/test_decode_mipchain_cases.py): at every level 4..top at least one output over the three colour channels
together differs between round-half-up and truncation; at every level with at least 32 outputs per channel, for every colour channel and the alpha
plane, at least 25 % of the outputs differ between round-half-up and truncation and at least 5 % differ from chained_from (the chain a caller
would build from the 1/8 output).  8 x 8 is the one-tile shape: its chain is levels 0..3 and it is exempt."""
import numpy as np

from tests import scaled_ref as SR
from tests import window_cases as WC

WHOLE_BLOCKS = (256, 128, "mixed")
IMAGES = WC.CASES + [WHOLE_BLOCKS]
CONDITION_CASES = [c for c in IMAGES if c[:2] != (8, 8)]
MIN_OUTPUTS, MIN_ROUNDING_SHARE, MIN_CHAINED_SHARE = 32, 0.25, 0.05


def mip_dims(w: int, h: int) -> list:
    """[(w >> k, h >> k) for k = 0 .. floor(log2(min(w, h)))]"""
    return [(w >> k, h >> k) for k in range(min(w, h).bit_length())]


def _cropped(a: np.ndarray, k: int) -> np.ndarray:
    h, w = a.shape[:2]
    return a[: h >> k << k, : w >> k << k]


def mip_sums(a: np.ndarray, k: int) -> np.ndarray:
    """the box sums (uint64) of level k of a [H, W, C] or [H, W] uint8 array: the crop to whole boxes, then SR.box_sums in steps that stay exact"""
    c = _cropped(np.asarray(a), k)
    if c.shape[0] == 0 or c.shape[1] == 0:
        raise ValueError(f"level {k} does not exist for {a.shape[1]} x {a.shape[0]}")
    first = min(k, 8)                                                       # 2^16 * 255 fits SR.box_sums' uint32
    s = SR.box_sums(c, first).astype(np.uint64)
    r = 1 << (k - first)
    return s.reshape((s.shape[0] // r, r, s.shape[1] // r, r) + s.shape[2:]).sum(axis=(1, 3), dtype=np.uint64)


def mip_reduce(a: np.ndarray, k: int) -> np.ndarray:
    """the rule of the module docstring: sums in uint64, rounded once"""
    return ((mip_sums(a, k) + np.uint64((1 << (2 * k)) >> 1)) >> np.uint64(2 * k)).astype(np.uint8)


def mip_truncate(a: np.ndarray, k: int) -> np.ndarray:
    return (mip_sums(a, k) >> np.uint64(2 * k)).astype(np.uint8)


def chained_from(a: np.ndarray, k: int) -> np.ndarray:
    """what the rule is NOT: §24's level 3 of `a`, then k - 3 rounded 2 x 2 means of the cropped result"""
    a = SR.box_reduce(np.asarray(a), 3)
    for _ in range(k - 3):
        a = SR.box_reduce(_cropped(a, 1), 1)
    return a


def condition_figures(rgb: np.ndarray, alpha: np.ndarray) -> list:
    """per level 4..top: (level, outputs per channel, colour outputs where rounding and truncation differ, [rounding share per plane],
    [chained share per plane]) with the planes R, G, B, alpha"""
    h, w = rgb.shape[:2]
    planes = [rgb[..., 0], rgb[..., 1], rgb[..., 2], alpha]
    out = []
    for k in range(4, len(mip_dims(w, h))):
        rounded = [mip_reduce(p, k) for p in planes]
        differ = [r != mip_truncate(p, k) for r, p in zip(rounded, planes)]
        out.append((k, rounded[0].size, int(sum(d.sum() for d in differ[:3])), [float(d.mean()) for d in differ],
                    [float((r != chained_from(p, k)).mean()) for r, p in zip(rounded, planes)]))
    return out


def condition_failures(figures: list) -> list:
    """what the condition misses (empty: it holds)"""
    out = []
    for k, n, colour, rounding, chained in figures:
        if colour < 1:
            out.append(f"level {k}: rounding and truncation agree on every colour output")
        if n >= MIN_OUTPUTS:
            out += [f"level {k} plane {i}: rounding share {r:.3f} < {MIN_ROUNDING_SHARE}" for i, r in enumerate(rounding) if r < MIN_ROUNDING_SHARE]
            out += [f"level {k} plane {i}: chained share {c:.3f} < {MIN_CHAINED_SHARE}" for i, c in enumerate(chained) if c < MIN_CHAINED_SHARE]
    return out
