"""Shared pieces of the reduced-resolution decode tests (yk_decode_output_scaled_device and its kin): the rule, the images, an alpha
plane per image, and the condition the images have to meet so that a wrong reduction cannot hide.

The rule: level = 0..3, s = 1 << level, out[Y][X][k] = (sum of the s x s box of the whole decode at (s X, s Y) + s s / 2) >> (2 level), straight
from level 0 in integers (box_reduce).  The images are those of tests/window_cases.py with the oracle's whole decode as level 0.

The condition (checked on the CPU by tests/test_decode_scaled_cases.py, on the oracle's decode and on the alpha plane, for 136 x 264, 520 x 264 and
264 x 136, every level 1..3 and every channel): at least 25 % of the outputs differ between round-half-up and truncation, at least 50 % differ from
the box's top-left sample, and at least one output is an exact tie (the sum modulo s s equals s s / 2).  A kernel that truncates, that
subsamples, or that rounds ties down therefore fails the GPU tests on every one of these images.  8 x 8 is the one-tile shape only (level 3 is a
single pixel there) and is exempt.

The alpha plane is a diagonal ramp over the full range plus Gaussian noise (sigma 24), clipped; it meets the condition as generated, so no
change of the generator is recorded here."""
import numpy as np

from tests import window_cases as WC

LEVELS = (1, 2, 3)
CASES = WC.CASES
CONDITION_CASES = [c for c in CASES if c[:2] != (8, 8)]
MIN_ROUNDING_SHARE, MIN_TOP_LEFT_SHARE, MIN_TIES, MIN_CHAINED_SHARE = 0.25, 0.50, 1, 0.10


def box_sums(a: np.ndarray, level: int) -> np.ndarray:
    """the s x s box sums (uint32) of a [H, W, C] or [H, W] uint8 array, s = 1 << level; H and W are multiples of s"""
    a = np.asarray(a)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise TypeError("box_reduce takes [H, W, C] or [H, W] uint8 arrays")
    s = 1 << level
    h, w = a.shape[:2]
    if h % s or w % s:
        raise ValueError(f"{w} x {h} does not divide by {s}")
    return a.astype(np.uint32).reshape((h // s, s, w // s, s) + a.shape[2:]).sum(axis=(1, 3), dtype=np.uint32)


def box_reduce(a: np.ndarray, level: int) -> np.ndarray:
    """the rule of the module docstring"""
    s = 1 << level
    return ((box_sums(a, level) + (s * s) // 2) >> (2 * level)).astype(np.uint8)


def chained_reduce(a: np.ndarray, level: int) -> np.ndarray:
    """what the rule is NOT: level times the 2 x 2 mean of the rounded means of the level before"""
    for _ in range(level):
        a = box_reduce(a, 1)
    return a


def alpha_plane(w: int, h: int) -> np.ndarray:
    """[h, w] uint8: a ramp from 0 (top left) to 255 (bottom right) plus noise, clipped -- analog alpha over the full range"""
    rng = np.random.default_rng(w * 31 + h)
    y, x = np.mgrid[0:h, 0:w]
    ramp = (x + y) * (255.0 / max(w + h - 2, 1))
    a = np.clip(np.rint(ramp + rng.normal(0.0, 24.0, (h, w))), 0, 255).astype(np.uint8)
    a.setflags(write=False)
    return a


def condition_figures(plane: np.ndarray, level: int) -> tuple:
    """(share of outputs where round-half-up and truncation differ, share that differ from the box's top-left sample, number of exact ties) of a
    [H, W] uint8 plane at `level`"""
    s = 1 << level
    sums = box_sums(plane, level)
    rounded, truncated = (sums + (s * s) // 2) >> (2 * level), sums >> (2 * level)
    return (float((rounded != truncated).mean()), float((rounded != plane[::s, ::s]).mean()), int((sums % (s * s) == (s * s) // 2).sum()))


def condition_failures(plane: np.ndarray, level: int) -> list:
    """what the condition misses for a plane at a level (empty: it holds)"""
    r, t, ties = condition_figures(plane, level)
    out = []
    if r < MIN_ROUNDING_SHARE:
        out.append(f"rounding share {r:.3f} < {MIN_ROUNDING_SHARE}")
    if t < MIN_TOP_LEFT_SHARE:
        out.append(f"top-left share {t:.3f} < {MIN_TOP_LEFT_SHARE}")
    if ties < MIN_TIES:
        out.append("no exact tie")
    return out
