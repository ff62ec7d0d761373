"""CPU side of the reduced-resolution decode tests: box_reduce of tests/scaled_ref.py equals a plain triple loop, and the images and
alpha planes the GPU tests use meet the condition of tests/scaled_ref.py, so that truncation, subsampling, ties rounded down and the chained
average would all show there."""
import numpy as np
import pytest

from tests import scaled_ref as SR
from tests import window_cases as WC


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_box_reduce_equals_a_plain_triple_loop(level):
    rng = np.random.default_rng(16 * 24 + level)
    a = rng.integers(0, 256, (16, 24, 3), dtype=np.uint8)
    a[:8, :8] = 255                                                          # the largest sum there is
    s = 1 << level
    want = np.zeros((16 // s, 24 // s, 3), dtype=np.uint8)
    for y in range(16 // s):
        for x in range(24 // s):
            for k in range(3):
                total = 0
                for dy in range(s):
                    for dx in range(s):
                        total += int(a[s * y + dy, s * x + dx, k])
                want[y, x, k] = (total + s * s // 2) >> (2 * level)
    got = SR.box_reduce(a, level)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(SR.box_reduce(a[..., 1], level), want[..., 1])      # [H, W] as well
    if level == 0:
        assert np.array_equal(got, a)
    with pytest.raises(ValueError):
        SR.box_reduce(a[:12, :12], 3)
    with pytest.raises(TypeError):
        SR.box_reduce(a.astype(np.int32), 1)


@pytest.mark.parametrize("w,h,kind", SR.CONDITION_CASES, ids=lambda v: str(v))
def test_the_images_meet_the_condition(oracle_built, w, h, kind):
    ref = WC.reference(w, h, kind)
    for level in SR.LEVELS:
        for k in range(3):
            figures = SR.condition_figures(ref.rgb[..., k], level)
            print(f"{w} x {h} level {level} channel {k}: rounding {figures[0]:.3f} top-left {figures[1]:.3f} ties {figures[2]}")
            assert SR.condition_failures(ref.rgb[..., k], level) == [], (w, h, level, k, figures)


@pytest.mark.parametrize("w,h,kind", SR.CONDITION_CASES, ids=lambda v: str(v))
def test_the_alpha_planes_meet_the_condition(w, h, kind):
    a = SR.alpha_plane(w, h)
    assert a.shape == (h, w) and a.dtype == np.uint8 and a.min() == 0 and a.max() == 255
    assert np.array_equal(a, SR.alpha_plane(w, h))                           # the same plane every time
    for level in SR.LEVELS:
        figures = SR.condition_figures(a, level)
        print(f"{w} x {h} level {level} alpha: rounding {figures[0]:.3f} top-left {figures[1]:.3f} ties {figures[2]}")
        assert SR.condition_failures(a, level) == [], (w, h, level, figures)


@pytest.mark.parametrize("w,h,kind", SR.CONDITION_CASES, ids=lambda v: str(v))
def test_the_chained_average_is_another_function_on_these_images(oracle_built, w, h, kind):
    ref = WC.reference(w, h, kind)
    assert np.array_equal(SR.chained_reduce(ref.rgb, 1), SR.box_reduce(ref.rgb, 1))
    for level in (2, 3):
        share = float((SR.chained_reduce(ref.rgb, level) != SR.box_reduce(ref.rgb, level)).mean())
        print(f"{w} x {h} level {level}: chained differs in {share:.3f}")
        assert share >= SR.MIN_CHAINED_SHARE, (w, h, level, share)


def test_the_one_tile_image_is_exempt_and_reduces_to_one_pixel(oracle_built):
    assert (8, 8, "smooth") in SR.CASES and (8, 8, "smooth") not in SR.CONDITION_CASES
    ref = WC.reference(8, 8, "smooth")
    assert SR.box_reduce(ref.rgb, 3).shape == (1, 1, 3)
