"""CPU side of the mip chain tests: mip_reduce of tests/mipchain_ref.py equals a plain loop where level 4 has a remainder in both
directions, its levels 0..3 are §24's box_reduce, mip_dims agrees with yk_decode_mip_levels, and the images and alpha planes the GPU tests use
meet the condition of tests/mipchain_ref.py, so that truncation and the chain built from the 1/8 output would both show there."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import mipchain_ref as MR
from tests import scaled_ref as SR
from tests import window_cases as WC


def test_mip_reduce_equals_a_plain_loop_with_remainders():
    w, h = 40, 24                                                            # level 4: 2 x 1 boxes, 8 columns and 8 rows left over
    rng = np.random.default_rng(w * h)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    a[:16, :16] = 255                                                        # the largest sum there is
    assert MR.mip_dims(w, h) == [(40, 24), (20, 12), (10, 6), (5, 3), (2, 1)]
    for k, (lw, lh) in enumerate(MR.mip_dims(w, h)):
        s = 1 << k
        want = np.zeros((lh, lw, 3), dtype=np.uint8)
        for y in range(lh):
            for x in range(lw):
                for c in range(3):
                    total = 0
                    for dy in range(s):
                        for dx in range(s):
                            total += int(a[s * y + dy, s * x + dx, c])
                    want[y, x, c] = (total + s * s // 2) >> (2 * k)
        got = MR.mip_reduce(a, k)
        assert got.dtype == np.uint8 and np.array_equal(got, want), k
        assert np.array_equal(MR.mip_reduce(a[..., 1], k), want[..., 1])      # [H, W] as well
    assert MR.mip_reduce(a, 4)[0, 0, 0] == 255
    with pytest.raises(ValueError):
        MR.mip_reduce(a, 5)


def test_levels_0_to_3_are_the_scaled_rule():
    rng = np.random.default_rng(7)
    a = rng.integers(0, 256, (136, 264, 3), dtype=np.uint8)
    for k in range(4):
        assert np.array_equal(MR.mip_reduce(a, k), SR.box_reduce(a, k)), k
    assert np.array_equal(MR.chained_from(a, 3), SR.box_reduce(a, 3))


def test_mip_dims_and_the_library_agree():
    from yaik_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)                                               # loading needs no device
    L.yk_decode_mip_levels.restype, L.yk_decode_mip_levels.argtypes = _lib.SIGNATURES["yk_decode_mip_levels"]
    for (w, h), n in (((8, 8), 4), ((136, 264), 8), ((16384, 8), 4), ((16384, 16384), 15), ((520, 264), 9), ((256, 128), 8)):
        dims = MR.mip_dims(w, h)
        assert len(dims) == n == L.yk_decode_mip_levels(w, h), (w, h)
        assert dims[0] == (w, h) and min(dims[-1]) == 1 and all(lw >= 1 and lh >= 1 for lw, lh in dims)
    assert _lib.YK_MIP_MAX_LEVELS == 15 == L.yk_decode_mip_levels(32760, 32760)
    for w, h in ((0, 8), (8, 12), (4, 8), (32768, 8), (-8, 8)):
        assert L.yk_decode_mip_levels(w, h) == -2, (w, h)                    # YK_ERR_BAD_ARG


@pytest.mark.parametrize("w,h,kind", MR.CONDITION_CASES, ids=lambda v: str(v))
def test_the_images_and_alpha_planes_meet_the_condition(oracle_built, w, h, kind):
    ref = WC.reference(w, h, kind)
    figures = MR.condition_figures(ref.rgb, SR.alpha_plane(w, h))
    assert [f[0] for f in figures] == list(range(4, len(MR.mip_dims(w, h))))
    for k, n, colour, rounding, chained in figures:
        print(f"{w} x {h} level {k}: {n} outputs, colour outputs that rounding changes {colour}, rounding " + " ".join(f"{r:.3f}" for r in rounding) +
              ", chained " + " ".join(f"{c:.3f}" for c in chained))
    assert MR.condition_failures(figures) == [], (w, h)


def test_the_one_tile_image_is_exempt_and_has_no_level_above_3(oracle_built):
    assert (8, 8, "smooth") in MR.IMAGES and (8, 8, "smooth") not in MR.CONDITION_CASES
    assert MR.mip_dims(8, 8) == [(8, 8), (4, 4), (2, 2), (1, 1)]
    assert MR.condition_figures(WC.reference(8, 8, "smooth").rgb, SR.alpha_plane(8, 8)) == []
