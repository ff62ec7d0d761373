"""One 'ALPM' encode path behind yk_alpha_values and yk_alpha_values_batch, and one pair of loops behind the mask modes of the decode: what a
handle that changes between the two entry points over the shared avState / avPay / avTab can get wrong, the box and class edges through both
entry points, and both mask-decode forms against the numpy restatement (tests/alpha_ref.py).  Every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

from tests import alpha_ref as R
from tests.test_alpha_6bit_mask import tile_mask
from tests.test_gpu_alpha_batch import _rgb, _same
from tests.test_gpu_alpha_mask_batch import _masked, _pixel_box, _selected, _want
from yaik_amd._lib import YaikError, lib
from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder, _chk

pytestmark = pytest.mark.gpu
YK_ERR_STATE = -4


@pytest.fixture(scope="module")
def enc():
    e = HipTileEncoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def one():
    e = HipTileEncoder(0)
    yield e
    e.close()


def _box(h, w, y0, y1, x0, x1, kind, rng):
    """one alpha plane (int32): rows y0..y1-1, columns x0..x1-1 hold the named class, its corners are set so that the box is exactly that"""
    a = np.zeros((h, w), np.int32)
    if kind == "analog":
        a[y0:y1, x0:x1] = rng.integers(0, 256, (y1 - y0, x1 - x0))
        a[y0, x0] = a[y1 - 1, x1 - 1] = 77
    elif kind == "binary":
        a[y0:y1, x0:x1] = 255 * rng.integers(0, 2, (y1 - y0, x1 - x0))
        a[y0, x0] = a[y1 - 1, x1 - 1] = 255
        a[y0 + 1, x0] = 0                                      # never all 255
    elif kind == "all255":
        a[y0:y1, x0:x1] = 255
    elif kind == "low":                                        # 1..3 only: v >> 2 == 0 everywhere, an empty box
        a[y0:y1, x0:x1] = rng.integers(1, 4, (y1 - y0, x1 - x0))
    else:
        raise ValueError(kind)
    return a


def _planes(alpha, f=0):
    h, w = alpha.shape
    return np.concatenate([_rgb(h, w, f), alpha[None]])


def _batch(enc, alphas, what):
    """alpha_values_batch() of the frames with these alpha planes; every frame against the restatement on the bounds the handle reports"""
    import torch
    frames = np.stack([_planes(a, f) for f, a in enumerate(alphas)])
    enc.set_batch(torch.from_numpy(frames).cuda())
    enc.encode_batch()
    got = enc.alpha_values_batch()
    assert len(got) == len(alphas)
    for f, a in enumerate(alphas):
        enc.select_frame(f)
        _same(got[f], R.encode(a, enc.alpha_result()["bounds"], None, True), (what, f))
    return got


def _single(enc, alpha, force8bit, what):
    """set_image + mip_prefilter + alpha_values(force8bit) against the restatement; the single call publishes no batch slot"""
    if getattr(enc, "frames", 1) != 1:                          # yk_set_image keeps the frame count of a batch of the same shape
        _chk(enc._h, lib().yk_set_batch(enc._h, 1))
    enc.set_image(_planes(alpha))
    bounds = enc.mip_prefilter()["bounds"]
    got = enc.alpha_values(force8bit)
    _same(got, R.encode(alpha, bounds, None if force8bit else tile_mask(alpha, bounds), force8bit), what)
    dev, nb = C.c_void_p(), C.c_size_t()
    rc = lib().yk_alpha_payload_device(enc._h, 0, C.byref(dev), C.byref(nb))
    assert rc == YK_ERR_STATE and dev.value is None and nb.value == 0, (what, rc)
    with pytest.raises(YaikError, match="yk_alpha_values_batch first"):
        _chk(enc._h, rc)
    return got


# ---- 1. one handle between the two entry points ------------------------------------------------------------------------------------------------
def test_call_sequence_on_one_handle(enc):
    w, h = 80, 48
    rng = np.random.default_rng(7)
    seven = [_box(h, w, 1, 47, 2, 79, "analog", rng), _box(h, w, 0, 48, 0, 80, "binary", rng), _box(h, w, 0, 48, 0, 80, "all255", rng),
             _box(h, w, 3, 40, 5, 70, "low", rng), _box(h, w, 10, 20, 20, 33, "analog", rng), np.zeros((h, w), np.int32),
             _box(h, w, 4, 44, 9, 71, "binary", rng)]
    got = _batch(enc, seven, "seven")
    assert [None if g is None else g["mode"] for g in got] == [6, 1, None, None, 6, None, 1]
    g = _single(enc, _box(h, w, 20, 26, 36, 44, "binary", rng), True, "single binary")
    assert g["mode"] == 1 and g["bbox"] == (32, 20, 16, 6)
    g = _single(enc, _box(h, w, 17, 30, 21, 50, "analog", rng), False, "single analog, 6 bit")
    assert g["mode"] == 3 and g["bbox"] == (20, 17, 32, 13)
    got = _batch(enc, [_box(h, w, 30, 41, 50, 63, "analog", rng), _box(h, w, 2, 9, 4, 28, "binary", rng), _box(h, w, 8, 30, 8, 40, "low", rng)], "three")
    assert [None if g is None else g["mode"] for g in got] == [6, 1, None]


# ---- 2. box and class edges, through the single call and as frame 1 of a batch of three ----------------------------------------------------------
# name: (w, h, rows, columns, class, mode and bbox expected of force8bit = True)
EDGES = {
    "binary_4mod8_both_sides": (80, 48, (5, 30), (12, 36), "binary", (1, (8, 5, 32, 25))),       # re-aligned to 8 the box grows on both sides
    "binary_to_right_edge_w72": (72, 40, (3, 38), (50, 72), "binary", (1, (48, 3, 24, 35))),
    "analog_last_pixel": (72, 40, (39, 40), (71, 72), "analog", (6, (68, 39, 4, 1))),
    "all_below_4": (80, 48, (6, 41), (10, 67), "low", None),                                      # an empty box: no chunk
    "all_255": (80, 48, (8, 20), (16, 32), "all255", None),                                       # no chunk
    "analog_6bit_next_to_8bit": (80, 48, (9, 37), (18, 61), "analog", (6, (16, 9, 48, 28))),
}


@pytest.mark.parametrize("name", list(EDGES))
def test_box_and_class_edges(enc, one, name):
    w, h, (y0, y1), (x0, x1), kind, want = EDGES[name]
    rng = np.random.default_rng(11)
    a = _box(h, w, y0, y1, x0, x1, kind, rng)
    got = _single(one, a, True, (name, "single"))
    assert (None if got is None else (got["mode"], got["bbox"])) == want
    fillers = _box(h, w, 0, h, 0, w, "analog", rng), _box(h, w, 1, h - 1, 4, w - 4, "binary", rng)
    three = _batch(enc, [fillers[0], a, fillers[1]], name)
    _same(three[1], got, (name, "batch against single"))
    if name == "analog_6bit_next_to_8bit":
        six = _single(one, a, False, (name, "single, 6 bit"))
        assert six["mode"] == 3 and six["bbox"] == got["bbox"] and three[1]["mode"] == 6


# ---- 3. mask decode: both forms against the restatement -----------------------------------------------------------------------------------------
def test_mask_modes_both_forms_against_restatement():
    """80 x 48, a box 68 wide: two 64-lane steps per row, the second one partial"""
    w, h, bbox, grid = 80, 48, (8, 3, 68, 40), (0, 0, 5, 3)
    rng = np.random.default_rng(23)
    bits = np.packbits(np.array([1, 0, 1, 1, 0, 0, 1, 1, 0, 1, 1, 1, 0, 1, 1], np.uint8), bitorder="little")
    assert 0 < _selected(bbox, bits, grid) < bbox[2] * bbox[3]
    ent = [_masked(rng, 2, bbox, grid, bits=bits), _masked(rng, 3, bbox, grid, bits=bits)]
    want = [_want(e, w, h, 255) for e in ent]
    assert want[0].any() and not np.array_equal(want[0], want[1])
    dec = HipTileDecoder(0)
    try:
        for e, p in zip(ent, want):                                         # yk_decode_alpha with the decoded mask
            dec.begin(w, h)
            mask = dec.decompress_1bit_tiled(e[3], grid[2], grid[3])
            np.testing.assert_array_equal(dec.decompress_alpha(e[0], e[1], e[2], mask, _pixel_box(grid)), p, err_msg=f"single, mode {e[0]}")
        dec.begin_batch(w, h, len(ent))                                     # yk_decode_alpha_mask_batch_device with the tile bitmap
        dec.decompress_alpha_batch(ent)
        assert dec.alpha_batch_status().tolist() == [0, 0]
        for f, p in enumerate(want):
            dec.select_frame(f)
            np.testing.assert_array_equal(dec.alpha_plane(), p, err_msg=f"batch, mode {ent[f][0]}")
    finally:
        dec.close()
