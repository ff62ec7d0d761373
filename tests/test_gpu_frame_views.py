"""The per-frame views of a handle (yk_frame / yk_dec_frame): a selected frame of a batch encoded on its own through the single-image entry
points, a refused bind, and the decode side's select_frame, each against a fresh single-image handle, byte for byte.  The shapes are the
smallest that reach every branch of the launchers: 72 x 40 (9 tiles wide: no run sums, yk_scan2_kernel, a ragged macro-tile column, an odd
tile4 stride) and 128 x 64 (16 tiles wide: the run-sum path)."""
import ctypes as C

import numpy as np
import pytest

from tests.images import edge_image
from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder

pytestmark = pytest.mark.gpu
YK_ERR_BAD_ARG = -2
SHAPES = [(72, 40), (128, 64)]
KINDS = ["mixed", "smooth", "photo"]


def _torch():
    import torch
    return torch


def _images(w, h, n_planes, seed=50):
    return [edge_image(w, h, k, n_planes, seed=seed + f) for f, k in enumerate(KINDS)]


def _dev(images):
    """int32 planes [n, h, w] per frame -> torch int32 [F, n, h, w] on the device"""
    return _torch().from_numpy(np.ascontiguousarray(np.stack(images).astype(np.int32))).cuda()


def _results(e):
    """every per-frame result of the selected frame, through the single-image getters"""
    out = {}
    a = e.alpha_result()
    out["alpha"] = [np.asarray(a["has_chunk"]), a["bounds"], np.asarray(a["remaining"]), a["tile_bbox"], a["bitmap"]]
    out["bitmaps"] = [e.gradient_bitmap(p) for p in range(7)]
    out["counts"] = [e.gradient_counts()]
    out["coverage"] = [e.coverage()]
    out["corners"] = [e.gradient_corners(p) for p in range(7)]
    out["range"] = [np.asarray(v) for p in range(3) for v in e.range_streams(p)]
    out["1d"] = list(e.dynamic_tile_compressor())
    return out


def _assert_same(got, want, what):
    assert got.keys() == want.keys()
    for k in want:
        assert len(got[k]) == len(want[k]), (what, k)
        for i, (g, w) in enumerate(zip(got[k], want[k])):
            assert np.array_equal(g, w), (what, k, i)


def _fresh_single(planes):
    e = HipTileEncoder(0)
    try:
        e.set_image(_torch().from_numpy(planes).cuda())
        e.mip_prefilter()
        e.encode(3, False)
        return _results(e)
    finally:
        e.close()


# ---- 1. a selected frame encoded on its own -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sel", [2, 0])
@pytest.mark.parametrize("n_planes", [3, 4], ids=["rgb", "rgba"])
@pytest.mark.parametrize("w,h", SHAPES)
def test_selected_frame_encoded_alone(w, h, n_planes, sel):
    images = _images(w, h, n_planes)
    e = HipTileEncoder(0)
    try:
        e.set_batch(_dev(images))
        e.encode_batch(3, False)
        before = []
        for f in range(3):
            e.select_frame(f)
            before.append(_results(e))
        assert any(int(b["counts"][0].sum()) for b in before) and any(b["1d"][0].size for b in before)
        e.select_frame(sel)
        if n_planes == 4:
            e.alpha_reject()
            e.alpha_finish(None)
        e.encode(3, False)
        _assert_same(_results(e), _fresh_single(images[sel]), (w, h, n_planes, "selected", sel))
        for f in range(3):
            if f != sel:
                e.select_frame(f)
                _assert_same(_results(e), before[f], (w, h, n_planes, "untouched", f))
        e.select_frame(sel)                                                    # and back: the frame's own results are still its own
        _assert_same(_results(e), before[sel], (w, h, n_planes, "selected against the batch's", sel))
    finally:
        e.close()


# ---- 2. a refused bind changes nothing ------------------------------------------------------------------------------------------------------
def _ptrs(t, n, plane_elems, skew_plane=None):
    return (C.c_void_p * 4)(*[t.data_ptr() + i * plane_elems * 4 + (4 if i == skew_plane else 0) if i < n else None for i in range(4)])


@pytest.mark.parametrize("w,h", SHAPES)
def test_refused_bind_single_image(w, h):
    planes = edge_image(w, h, "mixed", 4, seed=61)
    e = HipTileEncoder(0)
    try:
        t = _torch().from_numpy(planes).cuda()
        e.set_image(t)
        e.mip_prefilter()
        e.encode(3, False)
        want = _results(e)
        rc = e._L.yk_bind_device_planes(e._h, _ptrs(t, 4, w * h, skew_plane=1), w)
        assert rc == YK_ERR_BAD_ARG and b"16-byte aligned" in e._L.yk_last_error(e._h)
        assert e.validate_planes() == 0                                        # the planes of before the refusal are still bound
        e.mip_prefilter()
        e.encode(3, False)
        _assert_same(_results(e), want, (w, h, "after the refused bind"))
    finally:
        e.close()


@pytest.mark.parametrize("w,h", SHAPES)
def test_refused_bind_batch(w, h):
    images = _images(w, h, 4, seed=70)
    e = HipTileEncoder(0)
    try:
        t = _dev(images)
        e.set_batch(t)
        e.encode_batch(3, False)
        want = []
        for f in range(3):
            e.select_frame(f)
            want.append(_results(e))
        rc = e._L.yk_bind_device_batch(e._h, _ptrs(t, 4, w * h, skew_plane=1), w, C.c_size_t(4 * w * h))
        assert rc == YK_ERR_BAD_ARG and b"16-byte aligned" in e._L.yk_last_error(e._h)
        assert e.validate_planes() == 0
        e.encode_batch(3, False)
        for f in range(3):
            e.select_frame(f)
            _assert_same(_results(e), want[f], (w, h, "after the refused bind", f))
    finally:
        e.close()


# ---- 3. decode: select_frame in any order ---------------------------------------------------------------------------------------------------
def test_decode_select_frame_any_order():
    torch = _torch()
    w, h = 72, 40
    enc, dec, one = HipTileEncoder(0), HipTileDecoder(0), HipTileDecoder(0)
    try:
        enc.set_batch(_dev(_images(w, h, 3, seed=80)))
        enc.encode_batch(3, False)
        dec.begin_batch(w, h, 3)
        dec.decode_batch_from_encoder(enc)
        for f in (2, 0, 1):
            enc.select_frame(f)
            one.begin(w, h)
            one.decode_from_encoder(enc)
            dec.select_frame(f)
            assert np.array_equal(dec.planes(), one.planes()), f
            assert np.array_equal(dec.tile4x4(), one.tile4x4()), f
            assert np.array_equal(dec.tile4x4(all_planes=True), one.tile4x4(all_planes=True)), f
            assert torch.equal(dec.image_device(), one.image_device()), f
    finally:
        enc.close(); dec.close(); one.close()
