"""'MIPM' bitmaps for batches: yk_alpha_bitmaps_batch + yk_alpha_bitmap_device (HipTileEncoder.alpha_bitmaps_batch / alpha_bitmaps_device).  Every
comparison is bit-exact, against three sources: a second handle that runs the single-image MipPrefilter on the frame, select_frame +
alpha_result on the batch handle itself, and the numpy restatement of the bit rule (tests/mip_ref.py) on the frame's own keep flags."""
import ctypes as C

import numpy as np
import pytest

from tests import mip_ref as M
from yaik_amd._lib import lib
from yaik_amd.encoder import HipTileEncoder, _MipInfoC

pytestmark = pytest.mark.gpu
YK_ERR_BAD_ARG, YK_ERR_STATE = -2, -4
# 16 x 16: one tile; 72 x 40: 5 x 3 tiles, part tiles on both edges; 1040 x 520: 65 x 33 tiles, a row of bits longer than a wave and never byte-aligned
SHAPES = [(16, 16), (72, 40), (1040, 520)]
COUNTS = [1, 2, 7, 33]
DISTINCT = 12                                                                # frames of a large batch repeat after this many: one reference each


def _torch():
    import torch
    return torch


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


def _frames(w, h, n, first=0, seed=0, channels=4):
    base = M.frames_u8(w, h, min(n, DISTINCT), first, seed, channels)
    return base[np.arange(n) % base.shape[0]]


def _same(got, want, what, remaining=False):
    assert got["has_chunk"] == want["has_chunk"], (what, got, want)
    assert np.array_equal(got["bounds"], want["bounds"]) and np.array_equal(got["tile_bbox"], want["tile_bbox"]), (what, got, want)
    np.testing.assert_array_equal(got["bitmap"], want["bitmap"], err_msg=str(what))
    assert ("remaining" in got) == remaining


def _check_batch(enc, one, frames, ref=None):
    torch = _torch()
    ref = {} if ref is None else ref
    n, h, w, ch = frames.shape
    enc.set_batch_u8(torch.from_numpy(frames).cuda())
    enc.encode_batch()
    got = enc.alpha_bitmaps_batch()
    dev = enc.alpha_bitmaps_device()
    assert len(got) == n and len(dev) == n
    slot = (((w + 15) // 16 * ((h + 15) // 16) + 7) // 8 + 15) & ~15
    ptrs = [d["ptr"] for d in dev if d["nbytes"]]
    assert all(p % 16 == 0 for p in ptrs) and len(set(ptrs)) == len(ptrs)
    assert all(b - a >= slot for a, b in zip(sorted(ptrs), sorted(ptrs)[1:]))  # one slot per frame
    for f in range(n):
        k = f % DISTINCT
        assert dev[f]["nbytes"] == got[f]["bitmap"].size and (dev[f]["ptr"] != 0) == (got[f]["bitmap"].size != 0)
        enc.select_frame(f)
        _same(got[f], {k2: v for k2, v in enc.alpha_result().items() if k2 != "remaining"}, (f, "select_frame + alpha_result"))
        if k not in ref:
            one.set_image_u8(frames[f])
            ref[k] = {k2: v for k2, v in one.mip_prefilter().items() if k2 != "remaining"}
        _same(got[f], ref[k], (f, "single handle"))
        if ch == 4:
            has, tb, bits = M.mip_bits(M.keep_flags(frames[f, ..., 3]), got[f]["bounds"], w, h)
            _same(got[f], {"has_chunk": has, "bounds": got[f]["bounds"], "tile_bbox": tb, "bitmap": bits}, (f, "restatement"))
    return got


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_bitmaps_of_every_frame(enc, one, w, h, n):
    first = SHAPES.index((w, h)) * 2 + n                                   # every kind comes first in some small batch
    got = _check_batch(enc, one, _frames(w, h, n, first=first))
    if n >= len(M.KINDS):                                                  # the kinds are what their names say
        by_kind = {M.KINDS[(first + f) % len(M.KINDS)]: g for f, g in enumerate(got[:len(M.KINDS)])}
        mtw, mth = (w + 15) // 16, (h + 15) // 16
        for kind in ("span", "all255"):                                    # the box is the whole image only where the image ends on a tile edge
            g = by_kind[kind]
            if (w | h) & 15:
                assert g["has_chunk"] and g["tile_bbox"].tolist() == [0, 0, mtw, mth], (kind, g)
            else:
                assert not g["has_chunk"] and g["bitmap"].size == 0, (kind, g)
        if (w | h) & 15:
            assert int(np.unpackbits(by_kind["all255"]["bitmap"]).sum()) == mtw * mth
        zero = by_kind["zero"]
        assert zero["has_chunk"] and zero["bitmap"].size == 0 and zero["bounds"][2] < zero["bounds"][0]
        if mtw * mth > 1:
            assert by_kind["last_tile"]["has_chunk"] and by_kind["last_tile"]["bitmap"].tolist() == [1]
            assert by_kind["part_tile"]["has_chunk"] and by_kind["part_tile"]["bitmap"].tolist() == [1]
            assert by_kind["box_holes"]["has_chunk"]
        if w >= 1040:
            holes = by_kind["box_holes"]
            nbits = int(holes["tile_bbox"][2]) * int(holes["tile_bbox"][3])
            assert 0 < int(np.unpackbits(holes["bitmap"]).sum()) < nbits      # rejected tiles inside the box


def test_rgb_handles_launch_nothing(enc):
    torch = _torch()
    w, h, n = 72, 40, 3
    enc.set_batch_u8(torch.from_numpy(_frames(w, h, n, channels=3)).cuda())
    enc.encode_batch()
    got = enc.alpha_bitmaps_batch()
    for f in range(n):
        enc.select_frame(f)
        _same(got[f], {k: v for k, v in enc.alpha_result().items() if k != "remaining"}, f)
        assert not got[f]["has_chunk"] and got[f]["bounds"].tolist() == [0, 0, w, h] and got[f]["tile_bbox"].tolist() == [0, 0, 0, 0]
    assert [d["ptr"] for d in enc.alpha_bitmaps_device()] == [0] * n


def test_batch_of_one_after_mip_prefilter(enc):
    frames = _frames(72, 40, 6, first=0, seed=3)
    for f in range(6):
        enc.set_image_u8(frames[f])
        want = enc.mip_prefilter()
        (got,) = enc.alpha_bitmaps_batch()
        _same(got, {k: v for k, v in want.items() if k != "remaining"}, f)


def test_four_batches_in_a_row(enc, one):
    _check_batch(enc, one, _frames(72, 40, 7, first=0, seed=1))
    _check_batch(enc, one, _frames(72, 40, 3, first=3, seed=2))             # fewer frames
    _check_batch(enc, one, _frames(16, 16, 3, first=0, seed=3))             # then a smaller shape
    _check_batch(enc, one, _frames(16, 16, 2, first=3, seed=4))             # then other kinds in the same slots


def test_alpha_values_are_not_disturbed(enc):
    torch = _torch()
    frames = _frames(72, 40, 7, first=0, seed=5)
    frames[1, 4:30, 9:50, 3] = np.arange(26 * 41, dtype=np.uint32).reshape(26, 41).astype(np.uint8) | 4    # 8-bit analog alpha
    frames[3, 8:24, 16:48, 3] = 255                                                                        # binary
    enc.set_batch_u8(torch.from_numpy(frames).cuda())
    enc.encode_batch()
    before = enc.alpha_values_batch()
    dev_before = enc.alpha_payloads_device()
    bits = enc.alpha_bitmaps_batch()
    after_payloads = []
    for f, e in enumerate(dev_before):                                     # the payloads where they were, unchanged, without a new values call
        if e is None:
            after_payloads.append(None)
            continue
        pay = np.empty(e[3], np.uint8)
        assert lib().yk_device_download(enc._h, pay.ctypes.data, C.c_void_p(e[2]), pay.size) == 0
        after_payloads.append(pay)
    assert sum(e is not None for e in before) >= 2
    for f, e in enumerate(before):
        assert (e is None) == (after_payloads[f] is None)
        if e is not None:
            np.testing.assert_array_equal(after_payloads[f], e["payload"], err_msg=f"frame {f}")
    after = enc.alpha_values_batch()                                        # and a new values call gives the same again, the bitmaps stay
    for a, b in zip(before, after):
        assert (a is None) == (b is None)
        if a is not None:
            assert a["mode"] == b["mode"] and a["bbox"] == b["bbox"]
            np.testing.assert_array_equal(a["payload"], b["payload"])
    again = enc.alpha_bitmaps_device()
    for f, d in enumerate(again):
        got = np.zeros(d["nbytes"], np.uint8)
        if got.size:
            assert lib().yk_device_download(enc._h, got.ctypes.data, C.c_void_p(d["ptr"]), got.size) == 0
        np.testing.assert_array_equal(got, bits[f]["bitmap"])


def _refused(h, rc, code, word):
    assert rc == code, (rc, code, word)
    msg = lib().yk_last_error(h).decode()
    assert word in msg, (word, msg)


def test_refusals(enc, one):
    torch = _torch()
    L = lib()
    w, h, n = 72, 40, 3
    frames = _frames(w, h, n, first=0, seed=7)
    infos = (_MipInfoC * n)()
    dev, nb = C.c_void_p(), C.c_size_t()
    enc.set_batch_u8(torch.from_numpy(frames).cuda())
    _refused(enc._h, L.yk_alpha_bitmaps_batch(enc._h, infos), YK_ERR_STATE, "alpha stage")            # before the alpha stage has run
    _refused(enc._h, L.yk_alpha_bitmap_device(enc._h, 0, C.byref(dev), C.byref(nb)), YK_ERR_STATE, "yk_alpha_bitmaps_batch first")
    enc.encode_batch()
    _refused(enc._h, L.yk_alpha_bitmap_device(enc._h, 0, C.byref(dev), C.byref(nb)), YK_ERR_STATE, "yk_alpha_bitmaps_batch first")
    _refused(enc._h, L.yk_alpha_bitmaps_batch(enc._h, None), YK_ERR_BAD_ARG, "infos")
    assert L.yk_alpha_bitmaps_batch(enc._h, infos) == 0                      # the handle still works
    for f in (-1, n):
        _refused(enc._h, L.yk_alpha_bitmap_device(enc._h, f, C.byref(dev), C.byref(nb)), YK_ERR_BAD_ARG, "frame out of range")
        assert dev.value is None and nb.value == 0
    _refused(enc._h, L.yk_alpha_bitmap_device(enc._h, 0, None, C.byref(nb)), YK_ERR_BAD_ARG, "NULL result pointer")
    assert L.yk_alpha_bitmap_device(enc._h, 0, C.byref(dev), C.byref(nb)) == 0 and dev.value and nb.value == infos[0].nBytes > 0   # box_holes
    assert L.yk_alpha_bitmap_device(enc._h, 2, C.byref(dev), C.byref(nb)) == 0 and dev.value is None and nb.value == 0             # zero: no bits
    enc.encode_batch()                                                       # a new encode: the slots are stale
    _refused(enc._h, L.yk_alpha_bitmap_device(enc._h, 0, C.byref(dev), C.byref(nb)), YK_ERR_STATE, "yk_alpha_bitmaps_batch first")
    # a stripe: 128 owned rows + 1 halo row of a 192-row image
    planes = np.zeros((4, 129, 80), np.int32)
    planes[3, 5, 7] = 200
    enc.set_image(planes, full_h=192, y0=0, halo_rows=1)
    enc.alpha_reject()
    enc.alpha_finish(np.array([0, 0, 80, 192], np.int32))
    _refused(enc._h, L.yk_alpha_bitmaps_batch(enc._h, infos), YK_ERR_STATE, "stripe")
    fresh = HipTileEncoder(0)
    try:                                                                     # before any image
        _refused(fresh._h, L.yk_alpha_bitmaps_batch(fresh._h, infos), YK_ERR_STATE, "yk_set_image first")
    finally:
        fresh.close()
    _check_batch(enc, one, frames)                                           # and still works afterwards
