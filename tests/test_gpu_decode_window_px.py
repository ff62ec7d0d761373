"""Windows at any pixel offset and size on the GPU (yk_decode_set_window_px, yk_decode_render_windows_px_device, yk_decode_set_batch_windows_px,
DESIGN §27): every window of tests/window_px_cases.py equals ref.rgb[y0:y0 + wh, x0:x0 + ww] of the oracle's whole decode, bit for bit, through
the single-image call, the prepared image and the batch; no byte outside the window's pixels is written in any layout; an 8-aligned rectangle
gives the bytes of the aligned call; refusals come before any launch and leave the handle usable; `.yaik` files take the same path."""
import ctypes as C

import numpy as np
import pytest

from tests import batch_window_cases as BW
from tests import window_cases as WC
from tests import window_px_cases as PX
from tests.test_gpu_decode_batch_window import _alpha_entries, _decode_batch, _padded_batch
from tests.test_gpu_decode_prepared import _counts, _prepare
from tests.test_gpu_decode_prepared import _padded_batch as _padded_k
from tests.test_gpu_decode_prepared import _refs as _prepared_refs
from tests.test_gpu_decode_window import _alpha_plane, _decode, _padded, _refs

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
YK_ERR_BAD_ARG, YK_ERR_STATE, YK_STAGE_DEC_DETILE = -2, -4, 5
BIG = [c for c in WC.CASES if c[:2] != (8, 8)]


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def dec():
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def dec2():
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    yield d
    d.close()


def _np(t):
    return t.cpu().numpy()


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ---- 1: every case and window, both gradient paths -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["per_pass", "all_pass"])
@pytest.mark.parametrize("w,h,kind,win", PX.all_case_windows(), ids=_ids)
def test_px_window_equals_the_oracle_crop(dec, oracle_built, w, h, kind, win, path):
    ref, key = _refs(w, h, kind)
    dec.begin(w, h)
    dec.set_window(*win, px=True)
    assert dec.window == win and dec.window_cover == PX.cover(win)
    _decode(dec, ref, key, path)
    got = dec.image_window_device()
    assert tuple(got.shape) == (win[3], win[2], 3)
    assert np.array_equal(_np(got), ref.crop(win))
    assert np.array_equal(dec.tile4x4(), ref.tile4)                          # whole-image and exact
    cx, cy, cw, ch = PX.cover(win)                                           # the planes are exact inside the cover
    inside = np.s_[:, cy // 8:(cy + ch) // 8, cx // 8:(cx + cw) // 8]
    assert np.array_equal(WC.tiles_of(dec.planes(), w, h)[inside], WC.tiles_of(ref.planes, w, h)[inside])


# ---- 2: layouts; every byte outside the pixels keeps the sentinel ----------------------------------------------------------------------------
def _layout_windows(w, h):
    return [(3, 5, 13, 11), (w - 13, h - 11, 13, 11), (7, 7, 2, 2), (1, 1, w - 2, h - 2)]


LAYOUTS = [(3, None, False), (4, 77, False), (4, None, False), (3, None, True), (4, None, True), (4, 77, True)]   # channels, alpha (None: the plane), planar


@pytest.mark.parametrize("w,h,kind", BIG, ids=_ids)
def test_layouts_write_the_crop_and_nothing_else(dec, oracle_built, w, h, kind):
    torch = _torch()
    ref, key = _refs(w, h, kind)
    for win in _layout_windows(w, h):
        x0, y0, ww, wh = win
        dec.begin(w, h)
        dec.set_window(*win, px=True)
        alpha = _alpha_plane(dec, w, h, seed=w + h)                          # the plane stays whole; the window reads it at (x0, y0)
        _decode(dec, ref, key, "all_pass")
        rgb, a_crop = ref.crop(win), alpha[y0:y0 + wh, x0:x0 + ww]
        for channels, a_arg, planar in LAYOUTS:
            a_want = None if channels == 3 else a_crop if a_arg is None else np.full((wh, ww), a_arg, np.uint8)
            want = rgb if a_want is None else np.concatenate([rgb, a_want[..., None]], axis=2)
            exp = np.ascontiguousarray(want.transpose(2, 0, 1)) if planar else want
            buf, view, nbuf, nview = _padded(torch, exp.shape, planar, pad=11)
            assert dec.image_window_device(out=view, channels=channels, alpha=a_arg, planar=planar) is view
            assert np.array_equal(_np(view), exp), (win, channels, a_arg, planar)
            nview[...] = exp
            assert np.array_equal(_np(buf), nbuf), (win, channels, a_arg, planar, "a byte outside the pixels changed")
        with pytest.raises(ValueError, match="window"):                      # the cover's shape is not the window's
            dec.image_window_device(out=torch.empty((PX.cover(win)[3], PX.cover(win)[2], 3), dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("w,h,kind", BIG[:2], ids=_ids)
def test_prepared_and_batch_layouts_write_the_crops_and_nothing_else(dec, oracle_built, w, h, kind):
    torch = _torch()
    # K windows of a prepared image: the three 13 x 11 / 2 x 2 origins as one call per size
    ref, calls = _prepared_refs(w, h, kind)
    for (ww, wh), origins in (((13, 11), [(3, 5), (w - 13, h - 11), (8, 16)]), ((2, 2), [(7, 7), (w - 2, h - 2)]), ((w - 2, h - 2), [(1, 1), (2, 0)])):
        dec.begin(w, h)
        alpha = _alpha_plane(dec, w, h, seed=w + h)
        dec.prepare(calls, remap_range=0)
        rgb = np.stack([ref.crop((x0, y0, ww, wh)) for x0, y0 in origins])
        a_crop = np.stack([alpha[y0:y0 + wh, x0:x0 + ww] for x0, y0 in origins])
        for channels, a_arg, planar in LAYOUTS:
            a_want = None if channels == 3 else a_crop if a_arg is None else np.full(a_crop.shape, a_arg, np.uint8)
            want = rgb if a_want is None else np.concatenate([rgb, a_want[..., None]], axis=3)
            exp = np.ascontiguousarray(want.transpose(0, 3, 1, 2)) if planar else want
            buf, view, nbuf, nview = _padded_k(torch, exp.shape, planar, pad=11)
            assert dec.render_windows(origins, ww, wh, out=view, channels=channels, alpha=a_arg, planar=planar, px=True) is view
            assert np.array_equal(_np(view), exp), (ww, wh, channels, a_arg, planar)
            nview[...] = exp
            assert np.array_equal(_np(buf), nbuf), (ww, wh, channels, a_arg, planar, "a byte outside the pixels changed")
    # a batch: per-frame origins, alpha from the batch planes
    n = 3
    refs = BW.batch_references(w, h, kind, n)
    for (ww, wh), origins in (((13, 11), [(3, 5), (w - 13, h - 11), (9, 10)]), ((2, 2), [(7, 7), (w - 2, h - 2), (0, 0)]), ((w - 2, h - 2), [(1, 1), (2, 0), (0, 2)])):
        dec.begin_batch(w, h, n)
        dec.set_batch_windows(origins, ww, wh, px=True)
        dec.decompress_alpha_batch(_alpha_entries(w, h, n, seed=w + h + n), 255, sync=False)
        _decode_batch(dec, refs)
        alpha = []
        for f in range(n):
            dec.select_frame(f)
            alpha.append(dec.alpha_plane())
        rgb = BW.crops(refs, (ww, wh), origins)
        a_crop = np.stack([alpha[f][y0:y0 + wh, x0:x0 + ww] for f, (x0, y0) in enumerate(origins)])
        for channels, kw, a_want in ((3, {}, None), (4, {"alpha": 77}, np.full(a_crop.shape, 77, np.uint8)), (4, {"alpha_from_planes": True}, a_crop)):
            want = rgb if a_want is None else np.concatenate([rgb, a_want[..., None]], axis=3)
            for planar in (False, True):
                exp = torch.from_numpy(np.ascontiguousarray(want.transpose(0, 3, 1, 2)) if planar else want).cuda()
                buf, view, mask = _padded_batch(torch, n, wh, ww, channels, planar)
                assert dec.image_batch_windows_device(out=view, channels=channels, planar=planar, **kw) is view
                assert torch.equal(view, exp), (ww, wh, channels, kw, planar)
                assert (buf[~mask] == SENTINEL).all(), (ww, wh, channels, kw, planar, "a byte outside the pixels changed")


# ---- 3: an 8-aligned rectangle through each new call gives the bytes of the aligned call ----------------------------------------------------
def test_aligned_rectangles_give_the_bytes_of_the_aligned_calls(dec, dec2, oracle_built):
    torch = _torch()
    w, h, kind = 520, 264, "mixed"
    ref, key = _refs(w, h, kind)
    for win in (WC.SCAN_BLOCK_WINDOW, (0, 0, w, h), (w - 8, h - 8, 8, 8)):
        outs = []
        for d, px in ((dec, False), (dec2, True)):
            d.begin(w, h)
            d.set_window(*win, px=px)
            assert d.window == win and d.window_cover == win
            _decode(d, ref, key, "all_pass")
            outs.append(d.image_window_device(channels=4, alpha=9))
        assert torch.equal(outs[0], outs[1]) and np.array_equal(_np(outs[1])[..., :3], ref.crop(win)), win
    _, calls = _prepared_refs(w, h, kind)
    origins, (ww, wh) = [(0, 0), (192, 112), (w - 192, h - 40), (200, 120)], (192, 40)
    _prepare(dec, w, h, calls); _prepare(dec2, w, h, calls)
    a, b = dec.render_windows(origins, ww, wh), dec2.render_windows(origins, ww, wh, px=True)
    assert torch.equal(a, b) and dec.prepared_blocks == dec2.prepared_blocks
    n = 4
    refs = BW.batch_references(w, h, kind, n)
    outs = []
    for d, px in ((dec, False), (dec2, True)):
        d.begin_batch(w, h, n)
        d.set_batch_windows(origins, ww, wh, px=px)
        assert d.batch_window_covers[0].tolist() == [list(o) for o in origins] and d.batch_window_covers[1:] == (ww, wh)
        _decode_batch(d, refs)
        outs.append(d.image_batch_windows_device(channels=3, planar=True))
    assert torch.equal(outs[0], outs[1]) and np.array_equal(_np(outs[1]).transpose(0, 2, 3, 1), BW.crops(refs, (ww, wh), origins))


# ---- 4: the prepared image -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,kind", WC.CASES, ids=_ids)
def test_render_windows_px_equals_the_crops(dec, oracle_built, w, h, kind):
    ref, calls = _prepared_refs(w, h, kind)
    total = ((w + 63) // 64) * ((h + 63) // 64)
    for (ww, wh), origins in PX.origin_sets(w, h):
        _prepare(dec, w, h, calls)
        _counts(dec)
        got = dec.render_windows(origins, ww, wh, px=True)
        assert tuple(got.shape) == (len(origins), wh, ww, 3)
        assert np.array_equal(_np(got), np.stack([ref.crop((x0, y0, ww, wh)) for x0, y0 in origins])), (ww, wh)
        assert dec.prepared_blocks == (PX.touched_blocks(w, h, origins, ww, wh), total), (ww, wh)
        first = _counts(dec)
        assert first[2] == 1 and (first == (1, 1, 1) or (w, h) == (8, 8)), (ww, wh, first)   # the intervals of the aligned call
        # the same blocks again: the de-tile interval alone
        assert np.array_equal(_np(dec.render_window(*origins[-1], ww, wh, px=True)), ref.crop(origins[-1] + (ww, wh)))
        assert _counts(dec) == (0, 0, 1), (ww, wh)
        assert dec.prepared_blocks == (PX.touched_blocks(w, h, origins, ww, wh), total)
        assert np.array_equal(dec.tile4x4(), ref.tile4)
    # every window of the single-image list, one after the other, from one prepare
    _prepare(dec, w, h, calls)
    for win in PX.windows(w, h):
        assert np.array_equal(_np(dec.render_window(*win, px=True)), ref.crop(win)), win
    assert dec.prepared_blocks == (total, total)


def test_aligned_scaled_and_pixel_calls_mix_on_one_prepared_image(dec, dec2, oracle_built):
    torch = _torch()
    w, h, kind = 520, 264, "mixed"
    ref, calls = _prepared_refs(w, h, kind)
    dec2.begin(w, h)
    dec2.decode_streams(calls, remap_range=0)
    half = dec2.image_scaled_device(1)                                       # the whole decode at 1/2 size: what a scaled window is a crop of
    _prepare(dec, w, h, calls)
    _counts(dec)
    assert np.array_equal(_np(dec.render_window(67, 3, 50, 9, px=True)), ref.crop((67, 3, 50, 9)))          # block 1
    assert dec.prepared_blocks[0] == 1 and _counts(dec) == (1, 1, 1)
    assert np.array_equal(_np(dec.render_window(64, 0, 64, 64)), ref.crop((64, 0, 64, 64)))                 # aligned, the same block: only its de-tile
    assert dec.prepared_blocks[0] == 1 and _counts(dec) == (0, 0, 1)
    got = dec.render_windows_scaled(1, [(64, 0), (128, 64)], 64, 64)                                         # scaled: one block is new
    assert torch.equal(got[0], half[0:32, 32:64]) and torch.equal(got[1], half[32:64, 64:96])
    assert dec.prepared_blocks[0] == 2 and _counts(dec) == (1, 1, 1)
    assert np.array_equal(_np(dec.render_window(125, 60, 9, 9, px=True)), ref.crop((125, 60, 9, 9)))        # four blocks, two of them rendered
    assert dec.prepared_blocks[0] == 4 and _counts(dec) == (1, 1, 1)
    assert np.array_equal(_np(dec.render_window(64, 0, 128, 128)), ref.crop((64, 0, 128, 128)))             # aligned over all four: nothing new
    assert dec.prepared_blocks[0] == 4 and _counts(dec) == (0, 0, 1)


# ---- 5: batches ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,kind,n", BW.BATCHES, ids=_ids)
def test_batch_px_windows_equal_the_per_frame_crops(dec, oracle_built, w, h, kind, n):
    torch = _torch()
    refs = BW.batch_references(w, h, kind, n)
    for (ww, wh), origins in PX.origin_sets(w, h, n):
        dec.begin_batch(w, h, n)
        assert dec.batch_windows is None and dec.batch_window_covers is None
        dec.set_batch_windows(np.asarray(origins, dtype=np.int64), ww, wh, px=True)
        got_o, got_w, got_h = dec.batch_windows
        assert got_o.tolist() == [list(o) for o in origins] and (got_w, got_h) == (ww, wh)
        cov, cw, ch = dec.batch_window_covers
        assert [tuple(c) + (cw, ch) for c in cov.tolist()] == [PX.shared_cover((x0, y0, ww, wh), w, h) for x0, y0 in origins]
        dec.decompress_alpha_batch(_alpha_entries(w, h, n, seed=w + h + n), 255, sync=False)
        _decode_batch(dec, refs)
        alpha = []
        for f in range(n):
            dec.select_frame(f)
            alpha.append(dec.alpha_plane())
            assert np.array_equal(dec.tile4x4(), refs[f].tile4), f
            cx, cy = cov[f]
            inside = np.s_[:, cy // 8:(cy + ch) // 8, cx // 8:(cx + cw) // 8]     # the planes are exact inside the frame's cover
            assert np.array_equal(WC.tiles_of(dec.planes(), w, h)[inside], WC.tiles_of(refs[f].planes, w, h)[inside]), f
        rgb = BW.crops(refs, (ww, wh), origins)
        assert np.array_equal(_np(dec.image_batch_windows_device()), rgb), (ww, wh)
        a_crop = np.stack([alpha[f][y0:y0 + wh, x0:x0 + ww] for f, (x0, y0) in enumerate(origins)])
        got = dec.image_batch_windows_device(channels=4, alpha_from_planes=True)
        assert np.array_equal(_np(got), np.concatenate([rgb, a_crop[..., None]], axis=3)), (ww, wh)
        with pytest.raises(ValueError, match="windows need"):                 # the covers' shape is not the windows'
            dec.image_batch_windows_device(out=torch.empty((n, ch + 1, cw, 3), dtype=torch.uint8, device="cuda"))


def test_two_px_batches_back_to_back_read_their_own_tables(dec, oracle_built):
    w, h, kind, n = 136, 264, "mixed", 3
    refs_a, refs_b = BW.batch_references(w, h, kind, n), BW.batch_references(w, h, kind, n, second=True)
    size, o_a, o_b = (13, 11), [(3, 5), (123, 253), (61, 59)], [(70, 9), (1, 130), (122, 2)]
    dec.begin_batch(w, h, n)
    dec.set_batch_windows(o_a, *size, px=True)
    _decode_batch(dec, refs_a, sync=False)
    out_a = dec.image_batch_windows_device()                                 # queued; the next batch's table is written behind it
    dec.begin_batch(w, h, n)
    dec.set_batch_windows(o_b, *size, px=True)
    _decode_batch(dec, refs_b, sync=False)
    out_b = dec.image_batch_windows_device()
    dec.synchronize()
    assert np.array_equal(_np(out_a), BW.crops(refs_a, size, o_a))
    assert np.array_equal(_np(out_b), BW.crops(refs_b, size, o_b))
    assert not np.array_equal(_np(out_b), BW.crops(refs_b, size, o_a))
    # an aligned batch after a pixel batch, and a pixel batch after it: neither keeps the other's state
    dec.begin_batch(w, h, n)
    dec.set_batch_windows([(56, 56), (56, 120), (56, 184)], 32, 32)
    _decode_batch(dec, refs_a)
    assert np.array_equal(_np(dec.image_batch_windows_device()), BW.crops(refs_a, (32, 32), [(56, 56), (56, 120), (56, 184)]))
    dec.begin_batch(w, h, n)
    dec.set_batch_windows(o_b, *size, px=True)
    _decode_batch(dec, refs_a)
    assert np.array_equal(_np(dec.image_batch_windows_device()), BW.crops(refs_a, size, o_b))


# ---- 6: refusals -----------------------------------------------------------------------------------------------------------------------------
def _rc(fn, *args):
    return int(fn(*args))


def test_refusals_come_first_and_leave_the_handle_usable(dec, oracle_built):
    torch = _torch()
    from yaik_amd._lib import YaikError, lib
    from yaik_amd.decoder import HipTileDecoder
    L = lib()
    w, h, kind = 136, 264, "mixed"
    ref, key = _refs(w, h, kind)
    _, calls = _prepared_refs(w, h, kind)
    win = (3, 5, 13, 11)
    out = torch.full((4, 11, 13, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    bad_windows = ((130, 0, 7, 8), (0, 260, 8, 5), (0, 0, 137, 8), (0, 0, 8, 265), (136, 0, 1, 1), (0, 264, 1, 1),        # outside the image
                   (0, 0, 0, 8), (0, 0, 8, 0), (0, 0, -3, -3), (0, 0, -8, 8),                                              # ww, wh < 1
                   (-1, 0, 8, 8), (0, -1, 8, 8), (-8, -8, 8, 8), (2 ** 31 - 8, 0, 16, 8))                                  # negative origin, overflow
    xy2 = lambda x0, y0: (C.c_int * 2)(x0, y0)
    fresh = HipTileDecoder(0)
    try:
        # the wrong kind of handle, and the wrong moment
        assert _rc(L.yk_decode_set_window_px, fresh._h, *win) == YK_ERR_STATE                  # before any begin
        assert b"yk_decode_set_window_px" in L.yk_last_error(fresh._h)
        assert _rc(L.yk_decode_set_batch_windows_px, fresh._h, xy2(3, 5), 13, 11) == YK_ERR_STATE
        assert b"yk_decode_set_batch_windows_px" in L.yk_last_error(fresh._h)
        assert _rc(L.yk_decode_render_windows_px_device, fresh._h, 1, xy2(3, 5), 13, 11, out.data_ptr(), 39, 0, 0, 3, 0) == YK_ERR_STATE
        assert b"yk_decode_render_windows_px_device" in L.yk_last_error(fresh._h)
        fresh.begin_batch(w, h, 1)
        assert _rc(L.yk_decode_set_window_px, fresh._h, *win) == YK_ERR_STATE                  # a batch, even of one frame
        assert b"yk_decode_set_window_px" in L.yk_last_error(fresh._h) and b"batch" in L.yk_last_error(fresh._h)
        fresh.begin(w, h)
        assert _rc(L.yk_decode_set_batch_windows_px, fresh._h, xy2(3, 5), 13, 11) == YK_ERR_STATE      # a single image
        assert _rc(L.yk_decode_render_windows_px_device, fresh._h, 1, xy2(3, 5), 13, 11, out.data_ptr(), 39, 0, 0, 3, 0) == YK_ERR_STATE   # not prepared
        with pytest.raises(YaikError, match="yk_decode_set_batch_windows_px"):
            fresh.set_batch_windows([(3, 5)], 13, 11, px=True)
        assert fresh.batch_windows is None
    finally:
        fresh.close()
    # a single image: bad rectangles, then too late
    dec.begin(w, h)
    for bad in bad_windows:
        assert _rc(L.yk_decode_set_window_px, dec._h, *bad) == YK_ERR_BAD_ARG, bad
        assert b"yk_decode_set_window_px" in L.yk_last_error(dec._h)
    dec.set_window(*win, px=True)
    dec.set_window(0, 0, 0, 0, px=True)                                      # ww == wh == 0 clears
    assert dec.window is None
    dec.set_window(*win, px=True)
    dec.begin(w, h)                                                          # begin clears
    assert dec.window is None
    _decode(dec, ref, key, "per_pass")
    assert np.array_equal(_np(dec.image_device()), ref.rgb)                  # no window survived: the whole-image call works
    for args in (win, (0, 0, 0, 0)):
        assert _rc(L.yk_decode_set_window_px, dec._h, *args) == YK_ERR_STATE                   # after a chunk was decoded
        assert b"yk_decode_set_window_px" in L.yk_last_error(dec._h) and b"chunk" in L.yk_last_error(dec._h)
    assert np.array_equal(_np(dec.image_device()), ref.rgb)
    # outputs under a pixel window
    dec.begin(w, h)
    dec.set_window(*win, px=True)
    _decode(dec, ref, key, "all_pass")
    for level in (1, 2, 3):
        with pytest.raises(YaikError, match="pixel window") as e:
            dec.image_scaled_device(level)
        assert f"error {YK_ERR_STATE}" in str(e.value) and "yk_decode_output_scaled_device" in str(e.value)
    with pytest.raises(YaikError, match="window"):
        dec.image_device()
    assert _rc(L.yk_decode_output_window_device, dec._h, out.data_ptr(), 13 * 3 - 1, 0, 3, 0) == YK_ERR_BAD_ARG          # the pitch check is against ww x wh
    assert _rc(L.yk_decode_output_window_device, dec._h, out.data_ptr(), 13, 13 * 11 - 1, 3, 0) == YK_ERR_BAD_ARG
    assert (out == SENTINEL).all()
    assert np.array_equal(_np(dec.image_scaled_device(0)), ref.crop(win))    # level 0 is the full-size window
    assert np.array_equal(_np(dec.image_window_device()), ref.crop(win))
    # a prepared image
    _prepare(dec, w, h, calls)
    before = dec.prepared_blocks
    for bad in bad_windows:
        assert _rc(L.yk_decode_render_windows_px_device, dec._h, 1, xy2(*bad[:2]), bad[2], bad[3], out.data_ptr(), 4096, 0, 0, 3, 0) == YK_ERR_BAD_ARG, bad
        assert b"yk_decode_render_windows_px_device" in L.yk_last_error(dec._h)
    for args in ((1, None, 13, 11, out.data_ptr(), 39, 0, 0, 3, 0), (0, xy2(3, 5), 13, 11, out.data_ptr(), 39, 0, 0, 3, 0), (1, xy2(3, 5), 13, 11, None, 39, 0, 0, 3, 0),
                 (1, xy2(3, 5), 13, 11, out.data_ptr(), 38, 0, 0, 3, 0), (1, xy2(3, 5), 13, 11, out.data_ptr(), 39, 0, 0, 5, 0),
                 ((2, (C.c_int * 4)(3, 5, 9, 10), 13, 11, out.data_ptr(), 39, 0, 39 * 11 - 1, 3, 0))):
        assert _rc(L.yk_decode_render_windows_px_device, dec._h, *args) == YK_ERR_BAD_ARG, args
        assert b"yk_decode_render_windows_px_device" in L.yk_last_error(dec._h)
    assert _rc(L.yk_decode_render_windows_px_device, dec._h, 1, xy2(3, 5), 13, 11, out.data_ptr(), 39 * 4, 0, 0, 4, -1) == YK_ERR_STATE   # no 'ALPM' plane
    assert _rc(L.yk_decode_set_window_px, dec._h, *win) == YK_ERR_STATE      # a prepared image takes no window
    assert dec.prepared_blocks == before and (out == SENTINEL).all()         # nothing was rendered, nothing written
    assert np.array_equal(_np(dec.render_window(*win, px=True)), ref.crop(win))
    # a batch
    n = 3
    refs = BW.batch_references(w, h, kind, n)
    origins = [(3, 5), (123, 253), (61, 59)]
    tab = lambda o: (C.c_int * (2 * len(o)))(*[v for p in o for v in p])
    dec.begin_batch(w, h, n)
    for bad in bad_windows:
        assert _rc(L.yk_decode_set_batch_windows_px, dec._h, tab(origins[:2] + [bad[:2]]), bad[2], bad[3]) == YK_ERR_BAD_ARG, bad
        assert b"yk_decode_set_batch_windows_px" in L.yk_last_error(dec._h)
    assert _rc(L.yk_decode_set_batch_windows_px, dec._h, None, 13, 11) == YK_ERR_BAD_ARG                                  # NULL table
    assert b"yk_decode_set_batch_windows_px" in L.yk_last_error(dec._h)
    dec.set_batch_windows(origins, 13, 11, px=True)
    assert _rc(L.yk_decode_set_batch_windows_px, dec._h, tab(origins[:2] + [(130, 0)]), 13, 11) == YK_ERR_BAD_ARG
    assert _rc(L.yk_decode_output_batch_windows_device, dec._h, out.data_ptr(), 39, 0, 39 * 11, 3, 0) == YK_ERR_STATE     # the refused set left no windows
    dec.set_batch_windows(origins, 13, 11, px=True)
    _decode_batch(dec, refs)
    assert _rc(L.yk_decode_set_batch_windows_px, dec._h, tab(origins), 13, 11) == YK_ERR_STATE                            # after a chunk was decoded
    assert b"yk_decode_set_batch_windows_px" in L.yk_last_error(dec._h) and b"chunk" in L.yk_last_error(dec._h)
    assert _rc(L.yk_decode_output_batch_windows_device, dec._h, out.data_ptr(), 38, 0, 39 * 11, 3, 0) == YK_ERR_BAD_ARG   # pitch checks against ww x wh
    assert _rc(L.yk_decode_output_batch_windows_device, dec._h, out.data_ptr(), 39, 0, 39 * 11 - 1, 3, 0) == YK_ERR_BAD_ARG
    assert (out == SENTINEL).all()
    with pytest.raises(YaikError, match="windows"):
        dec.image_batch_device()
    assert np.array_equal(_np(dec.image_batch_windows_device()), BW.crops(refs, (13, 11), origins))


# ---- 7: one de-tile interval per output call -------------------------------------------------------------------------------------------------
def test_one_detile_interval_per_output_call(dec, oracle_built):
    w, h, kind = 136, 264, "mixed"
    ref, key = _refs(w, h, kind)
    dec.begin(w, h)
    dec.set_window(61, 59, 7, 9, px=True)
    _decode(dec, ref, key, "all_pass")
    dec.synchronize()
    dec.stage_ms(YK_STAGE_DEC_DETILE)                                        # fold what earlier tests left
    for n in (1, 3):
        for _ in range(n):
            dec.image_window_device()
        dec.synchronize()
        ms, calls = dec.stage_ms(YK_STAGE_DEC_DETILE)
        assert calls == n and ms > 0
    refs = BW.batch_references(w, h, kind, 3)
    dec.begin_batch(w, h, 3)
    dec.set_batch_windows([(3, 5), (123, 253), (61, 59)], 13, 11, px=True)
    _decode_batch(dec, refs)
    dec.stage_ms(YK_STAGE_DEC_DETILE)
    for _ in range(2):
        dec.image_batch_windows_device()
    dec.synchronize()
    assert dec.stage_ms(YK_STAGE_DEC_DETILE)[1] == 2


# ---- 8: .yaik files --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files():
    from yaik_amd import files as F
    F.set_device_palette(False)
    yield F
    F.set_device_palette(False)


@pytest.fixture(scope="module")
def file_streams(files):
    """three streams of 136 x 264 "mixed" frames with an 'ALPM' chunk, and the first frame's stream without one"""
    torch = _torch()
    from tests.images import edge_image
    w, h = 136, 264
    frames = [edge_image(w, h, "mixed", 4, seed=BW.frame_seed(w, h, f)) for f in range(3)]
    hwc = torch.from_numpy(np.stack([np.ascontiguousarray(p.transpose(1, 2, 0)).astype(np.uint8) for p in frames])).cuda()
    rgba = files.encode_files_device(hwc, emit_alpha=True)
    rgb = files.encode_file_device(hwc[0, ..., :3].contiguous())
    assert all(files.has_alpha_chunk(s) for s in rgba) and not files.has_alpha_chunk(rgb)
    return rgb, rgba


def test_file_px_windows_equal_the_crops_of_the_whole_file_decode(files, file_streams):
    torch = _torch()
    w, h = 136, 264
    rgb, rgba = file_streams
    for stream, c in ((rgb, 3), (rgba[0], 4)):
        whole = files.decode_file_device(stream)
        assert tuple(whole.shape) == (h, w, c)
        for win in PX.windows(w, h):                                          # one window
            x0, y0, ww, wh = win
            got = files.decode_file_window_device(stream, win, px=True)
            assert tuple(got.shape) == (wh, ww, c) and torch.equal(got, whole[y0:y0 + wh, x0:x0 + ww]), (c, win)
        for (ww, wh), origins in PX.origin_sets(w, h):                        # K windows
            got = files.decode_file_windows_device(stream, origins, ww, wh, px=True)
            assert files.last_windows_prepared()
            assert torch.equal(got, torch.stack([whole[y0:y0 + wh, x0:x0 + ww] for x0, y0 in origins])), (c, ww, wh)
        assert torch.equal(files.decode_file_device(stream), whole)           # the slot's handle goes back to whole images
    whole = files.decode_files_device(rgba, channels=4)                       # a batch of files
    for (ww, wh), origins in PX.origin_sets(w, h, 3):
        want = torch.stack([whole[f, y0:y0 + wh, x0:x0 + ww] for f, (x0, y0) in enumerate(origins)])
        for channels in (3, 4):
            got = files.decode_files_windows_device(rgba, origins, (ww, wh), channels=channels, px=True)
            assert files.last_batch_info()["fallbacks"] == 0
            assert torch.equal(got, want[..., :channels]), (ww, wh, channels)
    from yaik_amd.files import ERROR_NAMES, YaikFileError
    for call in (lambda: files.decode_file_window_device(rgb, (130, 0, 7, 8), px=True), lambda: files.decode_file_windows_device(rgb, [(0, 260)], 8, 5, px=True),
                 lambda: files.decode_files_windows_device(rgba, [(0, 0), (124, 0), (0, 0)], (13, 11), px=True)):
        with pytest.raises(YaikFileError) as e:
            call()
        assert ERROR_NAMES[e.value.code] == "YAIK_DECIMG_INVALIDCTX"
    assert files.decode_file_window_device(rgb, (3, 5, 13, 11), px=True).shape == (11, 13, 3)      # the slot was released each time
