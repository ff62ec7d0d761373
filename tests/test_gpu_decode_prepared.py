"""Many windows of one image on the GPU (yk_decode_prepare_device / yk_decode_render_windows_device): after one prepare every window
equals the crop of the whole decode, bit for bit -- against the oracle's whole decode on the images and windows of tests/window_cases.py and
tests/prepared_cases.py, against a whole GPU decode on encoder streams at 1024 x 1024 and on .yaik files; a 64x64 block is rendered once (the
stage intervals show the skipped work), blocks no window asked for are not written, inputs may go after prepare, and every call that does not
fit a prepared image refuses and leaves the handle usable."""
import ctypes as C

import numpy as np
import pytest

from tests import prepared_cases as PC
from tests import window_cases as WC

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
YK_ERR_BAD_ARG, YK_ERR_HIP, YK_ERR_STATE = -2, -3, -4
YK_STAGE_DEC_GRADIENT, YK_STAGE_DEC_1D, YK_STAGE_DEC_DETILE = 3, 4, 5
STAGES = (YK_STAGE_DEC_GRADIENT, YK_STAGE_DEC_1D, YK_STAGE_DEC_DETILE)


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


def _upload(ref):
    """the oracle's streams of `ref` in device memory: (tensors to keep alive, the call list of decode_streams / prepare)"""
    torch = _torch()
    keep, calls = [], []
    for sx, sy, cnt, bm, rgb in ref.passes:
        if cnt:
            tb = torch.from_numpy(np.ascontiguousarray(bm)).cuda()
            tr = torch.from_numpy(np.concatenate([rgb, np.zeros(1, np.uint8)])).cuda()
            keep += [tb, tr]
            calls.append(("g", sx, sy, tb.data_ptr(), bm.size, tr.data_ptr(), rgb.size))
    tt, tp = torch.from_numpy(np.ascontiguousarray(ref.typ)).cuda(), torch.from_numpy(np.ascontiguousarray(ref.pix)).cuda()
    keep += [tt, tp]
    calls.append(("1", tt.data_ptr(), ref.typ.size, tp.data_ptr(), ref.pix.size))
    torch.cuda.synchronize()
    return keep, calls


_DEVICE_STREAMS = {}


def _refs(w, h, kind, second=False):
    """the oracle's reference of an image and its streams in device memory (uploaded once per image, kept alive here)"""
    key = (w, h, kind, second)
    ref = WC.reference(w, h, kind, second)
    if key not in _DEVICE_STREAMS:
        _DEVICE_STREAMS[key] = _upload(ref)
    return ref, _DEVICE_STREAMS[key][1]


def _prepare(d, w, h, calls):
    d.begin(w, h)
    d.prepare(calls, remap_range=0)


def _counts(d):
    """the intervals of the three decode stages since the last look (synchronises)"""
    d.synchronize()
    return tuple(d.stage_ms(s)[1] for s in STAGES)


def _np(t):
    return t.cpu().numpy()


# ---- 1 + 3: every window from one prepare, in both orders; repeats only de-tile --------------------------------------------------------------
@pytest.mark.parametrize("order", ["listed", "reversed"])
@pytest.mark.parametrize("w,h,kind", WC.CASES, ids=lambda v: str(v))
def test_every_window_from_one_prepare(dec, dec2, oracle_built, w, h, kind, order):
    ref, calls = _refs(w, h, kind)
    wins = PC.case_windows(w, h)
    if order == "reversed":                                                  # on another handle: overlapping windows then meet rendered and
        wins, dec = wins[::-1], dec2                                         # unrendered blocks in another mix
    _prepare(dec, w, h, calls)
    total = ((w + 63) // 64) * ((h + 63) // 64)
    assert dec.prepared_blocks == (0, total)
    assert np.array_equal(dec.tile4x4(), ref.tile4)                          # the marks are whole before any pixel exists
    rendered = 0
    for win in wins:
        got = dec.render_window(*win)
        assert tuple(got.shape) == (win[3], win[2], 3)
        assert np.array_equal(_np(got), ref.crop(win)), win
        now, tot = dec.prepared_blocks
        assert tot == total and rendered <= now <= total
        rendered = now
    assert rendered == total                                                 # (0, 0, w, h) is one of the windows
    assert np.array_equal(dec.tile4x4(), ref.tile4)                          # no render changed a mark
    assert np.array_equal(dec.planes(), ref.planes)
    # every block is rendered: a repeated window costs its de-tile and nothing else
    _counts(dec)
    for win in wins:
        assert np.array_equal(_np(dec.render_window(*win)), ref.crop(win)), win
        assert _counts(dec) == (0, 0, 1), win
        assert dec.prepared_blocks == (total, total)


def test_a_window_with_one_new_block_renders_one_block(dec, oracle_built):
    w, h, kind = 520, 264, "mixed"
    ref, calls = _refs(w, h, kind)
    dec.begin(w, h)
    _counts(dec)                                                             # fold what earlier tests left
    dec.prepare(calls, remap_range=0)
    assert _counts(dec) == (1, 1, 0)                                         # prepare: one gradient and one 1-D interval, no de-tile
    for win, blocks, want in (((0, 0, 8, 8), 1, (1, 1, 1)), ((8, 8, 56, 56), 1, (0, 0, 1)), ((56, 0, 16, 8), 2, (1, 1, 1)), ((0, 0, 128, 64), 2, (0, 0, 1)),
                              ((512, 256, 8, 8), 3, (1, 1, 1)), ((0, 0, 128, 72), 5, (1, 1, 1))):
        assert np.array_equal(_np(dec.render_window(*win)), ref.crop(win)), win
        assert dec.prepared_blocks == (blocks, 45), win
        assert _counts(dec) == want, win


# ---- 2: one call for K windows equals the loop -----------------------------------------------------------------------------------------------
def _alpha_plane(d, w, h, seed):
    """an 8-bit 'ALPM' plane decoded on d (mode 6, a box that leaves the first 8 rows and columns out); returns the plane [h, w] as the library holds it"""
    rng = np.random.default_rng(seed)
    return d.decompress_alpha(6, (8, 8, w - 8, h - 8), rng.integers(1, 256, (w - 8) * (h - 8)).astype(np.uint8))


def _padded_batch(torch, shape, planar, pad):
    """a sentinel-filled buffer and a [K, ...] view of it with row, plane and window padding, at an odd offset; returns buf, view and the same pair in numpy"""
    if planar:
        k, c, hh, ww = shape
        row, off = ww + pad, 3
        plane = row * hh + 13
        frame = c * plane + 29
        strides = (frame, plane, row, 1)
    else:
        k, hh, ww, c = shape
        row, off = ww * c + pad, 5
        frame = row * hh + 29
        strides = (frame, row, c, 1)
    n = off + k * frame + 64
    buf = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, shape, strides, off)
    nbuf = np.full(n, SENTINEL, np.uint8)
    nview = np.lib.stride_tricks.as_strided(nbuf[off:], shape, strides)
    return buf, view, nbuf, nview


def test_one_call_for_k_windows_equals_the_loop(dec, dec2, oracle_built):
    torch = _torch()
    w, h, kind = 520, 264, "mixed"
    ref, calls = _refs(w, h, kind)
    ww, wh = PC.K8_SIZE
    origins = PC.K8_ORIGINS
    K = len(origins)
    want_rgb = np.stack([ref.crop((x0, y0, ww, wh)) for x0, y0 in origins])
    # the one call renders every block its windows need, once ...
    dec.begin(w, h)
    alpha = _alpha_plane(dec, w, h, seed=w + h)                              # legal before prepare; the plane stays whole
    dec.prepare(calls, remap_range=0)
    _counts(dec)
    first = dec.render_windows(origins, ww, wh, channels=3)
    assert tuple(first.shape) == (K, wh, ww, 3) and np.array_equal(_np(first), want_rgb)
    assert _counts(dec) == (1, 1, 1)
    assert dec.prepared_blocks == (int(PC.block_mask(w, h, origins, ww, wh).sum()), 45)
    # ... the loop on another handle meets rendered and unrendered blocks window after window
    _prepare(dec2, w, h, calls)
    for k, (x0, y0) in enumerate(origins):
        assert torch.equal(dec2.render_window(x0, y0, ww, wh), first[k]), (x0, y0)
    assert dec2.prepared_blocks == dec.prepared_blocks
    a_crop = np.stack([alpha[y0:y0 + wh, x0:x0 + ww] for x0, y0 in origins])
    assert a_crop.any()
    for channels, a_arg, a_want in ((3, None, None), (4, None, a_crop), (4, 77, np.full((K, wh, ww), 77, np.uint8)), (None, None, a_crop)):
        want = want_rgb if a_want is None else np.concatenate([want_rgb, a_want[..., None]], axis=3)
        for planar in (False, True):
            exp = np.ascontiguousarray(want.transpose(0, 3, 1, 2)) if planar else want
            got = dec.render_windows(origins, ww, wh, channels=channels, alpha=a_arg, planar=planar)
            assert np.array_equal(_np(got), exp), (channels, a_arg, planar)
            buf, view, nbuf, nview = _padded_batch(torch, exp.shape, planar, pad=11)
            out = dec.render_windows(origins, ww, wh, out=view, channels=channels, alpha=a_arg, planar=planar)
            assert out is view
            nview[...] = exp
            assert np.array_equal(_np(buf), nbuf), (channels, a_arg, planar)   # nothing outside the pixel bytes changed
            one = dec.render_window(*origins[3], ww, wh, channels=channels, alpha=a_arg, planar=planar)
            assert np.array_equal(_np(one), exp[3]), (channels, a_arg, planar)
    assert _counts(dec)[:2] == (0, 0)                                        # all of that was de-tiling
    with pytest.raises(ValueError, match="window"):
        dec.render_windows(origins, ww, wh, out=torch.empty((K - 1, wh, ww, 3), dtype=torch.uint8, device="cuda"))
    # an 'ALPM' plane decoded after prepare is read as well
    alpha2 = _alpha_plane(dec, w, h, seed=7)
    got = _np(dec.render_windows(origins[:2], ww, wh))
    assert np.array_equal(got[..., 3], np.stack([alpha2[y0:y0 + wh, x0:x0 + ww] for x0, y0 in origins[:2]])) and np.array_equal(got[..., :3], want_rgb[:2])


# ---- 4: blocks no window asked for are not written -------------------------------------------------------------------------------------------
def test_blocks_no_window_asked_for_keep_the_previous_image(dec, oracle_built):
    w, h, kind = 520, 264, "mixed"
    ref_a, calls_a = _refs(w, h, kind)
    ref_b, calls_b = _refs(w, h, kind, second=True)
    dec.begin(w, h)
    dec.decode_streams(calls_a, remap_range=0)
    assert np.array_equal(dec.planes(), ref_a.planes)
    _prepare(dec, w, h, calls_b)
    a, b = WC.tiles_of(ref_a.planes, w, h), WC.tiles_of(ref_b.planes, w, h)
    assert np.array_equal(dec.planes(), ref_a.planes), "prepare wrote a plane byte"
    wins = [WC.SCAN_BLOCK_WINDOW, (512, 256, 8, 8)]
    mask = np.zeros((5, 9), dtype=bool)
    for win in wins:
        assert np.array_equal(_np(dec.render_window(*win)), ref_b.crop(win))
        mask |= PC.block_mask(w, h, [win[:2]], win[2], win[3])
    assert dec.prepared_blocks == (int(mask.sum()), 45)
    inside = PC.tiles_in_blocks(w, h, mask)
    got = WC.tiles_of(dec.planes(), w, h)
    assert np.array_equal(got[:, inside], b[:, inside])
    assert np.array_equal(got[:, ~inside], a[:, ~inside]), "a tile outside the rendered 64-blocks was written"
    assert (a[:, ~inside] != b[:, ~inside]).any()                            # ... and the two images differ there, so a write would show
    for win in wins:                                                         # the rendered blocks are the windows rounded out to 64, no more
        assert (~WC.outside_rounded(w, h, win) <= inside).all()
    assert np.array_equal(inside, ~(WC.outside_rounded(w, h, wins[0]) & WC.outside_rounded(w, h, wins[1])))
    assert np.array_equal(_np(dec.render_window(0, 0, w, h)), ref_b.rgb)
    assert np.array_equal(dec.planes(), ref_b.planes)
    assert dec.prepared_blocks == (45, 45)
    assert np.array_equal(dec.tile4x4(), ref_b.tile4)


# ---- 5: no stale state -----------------------------------------------------------------------------------------------------------------------
def test_no_state_of_the_previous_image_survives(dec, oracle_built):
    w, h, kind = 520, 264, "mixed"
    ref_a, calls_a = _refs(w, h, kind)
    ref_b, calls_b = _refs(w, h, kind, second=True)
    win = PC.SCAN_BLOCK_BLOCK
    _prepare(dec, w, h, calls_b)
    assert np.array_equal(_np(dec.render_window(*win)), ref_b.crop(win))
    _prepare(dec, w, h, calls_a)
    assert dec.prepared_blocks == (0, 45)
    assert np.array_equal(_np(dec.render_window(*win)), ref_a.crop(win))     # rendered again, from A's lattice and streams
    assert dec.prepared_blocks == (1, 45)
    for ref, calls, prepared in ((ref_a, calls_a, False), (ref_b, calls_b, True), (ref_a, calls_a, False)):
        dec.begin(w, h)
        if prepared:
            dec.prepare(calls, remap_range=0)
            assert np.array_equal(_np(dec.render_window(0, 0, w, h)), ref.rgb)
        else:
            dec.decode_streams(calls, remap_range=0)
            assert np.array_equal(_np(dec.image_device()), ref.rgb)
        assert np.array_equal(dec.planes(), ref.planes) and np.array_equal(dec.tile4x4(), ref.tile4)


# ---- 6: the inputs may go after prepare ------------------------------------------------------------------------------------------------------
def test_inputs_are_released_by_prepare(dec, oracle_built):
    w, h, kind = 136, 264, "mixed"
    ref = WC.reference(w, h, kind)
    keep, calls = _upload(ref)                                               # this test's own copies
    dec.begin(w, h)
    dec.prepare(calls, remap_range=0, sync=True)
    for t in keep:
        t.fill_(SENTINEL)
    _torch().cuda.synchronize()
    for win in PC.case_windows(w, h)[::-1]:
        assert np.array_equal(_np(dec.render_window(*win)), ref.crop(win)), win
    assert np.array_equal(dec.planes(), ref.planes)


# ---- 7: an image without a 1-D chunk ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,kind", [(520, 264, "mixed"), (136, 264, "mixed")])
def test_no_1d_chunk(dec, dec2, oracle_built, w, h, kind):
    ref_a, calls_a = _refs(w, h, kind)
    ref_b, calls_b = _refs(w, h, kind, second=True)
    grads = [c for c in calls_b if c[0] == "g"]
    dec2.begin(w, h)
    dec2.decode_streams(grads, remap_range=0)
    whole = _np(dec2.image_device())                                         # B's gradient tiles, zeros elsewhere
    dec.begin(w, h)
    dec.decode_streams(calls_a, remap_range=0)                               # the planes hold image A: zeros have to be written, not found
    dec.begin(w, h)
    dec.prepare(grads, remap_range=0)
    _counts(dec)
    for k, win in enumerate(PC.case_windows(w, h)[::-1]):
        x0, y0, ww, wh = win
        assert np.array_equal(_np(dec.render_window(*win)), whole[y0:y0 + wh, x0:x0 + ww]), win
        if k == 0:
            assert _counts(dec) == (1, 0, 1)                                 # no 1-D interval without 1-D streams
    assert (whole == 0).all(axis=2).any() and whole.any()
    assert np.array_equal(dec.tile4x4(), ref_b.tile4)


# ---- 8: encoder streams at 1024 x 1024 -------------------------------------------------------------------------------------------------------
def test_encoder_streams_1024_sixteen_windows_in_one_call(dec, dec2):
    torch = _torch()
    from yaik_amd.encoder import HipTileEncoder
    from yaik_amd.synth import synth_planes
    n = 1024
    enc = HipTileEncoder(0)
    try:
        enc.set_image(synth_planes(n, n_planes=3))
        enc.encode(3, False, False)
        dec2.begin(n, n)
        dec2.decode_from_encoder(enc)
        whole, want4 = dec2.image_device(), dec2.tile4x4()
        rng = np.random.default_rng(1024)
        ww, wh = 136, 72
        origins = [(int(rng.integers(0, (n - ww) // 8 + 1)) * 8, int(rng.integers(0, (n - wh) // 8 + 1)) * 8) for _ in range(16)]
        dec.begin(n, n)
        dec.prepare_from_encoder(enc)
        got = dec.render_windows(origins, ww, wh)
        for k, (x0, y0) in enumerate(origins):
            assert torch.equal(got[k], whole[y0:y0 + wh, x0:x0 + ww]), (x0, y0)
        assert dec.prepared_blocks == (int(PC.block_mask(n, n, origins, ww, wh).sum()), 256)
        assert np.array_equal(dec.tile4x4(), want4)
        assert torch.equal(dec.render_window(0, 0, n, n), whole)
    finally:
        dec.synchronize(); dec2.synchronize()
        enc.close()


# ---- 9: refusals leave the handle usable -----------------------------------------------------------------------------------------------------
def _rc(fn, *args):
    return int(fn(*args))


def _raw_prepare(L, d, calls, repeat_first=0):
    g = [c for c in calls if c[0] == "g"]
    g = g + [g[0]] * repeat_first
    d1 = [c for c in calls if c[0] == "1"][0]
    n = len(g)
    return _rc(L.yk_decode_prepare_device, d._h, n, (C.c_int * n)(*[c[1] for c in g]), (C.c_int * n)(*[c[2] for c in g]), (C.c_void_p * n)(*[c[3] for c in g]),
               (C.c_size_t * n)(*[c[4] for c in g]), (C.c_void_p * n)(*[c[5] for c in g]), (C.c_size_t * n)(*[c[6] for c in g]), 0, d1[1], d1[2], d1[3], d1[4], 15)


def test_refusals_leave_the_handle_usable(dec, oracle_built):
    torch = _torch()
    from yaik_amd._lib import YaikError, lib
    from yaik_amd.decoder import HipTileDecoder
    L = lib()
    w, h, kind = 136, 264, "mixed"
    ref, calls = _refs(w, h, kind)
    grads = [c for c in calls if c[0] == "g"]
    win = (56, 56, 24, 16)
    out = torch.empty((2, 16, 24, 3), dtype=torch.uint8, device="cuda")
    xy = (C.c_int * 4)(56, 56, 0, 0)
    render = lambda d, n=1, xy=xy, ww=24, wh=16, row=72, wb=72 * 16: _rc(L.yk_decode_render_windows_device, d._h, n, xy, ww, wh, out.data_ptr(), row, 0, wb, 3, 0)
    r, t = C.c_int(), C.c_int()
    blocks = lambda d: _rc(L.yk_decode_prepared_blocks, d._h, C.byref(r), C.byref(t))

    def usable(d):
        _prepare(d, w, h, calls)
        assert np.array_equal(_np(d.render_window(*win)), ref.crop(win))

    fresh = HipTileDecoder(0)
    try:
        assert render(fresh) == YK_ERR_STATE and blocks(fresh) == YK_ERR_STATE       # before any begin
        assert _raw_prepare(L, fresh, calls) == YK_ERR_STATE
        assert b"yk_decode_begin" in L.yk_last_error(fresh._h)
        for frames in (2, 1):
            fresh.begin_batch(w, h, frames)
            assert _raw_prepare(L, fresh, calls) == YK_ERR_STATE                     # a batch, of one frame as well
            assert b"batch" in L.yk_last_error(fresh._h)
        usable(fresh)
    finally:
        fresh.close()
    dec.begin(w, h)
    assert render(dec) == YK_ERR_STATE and blocks(dec) == YK_ERR_STATE               # begun, not prepared
    assert b"yk_decode_prepare_device" in L.yk_last_error(dec._h)
    dec.set_window(0, 0, 8, 8)
    assert _raw_prepare(L, dec, calls) == YK_ERR_STATE                               # under a window
    assert b"window" in L.yk_last_error(dec._h)
    dec.begin(w, h)
    dec.decode_streams(grads, remap_range=0)
    assert _raw_prepare(L, dec, calls) == YK_ERR_STATE                               # after a chunk
    assert b"chunk" in L.yk_last_error(dec._h)
    dec.begin(w, h)
    assert _raw_prepare(L, dec, calls, repeat_first=8 - len(grads)) == YK_ERR_BAD_ARG   # an eighth pass
    assert b"yk_decode_set_window" in L.yk_last_error(dec._h)
    assert _raw_prepare(L, dec, calls) == 0                                          # ... and the refusal changed nothing: the image is still fresh
    assert _raw_prepare(L, dec, calls) == YK_ERR_STATE                               # twice
    assert b"prepared already" in L.yk_last_error(dec._h)
    # while prepared: no further chunk, no window, no whole-image call
    src = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    first = [c for c in ref.passes if c[2]][0]
    for call in (lambda: dec.decode_streams(calls, remap_range=0), lambda: dec.decode_streams(grads, per_pass=True, remap_range=0),
                 lambda: dec.decode_streams(calls[-1:]), lambda: dec.decompress_gradient(first[0], first[1], first[3], first[4]),
                 lambda: dec.decompress_1d(ref.typ, ref.pix), lambda: dec.set_window(0, 0, 8, 8), lambda: dec.image_device(), lambda: dec.image(),
                 lambda: dec.image_window_device(), lambda: dec.compare_device(src)):
        with pytest.raises(YaikError, match="yk_decode_render_windows_device") as e:
            call()
        assert f"error {YK_ERR_STATE}" in str(e.value)
    assert L.yk_decode_split_masks(dec._h) == YK_ERR_STATE
    one = np.zeros(16, dtype=np.uint8)                                               # refused before the palette decode looks at the payload
    assert _rc(L.yk_decode_gradient_palette, dec._h, 2, 2, one.ctypes.data, one.size, one.ctypes.data, one.size, 3, 1) == YK_ERR_STATE
    assert b"yk_decode_gradient_palette" in L.yk_last_error(dec._h) and b"prepared" in L.yk_last_error(dec._h)
    assert dec.window is None
    # bad windows: nothing is queued, no block changes hands
    assert np.array_equal(_np(dec.render_window(*win)), ref.crop(win))
    before = dec.prepared_blocks
    _counts(dec)
    for n, o, ww, wh in ((1, (4, 0), 8, 8), (1, (0, 4), 8, 8), (1, (0, 0), 12, 8), (1, (0, 0), 8, 12), (1, (0, 0), 0, 0), (1, (-8, 0), 8, 8), (1, (136, 0), 8, 8),
                         (1, (0, 264), 8, 8), (1, (120, 0), 24, 16), (1, (0, 256), 24, 16), (1, (0, 0), 144, 8), (1, (2 ** 31 - 8, 0), 16, 8), (2, (0, 0, 0, 260), 8, 8),
                         (0, (0, 0), 8, 8), (1025, (0, 0), 8, 8), (-1, (0, 0), 8, 8)):
        bad = (C.c_int * max(len(o), 2 * 1025))(*o)
        assert render(dec, n, bad, ww, wh, max(ww, 1) * 3, max(ww, 1) * 3 * max(wh, 1)) == YK_ERR_BAD_ARG, (n, o, ww, wh)
    assert b"window" in L.yk_last_error(dec._h).lower() or b"nWindows" in L.yk_last_error(dec._h)
    assert render(dec, 1, None) == YK_ERR_BAD_ARG
    assert render(dec, 2, xy, wb=72 * 16 - 1) == YK_ERR_BAD_ARG                      # windowBytes too small for a window
    assert b"window stride" in L.yk_last_error(dec._h)
    assert render(dec, 2, xy, row=71) == YK_ERR_BAD_ARG
    assert _rc(L.yk_decode_render_windows_device, dec._h, 1, xy, 24, 16, None, 72, 0, 72 * 16, 3, 0) == YK_ERR_BAD_ARG
    assert _rc(L.yk_decode_render_windows_device, dec._h, 1, xy, 24, 16, out.data_ptr(), 72, 0, 72 * 16, 5, 0) == YK_ERR_BAD_ARG
    assert _rc(L.yk_decode_render_windows_device, dec._h, 1, xy, 24, 16, out.data_ptr(), 96, 0, 96 * 16, 4, 256) == YK_ERR_BAD_ARG
    assert _rc(L.yk_decode_render_windows_device, dec._h, 1, xy, 24, 16, out.data_ptr(), 96, 0, 96 * 16, 4, -1) == YK_ERR_STATE    # no 'ALPM' plane was decoded
    assert dec.prepared_blocks == before and _counts(dec) == (0, 0, 0)
    assert render(dec, 2) == 0                                                       # the good call after all of them
    dec.synchronize()
    assert np.array_equal(_np(out[0]), ref.crop(win)) and np.array_equal(_np(out[1]), ref.crop((0, 0, 24, 16)))
    assert np.array_equal(dec.tile4x4(), ref.tile4)
    usable(dec)


def test_a_begin_that_does_not_fit_ends_the_prepared_image(oracle_built):
    """a begin that fails for device memory releases the decode buffers: the image prepared in them is gone with them, the render calls refuse on
    the host and queue nothing, and the next begin + prepare serves windows again"""
    from yaik_amd._lib import lib
    from yaik_amd.decoder import HipTileDecoder
    torch = _torch()
    L = lib()
    w, h, kind = 136, 264, "mixed"
    ref, calls = _refs(w, h, kind)
    win = (56, 56, 24, 16)
    out = torch.full((16, 24, 3), 0xEE, dtype=torch.uint8, device="cuda")
    xy = (C.c_int * 2)(56, 56)
    r, t = C.c_int(), C.c_int()
    d = HipTileDecoder(0)
    try:
        _prepare(d, w, h, calls)
        assert np.array_equal(_np(d.render_window(*win)), ref.crop(win))
        _counts(d)
        assert L.yk_decode_begin_batch(d._h, 32760, 32760, 1024) == YK_ERR_HIP and b"do not fit" in L.yk_last_error(d._h)
        assert _rc(L.yk_decode_render_windows_device, d._h, 1, xy, 24, 16, out.data_ptr(), 72, 0, 72 * 16, 3, 0) == YK_ERR_STATE
        assert b"yk_decode_prepare_device" in L.yk_last_error(d._h)
        assert _rc(L.yk_decode_prepared_blocks, d._h, C.byref(r), C.byref(t)) == YK_ERR_STATE
        assert _raw_prepare(L, d, calls) == YK_ERR_STATE                             # nothing is begun
        assert _counts(d) == (0, 0, 0) and (_np(out) == 0xEE).all()                  # nothing was queued
        _prepare(d, w, h, calls)
        assert d.prepared_blocks == (0, 15)
        assert np.array_equal(_np(d.render_window(*win)), ref.crop(win))
    finally:
        d.close()


# ---- 10: files -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files():
    from yaik_amd import files as F
    F.set_device_palette(False)
    yield F
    F.set_device_palette(False)


@pytest.fixture(scope="module")
def file_streams(files):
    """(rgb, rgba, subset): streams of a 136 x 264 "mixed" frame from encode_file_device without and with an 'ALPM' chunk, and the first with its
    4x4 'GTIL' chunk re-labelled as an R+G chunk (HeaderGradientTile::plane = 3)"""
    import struct
    torch = _torch()
    from tests.images import edge_image
    planes = edge_image(136, 264, "mixed", 4)
    hwc = torch.from_numpy(np.ascontiguousarray(planes.transpose(1, 2, 0)).astype(np.uint8)).cuda()
    rgb = files.encode_file_device(hwc[..., :3].contiguous())
    rgba = files.encode_file_device(hwc, emit_alpha=True)
    assert not files.has_alpha_chunk(rgb) and files.has_alpha_chunk(rgba)
    subset, p, bodies = bytearray(rgb), 12, []
    while p + 8 <= len(subset):
        tag, ln = struct.unpack_from("<II", subset, p)
        if tag == 0xDEADBEEF:
            break
        if tag == 0x4C495447 and subset[p + 8 + 26] & 7 == 2 and (subset[p + 8 + 26] >> 3) & 7 == 2:
            bodies.append(p + 8)
        p += 8 + ln
    assert len(bodies) == 1 and subset[bodies[0] + 27] == 7
    subset[bodies[0] + 27] = 3
    return rgb, rgba, bytes(subset)


def test_file_windows_equal_the_crops_of_the_whole_file_decode(files, file_streams):
    torch = _torch()
    w, h = 136, 264
    for stream, c, prepared in zip(file_streams, (3, 4, 3), (True, True, False)):
        whole = files.decode_file_device(stream)
        assert tuple(whole.shape) == (h, w, c)
        for win in PC.case_windows(w, h):
            x0, y0, ww, wh = win
            got = files.decode_file_windows_device(stream, [(x0, y0)], ww, wh)
            assert files.last_windows_prepared() is prepared
            assert tuple(got.shape) == (1, wh, ww, c) and torch.equal(got[0], whole[y0:y0 + wh, x0:x0 + ww]), (c, win)
        origins = [(56, 56), (0, 0), (112, 248), (56, 56), (112, 0), (0, 248)]
        got = files.decode_file_windows_device(stream, origins, 24, 16)
        assert files.last_windows_prepared() is prepared
        for k, (x0, y0) in enumerate(origins):
            assert torch.equal(got[k], whole[y0:y0 + 16, x0:x0 + 24]), (c, x0, y0)
        assert torch.equal(files.decode_file_device(stream), whole)          # the slot's handle goes back to whole images
    assert not torch.equal(files.decode_file_device(file_streams[2]), files.decode_file_device(file_streams[0]))   # the subset chunk was really read another way


def test_file_windows_outside_the_image_are_refused(files, file_streams):
    from yaik_amd.files import ERROR_NAMES, YaikFileError
    for origins, ww, wh in (([(136, 0)], 8, 8), ([(0, 264)], 8, 8), ([(8, 0)], 136, 8), ([(0, 8)], 8, 264), ([(0, 0), (120, 0)], 24, 16)):
        for stream in (file_streams[0], file_streams[2]):
            with pytest.raises(YaikFileError) as e:
                files.decode_file_windows_device(stream, origins, ww, wh)
            assert ERROR_NAMES[e.value.code] == "YAIK_DECIMG_INVALIDCTX"
    assert files.decode_file_windows_device(file_streams[0], [(0, 0)], 8, 8).shape == (1, 8, 8, 3)      # the slot was released each time
