"""Decode batches (yk_decode_begin_batch and the three *_batch_device entry points; HipTileDecoder.begin_batch / decode_batch_streams /
image_batch_device): every frame of a batch against the CPU oracle and against the decode of that frame alone, bit for bit; degenerate frames;
output layouts with sentinels; every refusal; reuse of a handle; batches from a batch encoder at BASELINE config-4 scale."""
import ctypes as C

import numpy as np
import pytest

from oracle.pyoracle import PASSES, OracleDecoder, OracleEncoder, detile
from tests.images import edge_image, synth_planes
from tests.ragged import SHAPES, oracle_streams, psnr, source
from yaik_amd._lib import YaikError, lib
from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder

pytestmark = pytest.mark.gpu
YK_ERR_BAD_ARG, YK_ERR_HIP, YK_ERR_STATE, YK_ERR_RANGE = -2, -3, -4, -5
YK_STAGE_DEC_GRADIENT, YK_STAGE_DEC_1D, YK_STAGE_DEC_DETILE = 3, 4, 5
SENTINEL = 0xA5
KINDS = ["smooth", "noise", "mixed", "flat", "synth"]            # the two degenerate kinds (noise, flat) each between ordinary frames


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def dec():
    d = HipTileDecoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def one():
    d = HipTileDecoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def enc():
    e = HipTileEncoder(0)
    yield e
    e.close()


def _image(w, h, kind, seed=7):
    return synth_planes(w, h, n_planes=3, seed=1000 + seed) if kind == "synth" else edge_image(w, h, kind, 3, seed=seed)


def _calls(passes, typ, pix, gradient=True, one_d=True):
    """the call list of decode_batch_streams from host streams: all seven passes (an empty pass: the oracle's all-zero bitmap, no colours)"""
    calls = [("g", sx, sy, bm, bm.size, rgb, rgb.size) for sx, sy, cnt, bm, rgb in passes] if gradient else []
    if one_d:
        calls.append(("1", typ, typ.size, pix, pix.size))
    return calls


def _oracle_decode(w, h, passes, typ, pix):
    """(planes after the gradient chunks, tile4x4Mask, planes after the 1-D chunk) of the CPU oracle"""
    od = OracleDecoder(w, h)
    for sx, sy, cnt, bm, rgb in passes:
        if cnt:
            od.gradient(sx, sy, bm, rgb)
    grad, t4 = od.planes().copy(), od.tile4x4().copy()
    od.split_masks()
    od.decode_1d(typ, pix)
    return grad, t4, od.planes().copy()


def _check_batch_against_oracle(dec, w, h, images):
    """gradient chunks of all frames in one call, then the 1-D chunks in one call: every frame exactly the oracle's; returns the PSNRs"""
    streams = [oracle_streams(p) for p in images]
    want = [_oracle_decode(w, h, *s) for s in streams]
    n = len(images)
    dec.begin_batch(w, h, n)
    dec.decode_batch_streams([_calls(*s, one_d=False) for s in streams], remap_range=0)
    for f in range(n):
        dec.select_frame(f)
        assert np.array_equal(dec.planes(), want[f][0]), (f, "gradient fill differs")
        assert np.array_equal(dec.tile4x4(), want[f][1]), (f, "tile4x4Mask differs")
    dec.decode_batch_streams([_calls(*s, gradient=False) for s in streams], remap_range=0)
    out = []
    for f in range(n):
        dec.select_frame(f)
        gp = dec.planes()
        assert np.array_equal(gp, want[f][2]), (f, "1-D range fill differs")
        assert np.array_equal(dec.tile4x4(), want[f][1]), f
        rec = np.stack([detile(gp[c], w, h) for c in range(3)])
        out.append(psnr(rec, images[f][:3]))
    return out


# ---- 1. oracle parity, 4. degenerate frames between ordinary ones ---------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(208, 144), (256, 256)])
def test_batch_matches_oracle(dec, oracle_built, w, h):
    images = [_image(w, h, k) for k in KINDS]
    # the degenerate frames this batch relies on, checked on the oracle: the noise image has no gradient tile at all, the flat image is covered
    # completely by gradient tiles (empty 1-D streams); both sit between ordinary frames
    noise, flat = oracle_streams(images[KINDS.index("noise")]), oracle_streams(images[KINDS.index("flat")])
    for k in ("mixed", "synth"):                                          # ordinary neighbours: gradient tiles and 1-D bytes
        o = oracle_streams(images[KINDS.index(k)])
        assert sum(p[2] for p in o[0]) > 0 and o[1].size > 0
    assert sum(p[2] for p in noise[0]) == 0 and noise[1].size > 0
    assert sum(p[2] for p in flat[0]) > 0 and flat[1].size == 0 and flat[2].size == 0
    psnrs = _check_batch_against_oracle(dec, w, h, images)
    print(f"{w}x{h} PSNR vs source per frame:", {k: round(p, 2) for k, p in zip(KINDS, psnrs)})
    for k, p in zip(KINDS, psnrs):
        assert p > 30.0, (k, p)


# ---- 2. ragged shapes -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,kind", [s for s in SHAPES if (s[0], s[1]) in ((24, 40), (200, 72), (1920, 1080))])
def test_ragged_batch_matches_oracle(dec, oracle_built, w, h, kind):
    images = [source(w, h, kind), edge_image(w, h, "mixed", 3, seed=w + 1), edge_image(w, h, "smooth", 3, seed=h + 2)]
    psnrs = _check_batch_against_oracle(dec, w, h, images)
    print(f"{w}x{h} PSNR vs source per frame:", [round(p, 2) for p in psnrs])


# ---- 3. batch equals single -----------------------------------------------------------------------------------------------------------------
def _raw_device_streams(planes):
    """the oracle's streams as an encoder leaves them in HBM (corner streams NOT yet remapped): (tensors kept alive, call list of encoder_streams)"""
    torch = _torch()
    enc = OracleEncoder(planes)
    keep, calls = [], []
    for sx, sy in PASSES:
        cnt, bm, rgb = enc.fitting_quad_smooth(sx, sy)
        tb = torch.from_numpy(np.ascontiguousarray(bm)).cuda()
        tr = torch.from_numpy(np.concatenate([rgb, np.zeros(16, np.uint8)])).cuda()
        keep += [tb, tr]
        calls.append(("g", sx, sy, tb.data_ptr(), bm.size, tr.data_ptr(), rgb.size, cnt))
    for p in range(3):
        enc.dynamic_tile_compressor(p)
    pix, typ = enc.streams_1d()
    tt = torch.from_numpy(np.concatenate([typ, np.zeros(16, np.uint8)])).cuda()
    tp = torch.from_numpy(np.concatenate([pix, np.zeros(16, np.uint8)])).cuda()
    keep += [tt, tp]
    calls.append(("1", tt.data_ptr(), typ.size, tp.data_ptr(), pix.size))
    torch.cuda.synchronize()
    return keep, calls


def _single_calls(calls):
    """what decode_streams takes: the passes with tiles (as encoder_streams lists them); a frame without 1-D bytes has no 1-D entry"""
    return [c[:7] for c in calls if c[0] == "g" and c[7]] + [c for c in calls if c[0] == "1" and c[2]]


@pytest.mark.parametrize("w,h", [(208, 144), (256, 256)])
def test_batch_equals_single(dec, one, oracle_built, w, h):
    torch = _torch()
    images = [_image(w, h, k, seed=11) for k in KINDS]
    dev = [_raw_device_streams(p) for p in images]
    n = len(images)
    dec.begin_batch(w, h, n)
    dec.decode_batch_streams([[c[:7] if c[0] == "g" else c for c in calls] for _, calls in dev])
    batch_img = dec.image_batch_device()
    assert batch_img.shape == (n, h, w, 3)
    got = []
    for f in range(n):
        dec.select_frame(f)
        got.append((dec.planes(), dec.tile4x4(), dec.image_device().clone()))
        assert torch.equal(batch_img[f], got[f][2]), f
    for f in range(n):
        one.begin(w, h)
        one.decode_streams(_single_calls(dev[f][1]))
        assert np.array_equal(one.planes(), got[f][0]), f
        assert np.array_equal(one.tile4x4(), got[f][1]), f
        assert torch.equal(one.image_device(), got[f][2]), f
    # frame 2 (gradient tiles and 1-D bytes) decoded once more, alone, through the single-image entry points of the batch handle
    assert dev[2][1][-1][2] > 0 and sum(c[7] for c in dev[2][1][:-1]) > 0
    dec.select_frame(2)
    dec.decode_streams(_single_calls(dev[2][1]))
    for f in (1, 2, 3):
        dec.select_frame(f)
        assert np.array_equal(dec.planes(), got[f][0]) and np.array_equal(dec.tile4x4(), got[f][1]), f
        assert torch.equal(dec.image_device(), got[f][2]), f


def test_one_frame_through_the_batch_api_equals_the_existing_path(dec, one, oracle_built):
    w, h = 208, 144
    planes = _image(w, h, "mixed", seed=3)
    passes, typ, pix = oracle_streams(planes)
    one.begin(w, h)
    for sx, sy, cnt, bm, rgb in passes:
        if cnt:
            one.decompress_gradient(sx, sy, bm, rgb)
    one.decompress_1d(typ, pix)
    dec.begin_batch(w, h, 1)
    dec.decode_batch_streams([_calls(passes, typ, pix)], remap_range=0)
    assert np.array_equal(dec.planes(), one.planes()) and np.array_equal(dec.tile4x4(), one.tile4x4())
    img = dec.image_batch_device()
    assert img.shape == (1, h, w, 3) and _torch().equal(img[0], one.image_device())


# ---- 5. from a batch encoder ----------------------------------------------------------------------------------------------------------------
def _u8_frames(images):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(np.stack([np.moveaxis(p[:3], 0, -1) for p in images]).astype(np.uint8))).cuda()


def _single_from_encoder(one, enc, f, w, h):
    enc.select_frame(f)
    one.begin(w, h)
    one.decode_from_encoder(enc)
    return one.image_device().clone()


def test_from_a_batch_encoder(dec, one, enc):
    torch = _torch()
    w, h = 264, 136
    images = [_image(w, h, k, seed=21) for k in ("mixed", "smooth", "noise", "synth")]
    frames = _u8_frames(images)
    enc.set_batch_u8(frames)
    enc.encode_batch(3, False)
    dec.begin_batch(w, h, 4)
    dec.decode_batch_from_encoder(enc)
    got = dec.image_batch_device()
    assert got.shape == (4, h, w, 3) and got.dtype == torch.uint8
    for f in range(4):
        want = _single_from_encoder(one, enc, f, w, h)
        assert torch.equal(got[f], want), f
        err = (got[f].cpu().numpy().astype(np.int64) - frames[f].cpu().numpy()).ravel()
        p = psnr(got[f].cpu().numpy(), frames[f].cpu().numpy())
        print(f"frame {f}: max |err| = {int(np.abs(err).max())}, PSNR = {p:.2f} dB")
        assert p > 30.0, (f, p)


# ---- 6. output layouts ----------------------------------------------------------------------------------------------------------------------
def _decoded_batch(dec, w, h, n, seed=31):
    images = [_image(w, h, KINDS[f % len(KINDS)], seed=seed + f) for f in range(n)]
    streams = [oracle_streams(p) for p in images]
    dec.begin_batch(w, h, n)
    dec.decode_batch_streams([_calls(*s) for s in streams], remap_range=0)
    want = []
    for f in range(n):
        dec.select_frame(f)
        want.append(dec.image_device().clone())
    return _torch().stack(want)


@pytest.mark.parametrize("planar", [False, True], ids=["hwc", "chw"])
@pytest.mark.parametrize("channels,alpha", [(3, 255), (4, 200), (4, 0)], ids=["rgb", "rgba200", "rgba0"])
def test_output_layouts_leave_every_other_byte(dec, oracle_built, planar, channels, alpha):
    torch = _torch()
    w, h, n = 200, 72, 3
    rgb = _decoded_batch(dec, w, h, n)                                        # [n, h, w, 3]
    want = rgb if channels == 3 else torch.cat([rgb, torch.full((n, h, w, 1), alpha, dtype=torch.uint8, device="cuda")], dim=-1)
    if planar:
        want = want.permute(0, 3, 1, 2)
    got = dec.image_batch_device(channels=channels, alpha=alpha, planar=planar)
    assert torch.equal(got, want)
    for extra_row, extra_plane, extra_frame in ((0, 0, 0), (48, 7, 29), (5, 0, 1)):
        for offset in (0, 1, 3):
            row = (w if planar else w * channels) + extra_row
            if planar:
                plane = row * h + extra_plane
                frame = plane * channels + extra_frame
                shape, strides = (n, channels, h, w), (frame, plane, row, 1)
            else:
                frame = row * h + extra_frame
                shape, strides = (n, h, w, channels), (frame, row, channels, 1)
            size = offset + frame * n + 64
            buf = torch.full((size,), SENTINEL, dtype=torch.uint8, device="cuda")
            out = torch.as_strided(buf, shape, strides, offset)
            assert dec.image_batch_device(out, channels=channels, alpha=alpha, planar=planar) is out
            assert torch.equal(out, want), (extra_row, offset)
            mask = torch.zeros(size, dtype=torch.bool, device="cuda")
            torch.as_strided(mask, shape, strides, offset).fill_(True)
            assert (buf[~mask] == SENTINEL).all(), (extra_row, offset, "a byte outside the pixels changed")
    # views of a larger tensor: a window of frames, rows and columns of a bigger batch
    if planar:
        big = torch.full((n + 2, channels, h + 9, w + 24), SENTINEL, dtype=torch.uint8, device="cuda")
        view = big[1:1 + n, :, 4:4 + h, 8:8 + w]
    else:
        big = torch.full((n + 2, h + 9, w + 24, channels), SENTINEL, dtype=torch.uint8, device="cuda")
        view = big[1:1 + n, 4:4 + h, 8:8 + w, :]
    dec.image_batch_device(view, channels=channels, alpha=alpha, planar=planar)
    assert torch.equal(view, want)
    keep = torch.ones_like(big, dtype=torch.bool)
    (keep[1:1 + n, :, 4:4 + h, 8:8 + w] if planar else keep[1:1 + n, 4:4 + h, 8:8 + w, :]).fill_(False)
    assert (big[keep] == SENTINEL).all()
    with pytest.raises(ValueError):
        dec.image_batch_device(view[:2], channels=channels, alpha=alpha, planar=planar)          # two frames for a batch of three


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------------
def _err(d):
    return lib().yk_last_error(d._h).decode()


def test_batch_calls_before_any_begin():
    L = lib()
    d = HipTileDecoder(0)
    try:
        one_i, one_p, one_s = (C.c_int * 1)(4), (C.c_void_p * 1)(16), (C.c_size_t * 1)(0)
        assert L.yk_decode_select_frame(d._h, 0) == YK_ERR_STATE and "begin" in _err(d)
        assert L.yk_decode_gradient_all_batch_device(d._h, 1, one_i, one_i, one_p, one_s, one_p, one_s, 0) == YK_ERR_STATE and "begin" in _err(d)
        assert L.yk_decode_1d_batch_device(d._h, one_p, one_s, one_p, one_s, 15) == YK_ERR_STATE and "begin" in _err(d)
        assert L.yk_decode_output_batch_device(d._h, 16, 64, 0, 64 * 8, 3, 255) == YK_ERR_STATE and "begin" in _err(d)
        d.begin(8, 8)                                                         # the handle is usable afterwards
        assert d.planes().shape == (3, 64)
    finally:
        d.close()


def test_refusals_write_nothing_and_leave_the_handle_usable(oracle_built):
    torch = _torch()
    L = lib()
    w, h, n = 72, 40, 3
    images = [_image(w, h, k, seed=41) for k in ("mixed", "smooth", "mixed")]
    streams = [oracle_streams(p) for p in images]
    want = [_oracle_decode(w, h, *s)[2] for s in streams]
    d = HipTileDecoder(0)
    try:
        def good():
            d.begin_batch(w, h, n)
            d.decode_batch_streams([_calls(*s) for s in streams], remap_range=0)
            for f in range(n):
                d.select_frame(f)
                assert np.array_equal(d.planes(), want[f]), f

        def untouched():
            for f in range(n):
                assert L.yk_decode_select_frame(d._h, f) == 0
                assert np.array_equal(d.planes(), want[f]), f

        good()
        for bad in (0, -1, 1025):
            assert L.yk_decode_begin_batch(d._h, w, h, bad) == YK_ERR_BAD_ARG and "nFrames" in _err(d)
        for bad in (w + 4, 4):
            assert L.yk_decode_begin_batch(d._h, bad, h, 2) == YK_ERR_BAD_ARG
        untouched()
        for bad in (-1, n, 1 << 20):
            assert L.yk_decode_select_frame(d._h, bad) == YK_ERR_BAD_ARG and "frame out of range" in _err(d)
        # valid tables for the gradient call, then one field wrong at a time
        P = 7
        dev_bm = [torch.from_numpy(np.ascontiguousarray(p[3])).cuda() for s in streams for p in s[0]]
        dev_rgb = [torch.from_numpy(np.concatenate([p[4], np.zeros(16, np.uint8)])).cuda() for s in streams for p in s[0]]
        torch.cuda.synchronize()
        sx, sy = [p[0] for p in PASSES], [p[1] for p in PASSES]
        nb = [p[3].size for p in streams[0][0]]
        bm, rgb = [t.data_ptr() for t in dev_bm], [t.data_ptr() for t in dev_rgb]
        nr = [p[4].size for s in streams for p in s[0]]

        def grad(n_passes=P, sx=sx, sy=sy, bm=bm, nb=nb, rgb=rgb, nr=nr, null=None):
            arg = {"sx": (C.c_int * len(sx))(*sx), "sy": (C.c_int * len(sy))(*sy), "bm": (C.c_void_p * len(bm))(*bm),
                   "nb": (C.c_size_t * len(nb))(*nb), "rgb": (C.c_void_p * len(rgb))(*rgb), "nr": (C.c_size_t * len(nr))(*nr)}
            if null:
                arg[null] = None
            return L.yk_decode_gradient_all_batch_device(d._h, n_passes, arg["sx"], arg["sy"], arg["bm"], arg["nb"], arg["rgb"], arg["nr"], 0)

        for null in ("sx", "sy", "bm", "nb", "rgb", "nr"):
            assert grad(null=null) == YK_ERR_BAD_ARG and "NULL table" in _err(d), null
        assert grad(bm=bm[:9] + [None] + bm[10:]) == YK_ERR_BAD_ARG and "NULL tile bitmap" in _err(d)
        k = next(i for i, v in enumerate(nr) if v)
        assert grad(rgb=rgb[:k] + [None] + rgb[k + 1:]) == YK_ERR_BAD_ARG and "NULL colour stream" in _err(d)
        assert grad(sx=[5] + sx[1:]) == YK_ERR_BAD_ARG and "unsupported tile format" in _err(d)
        assert grad(sy=sy[:6] + [1]) == YK_ERR_BAD_ARG and "unsupported tile format" in _err(d)
        assert grad(n_passes=8, sx=sx + [4], sy=sy + [4], nb=nb + [nb[0]]) == YK_ERR_BAD_ARG and "passes" in _err(d)
        assert grad(n_passes=-1) == YK_ERR_BAD_ARG
        assert grad(nb=nb[:3] + [nb[3] - 1] + nb[4:]) == YK_ERR_RANGE and "shorter" in _err(d)
        untouched()
        # the 1-D call
        ty = [torch.from_numpy(np.concatenate([s[1], np.zeros(16, np.uint8)])).cuda() for s in streams]
        px = [torch.from_numpy(np.concatenate([s[2], np.zeros(32, np.uint8)])).cuda() for s in streams]
        torch.cuda.synchronize()
        nt, npx = [s[1].size for s in streams], [s[2].size for s in streams]
        assert all(nt) and all(npx)

        def d1(ty=[t.data_ptr() for t in ty], nt=nt, px=[t.data_ptr() for t in px], npx=npx, rng=15, null=None):
            arg = {"ty": (C.c_void_p * n)(*ty), "nt": (C.c_size_t * n)(*nt), "px": (C.c_void_p * n)(*px), "npx": (C.c_size_t * n)(*npx)}
            if null:
                arg[null] = None
            return L.yk_decode_1d_batch_device(d._h, arg["ty"], arg["nt"], arg["px"], arg["npx"], rng)

        for null in ("ty", "nt", "px", "npx"):
            assert d1(null=null) == YK_ERR_BAD_ARG and "NULL table" in _err(d), null
        assert d1(ty=[ty[0].data_ptr(), None, ty[2].data_ptr()]) == YK_ERR_BAD_ARG and "NULL 1-D stream" in _err(d)
        assert d1(px=[px[0].data_ptr(), px[1].data_ptr(), None]) == YK_ERR_BAD_ARG and "NULL 1-D stream" in _err(d)
        assert d1(px=[px[0].data_ptr() + 4, px[1].data_ptr(), px[2].data_ptr()]) == YK_ERR_BAD_ARG and "aligned" in _err(d)
        assert d1(rng=0) == YK_ERR_BAD_ARG
        untouched()
        # the output call: nothing is written
        size = 4 * w * h * n + 4096
        buf = torch.full((size,), SENTINEL, dtype=torch.uint8, device="cuda")
        p = buf.data_ptr()
        out = lambda *a: L.yk_decode_output_batch_device(d._h, *a)
        assert out(None, w * 3, 0, w * 3 * h, 3, 255) == YK_ERR_BAD_ARG and "NULL" in _err(d)
        for ch in (0, 1, 2, 5):
            assert out(p, w * 4, 0, w * 4 * h, ch, 255) == YK_ERR_BAD_ARG and "channels" in _err(d)
        assert out(p, w * 3 - 1, 0, w * 3 * h, 3, 255) == YK_ERR_BAD_ARG and "pitch" in _err(d)
        assert out(p, w * 4 - 1, 0, w * 4 * h, 4, 255) == YK_ERR_BAD_ARG
        assert out(p, w - 1, w * h, 4 * w * h, 4, 255) == YK_ERR_BAD_ARG                   # CHW row shorter than w
        assert out(p, w, w * h - 1, 4 * w * h, 4, 255) == YK_ERR_BAD_ARG                   # CHW plane shorter than rowBytes * h
        assert out(p, w * 3, 0, w * 3 * h - 1, 3, 255) == YK_ERR_BAD_ARG and "frame stride" in _err(d)
        assert out(p, w, w * h, 3 * w * h - 1, 3, 255) == YK_ERR_BAD_ARG and "frame stride" in _err(d)
        for a in (-1, -2, 256, 1000):
            assert out(p, w * 4, 0, w * 4 * h, 4, a) == YK_ERR_BAD_ARG and "alpha" in _err(d), a
        d.synchronize()
        assert (buf == SENTINEL).all(), "a refused output call wrote"
        assert out(p, w * 3, 0, w * 3 * h, 3, 1000) == 0                                  # alpha is ignored with 3 channels
        d.synchronize()
        assert (buf[w * 3 * h * n:] == SENTINEL).all() and not (buf[: w * 3 * h * n] == SENTINEL).all()
        buf.fill_(SENTINEL)
        # the calls a batch does not support: YK_ERR_STATE, nothing touched
        host = np.full(4 * w * h + 64, SENTINEL, np.uint8)
        i4 = (C.c_int32 * 4)(0, 0, 8, 8)
        null6, null4, sz6, sz4, used = (C.c_void_p * 6)(), (C.c_void_p * 4)(), (C.c_size_t * 6)(), (C.c_size_t * 4)(), (C.c_size_t * 6)()
        unsupported = {
            "yk_decode_alpha": lambda: L.yk_decode_alpha(d._h, 6, i4, host.ctypes.data, 64, None, 0, None, 0),
            "yk_decode_output_alpha": lambda: L.yk_decode_output_alpha(d._h, host.ctypes.data, w * 4),
            "yk_decode_output_reference_rgba": lambda: L.yk_decode_output_reference_rgba(d._h, host.ctypes.data, w * 4 + 1, host.ctypes.data, w),
            "yk_decode_gradient_planes": lambda: L.yk_decode_gradient_planes(d._h, 1, 1, host.ctypes.data, 4096, host.ctypes.data, 12),
            "yk_decode_split_masks": lambda: L.yk_decode_split_masks(d._h),
            "yk_decode_lut3d": lambda: L.yk_decode_lut3d(d._h, null6, sz6, None, 0, None, null4, sz4, used),
            "yk_decode_mask": lambda: L.yk_decode_mask(d._h, host.ctypes.data, 1, 1, host.ctypes.data, 64),
        }
        for name, call in unsupported.items():
            assert call() == YK_ERR_STATE, name
            assert name in _err(d) and "batch" in _err(d), (name, _err(d))
        assert (host == SENTINEL).all()
        untouched()
        good()                                                                # and the handle still decodes
        # an allocation that does not fit: every decode buffer is released, the next begin works
        assert L.yk_decode_begin_batch(d._h, 32760, 32760, 1024) == YK_ERR_HIP and "do not fit" in _err(d)
        assert L.yk_decode_select_frame(d._h, 0) == YK_ERR_STATE
        good()
    finally:
        d.close()


def test_a_pass_of_2_to_the_25_tile_slots_is_refused():
    """the 4x4 pass of a 32760 x 16392 image has 2^25 + 65536 slots: the single-image call falls back to pass after pass, the batch form refuses"""
    torch = _torch()
    L = lib()
    w, h = 32760, 16392
    slots = ((w + 31) // 32) * ((h + 31) // 32) * 64
    assert slots >= 1 << 25
    d = HipTileDecoder(0)
    try:
        d.begin_batch(w, h, 1)
        bm = torch.zeros(slots // 8, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        one_i = (C.c_int * 1)(2)
        ptr, nb, nr = (C.c_void_p * 1)(bm.data_ptr()), (C.c_size_t * 1)(slots // 8), (C.c_size_t * 1)(0)
        null = (C.c_void_p * 1)()
        assert L.yk_decode_gradient_all_batch_device(d._h, 1, one_i, one_i, ptr, nb, null, nr, 0) == YK_ERR_BAD_ARG
        assert "2^25" in _err(d)
        d.begin(8, 8)
    finally:
        d.close()
        torch.cuda.empty_cache()


def test_stage_timers_record_one_interval_per_batch_call(dec, oracle_built):
    w, h, n = 72, 40, 4
    streams = [oracle_streams(_image(w, h, "mixed", seed=50 + f)) for f in range(n)]
    dec.begin_batch(w, h, n)
    for st in (YK_STAGE_DEC_GRADIENT, YK_STAGE_DEC_1D, YK_STAGE_DEC_DETILE):
        dec.stage_ms(st)
    for rep in range(2):
        dec.decode_batch_streams([_calls(*s) for s in streams], remap_range=0)
        dec.image_batch_device()
    dec.synchronize()
    assert [dec.stage_ms(st)[1] for st in (YK_STAGE_DEC_GRADIENT, YK_STAGE_DEC_1D, YK_STAGE_DEC_DETILE)] == [2, 2, 2]    # read and reset


def test_single_image_decode_of_one_frame_leaves_the_other_frames_defined(oracle_built):
    """The handle's buffers held another batch.  Then: frame 0 decoded completely through the single-image entry points, frame 1 only its
    gradient chunks, frame 2 nothing.  Cells no chunk wrote are zero, as in the oracle, in every frame (the planes are never cleared: the
    single 1-D decode of frame 0 must not leave the other frames' unmarked cells holding the previous batch)."""
    w, h = 136, 72
    d = HipTileDecoder(0)
    try:
        old = [_image(w, h, k, seed=71) for k in ("noise", "noise", "noise")]
        _check_batch_against_oracle(d, w, h, old)                             # every cell of every frame now holds noise
        images = [_image(w, h, k, seed=72) for k in ("mixed", "mixed", "synth")]
        streams = [oracle_streams(p) for p in images]
        want = [_oracle_decode(w, h, *s) for s in streams]
        d.begin_batch(w, h, 3)
        for f in (0, 1):
            d.select_frame(f)
            for sx, sy, cnt, bm, rgb in streams[f][0]:
                if cnt:
                    d.decompress_gradient(sx, sy, bm, rgb)
            if f == 0:
                d.decompress_1d(streams[f][1], streams[f][2])
        d.select_frame(1)
        assert np.array_equal(d.planes(), want[1][0]), "frame 1: gradient-only planes differ from the oracle"
        assert np.array_equal(d.tile4x4(), want[1][1])
        d.select_frame(2)
        assert not d.planes().any(), "frame 2: nothing was decoded, every cell is zero"
        d.select_frame(0)
        assert np.array_equal(d.planes(), want[0][2])
        # the other order: batch gradient chunks, a single 1-D decode of frame 2, then the other frames
        d.begin_batch(w, h, 3)
        d.decode_batch_streams([_calls(*s, one_d=False) for s in streams], remap_range=0)
        d.select_frame(2)
        d.decompress_1d(streams[2][1], streams[2][2])
        for f in (0, 1):
            d.select_frame(f)
            assert np.array_equal(d.planes(), want[f][0]), f
        d.select_frame(2)
        assert np.array_equal(d.planes(), want[2][2])
    finally:
        d.close()


# ---- 8. reuse -------------------------------------------------------------------------------------------------------------------------------
def test_reuse_leaves_nothing_stale(oracle_built):
    w, h = 136, 72
    d = HipTileDecoder(0)
    try:
        a = [_image(w, h, k, seed=61) for k in ("mixed", "noise", "smooth", "synth")]
        b = [_image(w, h, k, seed=62) for k in ("flat", "mixed", "noise", "smooth")]     # other content in every frame, same shape and count
        _check_batch_against_oracle(d, w, h, a)
        _check_batch_against_oracle(d, w, h, b)
        _check_batch_against_oracle(d, w, h, a[:2])                                       # another frame count
        _check_batch_against_oracle(d, w, h, b + a)
        # plain begin: one frame, the existing path
        passes, typ, pix = oracle_streams(a[0])
        want = _oracle_decode(w, h, passes, typ, pix)
        d.begin(w, h)
        assert d.frames == 1
        with pytest.raises(YaikError):
            d.select_frame(1)
        for sx, sy, cnt, bm, rgb in passes:
            if cnt:
                d.decompress_gradient(sx, sy, bm, rgb)
        assert np.array_equal(d.planes(), want[0]) and np.array_equal(d.tile4x4(), want[1])
        d.decompress_1d(typ, pix)
        assert np.array_equal(d.planes(), want[2])
        assert d.decompress_1bit_tiled(np.array([0x5A], np.uint8), 2, 2).size == 128      # a call a batch refuses works again
    finally:
        d.close()


# ---- 9. BASELINE config-4 scale -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,size,check", [(64, 2048, (0, 31, 63)), (256, 512, (0, 255))], ids=["64x2048", "256x512"])
def test_config4_scale_batch_equals_single(n, size, check):
    from yaik_amd.synth import synth_planes_torch
    torch = _torch()
    e, d, one = HipTileEncoder(0), HipTileDecoder(0), HipTileDecoder(0)
    try:
        frames = torch.empty((n, size, size, 3), dtype=torch.uint8, device="cuda")
        for f in range(n):
            frames[f] = synth_planes_torch(size, size, n_planes=3, seed=9000 + f, device="cuda").permute(1, 2, 0).to(torch.uint8)
        torch.cuda.synchronize()
        e.set_batch_u8(frames)
        e.encode_batch(3, False)
        d.begin_batch(size, size, n)
        d.decode_batch_from_encoder(e)
        got = d.image_batch_device()
        for f in check:
            want = _single_from_encoder(one, e, f, size, size)
            assert torch.equal(got[f], want), f
            d.select_frame(f)
            assert np.array_equal(d.planes(), one.planes()) and np.array_equal(d.tile4x4(), one.tile4x4()), f
            p = psnr(got[f].cpu().numpy(), frames[f].cpu().numpy())
            print(f"{n} x {size}^2 frame {f}: PSNR vs source {p:.2f} dB")
            assert p > 30.0
    finally:
        e.close(); d.close(); one.close()
        torch.cuda.empty_cache()
