"""Normalised fp16 / bf16 / fp32 outputs with a per-frame mirror on the GPU (yk_decode_output_norm_device, yk_decode_output_norm_batch_device,
YAIK_DecodeImagesNormToDevice) against tests/norm_ref.py on the oracle's crop.  The arithmetic is fully defined, so every comparison is
on bit patterns, with tolerance zero: single images (whole, an aligned window, pixel windows), every layout into sentinel-filled padded buffers,
batches with mixed mirror flags, RGBA from an encoder's planes, every refusal, `.yaik` files, and the uint8 calls after the new ones."""
import ctypes as C

import numpy as np
import pytest

from tests import batch_window_cases as BW
from tests import norm_ref as NR
from tests import window_cases as WC
from tests import window_px_cases as PX
from tests.test_gpu_decode_batch_window import _alpha_entries, _decode_batch
from tests.test_gpu_decode_window import _alpha_plane, _decode, _refs

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
YK_ERR_BAD_ARG, YK_ERR_STATE, YK_STAGE_DEC_DETILE = -2, -4, 5
BIG = [c for c in WC.CASES if c[:2] != (8, 8)]
SETS = NR.parameter_sets()
FLAGS = [True, False, True, True]


def _torch():
    import torch
    return torch


def _tdt(name):
    return getattr(_torch(), name)


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


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _rgba(rgb, alpha):
    """uint8 [..., 4] from [..., 3] and an alpha plane [...] or a constant"""
    a = np.full(rgb.shape[:-1], alpha, np.uint8) if np.isscalar(alpha) else alpha
    return np.concatenate([rgb, a[..., None]], axis=-1)


def _crop(a, win):
    x0, y0, ww, wh = win
    return a[y0:y0 + wh, x0:x0 + ww]


def _single_windows(w, h):
    """(window or None for the whole image, px) of test 1: whole, an aligned window, and the pixel windows that fit"""
    aligned = (8, 8, w - 16, h - 16) if w > 16 and h > 16 else (0, 0, 8, 8)
    px = [(3, 5, 13, 11), (w - 13, h - 11, 13, 11), (7, 7, 2, 2), (1, 1, w - 2, h - 2), (3, 5, 1, 1)]
    return [(None, False), (aligned, False)] + [(win, True) for win in px if PX.inside(win, w, h)]


def _begin(d, w, h, kind, win, px, alpha_seed=None):
    """the image decoded on d under `win` (None: whole); returns the uint8 RGBA pixels [wh, ww, 4] the outputs are made of (alpha 255 without a plane)"""
    ref, key = _refs(w, h, kind)
    d.begin(w, h)
    if win is not None:
        d.set_window(*win, px=px)
    alpha = _alpha_plane(d, w, h, seed=alpha_seed) if alpha_seed is not None else 255
    _decode(d, ref, key, "all_pass")
    full = (0, 0, w, h) if win is None else win
    return _rgba(ref.crop(full), alpha if np.isscalar(alpha) else _crop(alpha, full)), alpha


def test_the_reference_separates_fused_from_unfused():
    """set B on every byte value: a contracted fma would change 124..158 of the 256 fp32 results of every channel, so the fp32 comparisons below catch it"""
    v = np.arange(256, dtype=np.uint8).reshape(256, 1, 1).repeat(4, axis=2)
    diff = (NR.affine_f32(v, *SETS["B"]).view(np.uint32) != NR.affine_fused_f32(v, *SETS["B"]).view(np.uint32)).reshape(256, 4).sum(axis=0)
    assert all(124 <= int(n) <= 158 for n in diff), diff


# ---- 1: single images: every dtype, every parameter set, whole / aligned / pixel windows, mirror 0 and 1 -------------------------------------
@pytest.mark.parametrize("dtype", NR.DTYPES)
@pytest.mark.parametrize("w,h,kind", WC.CASES, ids=_ids)
def test_single_image_equals_the_reference(dec, oracle_built, w, h, kind, dtype):
    seen = np.zeros(256, bool)
    for win, px in _single_windows(w, h):
        pix, alpha = _begin(dec, w, h, kind, win, px, alpha_seed=w + h)
        seen[np.unique(pix[..., 3])] = True
        for name, (scale, bias) in SETS.items():
            want = NR.norm_ref(pix, dtype, scale, bias)
            for mirror in (False, True):
                got = dec.image_norm_device(_tdt(dtype), scale=scale, bias=bias, mirror=mirror, channels=4)
                assert got.dtype == _tdt(dtype) and tuple(got.shape) == pix.shape
                assert np.array_equal(NR.bits(got), want[:, ::-1] if mirror else want), (win, name, mirror)
        # three channels, and the defaults (scale 1, bias 0): the bytes themselves
        got = dec.image_norm_device(_tdt(dtype), channels=3)
        assert np.array_equal(NR.bits(got), NR.norm_ref(pix[..., :3], dtype, 1.0, 0.0)), win
    if (w, h) != (8, 8):
        assert seen.all()                                                    # every byte value went through the conversion, in the alpha channel


def test_mean_and_std_go_through_norm_params(dec, oracle_built):
    from yaik_amd.decoder import norm_params
    torch = _torch()
    w, h, kind = 136, 264, "mixed"
    pix, _ = _begin(dec, w, h, kind, (3, 5, 13, 11), True)
    mean, std = [0.485 * 255, 0.456 * 255, 0.406 * 255], [0.229 * 255, 0.224 * 255, 0.225 * 255]
    s, b = norm_params(mean, std)
    got = dec.image_norm_device(torch.float32, mean=mean, std=std, channels=3)
    assert np.array_equal(NR.bits(got), NR.norm_ref(pix[..., :3], "float32", s, b))
    got = dec.image_norm_device("bfloat16", mean=mean, std=std, channels=4, alpha=77, mirror=True)        # three values leave alpha at 1, 0
    assert np.array_equal(NR.bits(got), NR.norm_ref(_rgba(pix[..., :3], 77), "bfloat16", s, b, mirror=True))
    assert np.array_equal(NR.bits(got)[..., 3], np.full((11, 13), 0x429A, np.uint16))                      # bf16(77)


# ---- 2: layouts; every byte outside the pixels keeps the sentinel ----------------------------------------------------------------------------
def _padded(dtype, shape, planar, batch):
    """a sentinel-filled byte buffer, and a view of it in `dtype` of `shape` at an odd element offset with row, plane and frame padding;
    returns (bytes [n, es], view, mask [n] of the elements the view covers)"""
    torch = _torch()
    tdt, es = _tdt(dtype), NR.ELEM_BYTES[dtype]
    if planar:
        c, hh, ww = shape[-3:]
        row = ww + 11
        plane = row * hh + 13
        frame, strides, off = plane * c + 29, (plane, row, 1), 3
    else:
        hh, ww, c = shape[-3:]
        row = ww * c + 11
        frame, strides, off = row * hh + 29, (row, c, 1), 5
    n = off + frame * (shape[0] if batch else 1) + 64
    if batch:
        strides = (frame,) + strides
    raw = torch.full((n * es,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(raw.view(tdt), shape, strides, off)
    mask = torch.zeros(n, dtype=torch.bool, device="cuda")
    torch.as_strided(mask, shape, strides, off).fill_(True)
    return raw.view(n, es), view, mask


LAYOUTS = [(3, None, False), (4, 77, False), (4, None, False), (3, None, True), (4, None, True), (4, 77, True)]   # channels, alpha (None: the plane), planar


@pytest.mark.parametrize("dtype", NR.DTYPES)
@pytest.mark.parametrize("w,h,kind", BIG[:2], ids=_ids)
def test_layouts_write_the_pixels_and_nothing_else(dec, oracle_built, w, h, kind, dtype):
    scale, bias = SETS["B"]
    for win, px in [(None, False), ((8, 8, 24, 16), False)] + [(v, True) for v in ((3, 5, 13, 11), (w - 13, h - 11, 13, 11), (7, 7, 2, 2), (1, 1, w - 2, h - 2))]:
        pix, alpha = _begin(dec, w, h, kind, win, px, alpha_seed=w + h)
        for channels, a_arg, planar in LAYOUTS:
            src = pix[..., :3] if channels == 3 else pix if a_arg is None else _rgba(pix[..., :3], a_arg)
            for mirror in (False, True):
                want = NR.norm_ref(src, dtype, scale, bias, mirror)
                want = np.ascontiguousarray(want.transpose(2, 0, 1)) if planar else want
                raw, view, mask = _padded(dtype, want.shape, planar, False)
                assert dec.image_norm_device(dtype, scale=scale, bias=bias, mirror=mirror, out=view, channels=channels, alpha=a_arg, planar=planar) is view
                assert np.array_equal(NR.bits(view), want), (win, channels, a_arg, planar, mirror)
                assert bool((raw[~mask] == SENTINEL).all()), (win, channels, a_arg, planar, mirror, "a byte outside the pixels changed")


# ---- 3: batches ------------------------------------------------------------------------------------------------------------------------------
def _batch_alpha(d, n):
    out = []
    for f in range(n):
        d.select_frame(f)
        out.append(d.alpha_plane())
    d.select_frame(0)
    return out


def _batch_want(refs, alpha, size, origins, dtype, scale, bias, flags, channels=4):
    ww, wh = size
    frames = []
    for f, (r, (x0, y0)) in enumerate(zip(refs, origins)):
        px = _rgba(r.rgb[y0:y0 + wh, x0:x0 + ww], alpha[f][y0:y0 + wh, x0:x0 + ww])[..., :channels]
        frames.append(NR.norm_ref(px, dtype, scale, bias, bool(flags[f]) if flags is not None else False))
    return np.stack(frames)


@pytest.mark.parametrize("dtype", NR.DTYPES)
@pytest.mark.parametrize("w,h,kind,n", BW.BATCHES, ids=_ids)
def test_batches_equal_the_reference_frame_by_frame(dec, dec2, oracle_built, w, h, kind, n, dtype):
    torch = _torch()
    refs = BW.batch_references(w, h, kind, n)
    scale, bias = SETS["B"]
    flags = FLAGS[:n]
    aligned = BW.window_sets(w, h)[0]
    cases = [(None, (w, h), [(0, 0)] * n, False), ("aligned", aligned[1], aligned[2], False)]
    cases += [("px", size, origins, True) for size, origins in PX.origin_sets(w, h, n)]          # the far corner included: the shared cover pulled back
    for what, size, origins, px in cases:
        dec.begin_batch(w, h, n)
        if what is not None:
            dec.set_batch_windows(origins, *size, px=px)
        dec.decompress_alpha_batch(_alpha_entries(w, h, n, seed=w + h + n), 255, sync=False)
        _decode_batch(dec, refs)
        alpha = _batch_alpha(dec, n)
        for planar in (False, True):
            for mirror in (None, flags, torch.tensor([not f for f in flags])):
                fl = None if mirror is None else [bool(v) for v in mirror]
                want = _batch_want(refs, alpha, size, origins, dtype, scale, bias, fl)
                want = np.ascontiguousarray(want.transpose(0, 3, 1, 2)) if planar else want
                raw, view, mask = _padded(dtype, want.shape, planar, True)
                got = dec.image_norm_batch_device(dtype, scale=scale, bias=bias, mirror=mirror, out=view, channels=4, planar=planar, alpha_from_planes=True)
                assert got is view and np.array_equal(NR.bits(view), want), (what, size, planar, fl)
                assert bool((raw[~mask] == SENTINEL).all()), (what, size, planar, fl, "a byte outside the pixels changed")
        # three channels with a constant-free call, contiguous output
        got = dec.image_norm_batch_device(dtype, scale=scale, bias=bias, mirror=flags)
        assert np.array_equal(NR.bits(got), _batch_want(refs, alpha, size, origins, dtype, scale, bias, flags, channels=3)), (what, size)
    # each frame equals its single-image result: the 13 x 11 pixel windows (or the whole 8 x 8 frames) on a second handle
    size, origins = PX.origin_sets(w, h, n)[0]
    dec.begin_batch(w, h, n)
    dec.set_batch_windows(origins, *size, px=True)
    _decode_batch(dec, refs)
    batch = dec.image_norm_batch_device(dtype, scale=scale, bias=bias, mirror=flags, channels=4, alpha=9)
    for f in range(n):
        dec2.begin(w, h)
        dec2.set_window(*origins[f], *size, px=True)
        _decode(dec2, refs[f], None, "per_pass")
        one = dec2.image_norm_device(dtype, scale=scale, bias=bias, mirror=flags[f], channels=4, alpha=9)
        assert torch.equal(batch[f].view(torch.int16 if dtype != "float32" else torch.int32), one.view(torch.int16 if dtype != "float32" else torch.int32)), f


def test_two_batches_back_to_back_read_their_own_tables(dec, oracle_built):
    w, h, kind, n = 136, 264, "mixed", 3
    refs_a, refs_b = BW.batch_references(w, h, kind, n), BW.batch_references(w, h, kind, n, second=True)
    size, o_a, o_b = (13, 11), [(3, 5), (123, 253), (61, 59)], [(70, 9), (1, 130), (122, 2)]
    f_a, f_b = [True, False, True], [False, True, True]
    scale, bias = SETS["A"]
    dec.begin_batch(w, h, n)
    dec.set_batch_windows(o_a, *size, px=True)
    _decode_batch(dec, refs_a, sync=False)
    out_a = dec.image_norm_batch_device("float16", scale=scale, bias=bias, mirror=f_a)          # queued; the next batch's tables are written behind it
    dec.begin_batch(w, h, n)
    dec.set_batch_windows(o_b, *size, px=True)
    _decode_batch(dec, refs_b, sync=False)
    out_b = dec.image_norm_batch_device("float16", scale=scale, bias=bias, mirror=f_b)
    out_c = dec.image_norm_batch_device("float16", scale=scale, bias=bias, mirror=f_a)          # the same batch, other flags, no fence between
    dec.synchronize()
    want = lambda refs, o, fl: np.stack([NR.norm_ref(c, "float16", scale, bias, m) for c, m in zip(BW.crops(refs, size, o), fl)])
    assert np.array_equal(NR.bits(out_a), want(refs_a, o_a, f_a))
    assert np.array_equal(NR.bits(out_b), want(refs_b, o_b, f_b))
    assert np.array_equal(NR.bits(out_c), want(refs_b, o_b, f_a))
    assert not np.array_equal(NR.bits(out_b), NR.bits(out_c))


# ---- 4: RGBA from an encoder's planes ----------------------------------------------------------------------------------------------------------
def test_rgba_from_the_encoders_alpha_planes(dec, oracle_built):
    torch = _torch()
    from tests.test_gpu_encode_streams_batch import _rgba_frames, _u8
    from yaik_amd.encoder import HipTileEncoder
    w, h, n = 264, 136, 4
    origins, size = [(3, 5), (w - 100, h - 37), (61, 59), (120, 2)], (100, 37)
    enc = HipTileEncoder(0)
    try:
        enc.set_batch_u8(_u8(_rgba_frames(w, h)))
        enc.encode_batch(3, False)
        dec.begin_batch(w, h, n)
        dec.decode_batch_from_encoder(enc, alpha=True)
        whole = dec.image_batch_device(channels=4, alpha_from_planes=True).cpu().numpy()
        assert whole[..., 3].min() == 0 and whole[..., 3].max() == 255
        for dtype in NR.DTYPES:
            for name in ("A", "B"):
                scale, bias = SETS[name]
                got = dec.image_norm_batch_device(dtype, scale=scale, bias=bias, mirror=FLAGS, channels=4, alpha_from_planes=True, planar=True)
                want = np.stack([NR.norm_ref(whole[f], dtype, scale, bias, FLAGS[f]) for f in range(n)]).transpose(0, 3, 1, 2)
                assert np.array_equal(NR.bits(got), want), (dtype, name)
        dec.begin_batch(w, h, n)
        dec.decode_batch_from_encoder(enc, alpha=True, windows=(origins, *size), px=True)
        for dtype in NR.DTYPES:
            scale, bias = SETS["B"]
            got = dec.image_norm_batch_device(dtype, scale=scale, bias=bias, mirror=FLAGS, channels=4, alpha_from_planes=True)
            want = np.stack([NR.norm_ref(whole[f, y0:y0 + size[1], x0:x0 + size[0]], dtype, scale, bias, FLAGS[f]) for f, (x0, y0) in enumerate(origins)])
            assert np.array_equal(NR.bits(got), want), dtype
    finally:
        enc.close()


# ---- 5: refusals -------------------------------------------------------------------------------------------------------------------------------
def _rc(fn, *args):
    return int(fn(*args))


def test_refusals_come_first_and_leave_the_handle_usable(dec, oracle_built):
    torch = _torch()
    from yaik_amd._lib import lib
    from yaik_amd.decoder import HipTileDecoder
    from yaik_amd.encoder import NormC
    L = lib()
    w, h, kind = 136, 264, "mixed"
    win = (3, 5, 13, 11)
    ww, wh = win[2:]
    f4 = lambda *v: (C.c_float * 4)(*v)
    good = NormC(1, f4(1, 1, 1, 1), f4(0, 0, 0, 0))
    out = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    p = out.data_ptr()
    assert p % 4 == 0
    single, batch = L.yk_decode_output_norm_device, L.yk_decode_output_norm_batch_device
    row = ww * 3 * 2                                                         # fp16 HWC3 rows
    fresh = HipTileDecoder(0)
    try:
        assert _rc(single, fresh._h, C.byref(good), 0, p, row, 0, 3, 255) == YK_ERR_STATE              # before any begin
        assert b"yk_decode_output_norm_device" in L.yk_last_error(fresh._h)
        assert _rc(batch, fresh._h, C.byref(good), None, p, row, 0, row * wh, 3, 255) == YK_ERR_STATE
        assert b"yk_decode_output_norm_batch_device" in L.yk_last_error(fresh._h)
    finally:
        fresh.close()
    pix, _ = _begin(dec, w, h, kind, win, True)                              # no 'ALPM' plane
    nan, inf = float("nan"), float("inf")
    bad_norms = [NormC(0, f4(1, 1, 1, 1), f4(0, 0, 0, 0)), NormC(4, f4(1, 1, 1, 1), f4(0, 0, 0, 0)), NormC(-1, f4(1, 1, 1, 1), f4(0, 0, 0, 0)),
                 NormC(1, f4(1, nan, 1, 1), f4(0, 0, 0, 0)), NormC(1, f4(1, 1, 1, 1), f4(0, 0, inf, 0)), NormC(1, f4(-inf, 1, 1, 1), f4(0, 0, 0, 0)),
                 NormC(1, f4(1, 1, 1, 2.0 ** -101), f4(0, 0, 0, 0)), NormC(1, f4(1, 1, 1, 1), f4(2.0 ** 101, 0, 0, 0)), NormC(1, f4(1, 1, 1e-45, 1), f4(0, 0, 0, 0))]
    for bad in bad_norms:                                                    # bad dtype, parameters outside the rule
        assert _rc(single, dec._h, C.byref(bad), 0, p, row, 0, 3, 255) == YK_ERR_BAD_ARG
        assert b"yk_decode_output_norm_device" in L.yk_last_error(dec._h)
    f32 = NormC(3, f4(1, 1, 1, 1), f4(0, 0, 0, 0))
    for args in ((None, 0, p, row, 0, 3, 255), (C.byref(good), 0, None, row, 0, 3, 255),                                        # NULL
                 (C.byref(good), 0, p + 1, row, 0, 3, 255), (C.byref(good), 0, p, row + 1, 0, 3, 255),                          # misaligned base and pitch
                 (C.byref(good), 0, p, ww * 2, ww * 2 * wh + 1, 3, 255), (C.byref(f32), 0, p + 2, ww * 12, 0, 3, 255),
                 (C.byref(f32), 0, p, ww * 12 + 2, 0, 3, 255),
                 (C.byref(good), 0, p, row - 2, 0, 3, 255), (C.byref(f32), 0, p, ww * 12 - 4, 0, 3, 255),                        # pitches too small, against elements
                 (C.byref(good), 0, p, ww * 2 - 2, ww * 2 * wh, 3, 255), (C.byref(good), 0, p, ww * 2, ww * 2 * wh - 2, 3, 255),
                 (C.byref(good), 0, p, row, 0, 5, 255), (C.byref(good), 0, p, ww * 8, 0, 4, 256), (C.byref(good), 0, p, ww * 8, 0, 4, -2)):
        assert _rc(single, dec._h, *args) == YK_ERR_BAD_ARG, args
    assert _rc(single, dec._h, C.byref(good), 0, p, ww * 8, 0, 4, -1) == YK_ERR_STATE                   # alpha = -1 without a decoded plane
    assert b"alpha" in L.yk_last_error(dec._h)
    assert _rc(batch, dec._h, C.byref(good), None, p, row, 0, row * wh, 3, 255) == YK_ERR_STATE         # the batch call on an image with a window
    assert b"yk_decode_output_norm_batch_device" in L.yk_last_error(dec._h)
    assert bool((out == SENTINEL).all())                                     # nothing was written
    got = dec.image_norm_device("float16", channels=3)                       # a good call still gives the reference
    assert np.array_equal(NR.bits(got), NR.norm_ref(pix[..., :3], "float16", 1.0, 0.0))
    # a batch with pixel windows
    n = 3
    refs = BW.batch_references(w, h, kind, n)
    origins = [(3, 5), (123, 253), (61, 59)]
    dec.begin_batch(w, h, n)
    dec.set_batch_windows(origins, ww, wh, px=True)
    _decode_batch(dec, refs)
    flags = (C.c_uint8 * 3)(1, 0, 1)
    assert _rc(single, dec._h, C.byref(good), 0, p, row, 0, 3, 255) == YK_ERR_STATE                     # the single call on a batch with windows
    assert b"yk_decode_output_norm_device" in L.yk_last_error(dec._h) and b"windows" in L.yk_last_error(dec._h)
    for args in ((C.byref(good), flags, p, row, 0, row * wh - 2, 3, 255), (C.byref(good), flags, p, row, 0, row * wh + 1, 3, 255),   # frame stride small, misaligned
                 (C.byref(good), flags, p, row - 2, 0, row * wh, 3, 255), (C.byref(good), flags, p, ww * 2, ww * 2 * wh, ww * 2 * wh * 3 - 2, 3, 255),
                 (C.byref(bad_norms[0]), flags, p, row, 0, row * wh, 3, 255), (C.byref(bad_norms[3]), flags, p, row, 0, row * wh, 3, 255)):
        assert _rc(batch, dec._h, *args) == YK_ERR_BAD_ARG, args
        assert b"yk_decode_output_norm_batch_device" in L.yk_last_error(dec._h)
    assert _rc(batch, dec._h, C.byref(good), flags, p, ww * 8, 0, ww * 8 * wh, 4, -1) == YK_ERR_STATE   # no decoded alpha planes
    assert bool((out == SENTINEL).all())
    got = dec.image_norm_batch_device("float16", mirror=[1, 0, 1])
    want = np.stack([NR.norm_ref(c, "float16", 1.0, 0.0, m) for c, m in zip(BW.crops(refs, (ww, wh), origins), (True, False, True))])
    assert np.array_equal(NR.bits(got), want)
    # a prepared image has no normalised output
    from tests.test_gpu_decode_prepared import _prepare
    from tests.test_gpu_decode_prepared import _refs as _prepared_refs
    ref, calls = _prepared_refs(w, h, kind)
    _prepare(dec, w, h, calls)
    assert _rc(single, dec._h, C.byref(good), 0, p, w * 6, 0, 3, 255) == YK_ERR_STATE
    assert b"prepared" in L.yk_last_error(dec._h) and bool((out == SENTINEL).all())
    assert np.array_equal(dec.render_window(*win, px=True).cpu().numpy(), ref.crop(win))


# ---- 6: .yaik files ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files():
    from yaik_amd import files as F
    F.set_device_palette(False)
    yield F
    F.set_device_palette(False)


def test_files_equal_the_reference_of_the_whole_file_decode(files):
    torch = _torch()
    from tests.golden.make_golden import PARTIAL
    from tests.test_gpu_decode_files_windows import _analog_alpha, _frames, _plane_subset
    w = h = 128
    rng = np.random.default_rng(128)
    rgb = _frames(w, h, "mixed", 3, False)
    rgba = np.stack([np.concatenate([rgb[f], _analog_alpha(w, h, rng)[..., None]], axis=2) for f in range(3)])
    fixture = np.ascontiguousarray(PARTIAL["pp_planemix128_rgb"]().astype(np.uint8).transpose(1, 2, 0))
    fallback = _plane_subset(files.encode_file_device(fixture))              # a plane-subset stream: the batch planner hands it to the single-image chain
    plain = [files.encode_file_device(rgba[f], emit_alpha=True) for f in range(3)]
    mixed = [plain[0], fallback, plain[2], files.encode_file_device(rgb[1])]
    scale, bias = SETS["B"]
    for strs, fallbacks in ((plain, 0), (mixed, 1)):
        n = len(strs)
        whole = files.decode_files_device(strs, channels=4).cpu().numpy()
        assert files.last_batch_info()["fallbacks"] == fallbacks
        flags = FLAGS[:n]
        for dtype in NR.DTYPES:
            for channels, planar in ((4, False), (3, True)):
                got = files.decode_files_norm_device(strs, dtype, scale=scale, bias=bias, mirror=flags, channels=channels, planar=planar)
                assert files.last_batch_info()["fallbacks"] == fallbacks
                want = np.stack([NR.norm_ref(whole[f][..., :channels], dtype, scale, bias, flags[f]) for f in range(n)])
                assert np.array_equal(NR.bits(got), want.transpose(0, 3, 1, 2) if planar else want), (fallbacks, dtype, channels)
            for (ww, wh), origins in PX.origin_sets(w, h, n)[:2]:            # 13 x 11 and 100 x 37, the far corner included
                want = np.stack([NR.norm_ref(whole[f, y0:y0 + wh, x0:x0 + ww], dtype, scale, bias, flags[f]) for f, (x0, y0) in enumerate(origins)])
                raw, view, mask = _padded(dtype, want.shape, False, True)
                assert files.decode_files_norm_device(strs, dtype, scale=scale, bias=bias, origins=origins, size=(ww, wh), mirror=flags, out=view, channels=4) is view
                assert files.last_batch_info()["fallbacks"] == fallbacks
                assert np.array_equal(NR.bits(view), want), (fallbacks, dtype, ww, wh)
                assert bool((raw[~mask] == SENTINEL).all())
    from yaik_amd.files import ERROR_NAMES, YaikFileError
    with pytest.raises(YaikFileError) as e:                                  # a window outside the image: refused before a slot is taken
        files.decode_files_norm_device(plain, "float16", origins=[(0, 0), (124, 0), (0, 0)], size=(13, 11))
    assert ERROR_NAMES[e.value.code] == "YAIK_DECIMG_INVALIDCTX"
    assert tuple(files.decode_files_norm_device(plain, "float32").shape) == (3, h, w, 3)               # and the slot is free


# ---- 7: the uint8 calls after the new ones -----------------------------------------------------------------------------------------------------
def test_uint8_calls_give_the_same_bytes_after_the_new_calls(dec, oracle_built):
    torch = _torch()
    w, h, kind = 136, 264, "mixed"
    ref, key = _refs(w, h, kind)
    dec.begin(w, h)
    _decode(dec, ref, key, "all_pass")
    before = dec.image_device().clone()
    dec.synchronize()
    dec.stage_ms(YK_STAGE_DEC_DETILE)
    for dtype in NR.DTYPES:
        dec.image_norm_device(dtype, scale=SETS["B"][0], bias=SETS["B"][1], mirror=True)
    dec.synchronize()
    assert dec.stage_ms(YK_STAGE_DEC_DETILE)[1] == 3                         # one de-tile interval per call
    assert torch.equal(dec.image_device(), before) and np.array_equal(before.cpu().numpy(), ref.rgb)
    n = 3
    refs = BW.batch_references(w, h, kind, n)
    origins = [(3, 5), (123, 253), (61, 59)]
    dec.begin_batch(w, h, n)
    dec.set_batch_windows(origins, 13, 11, px=True)
    _decode_batch(dec, refs)
    before = dec.image_batch_windows_device().clone()
    dec.stage_ms(YK_STAGE_DEC_DETILE)
    for dtype in NR.DTYPES:
        dec.image_norm_batch_device(dtype, scale=SETS["B"][0], bias=SETS["B"][1], mirror=[1, 1, 0], planar=True)
    dec.synchronize()
    assert dec.stage_ms(YK_STAGE_DEC_DETILE)[1] == 3
    assert torch.equal(dec.image_batch_windows_device(), before) and np.array_equal(before.cpu().numpy(), BW.crops(refs, (13, 11), origins))
