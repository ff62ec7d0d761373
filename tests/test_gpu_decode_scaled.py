"""Reduced-resolution outputs on the GPU (yk_decode_output_scaled_device, yk_decode_output_scaled_batch_device,
yk_decode_render_windows_scaled_device): every output equals box_reduce (tests/scaled_ref.py) of the oracle's whole decode, bit for bit
-- whole images on both gradient paths, every window of tests/window_cases.py, prepared images, batches -- in HWC and CHW, with RGB, a decoded
alpha plane and a constant alpha, into padded destinations whose other bytes stay untouched; level 0 writes what the full-size call writes;
the planes are only read; encoder streams at 1024 x 1024 and .yaik files against the reduction of their own full-size decode; every refusal is
decided on the host, writes nothing and leaves the handle usable.  tests/test_decode_scaled_cases.py shows on the CPU that these images tell
truncation, subsampling, ties rounded down and the chained average apart from the rule."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import prepared_cases as PC
from tests import scaled_ref as SR
from tests import window_cases as WC
from tests.images import edge_image

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
YK_ERR_BAD_ARG, YK_ERR_STATE = -2, -4
YK_STAGE_DEC_GRADIENT, YK_STAGE_DEC_1D, YK_STAGE_DEC_DETILE = 3, 4, 5
STAGES = (YK_STAGE_DEC_GRADIENT, YK_STAGE_DEC_1D, YK_STAGE_DEC_DETILE)
# the de-tile kernels take YK_DT_THREADS / 4 * YK_DT_K = 256 tiles per workgroup: 256 x 128 is two whole workgroups, 8 x 8 one tile,
# 136 x 264 (561 tiles) two whole workgroups and the last-workgroup path
WHOLE_WORKGROUPS = (256, 128, "mixed")
assert (WHOLE_WORKGROUPS[0] // 8) * (WHOLE_WORKGROUPS[1] // 8) % 256 == 0
IMAGES = WC.CASES + [WHOLE_WORKGROUPS]
# eight windows of one size per prepared image: a duplicate pair, windows that share 64-blocks, the partial right block column and bottom block row
PREPARED = {(520, 264): (WC.SCAN_BLOCK_WINDOW[2:], [WC.SCAN_BLOCK_WINDOW[:2], WC.SCAN_BLOCK_WINDOW[:2], (0, 0), (64, 24), (328, 8), (328, 224), (0, 224), (136, 104)]),
            (136, 264): ((24, 16), [(0, 0), (0, 0), (8, 8), (112, 0), (112, 248), (56, 56), (0, 248), (56, 56)])}


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


_DEVICE_STREAMS = {}


def _refs(w, h, kind, second=False):
    """the oracle's reference of an image and the call list of its streams in device memory (uploaded once per image, kept alive here)"""
    torch = _torch()
    key = (w, h, kind, second)
    ref = WC.reference(w, h, kind, second)
    if key not in _DEVICE_STREAMS:
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
        _DEVICE_STREAMS[key] = (keep, calls)
    return ref, _DEVICE_STREAMS[key][1]


def _decode(d, ref, calls, path):
    """per_pass: decompress_gradient per pass + decompress_1d on host streams; all_pass: decode_streams on the uploaded streams"""
    if path == "per_pass":
        for sx, sy, cnt, bm, rgb in ref.passes:
            if cnt:
                d.decompress_gradient(sx, sy, bm, rgb)
        d.decompress_1d(ref.typ, ref.pix)
    else:
        d.decode_streams(calls, remap_range=0)


def _np(t):
    return t.cpu().numpy()


def _counts(d):
    """the intervals of the three decode stages since the last look (synchronises)"""
    d.synchronize()
    return tuple(d.stage_ms(s)[1] for s in STAGES)


def _padded(shape, planar, pad=11, off=1):
    """a sentinel-filled buffer and a view of `shape` ([..., h, w, C], or [..., C, h, w] with planar) with row, plane and frame padding, `off`
    bytes into it; returns buf, view and the same pair in numpy"""
    torch = _torch()
    if planar:
        c, hh, ww = shape[-3:]
        row = ww + pad
        plane = row * hh + 13
        frame = c * plane + 29
        strides = (plane, row, 1)
    else:
        hh, ww, c = shape[-3:]
        row = ww * c + pad
        frame = row * hh + 29
        strides = (row, c, 1)
    k = shape[0] if len(shape) == 4 else 1
    if len(shape) == 4:
        strides = (frame,) + strides
    n = off + k * frame + 64
    buf = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
    view = torch.as_strided(buf, shape, strides, off)
    nbuf = np.full(n, SENTINEL, np.uint8)
    nview = np.lib.stride_tricks.as_strided(nbuf[off:], shape, strides)
    return buf, view, nbuf, nview


def _chw(a):
    return np.ascontiguousarray(np.moveaxis(a, -1, -3))


def _with_alpha(rgb, a):
    return np.concatenate([rgb, a[..., None]], axis=-1)


# ---- whole images: every image, level and gradient path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["per_pass", "all_pass"])
@pytest.mark.parametrize("w,h,kind", IMAGES, ids=lambda v: str(v))
def test_whole_image_equals_the_reduced_oracle_decode(dec, oracle_built, w, h, kind, path):
    ref, calls = _refs(w, h, kind)
    dec.begin(w, h)
    _decode(dec, ref, calls, path)
    _counts(dec)
    for level in SR.LEVELS:
        got = dec.image_scaled_device(level)
        assert tuple(got.shape) == (h >> level, w >> level, 3)
        assert np.array_equal(_np(got), SR.box_reduce(ref.rgb, level)), level
        assert _counts(dec) == (0, 0, 1)                                     # one de-tile interval per scaled output
    assert np.array_equal(_np(dec.image_device()), ref.rgb)


@pytest.mark.parametrize("w,h,kind", [(136, 264, "mixed"), (520, 264, "mixed")], ids=lambda v: str(v))
def test_layouts_alpha_sources_and_untouched_bytes(dec, oracle_built, w, h, kind):
    ref, calls = _refs(w, h, kind)
    dec.begin(w, h)
    _decode(dec, ref, calls, "all_pass")
    plane = SR.alpha_plane(w, h)
    assert np.array_equal(dec.decompress_alpha(6, (0, 0, w, h), plane.ravel()), plane)
    for level in SR.LEVELS:
        rgb, a = SR.box_reduce(ref.rgb, level), SR.box_reduce(plane, level)
        for channels, a_arg, want in ((3, None, rgb), (4, None, _with_alpha(rgb, a)), (None, None, _with_alpha(rgb, a)),
                                      (4, 200, _with_alpha(rgb, np.full(a.shape, 200, np.uint8)))):
            for planar in (False, True):
                exp = _chw(want) if planar else want
                got = dec.image_scaled_device(level, channels=channels, alpha=a_arg, planar=planar)
                assert np.array_equal(_np(got), exp), (level, channels, a_arg, planar)
                buf, view, nbuf, nview = _padded(exp.shape, planar)
                assert dec.image_scaled_device(level, out=view, channels=channels, alpha=a_arg, planar=planar) is view
                nview[...] = exp
                assert np.array_equal(_np(buf), nbuf), (level, channels, a_arg, planar)      # every sentinel byte is unchanged


# ---- windows ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,kind,win", WC.all_case_windows(), ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_window_equals_the_reduced_oracle_crop(dec, oracle_built, w, h, kind, win):
    ref, calls = _refs(w, h, kind)
    x0, y0, ww, wh = win
    plane = SR.alpha_plane(w, h)
    dec.begin(w, h)
    dec.set_window(*win)
    _decode(dec, ref, calls, "per_pass" if (x0 + y0 + ww) & 8 else "all_pass")
    for level in SR.LEVELS:
        got = dec.image_scaled_device(level)
        assert tuple(got.shape) == (wh >> level, ww >> level, 3)
        assert np.array_equal(_np(got), SR.box_reduce(ref.crop(win), level)), level
        # the reduced window is the crop of the reduced image
        assert np.array_equal(_np(got), SR.box_reduce(ref.rgb, level)[y0 >> level:(y0 + wh) >> level, x0 >> level:(x0 + ww) >> level])
    dec.decompress_alpha(6, (0, 0, w, h), plane.ravel(), to_host=False)      # the 'ALPM' plane stays whole and is read at the window's offset
    for level in SR.LEVELS:
        want = _with_alpha(SR.box_reduce(ref.crop(win), level), SR.box_reduce(plane[y0:y0 + wh, x0:x0 + ww], level))
        assert np.array_equal(_np(dec.image_scaled_device(level, planar=True)), _chw(want)), level
    assert np.array_equal(_np(dec.image_window_device(channels=3)), ref.crop(win))


# ---- level 0 ----------------------------------------------------------------------------------------------------------------------------------
def test_level_0_writes_what_the_full_size_calls_write(dec, dec2, oracle_built):
    torch = _torch()
    w, h, kind = 136, 264, "mixed"
    ref, calls = _refs(w, h, kind)
    plane = SR.alpha_plane(w, h)
    dec.begin(w, h)
    _decode(dec, ref, calls, "all_pass")
    dec.decompress_alpha(6, (0, 0, w, h), plane.ravel(), to_host=False)
    for channels, a_arg, planar in ((3, None, False), (4, None, True), (4, 77, False)):
        full = dec.image_device(channels=channels, alpha=a_arg, planar=planar)
        assert torch.equal(dec.image_scaled_device(0, channels=channels, alpha=a_arg, planar=planar), full)
    win = (56, 56, 24, 16)
    dec.begin(w, h)
    dec.set_window(*win)
    _decode(dec, ref, calls, "all_pass")
    assert torch.equal(dec.image_scaled_device(0), dec.image_window_device()) and np.array_equal(_np(dec.image_scaled_device(0)), ref.crop(win))
    # a batch
    frames = _batch_refs()
    _decode_batch(dec2, frames)
    for channels, planar, from_planes in ((3, False, False), (4, True, False), (4, False, True)):
        full = dec2.image_batch_device(channels=channels, alpha=9, planar=planar, alpha_from_planes=from_planes)
        assert torch.equal(dec2.image_scaled_batch_device(0, channels=channels, alpha=9, planar=planar, alpha_from_planes=from_planes), full)
    # a prepared image
    (ww, wh), origins = PREPARED[(w, h)]
    dec.begin(w, h)
    dec.prepare(calls, remap_range=0)
    full = dec.render_windows(origins, ww, wh)
    assert torch.equal(dec.render_windows_scaled(0, origins, ww, wh), full)
    assert np.array_equal(_np(full), np.stack([ref.crop((x0, y0, ww, wh)) for x0, y0 in origins]))


# ---- prepared images --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(520, 264), (136, 264)])
def test_prepared_image_one_call_for_eight_reduced_windows(dec, oracle_built, w, h):
    from yaik_amd._lib import YaikError
    ref, calls = _refs(w, h, "mixed")
    (ww, wh), origins = PREPARED[(w, h)]
    assert len(origins) == 8 and len(set(origins)) < 8
    plane = SR.alpha_plane(w, h)
    crops = [ref.crop((x0, y0, ww, wh)) for x0, y0 in origins]
    want = {level: np.stack([SR.box_reduce(c, level) for c in crops]) for level in SR.LEVELS}
    mask = PC.block_mask(w, h, origins, ww, wh)
    total = mask.size
    assert mask[:, -1].any() and mask[-1, :].any() and int(mask.sum()) < sum(int(PC.block_mask(w, h, [o], ww, wh).sum()) for o in origins)
    dec.begin(w, h)
    dec.prepare(calls, remap_range=0)
    _counts(dec)
    first = dec.render_windows_scaled(1, origins, ww, wh)
    assert tuple(first.shape) == (8, wh >> 1, ww >> 1, 3) and np.array_equal(_np(first), want[1])
    assert _counts(dec) == (1, 1, 1)                                         # the new blocks at full size, then the reduced de-tile
    assert dec.prepared_blocks == (int(mask.sum()), total)                   # every block once
    assert np.array_equal(_np(dec.render_windows(origins, ww, wh)), np.stack(crops))     # a full-size call between them is still exact
    assert _counts(dec) == (0, 0, 1)
    for level in (3, 2):                                                     # another level over the same windows: a de-tile and nothing else
        assert np.array_equal(_np(dec.render_windows_scaled(level, origins, ww, wh)), want[level]), level
        assert _counts(dec) == (0, 0, 1), level
    assert dec.prepared_blocks == (int(mask.sum()), total)
    # the single-image call refuses on a prepared image, and a correct render follows
    with pytest.raises(YaikError, match="yk_decode_render_windows_scaled_device") as e:
        dec.image_scaled_device(1)
    assert f"error {YK_ERR_STATE}" in str(e.value)
    assert _counts(dec) == (0, 0, 0)
    # alpha from a plane decoded after prepare, CHW, a padded destination; then a constant alpha
    dec.decompress_alpha(6, (0, 0, w, h), plane.ravel(), to_host=False)
    a_crops = [plane[y0:y0 + wh, x0:x0 + ww] for x0, y0 in origins]
    for level in SR.LEVELS:
        exp = _chw(np.stack([_with_alpha(SR.box_reduce(c, level), SR.box_reduce(a, level)) for c, a in zip(crops, a_crops)]))
        buf, view, nbuf, nview = _padded(exp.shape, True)
        assert dec.render_windows_scaled(level, origins, ww, wh, out=view, planar=True) is view
        nview[...] = exp
        assert np.array_equal(_np(buf), nbuf), level
        assert np.array_equal(_np(dec.render_windows_scaled(level, origins, ww, wh, channels=4, alpha=31))[..., 3], np.full(want[level].shape[:3], 31, np.uint8))
    whole = dec.render_windows_scaled(2, [(0, 0)], w, h, channels=3)
    assert np.array_equal(_np(whole[0]), SR.box_reduce(ref.rgb, 2)) and dec.prepared_blocks == (total, total)
    assert np.array_equal(dec.planes(), ref.planes)


# ---- batches ----------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch_refs():
    """three frames of 136 x 264 with different content"""
    w, h = 136, 264
    return (WC.reference(w, h, "mixed"), WC.reference(w, h, "mixed", True), WC.Reference(edge_image(w, h, "photo", 3, seed=w + h)))


def _batch_alpha(w, h):
    """per frame: the analog plane, the same upside down, no chunk (the constant 201)"""
    a = SR.alpha_plane(w, h)
    return [a, np.ascontiguousarray(a[::-1]), np.full((h, w), 201, np.uint8)]


def _decode_batch(d, frames):
    w, h = frames[0].w, frames[0].h
    d.begin_batch(w, h, len(frames))
    d.decode_batch_streams([[("g", sx, sy, bm, bm.size, rgb, rgb.size) for sx, sy, cnt, bm, rgb in r.passes] + [("1", r.typ, r.typ.size, r.pix, r.pix.size)]
                            for r in frames], remap_range=0)
    planes = _batch_alpha(w, h)
    d.decompress_alpha_batch([(6, (0, 0, w, h), planes[0].ravel()), (6, (0, 0, w, h), planes[1].ravel()), None], 201)


def test_batch_every_frame_equals_its_reduced_oracle_decode(dec, oracle_built):
    frames = _batch_refs()
    w, h = frames[0].w, frames[0].h
    assert not np.array_equal(frames[0].rgb, frames[1].rgb) and not np.array_equal(frames[0].rgb, frames[2].rgb)
    _decode_batch(dec, frames)
    alphas = _batch_alpha(w, h)
    _counts(dec)
    for level in SR.LEVELS:
        rgb = np.stack([SR.box_reduce(r.rgb, level) for r in frames])
        a = np.stack([SR.box_reduce(p, level) for p in alphas])
        for channels, a_const, from_planes, want in ((3, 255, False, rgb), (4, 200, False, _with_alpha(rgb, np.full(a.shape, 200, np.uint8))),
                                                      (4, 255, True, _with_alpha(rgb, a))):
            for planar in (False, True):
                exp = _chw(want) if planar else want
                got = dec.image_scaled_batch_device(level, channels=channels, alpha=a_const, planar=planar, alpha_from_planes=from_planes)
                assert np.array_equal(_np(got), exp), (level, channels, from_planes, planar)
                assert _counts(dec) == (0, 0, 1)
                buf, view, nbuf, nview = _padded(exp.shape, planar)
                assert dec.image_scaled_batch_device(level, out=view, channels=channels, alpha=a_const, planar=planar, alpha_from_planes=from_planes) is view
                nview[...] = exp
                assert np.array_equal(_np(buf), nbuf), (level, channels, from_planes, planar)   # the bytes between rows, planes and frames are untouched
                _counts(dec)
    # the selected frame through the single-image call
    dec.select_frame(1)
    assert np.array_equal(_np(dec.image_scaled_device(2, channels=4, alpha=-1)), _with_alpha(SR.box_reduce(frames[1].rgb, 2), SR.box_reduce(alphas[1], 2)))
    dec.select_frame(0)


# ---- the planes are only read -----------------------------------------------------------------------------------------------------------------
def test_the_planes_are_only_read(dec, oracle_built):
    w, h, kind = 520, 264, "mixed"
    ref, calls = _refs(w, h, kind)
    dec.begin(w, h)
    _decode(dec, ref, calls, "all_pass")
    before = dec.planes()
    for level in SR.LEVELS:
        dec.image_scaled_device(level)
        dec.image_scaled_device(level, channels=4, alpha=5, planar=True)
    assert np.array_equal(dec.planes(), before) and np.array_equal(before, ref.planes)
    assert np.array_equal(_np(dec.image_device()), ref.rgb)
    assert np.array_equal(dec.tile4x4(), ref.tile4)


# ---- encoder streams at 1024 x 1024 -----------------------------------------------------------------------------------------------------------
def _torch_reduce(t, level):
    """the rule in torch integers, on an [..., H, W, C] uint8 tensor"""
    torch = _torch()
    s = 1 << level
    hh, ww, c = t.shape[-3:]
    v = t.to(torch.int32).reshape(t.shape[:-3] + (hh // s, s, ww // s, s, c)).sum(dim=(-2, -4))
    return ((v + (s * s) // 2) >> (2 * level)).to(torch.uint8)


def test_encoder_streams_1024(dec):
    torch = _torch()
    from yaik_amd.encoder import HipTileEncoder
    from yaik_amd.synth import synth_planes
    n = 1024
    enc = HipTileEncoder(0)
    try:
        enc.set_image(synth_planes(n, n_planes=3))
        enc.encode(3, False, False)
        dec.begin(n, n)
        dec.decode_from_encoder(enc)
        whole = dec.image_device()
        for level in SR.LEVELS:
            got = dec.image_scaled_device(level)
            assert tuple(got.shape) == (n >> level, n >> level, 3) and torch.equal(got, _torch_reduce(whole, level)), level
            assert torch.equal(dec.image_scaled_device(level, planar=True), _torch_reduce(whole, level).permute(2, 0, 1))
        assert torch.equal(dec.image_device(), whole)
        dec.begin(n, n)
        dec.prepare_from_encoder(enc)
        origins = [(0, 0), (888, 952), (440, 512), (440, 512)]
        got = dec.render_windows_scaled(3, origins, 136, 72)
        for k, (x0, y0) in enumerate(origins):
            assert torch.equal(got[k], _torch_reduce(whole[y0:y0 + 72, x0:x0 + 136], 3)), (x0, y0)
    finally:
        dec.synchronize()
        enc.close()


# ---- files ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def files():
    from yaik_amd import files as F
    F.set_device_palette(False)
    yield F
    F.set_device_palette(False)


@pytest.fixture(scope="module")
def file_streams(files):
    """(rgb, rgba): streams of a 136 x 264 "mixed" frame from encode_file_device without and with an 'ALPM' chunk (the analog alpha plane)"""
    torch = _torch()
    w, h = 136, 264
    colour = edge_image(w, h, "mixed", 3).astype(np.uint8)
    hwc = torch.from_numpy(np.ascontiguousarray(np.concatenate([colour, SR.alpha_plane(w, h)[None]]).transpose(1, 2, 0))).cuda()
    rgb = files.encode_file_device(hwc[..., :3].contiguous())
    rgba = files.encode_file_device(hwc, emit_alpha=True)
    assert not files.has_alpha_chunk(rgb) and files.has_alpha_chunk(rgba)
    return rgb, rgba


def test_files_equal_the_reduction_of_the_whole_file_decode(files, file_streams):
    torch = _torch()
    w, h = 136, 264
    for stream, c in zip(file_streams, (3, 4)):
        whole = files.decode_file_device(stream)
        assert tuple(whole.shape) == (h, w, c)
        assert torch.equal(files.decode_file_scaled_device(stream, 0), whole)
        for level in SR.LEVELS:
            got = files.decode_file_scaled_device(stream, level)
            assert tuple(got.shape) == (h >> level, w >> level, c) and torch.equal(got, _torch_reduce(whole, level)), (c, level)
        assert torch.equal(files.decode_file_device(stream), whole)          # the slot's handle goes back to whole images
    assert len(torch.unique(whole[..., 3])) > 16                             # the alpha that was averaged is analog, not a mask


def test_file_level_4_is_refused(files, file_streams):
    torch = _torch()
    stream = file_streams[0]
    with pytest.raises(ValueError, match="level"):
        files.decode_file_scaled_device(stream, 4)
    # the library's own refusal: YAIK_DECIMG_INVALIDCTX, nothing written, the slot released
    L, lib_handle = files.host_lib(), files.library()
    src = np.frombuffer(stream, dtype=np.uint8)
    for level in (4, -1):
        info = files.DecodedImage()
        assert L.YAIK_DecodeImagePre(lib_handle, src.ctypes.data, src.size, C.byref(info))
        out = torch.full((info.height, info.width, 3), SENTINEL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        info.outputImage, info.outputImageStride = out.data_ptr(), info.width * 3
        assert not L.YAIK_DecodeImageScaledToDevice(src.ctypes.data, src.size, C.byref(info), level)
        assert files.ERROR_NAMES[L.YAIK_GetErrorCode()] == "YAIK_DECIMG_INVALIDCTX"
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all())
    assert tuple(files.decode_file_scaled_device(stream, 3).shape) == (33, 17, 3)


# ---- refusals: decided on the host, nothing written, the handle usable --------------------------------------------------------------------------
def _rc(fn, *args):
    return int(fn(*args))


def test_refusals_write_nothing_and_a_correct_call_follows(dec, dec2, oracle_built):
    torch = _torch()
    from yaik_amd._lib import lib
    from yaik_amd.decoder import HipTileDecoder
    L = lib()
    w, h, kind = 136, 264, "mixed"
    ref, calls = _refs(w, h, kind)
    level = 2
    rw, rh = w >> level, h >> level
    out = torch.full((4 * rw * rh * 4 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    p = out.data_ptr()
    one = lambda d, *a: _rc(L.yk_decode_output_scaled_device, d._h, *a)
    batch = lambda d, *a: _rc(L.yk_decode_output_scaled_batch_device, d._h, *a)
    xy = (C.c_int * 4)(56, 56, 0, 0)
    render = lambda d, *a: _rc(L.yk_decode_render_windows_scaled_device, d._h, *a)

    def untouched(*ds):
        for d in ds:
            d.synchronize()
        assert bool((out == SENTINEL).all())

    fresh = HipTileDecoder(0)
    try:                                                                      # before any begin
        assert one(fresh, level, p, rw * 3, 0, 3, 0) == YK_ERR_STATE and b"yk_decode_begin" in L.yk_last_error(fresh._h)
        assert batch(fresh, level, p, rw * 3, 0, rw * 3 * rh, 3, 0) == YK_ERR_STATE
        assert render(fresh, level, 1, xy, 24, 16, p, 18, 0, 18 * 4, 3, 0) == YK_ERR_STATE
        untouched(fresh)
    finally:
        fresh.close()
    # the single image
    dec.begin(w, h)
    _decode(dec, ref, calls, "all_pass")
    _counts(dec)
    assert render(dec, level, 1, xy, 24, 16, p, 18, 0, 18 * 4, 3, 0) == YK_ERR_STATE      # a render call before prepare
    assert b"yk_decode_prepare_device" in L.yk_last_error(dec._h)
    for bad in (-1, 4):
        assert one(dec, bad, p, w * 3, 0, 3, 0) == YK_ERR_BAD_ARG and b"level" in L.yk_last_error(dec._h)
    assert one(dec, level, p, rw * 3 - 1, 0, 3, 0) == YK_ERR_BAD_ARG                      # a pitch one byte short of w >> level pixels
    assert one(dec, level, p, rw * 4 - 1, 0, 4, 0) == YK_ERR_BAD_ARG
    assert one(dec, level, p, rw - 1, rw * rh, 3, 0) == YK_ERR_BAD_ARG
    assert one(dec, level, p, rw, rw * rh - 1, 3, 0) == YK_ERR_BAD_ARG                    # planeBytes too small for the reduced plane
    assert one(dec, level, None, rw * 3, 0, 3, 0) == YK_ERR_BAD_ARG
    assert one(dec, level, p, rw * 3, 0, 2, 0) == YK_ERR_BAD_ARG
    assert one(dec, level, p, rw * 4, 0, 4, 256) == YK_ERR_BAD_ARG
    assert one(dec, level, p, rw * 4, 0, 4, -1) == YK_ERR_STATE                           # alpha = -1 without a decoded plane
    assert _counts(dec) == (0, 0, 0)
    untouched(dec)
    assert one(dec, level, p, rw * 3, 0, 3, 0) == 0                                       # the pitches of the REDUCED image are enough
    dec.synchronize()
    assert np.array_equal(_np(out[:rw * rh * 3]).reshape(rh, rw, 3), SR.box_reduce(ref.rgb, level)) and bool((out[rw * rh * 3:] == SENTINEL).all())
    assert one(dec, level, p, rw, rw * rh, 3, 0) == 0
    dec.synchronize()
    assert np.array_equal(_np(out[:rw * rh * 3]).reshape(3, rh, rw), _chw(SR.box_reduce(ref.rgb, level))) and bool((out[rw * rh * 3:] == SENTINEL).all())
    out.fill_(SENTINEL)
    # a batch
    frames = _batch_refs()
    dec2.begin_batch(w, h, 3)
    dec2.decode_batch_streams([[("g", sx, sy, bm, bm.size, rgb, rgb.size) for sx, sy, cnt, bm, rgb in r.passes] + [("1", r.typ, r.typ.size, r.pix, r.pix.size)]
                               for r in frames], remap_range=0)
    _counts(dec2)
    for bad in (-1, 4):
        assert batch(dec2, bad, p, w * 3, 0, w * 3 * h, 3, 0) == YK_ERR_BAD_ARG
    assert batch(dec2, level, p, rw * 3 - 1, 0, rw * 3 * rh, 3, 0) == YK_ERR_BAD_ARG
    assert batch(dec2, level, p, rw * 3, 0, rw * 3 * rh - 1, 3, 0) == YK_ERR_BAD_ARG       # frameBytes too small for a reduced frame
    assert b"frame stride" in L.yk_last_error(dec2._h)
    assert batch(dec2, level, p, rw, rw * rh - 1, rw * rh * 3, 3, 0) == YK_ERR_BAD_ARG
    assert batch(dec2, level, p, rw, rw * rh, rw * rh * 3 - 1, 3, 0) == YK_ERR_BAD_ARG
    assert batch(dec2, level, None, rw * 3, 0, rw * 3 * rh, 3, 0) == YK_ERR_BAD_ARG
    assert batch(dec2, level, p, rw * 3, 0, rw * 3 * rh, 2, 0) == YK_ERR_BAD_ARG
    assert batch(dec2, level, p, rw * 4, 0, rw * 4 * rh, 4, -2) == YK_ERR_BAD_ARG
    assert batch(dec2, level, p, rw * 4, 0, rw * 4 * rh, 4, -1) == YK_ERR_STATE            # no alpha planes were decoded for this batch
    assert _counts(dec2) == (0, 0, 0)
    untouched(dec2)
    assert batch(dec2, level, p, rw * 3, 0, rw * 3 * rh, 3, 0) == 0
    dec2.synchronize()
    assert np.array_equal(_np(out[:3 * rw * rh * 3]).reshape(3, rh, rw, 3), np.stack([SR.box_reduce(r.rgb, level) for r in frames]))
    assert bool((out[3 * rw * rh * 3:] == SENTINEL).all())
    out.fill_(SENTINEL)
    # a prepared image: windows of 24 x 16, reduced to 6 x 4
    dec.begin(w, h)
    dec.prepare(calls, remap_range=0)
    _counts(dec)
    for bad in (-1, 4):
        assert render(dec, bad, 2, xy, 24, 16, p, 72, 0, 72 * 16, 3, 0) == YK_ERR_BAD_ARG
    assert render(dec, level, 2, xy, 24, 16, p, 17, 0, 18 * 4, 3, 0) == YK_ERR_BAD_ARG
    assert render(dec, level, 2, xy, 24, 16, p, 18, 0, 18 * 4 - 1, 3, 0) == YK_ERR_BAD_ARG  # windowBytes too small for a reduced window
    assert b"window stride" in L.yk_last_error(dec._h)
    assert render(dec, level, 2, xy, 24, 16, p, 6, 6 * 4 - 1, 6 * 4 * 3, 3, 0) == YK_ERR_BAD_ARG
    assert render(dec, level, 2, xy, 24, 16, p, 6, 6 * 4, 6 * 4 * 3 - 1, 3, 0) == YK_ERR_BAD_ARG
    assert render(dec, level, 2, xy, 24, 16, None, 18, 0, 18 * 4, 3, 0) == YK_ERR_BAD_ARG
    assert render(dec, level, 2, xy, 24, 16, p, 18, 0, 18 * 4, 2, 0) == YK_ERR_BAD_ARG
    assert render(dec, level, 2, xy, 24, 16, p, 24, 0, 24 * 4, 4, -1) == YK_ERR_STATE
    assert render(dec, level, 2, None, 24, 16, p, 18, 0, 18 * 4, 3, 0) == YK_ERR_BAD_ARG
    assert render(dec, level, 2, (C.c_int * 4)(56, 56, 120, 0), 24, 16, p, 18, 0, 18 * 4, 3, 0) == YK_ERR_BAD_ARG   # a window outside the image
    assert render(dec, level, 2, (C.c_int * 4)(56, 56, 4, 0), 24, 16, p, 18, 0, 18 * 4, 3, 0) == YK_ERR_BAD_ARG
    assert one(dec, level, p, rw * 3, 0, 3, 0) == YK_ERR_STATE and b"yk_decode_render_windows_scaled_device" in L.yk_last_error(dec._h)
    assert _counts(dec) == (0, 0, 0) and dec.prepared_blocks == (0, 15)
    untouched(dec)
    assert render(dec, level, 2, xy, 24, 16, p, 18, 0, 18 * 4, 3, 0) == 0
    dec.synchronize()
    assert np.array_equal(_np(out[:2 * 72]).reshape(2, 4, 6, 3), np.stack([SR.box_reduce(ref.crop((56, 56, 24, 16)), level), SR.box_reduce(ref.crop((0, 0, 24, 16)), level)]))
    assert bool((out[2 * 72:] == SENTINEL).all())
