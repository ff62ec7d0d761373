"""Mip chains on the GPU (yk_decode_output_mipchain_device, yk_decode_output_mipchain_batch_device): every level of the whole chain
equals mip_reduce (tests/mipchain_ref.py) of the oracle's whole decode, bit for bit -- on both gradient paths, in HWC and CHW, with RGB, a decoded
alpha plane and a constant alpha, into padded destinations whose other bytes stay untouched; sub-ranges with and without tail levels; levels 0..3
are what the full-size and the scaled calls write; the planes are only read; batches and .yaik files; one de-tile interval per call; every
refusal is decided on the host, writes nothing and leaves the handle usable; and an all-white 8192 x 8192 image whose level-13 sum needs more than
32 bits.  tests/test_decode_mipchain_cases.py shows on the CPU that these images tell truncation and the chained average apart from the rule.

Shapes: 8 x 8 is one tile, a partial block and has no level above 3; 136 x 264 and 264 x 136 have partial blocks on both sides, remainders from
level 4 on and one tail level; 520 x 264 is 9 x 5 blocks with the tail levels 7 and 8 (level 8 is 2 x 1); 256 x 128 has whole blocks only."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import mipchain_ref as MR
from tests import scaled_ref as SR
from tests import window_cases as WC
from tests.images import edge_image

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
YK_ERR_BAD_ARG, YK_ERR_STATE = -2, -4
STAGES = (3, 4, 5)                                                          # YK_STAGE_DEC_GRADIENT, YK_STAGE_DEC_1D, YK_STAGE_DEC_DETILE


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def dec():
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    yield d
    d.close()


_DEVICE_STREAMS = {}


def _refs(w, h, kind):
    """the oracle's reference of an image and the call list of its streams in device memory (uploaded once per image, kept alive here)"""
    torch = _torch()
    key = (w, h, kind)
    ref = WC.reference(w, h, kind)
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


@functools.lru_cache(maxsize=None)
def _chain(w, h, kind):
    """mip_reduce of the oracle's decode and of the alpha plane at every level: computed once per image"""
    ref, plane = WC.reference(w, h, kind), SR.alpha_plane(w, h)
    n = len(MR.mip_dims(w, h))
    return [MR.mip_reduce(ref.rgb, k) for k in range(n)], [MR.mip_reduce(plane, k) for k in range(n)]


def _into_padded(call, wants, planar, **kw):
    """call(out=[padded views]) and compare every byte of every buffer: the pixels are `wants`, the rest is the sentinel"""
    bufs = [_padded(x.shape, planar) for x in wants]
    views = [b[1] for b in bufs]
    got = call(out=views, planar=planar, **kw)
    assert len(got) == len(views) and all(g is v for g, v in zip(got, views))
    for i, ((buf, view, nbuf, nview), want) in enumerate(zip(bufs, wants)):
        nview[...] = want
        assert np.array_equal(_np(buf), nbuf), i


# ---- whole chains: every image on both gradient paths -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["per_pass", "all_pass"])
@pytest.mark.parametrize("w,h,kind", MR.IMAGES, ids=lambda v: str(v))
def test_whole_chain_equals_the_reduced_oracle_decode(dec, oracle_built, w, h, kind, path):
    ref, calls = _refs(w, h, kind)
    rgb, _ = _chain(w, h, kind)
    dec.begin(w, h)
    _decode(dec, ref, calls, path)
    _counts(dec)
    assert dec.mip_levels() == len(rgb) == len(MR.mip_dims(w, h))
    got = dec.image_mipchain_device()
    assert _counts(dec) == (0, 0, 1)                                         # one de-tile interval, no gradient or 1-D interval
    assert len(got) == len(rgb)
    for k, (g, want) in enumerate(zip(got, rgb)):
        assert tuple(g.shape) == (h >> k, w >> k, 3)
        assert np.array_equal(_np(g), want), k
    assert np.array_equal(_np(got[0]), ref.rgb)


@pytest.mark.parametrize("w,h,kind", MR.IMAGES, ids=lambda v: str(v))
def test_layouts_alpha_sources_and_untouched_bytes(dec, oracle_built, w, h, kind):
    ref, calls = _refs(w, h, kind)
    rgb, a = _chain(w, h, kind)
    dec.begin(w, h)
    _decode(dec, ref, calls, "all_pass")
    dec.decompress_alpha(6, (0, 0, w, h), SR.alpha_plane(w, h).ravel(), to_host=False)
    rgba = [_with_alpha(c, p) for c, p in zip(rgb, a)]
    const = [_with_alpha(c, np.full(p.shape, 200, np.uint8)) for c, p in zip(rgb, a)]
    for channels, a_arg, wants in ((3, None, rgb), (None, None, rgba), (4, 200, const)):
        for planar in (False, True):
            exp = [_chw(x) for x in wants] if planar else wants
            got = dec.image_mipchain_device(channels=channels, alpha=a_arg, planar=planar)
            for k, (g, want) in enumerate(zip(got, exp)):
                assert np.array_equal(_np(g), want), (k, channels, a_arg, planar)
            _into_padded(dec.image_mipchain_device, exp, planar, channels=channels, alpha=a_arg)


# ---- sub-ranges ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,kind", [(520, 264, "mixed"), (136, 264, "mixed")], ids=lambda v: str(v))
def test_sub_ranges_and_the_planes_are_only_read(dec, oracle_built, w, h, kind):
    torch = _torch()
    ref, calls = _refs(w, h, kind)
    rgb, a = _chain(w, h, kind)
    top = len(rgb) - 1
    dec.begin(w, h)
    _decode(dec, ref, calls, "all_pass")
    dec.decompress_alpha(6, (0, 0, w, h), SR.alpha_plane(w, h).ravel(), to_host=False)
    before = dec.planes()
    _counts(dec)
    whole = dec.image_mipchain_device(channels=4)
    for first, count in ((4, 1), (5, 3), (7, top - 6), (0, 4), (4, 3), (3, None), (top, 1)):
        n = top + 1 - first if count is None else count
        for planar in (False, True):
            _counts(dec)
            got = dec.image_mipchain_device(first, count, channels=4, planar=planar)
            assert _counts(dec) == (0, 0, 1)
            assert len(got) == n
            for i, g in enumerate(got):
                want = _with_alpha(rgb[first + i], a[first + i])
                assert np.array_equal(_np(g), _chw(want) if planar else want), (first, count, i, planar)
                assert torch.equal(g.permute(1, 2, 0) if planar else g, whole[first + i])      # with or without a tail launch: the same bytes
            _into_padded(functools.partial(dec.image_mipchain_device, first, count), [_chw(_with_alpha(rgb[k], a[k])) if planar else _with_alpha(rgb[k], a[k])
                                                                                       for k in range(first, first + n)], planar, channels=4)
    # (0, 4) is the full-size call and the three scaled calls
    low = dec.image_mipchain_device(0, 4, channels=4, alpha=77, planar=True)
    assert torch.equal(low[0], dec.image_device(channels=4, alpha=77, planar=True))
    for k in (1, 2, 3):
        assert torch.equal(low[k], dec.image_scaled_device(k, channels=4, alpha=77, planar=True)), k
    assert np.array_equal(dec.planes(), before) and np.array_equal(before, ref.planes)
    assert np.array_equal(dec.tile4x4(), ref.tile4)


# ---- batches ------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batch_refs():
    """three frames of 136 x 264 with different content"""
    w, h = 136, 264
    return (WC.reference(w, h, "mixed"), WC.reference(w, h, "mixed", True), WC.Reference(edge_image(w, h, "photo", 3, seed=w + h)))


def _batch_alpha(w, h):
    """per frame: the analog plane, the same upside down, no chunk (the constant 201)"""
    a = SR.alpha_plane(w, h)
    return [a, np.ascontiguousarray(a[::-1]), np.full((h, w), 201, np.uint8)]


def _decode_batch(d, frames, with_alpha=True):
    w, h = frames[0].w, frames[0].h
    d.begin_batch(w, h, len(frames))
    d.decode_batch_streams([[("g", sx, sy, bm, bm.size, rgb, rgb.size) for sx, sy, cnt, bm, rgb in r.passes] + [("1", r.typ, r.typ.size, r.pix, r.pix.size)]
                            for r in frames], remap_range=0)
    if with_alpha:
        planes = _batch_alpha(w, h)
        d.decompress_alpha_batch([(6, (0, 0, w, h), planes[0].ravel()), (6, (0, 0, w, h), planes[1].ravel()), None], 201)


def test_batch_every_frame_equals_its_reduced_oracle_decode(dec, oracle_built):
    frames = _batch_refs()
    w, h = frames[0].w, frames[0].h
    n = len(MR.mip_dims(w, h))
    _decode_batch(dec, frames)
    alphas = _batch_alpha(w, h)
    rgb = [np.stack([MR.mip_reduce(r.rgb, k) for r in frames]) for k in range(n)]
    a = [np.stack([MR.mip_reduce(p, k) for p in alphas]) for k in range(n)]
    _counts(dec)
    for channels, a_const, from_planes, wants in ((3, 255, False, rgb), (4, 200, False, [_with_alpha(c, np.full(p.shape, 200, np.uint8)) for c, p in zip(rgb, a)]),
                                                  (4, 255, True, [_with_alpha(c, p) for c, p in zip(rgb, a)])):
        for planar in (False, True):
            exp = [_chw(x) for x in wants] if planar else wants
            got = dec.image_mipchain_batch_device(channels=channels, alpha=a_const, planar=planar, alpha_from_planes=from_planes)
            assert _counts(dec) == (0, 0, 1)
            for k, (g, want) in enumerate(zip(got, exp)):
                assert tuple(g.shape) == want.shape and np.array_equal(_np(g), want), (k, channels, from_planes, planar)
            _into_padded(dec.image_mipchain_batch_device, exp, planar, channels=channels, alpha=a_const, alpha_from_planes=from_planes)
            _into_padded(functools.partial(dec.image_mipchain_batch_device, 5, 3), exp[5:8], planar, channels=channels, alpha=a_const, alpha_from_planes=from_planes)
            _counts(dec)
    # the selected frame through the single-image call
    dec.select_frame(1)
    got = dec.image_mipchain_device(channels=4, alpha=-1)
    for k in range(n):
        assert np.array_equal(_np(got[k]), _with_alpha(rgb[k][1], a[k][1])), k
    dec.select_frame(0)
    # a batch without alpha planes: constants only
    _decode_batch(dec, frames, with_alpha=False)
    got = dec.image_mipchain_batch_device(4, None, channels=4, alpha=9)
    for k, g in enumerate(got, 4):
        assert np.array_equal(_np(g), _with_alpha(rgb[k], np.full(a[k].shape, 9, np.uint8))), k


# ---- files --------------------------------------------------------------------------------------------------------------------------------------
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


def test_files_equal_the_chain_of_the_whole_file_decode(files, file_streams):
    torch = _torch()
    w, h = 136, 264
    for stream, c in zip(file_streams, (3, 4)):
        whole = files.decode_file_device(stream)
        want = [MR.mip_reduce(_np(whole), k) for k in range(8)]
        got = files.decode_file_mipchain_device(stream)
        assert len(got) == 8 and torch.equal(got[0], whole)
        for k in range(8):
            assert tuple(got[k].shape) == (h >> k, w >> k, c) and np.array_equal(_np(got[k]), want[k]), (c, k)
        part = files.decode_file_mipchain_device(stream, 5, 2)
        assert len(part) == 2 and np.array_equal(_np(part[0]), want[5]) and np.array_equal(_np(part[1]), want[6])
        assert torch.equal(files.decode_file_device(stream), whole)          # the slot's handle goes back to whole images
    with pytest.raises(ValueError, match="levels"):
        files.decode_file_mipchain_device(file_streams[0], 8)
    with pytest.raises(ValueError, match="levels"):
        files.decode_file_mipchain_device(file_streams[0], 5, 4)
    # the library's own refusals: YAIK_DECIMG_INVALIDCTX, nothing written, the slot released
    L, lib_handle = files.host_lib(), files.library()
    src = np.frombuffer(file_streams[0], dtype=np.uint8)
    out = torch.full((h * w * 3,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for first, n, null_at in ((-1, 1, None), (0, 9, None), (8, 1, None), (0, 0, None), (0, 16, None), (4, 2, 1)):
        info = files.DecodedImage()
        assert L.YAIK_DecodeImagePre(lib_handle, src.ctypes.data, src.size, C.byref(info))
        images = (C.c_void_p * 16)(*[None if i == null_at else out.data_ptr() for i in range(16)])
        strides = (C.c_uint32 * 16)(*[w * 3] * 16)
        assert not L.YAIK_DecodeImageMipchainToDevice(src.ctypes.data, src.size, C.byref(info), first, n, images, strides)
        assert files.ERROR_NAMES[L.YAIK_GetErrorCode()] == "YAIK_DECIMG_INVALIDCTX"
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert [tuple(t.shape) for t in files.decode_file_mipchain_device(file_streams[0], 6)] == [(4, 2, 3), (2, 1, 3)]


# ---- refusals: decided on the host, nothing written, the handle usable ----------------------------------------------------------------------------
def test_refusals_write_nothing_and_a_correct_call_follows(dec, oracle_built):
    torch = _torch()
    from yaik_amd._lib import MipLevel, lib
    from yaik_amd.decoder import HipTileDecoder
    L = lib()
    w, h, kind = 136, 264, "mixed"
    ref, calls = _refs(w, h, kind)
    rgb, _ = _chain(w, h, kind)
    out = torch.full((w * h * 4 * 3 + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    p = out.data_ptr()

    def table(first, n, channels=3, planar=False, short_row=None, short_plane=None, null_at=None, mixed_at=None, frames=1, short_frame=None):
        """tight levels one after the other from p; level `short_*` is one byte short, `null_at` has no pointer, `mixed_at` the other layout"""
        t, at = (MipLevel * max(n, 1))(), p
        for i in range(n):
            lw, lh = w >> (first + i), h >> (first + i)
            pl = planar != (i == mixed_at)
            row = lw if pl else lw * channels
            plane = row * lh if pl else 0
            frame = row * lh * (channels if pl else 1)
            t[i] = MipLevel(None if i == null_at else at, row - (i == short_row), plane - (i == short_plane), frame - (i == short_frame))
            at += frame * frames
        return t

    one = lambda d, first, n, t, ch=3, al=0: int(L.yk_decode_output_mipchain_device(d._h, first, n, t, ch, al))
    batch = lambda d, first, n, t, ch=3, al=0: int(L.yk_decode_output_mipchain_batch_device(d._h, first, n, t, ch, al))

    def untouched(d):
        d.synchronize()
        assert bool((out == SENTINEL).all())

    fresh = HipTileDecoder(0)
    try:                                                                      # before any begin
        assert one(fresh, 0, 1, table(0, 1)) == YK_ERR_STATE and b"yk_decode_begin" in L.yk_last_error(fresh._h)
        assert batch(fresh, 0, 1, table(0, 1)) == YK_ERR_STATE
        untouched(fresh)
    finally:
        fresh.close()
    dec.begin(w, h)
    _decode(dec, ref, calls, "all_pass")
    _counts(dec)
    for call in (one, batch):
        for first, n in ((-1, 1), (8, 1), (0, 0), (0, 9), (0, 16), (5, 4), (7, 2)):      # the chain has levels 0..7; never more than 15
            assert call(dec, first, n, table(max(first, 0), min(n, 8))) == YK_ERR_BAD_ARG, (first, n)
            assert b"levels" in L.yk_last_error(dec._h)
        assert call(dec, 0, 8, None) == YK_ERR_BAD_ARG
        assert call(dec, 0, 8, table(0, 8, null_at=5)) == YK_ERR_BAD_ARG and b"NULL" in L.yk_last_error(dec._h)
        for lvl in (0, 4, 7):                                                 # a pitch one byte short of that level's own row
            assert call(dec, 0, 8, table(0, 8, short_row=lvl)) == YK_ERR_BAD_ARG and b"pitch" in L.yk_last_error(dec._h)
            assert call(dec, 0, 8, table(0, 8, 4, short_row=lvl), 4) == YK_ERR_BAD_ARG
            assert call(dec, 0, 8, table(0, 8, planar=True, short_row=lvl)) == YK_ERR_BAD_ARG
            assert call(dec, 0, 8, table(0, 8, planar=True, short_plane=lvl)) == YK_ERR_BAD_ARG
        assert call(dec, 0, 8, table(0, 8, mixed_at=3)) == YK_ERR_BAD_ARG and b"HWC" in L.yk_last_error(dec._h)
        assert call(dec, 0, 8, table(0, 8, planar=True, mixed_at=6)) == YK_ERR_BAD_ARG
        assert call(dec, 0, 8, table(0, 8), 2) == YK_ERR_BAD_ARG
        assert call(dec, 0, 8, table(0, 8, 4), 4, 256) == YK_ERR_BAD_ARG
        assert call(dec, 0, 8, table(0, 8, 4), 4, -1) == YK_ERR_STATE         # alpha = -1 without a decoded plane
    assert _counts(dec) == (0, 0, 0)
    untouched(dec)
    assert one(dec, 0, 8, table(0, 8)) == 0                                   # tight pitches of every level's own size are enough
    dec.synchronize()
    at = 0
    for k in range(8):
        n = rgb[k].size
        assert np.array_equal(_np(out[at:at + n]).reshape(rgb[k].shape), rgb[k]), k
        at += n
    assert bool((out[at:] == SENTINEL).all())
    out.fill_(SENTINEL)
    # a window set, then a prepared image: windows have no chain
    dec.begin(w, h)
    dec.set_window(56, 56, 24, 16)
    _decode(dec, ref, calls, "all_pass")
    _counts(dec)
    assert one(dec, 0, 1, table(0, 1)) == YK_ERR_STATE and b"windows have no chain" in L.yk_last_error(dec._h)
    assert _counts(dec) == (0, 0, 0)
    dec.begin(w, h)
    dec.prepare(calls, remap_range=0)
    _counts(dec)
    for call in (one, batch):
        assert call(dec, 0, 1, table(0, 1)) == YK_ERR_STATE and b"windows have no chain" in L.yk_last_error(dec._h)
    assert _counts(dec) == (0, 0, 0)
    untouched(dec)
    # a batch: the frame stride of a level, then a correct call
    frames = _batch_refs()
    _decode_batch(dec, frames, with_alpha=False)
    _counts(dec)
    for lvl in (0, 2):
        assert batch(dec, 4, 4, table(4, 4, frames=3, short_frame=lvl)) == YK_ERR_BAD_ARG and b"frame stride" in L.yk_last_error(dec._h)
        assert batch(dec, 4, 4, table(4, 4, planar=True, frames=3, short_frame=lvl)) == YK_ERR_BAD_ARG
    assert batch(dec, 4, 4, table(4, 4, 4, frames=3), 4, -1) == YK_ERR_STATE and b"alpha planes" in L.yk_last_error(dec._h)
    assert _counts(dec) == (0, 0, 0)
    untouched(dec)
    assert batch(dec, 4, 4, table(4, 4, frames=3)) == 0
    dec.synchronize()
    at = 0
    for k in range(4, 8):
        want = np.stack([MR.mip_reduce(r.rgb, k) for r in frames])
        assert np.array_equal(_np(out[at:at + want.size]).reshape(want.shape), want), k
        at += want.size
    assert bool((out[at:] == SENTINEL).all())


# ---- the wide-sum case ----------------------------------------------------------------------------------------------------------------------------
def test_all_white_8192_needs_sums_wider_than_32_bits(dec):
    """level 13 of 8192 x 8192 sums 2^26 bytes of 255: a 32-bit tail fails there"""
    torch = _torch()
    from yaik_amd.encoder import HipTileEncoder
    n = 8192
    enc = HipTileEncoder(0)
    try:
        enc.set_image_u8(torch.full((n, n, 3), 255, dtype=torch.uint8, device="cuda"))
        enc.encode(3, False, False)
        dec.begin(n, n)
        dec.decode_from_encoder(enc)
        whole = dec.image_device()
        white = int(whole[0, 0, 0])                                          # the codec is lossy: white decodes to 254 with these settings
        assert bool((whole == white).all()) and (white << 26) >= 1 << 32     # a constant whose level-13 sum does not fit 32 bits
        got = dec.image_mipchain_device()
        assert len(got) == 14 and torch.equal(got[0], whole)
        sums = whole.to(torch.int64).reshape(n // 64, 64, n // 64, 64, 3).sum(dim=(1, 3))      # the 64 x 64 box sums, then int64 all the way
        for k in range(1, 14):
            s = 1 << k
            if k < 6:
                v = whole.reshape(n // s, s, n // s, s, 3).sum(dim=(1, 3), dtype=torch.int64)
            else:
                r = 1 << (k - 6)
                v = sums.reshape(sums.shape[0] // r, r, sums.shape[1] // r, r, 3).sum(dim=(1, 3))
            want = ((v + (s * s) // 2) >> (2 * k)).to(torch.uint8)
            assert tuple(got[k].shape) == (n >> k, n >> k, 3) and torch.equal(got[k], want), k
            assert bool((got[k] == white).all()), k                          # the mean of a constant is that constant at every level
    finally:
        dec.synchronize()
        enc.close()
