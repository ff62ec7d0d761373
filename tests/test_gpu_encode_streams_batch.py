"""Batch stream builders (yk_encode_streams_batch + yk_batch_streams_table; HipTileEncoder.streams_batch, batch_calls_from_table and the default
path of HipTileDecoder.encoder_batch_streams): every frame's seven corner streams and two 1-D streams against the CPU oracle and against the
single-image path on the same and on a second handle, byte for byte; the packed layout; every refusal; reuse of a handle; stage timers; scale."""
import ctypes as C

import numpy as np
import pytest

from oracle.pyoracle import PASSES, OracleEncoder
from tests.images import edge_image
from tests.test_gpu_decode_batch import KINDS, _image
from yaik_amd._lib import YaikError
from yaik_amd.decoder import HipTileDecoder, batch_calls_from_table
from yaik_amd.encoder import HipTileEncoder, _FrameStreamsC

pytestmark = pytest.mark.gpu
YK_ERR_BAD_ARG, YK_ERR_STATE = -2, -4
YK_STAGE_CORNERS, YK_STAGE_RANGE1D, YK_STAGE_RANGE1D_PACK = 0, 1, 2


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


def _u8(images):
    """int32 planes [n, h, w] per frame -> torch uint8 [F, h, w, n] on the device"""
    return _torch().from_numpy(np.ascontiguousarray(np.stack([np.moveaxis(p, 0, -1) for p in images]).astype(np.uint8))).cuda()


def _encode_batch(enc, images):
    enc.set_batch_u8(_u8(images))
    enc.encode_batch(3, False)


def _single(e, f=None):
    """(7 corner streams, pix, type) of the selected frame through the single-image entry points"""
    if f is not None:
        e.select_frame(f)
    rgb = [e.gradient_corners(p) for p in range(7)]
    pix, typ = e.dynamic_tile_compressor()
    return rgb, pix, typ


def _same(row, want, what, corners=True, range1d=True):
    got = row.download()
    rgb, pix, typ = want
    for p in range(7):
        if corners:
            assert row.rgb_bytes[p] == rgb[p].size, (what, p, row.rgb_bytes[p], rgb[p].size)
            assert (row.rgb[p] == 0) == (rgb[p].size == 0), (what, p)
            assert np.array_equal(got["rgb"][p], rgb[p]), (what, "corner stream", p)
        else:
            assert row.rgb[p] == 0 and row.rgb_bytes[p] == 0, (what, p)
    if range1d:
        assert (row.pix_bytes, row.type_bytes) == (pix.size, typ.size), (what, row.pix_bytes, pix.size, row.type_bytes, typ.size)
        assert (row.pix == 0) == (pix.size == 0) and (row.type == 0) == (typ.size == 0), what
        assert np.array_equal(got["pix"], pix), (what, "1-D pixel stream")
        assert np.array_equal(got["type"], typ), (what, "1-D parameter stream")
    else:
        assert (row.pix, row.pix_bytes, row.type, row.type_bytes) == (0, 0, 0, 0), what


def _oracle(planes):
    o = OracleEncoder(planes)
    cnt, rgb = [], []
    for sx, sy in PASSES:
        n, _, raw = o.fitting_quad_smooth(sx, sy)
        cnt.append(n); rgb.append(np.asarray(raw, dtype=np.uint8))
    for p in range(3):
        o.dynamic_tile_compressor(p)
    pix, typ = o.streams_1d()
    return cnt, (rgb, np.asarray(pix, dtype=np.uint8), np.asarray(typ, dtype=np.uint8))


# ---- 1. oracle parity, degenerate frames between ordinary ones ------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(208, 144), (256, 256)])
def test_matches_oracle(enc, oracle_built, w, h):
    images = [_image(w, h, k, seed=7) for k in KINDS]
    want = [_oracle(p) for p in images]
    noise, flat = want[KINDS.index("noise")], want[KINDS.index("flat")]
    assert sum(noise[0]) == 0 and noise[1][1].size > 0                       # no gradient tile at all
    assert sum(flat[0]) > 0 and flat[1][1].size == 0 and flat[1][2].size == 0   # covered completely: empty 1-D streams
    for k in ("mixed", "synth"):
        o = want[KINDS.index(k)]
        assert sum(o[0]) > 0 and o[1][1].size > 0
    _encode_batch(enc, images)
    rows = enc.streams_batch()
    assert len(rows) == len(KINDS)
    for f, k in enumerate(KINDS):
        _same(rows[f], want[f][1], (w, h, k))
    n = rows[KINDS.index("noise")]
    assert n.rgb == [0] * 7 and n.rgb_bytes == [0] * 7 and n.pix and n.type
    fl = rows[KINDS.index("flat")]
    assert (fl.pix, fl.pix_bytes, fl.type, fl.type_bytes) == (0, 0, 0, 0) and sum(fl.rgb_bytes) > 0


# ---- 2. batch equals single on one handle ---------------------------------------------------------------------------------------------------
def _frames_for(w, h, n, seed):
    if (w, h) == (512, 512):
        return [_image(w, h, "mixed", seed=seed + f) for f in range(n)]
    return [_image(w, h, KINDS[(f + 2) % len(KINDS)], seed=seed + f) for f in range(n)]


@pytest.mark.parametrize("w,h,n", [(24, 40, 3), (200, 72, 3), (264, 136, 3), (512, 512, 3), (200, 72, 1), (200, 72, 2), (136, 264, 5)])
def test_batch_equals_single_on_one_handle(enc, w, h, n):
    if (w, h) == (512, 512):
        # the smallest size at which a frame spans several 1024-slot blocks in both scans: the 4x4 pass has (512/32)^2 swizzle blocks of 64 tile
        # slots = 2048 bitmap bytes (1024 per workgroup), and there are (512/8)^2 = 4096 8x8 tiles (1024 per workgroup)
        assert (w // 32) * (h // 32) * 64 // 8 > 1024 and (w // 8) * (h // 8) > 1024
    _encode_batch(enc, _frames_for(w, h, n, seed=40))
    rows = enc.streams_batch()
    assert len(rows) == n
    if (w, h) == (512, 512):
        assert rows[0].bitmap_bytes[6] == 2048
    single = [_single(enc, f) for f in range(n)]
    assert any(sum(r.rgb_bytes) for r in rows) and any(r.pix_bytes for r in rows)
    for f in range(n):
        _same(rows[f], single[f], (w, h, n, f))
    rows2 = enc.streams_batch()                                                # same layout, same bytes, and the single-image results are still there
    for f in range(n):
        assert (rows2[f].rgb, rows2[f].pix, rows2[f].type) == (rows[f].rgb, rows[f].pix, rows[f].type)
        _same(rows2[f], single[f], (w, h, n, f, "again"))


# ---- 3. RGBA batch --------------------------------------------------------------------------------------------------------------------------
def _rgba_frames(w, h):
    """edge_image's RGBA frames (transparent left and top border, holes); frame f's border is widened by another 16 * f pixels on one more side"""
    out = []
    for f, k in enumerate(("mixed", "smooth", "photo", "ramp")):
        p = edge_image(w, h, k, 4, seed=60 + f)
        if f == 1:
            p[3, :, w - 16:] = 0
        if f == 2:
            p[3, h - 32:, :] = 0
        if f == 3:
            p[3, :, : w // 8 + 48] = 0
            p[3, h - 16:, :] = 0
        out.append(p)
    return out


def test_rgba_batch_and_what(enc, one):
    w, h = 200, 136
    images = _rgba_frames(w, h)
    _encode_batch(enc, images)
    want = []
    for p in images:
        one.set_image_u8(np.ascontiguousarray(np.moveaxis(p, 0, -1).astype(np.uint8)))
        one.mip_prefilter()
        one.encode(3, False)
        want.append(_single(one))
    # the four frames really differ, in their corner streams and in their 1-D streams (a frame may have an empty 1-D stream: that is one more case)
    assert len({b"".join(s.tobytes() for s in x[0]) for x in want}) == 4 and len({x[1].tobytes() + x[2].tobytes() for x in want}) == 4
    for corners, range1d in ((True, False), (False, True), (True, True)):
        rows = enc.streams_batch(corners=corners, range1d=range1d)
        for f in range(4):
            _same(rows[f], want[f], (f, corners, range1d), corners, range1d)
            assert rows[f].bitmap_bytes == [enc._L.yk_gradient_bitmap_bytes(enc._h, p) for p in range(7)]


# ---- 4. layout ------------------------------------------------------------------------------------------------------------------------------
def test_layout_from_the_table(enc):
    w, h = 264, 136
    _encode_batch(enc, [_image(w, h, k, seed=21) for k in KINDS])
    rows = enc.streams_batch()
    spans = []
    for f, r in enumerate(rows):
        for ptr, n in list(zip(r.rgb, r.rgb_bytes)) + [(r.pix, r.pix_bytes), (r.type, r.type_bytes)]:
            assert (ptr == 0) == (n == 0)
            if ptr:
                assert ptr % 16 == 0, (f, hex(ptr))
                spans.append((ptr, ptr + n))
        enc.select_frame(f)
        assert r.bitmap == [int(enc._L.yk_gradient_bitmap_device(enc._h, p) or 0) for p in range(7)] and all(r.bitmap)
    spans.sort()
    assert len(spans) >= 10
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a1 <= b0, "streams overlap"
    used, extent = sum(b - a for a, b in spans), spans[-1][1] - spans[0][0]
    assert extent < used + 16 * len(spans)                                    # packed: nothing but the rounding to 16 between the streams
    calls = batch_calls_from_table(rows)
    assert [c[5] for c in calls[2] if c[0] == "g"] == rows[2].rgb and calls[2][7] == ("1", rows[2].type, rows[2].type_bytes, rows[2].pix, rows[2].pix_bytes)


# ---- 5. round trip --------------------------------------------------------------------------------------------------------------------------
def test_round_trip_default_equals_per_frame(enc):
    torch = _torch()
    w, h = 264, 136
    a, b = HipTileDecoder(0), HipTileDecoder(0)
    try:
        _encode_batch(enc, [_image(w, h, k, seed=21) for k in ("mixed", "smooth", "noise", "synth")])
        a.begin_batch(w, h, 4); b.begin_batch(w, h, 4)
        a.decode_batch_from_encoder(enc)
        assert a._batch_streams is None                                       # no copy, no buffer of the decoder's
        b.decode_batch_from_encoder(enc, per_frame=True)
        assert torch.equal(a.image_batch_device(), b.image_batch_device())
        _encode_batch(enc, _rgba_frames(w, h))
        a.begin_batch(w, h, 4); b.begin_batch(w, h, 4)
        a.decode_batch_from_encoder(enc, alpha=True)
        b.decode_batch_from_encoder(enc, alpha=True, per_frame=True)
        ia, ib = a.image_batch_device(channels=4, alpha_from_planes=True), b.image_batch_device(channels=4, alpha_from_planes=True)
        assert torch.equal(ia, ib) and int(ia[..., 3].min()) == 0 and int(ia[..., 3].max()) == 255
    finally:
        a.close(); b.close()


# ---- 6. refusals and state ------------------------------------------------------------------------------------------------------------------
def _refused(e, rc, code, word):
    msg = e._L.yk_last_error(e._h)
    assert rc == code, (rc, msg)
    assert msg and word in msg.decode(), msg


def _still_works(e):
    _encode_batch(e, [_image(24, 40, k, seed=77) for k in ("mixed", "synth")])
    rows = e.streams_batch()
    for f in range(2):
        _same(rows[f], _single(e, f), ("after a refusal", f))


def test_refusals():
    e = HipTileEncoder(0)
    L, tab = e._L, (_FrameStreamsC * 8)()
    try:
        w, h = 72, 40
        images = [_image(w, h, k, seed=5) for k in ("mixed", "synth", "smooth")]
        _encode_batch(e, images)
        rows = e.streams_batch()
        want = [_single(e, f) for f in range(3)]
        # bad arguments: nothing launched, the earlier table stays valid and its streams unchanged
        for what in (0, 4, -1, 7):
            _refused(e, L.yk_encode_streams_batch(e._h, what), YK_ERR_BAD_ARG, "what")
        _refused(e, L.yk_batch_streams_table(e._h, None), YK_ERR_BAD_ARG, "NULL")
        assert L.yk_batch_streams_table(e._h, tab) == 0 and [int(t.pix or 0) for t in tab[:3]] == [r.pix for r in rows]
        for f in range(3):
            _same(rows[f], want[f], ("after bad arguments", f))
        # a new encode invalidates the table; select_frame does not
        e.select_frame(2)
        assert L.yk_batch_streams_table(e._h, tab) == 0
        e.encode_batch(3, False)
        _refused(e, L.yk_batch_streams_table(e._h, tab), YK_ERR_STATE, "yk_encode_streams_batch first")
        _still_works(e)
        # before an encode (planes bound)
        e.set_batch_u8(_u8(images))
        _refused(e, L.yk_encode_streams_batch(e._h, 3), YK_ERR_STATE, "yk_encode_batch first")
        _refused(e, L.yk_batch_streams_table(e._h, tab), YK_ERR_STATE, "first")
        _still_works(e)
        # no planes bound
        assert L.yk_set_image(e._h, 64, 64, 3, 0, 64, 0) == 0
        _refused(e, L.yk_encode_streams_batch(e._h, 3), YK_ERR_STATE, "bind planes")
        _still_works(e)
        # a stripe
        big = _image(64, 128, "mixed", seed=3)
        e.set_image(big[:, :65], full_h=128, y0=0, halo_rows=1)
        e.encode(3, False)
        _refused(e, L.yk_encode_streams_batch(e._h, 3), YK_ERR_STATE, "stripe")
        _still_works(e)
        # after a plane-subset pass
        pm = edge_image(64, 64, "planemix", 3, seed=2)
        e.set_image(pm)
        e.encode(3, False)
        rows = e.streams_batch()
        assert len(rows) == 1
        want = _single(e)
        e.fitting_quad_smooth_planes(3, 2, 2)
        _refused(e, L.yk_encode_streams_batch(e._h, 3), YK_ERR_STATE, "plane-subset")
        assert L.yk_batch_streams_table(e._h, tab) == 0 and int(tab[0].pix or 0) == rows[0].pix      # the earlier table and its streams survive
        _same(rows[0], want, "after the plane-subset refusal")
        _still_works(e)
    finally:
        e.close()


def test_reuse_and_batch_of_one(enc, oracle_built):
    # another frame count, another shape, and back
    for (w, h, n, seed) in ((72, 40, 4, 1), (72, 40, 2, 2), (136, 72, 3, 3), (72, 40, 4, 1)):
        _encode_batch(enc, _frames_for(w, h, n, seed))
        rows = enc.streams_batch()
        assert len(rows) == n
        for f in range(n):
            _same(rows[f], _single(enc, f), (w, h, n, f))
    # a batch of one after encode() on a whole image, RGB and RGBA (the alpha stage of mip_prefilter), and after encode_frame()
    for planes in (_image(200, 72, "mixed", seed=9), edge_image(136, 72, "mixed", 4, seed=9)):
        enc.set_image(planes)
        if planes.shape[0] == 4:
            enc.mip_prefilter()
        enc.encode(3, False)
        rows = enc.streams_batch()
        assert len(rows) == 1
        _same(rows[0], _single(enc), planes.shape)
        if planes.shape[0] == 3:
            _same(rows[0], _oracle(planes)[1], ("oracle", planes.shape))
    enc.set_image(_image(200, 72, "synth", seed=9))
    enc.encode_frame(3, False)
    rows = enc.streams_batch()
    _same(rows[0], _single(enc), "encode_frame")


# ---- 7. stage timers ------------------------------------------------------------------------------------------------------------------------
def test_stage_timers(enc):
    _encode_batch(enc, _frames_for(200, 72, 3, seed=11))
    for st in (YK_STAGE_CORNERS, YK_STAGE_RANGE1D, YK_STAGE_RANGE1D_PACK):
        enc.stage_ms(st)
    for corners, range1d in ((True, True), (True, False), (False, True), (True, True)):
        enc.streams_batch(corners=corners, range1d=range1d)
        got = {st: enc.stage_ms(st) for st in (YK_STAGE_CORNERS, YK_STAGE_RANGE1D, YK_STAGE_RANGE1D_PACK)}
        assert got[YK_STAGE_CORNERS][1] == int(corners) and got[YK_STAGE_RANGE1D][1] == got[YK_STAGE_RANGE1D_PACK][1] == int(range1d), got
        assert all(ms > 0 for ms, k in got.values() if k) and all(ms == 0 for ms, k in got.values() if not k), got


# ---- 8. scale -------------------------------------------------------------------------------------------------------------------------------
def test_config4_scale_batch_equals_single():
    from yaik_amd.synth import synth_planes_torch
    torch = _torch()
    n, size, check = 64, 2048, (0, 31, 63)
    e = HipTileEncoder(0)
    try:
        frames = torch.empty((n, size, size, 3), dtype=torch.uint8, device="cuda")
        for f in range(n):
            frames[f] = synth_planes_torch(size, size, n_planes=3, seed=9000 + f, device="cuda").permute(1, 2, 0).to(torch.uint8)
        torch.cuda.synchronize()
        e.set_batch_u8(frames)
        e.encode_batch(3, False)
        rows = e.streams_batch()
        for f in check:
            _same(rows[f], _single(e, f), f)
        spans = [(p, p + k) for r in rows for p, k in list(zip(r.rgb, r.rgb_bytes)) + [(r.pix, r.pix_bytes), (r.type, r.type_bytes)] if p]
        extent = max(b for _, b in spans) - min(a for a, _ in spans)
        # the buffer of today's per-frame form (encoder_batch_streams(per_frame=True)): worst-case regions per frame
        up = lambda v: (v + 15) & ~15
        per_frame = up((size // 4 + 1) * (size // 4 + 1) * 3) + 7 * 16 + up(3 * size * size) + up(3 * (size // 8) * (size // 8) * 3)
        print(f"{n} x {size}^2: the batch's streams span {extent} bytes, the per-frame form's buffer {n * per_frame}")
        assert extent < n * per_frame
    finally:
        e.close()
        torch.cuda.empty_cache()
