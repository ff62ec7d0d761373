"""Round-trip quality on the device: yk_decode_compare_device / _batch_device / _planes_device (HipTileDecoder.compare_device /
compare_batch_device / compare_planes).  Decoded content comes from real decodes of small synthetic frames (encode_batch, then
decode_batch_from_encoder); expected values come from the numpy restatement (tests/quality_ref.py) on image_batch_device() / image() of the same
handle.  Every comparison is exact: integers with ==, no tolerances.

Shapes: 8 x 8 (one tile, a partial unit), 24 x 8, 16 x 16, 72 x 40 (both sides 8 mod 16), 136 x 8 (17 tiles: a second unit of one tile) with
40 x 24 (units that wrap rows of tiles), 1040 x 520 (8450 tiles: 34 workgroups, the last one partial).  The small shapes run with 1, 2, 7 and 33
frames in every source and layout; 1040 x 520 with 1 and 2 in every source and layout, and with 33 frames against the true source in one layout
(test_thirty_three_frames_of_several_workgroups)."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import quality_ref as Q
from tests.images import edge_image
from yaik_amd._lib import lib
from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder
from yaik_amd.quality import YkQuality, psnr_db, quality_dict

pytestmark = pytest.mark.gpu
YK_ERR_BAD_ARG, YK_ERR_STATE, YK_STAGE_DEC_COMPARE = -2, -4, 8
SMALL = [(8, 8), (24, 8), (16, 16), (72, 40), (136, 8), (40, 24)]
CASES = [(w, h, n) for (w, h) in SMALL for n in (1, 2, 7, 33)] + [(1040, 520, 1), (1040, 520, 2)]
SOURCES = ["true", "random", "self", "adversarial"]
SENTINEL = 0x5A5A5A5A


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def enc():
    e = HipTileEncoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def dec():
    d = HipTileDecoder(0)
    yield d
    d.close()


def _frames(w, h, n, seed=0):
    """n RGBA frames [n, h, w, 4] u8: gradients, noise blocks and jitter (tests/images.py 'mixed'), analog alpha inside a box and 0 around it"""
    rng = np.random.default_rng(seed * 7919 + w * 31 + h * 17 + n)
    out = np.zeros((n, h, w, 4), np.uint8)
    for f in range(n):
        out[f, :, :, :3] = np.moveaxis(edge_image(w, h, "mixed", 3, seed=seed + 3 * f + 1), 0, -1)
        a = np.zeros((h, w), np.uint8)
        x0, y0 = int(rng.integers(0, max(w // 3, 1))), int(rng.integers(0, max(h // 3, 1)))
        a[y0:, x0:] = rng.integers(4, 256, (h - y0, w - x0))
        if f % 3 == 2:
            a[:] = 255                                                     # a frame without an 'ALPM' chunk: opaque
        out[f, :, :, 3] = a
    return out


def _roundtrip(enc, dec, src, alpha=True):
    """encode the frames [n, h, w, 4], decode them as a batch on dec; returns the decoded RGBA frames [n, h, w, 4] (numpy)"""
    torch = _torch()
    n, h, w, _ = src.shape
    enc.set_batch_u8(torch.from_numpy(src).cuda(), n_planes=4 if alpha else 3)
    enc.encode_batch(3, False)
    dec.begin_batch(w, h, n)
    dec.decode_batch_from_encoder(enc, alpha=alpha)
    if alpha:
        return dec.image_batch_device(channels=4, alpha_from_planes=True).cpu().numpy()
    return dec.image_batch_device(channels=3).cpu().numpy()


def _source(kind, truth, decoded, seed=5):
    if kind == "true":
        return truth
    if kind == "random":                                                   # differences span the whole range
        return np.random.default_rng(seed).integers(0, 256, truth.shape, dtype=np.uint8)
    if kind == "self":                                                     # all zeros, psnr inf
        return decoded.copy()
    if kind == "adversarial":                                              # every |d| >= 128
        return np.where(decoded >= 128, 0, 255).astype(np.uint8)
    raise ValueError(kind)


def _refs(decoded, source, ch):
    return [Q.compare(decoded[f, :, :, :ch], source[f, :, :, :ch]) for f in range(decoded.shape[0])]


def _same(got, want, ch, what):
    assert len(got) == len(want), what
    for f, (g, r) in enumerate(zip(got, want)):
        for k in ("sse", "sad", "n_diff", "max_abs"):
            assert g[k] == r[k], (what, f, k, g[k], r[k])
        assert g["n_samples"] == r["n_samples"] and g["channels"] == ch, (what, f)
        assert g["psnr_db"] == [psnr_db(s, r["n_samples"]) for s in r["sse"]], (what, f)
        assert g["psnr_db_all"] == psnr_db(sum(r["sse"]), ch * r["n_samples"]), (what, f)
        if "tile_sse" in g:
            t = g["tile_sse"].cpu().numpy().astype(np.int64)
            assert t.shape == r["tile_sse"].shape and np.array_equal(t, r["tile_sse"]), (what, f, "tile map")


def _planes_tensor(x, pad=5, high=True):
    """[n, h, w, P] u8 -> torch int32 [n, P, h, w] view of a row-padded buffer; high: garbage above the low byte (only the low byte counts)"""
    torch = _torch()
    n, h, w, P = x.shape
    buf = np.full((n, P, h + 1, w + pad), -7, np.int32)
    v = np.moveaxis(x, -1, 1).astype(np.int32)
    if high:
        v = v | (np.arange(v.size, dtype=np.int64).reshape(v.shape) % 5 * 256).astype(np.int32)
    buf[:, :, :h, :w] = v
    return torch.from_numpy(buf).cuda()[:, :, :h, :w]


def _all_layouts(dec, decoded, source, what, alpha=True):
    """one source in every layout against the restatement; the batch calls, with the tile map"""
    torch = _torch()
    ref = {ch: _refs(decoded, source, ch) for ch in ((3, 4) if alpha else (3,))}
    x4 = torch.from_numpy(source).cuda()                                   # [n, h, w, 4]
    x3 = x4[..., :3].contiguous()
    _same(dec.compare_batch_device(x3, tile_map=True), ref[3], 3, (what, "hwc3"))
    _same(dec.compare_batch_device(x4, channels=3, tile_map=True), ref[3], 3, (what, "hwc4 / 3"))       # the fourth byte is skipped
    chw4, chw3 = x4.permute(0, 3, 1, 2).contiguous(), x3.permute(0, 3, 1, 2).contiguous()
    _same(dec.compare_batch_device(chw3, planar=True, tile_map=True), ref[3], 3, (what, "chw3"))
    _same(dec.compare_batch_device(chw4, channels=3, planar=True, tile_map=True), ref[3], 3, (what, "chw4 / 3"))
    p4 = _planes_tensor(source)
    _same(dec.compare_planes(p4, channels=3, tile_map=True), ref[3], 3, (what, "planes / 3"))
    _same(dec.compare_planes(p4[:, :3], tile_map=True), ref[3], 3, (what, "planes3"))
    if alpha:
        _same(dec.compare_batch_device(x4, tile_map=True), ref[4], 4, (what, "hwc4"))                  # the default: 4 with decoded alpha planes
        _same(dec.compare_batch_device(chw4, channels=4, planar=True, tile_map=True), ref[4], 4, (what, "chw4"))
        _same(dec.compare_planes(p4, tile_map=True), ref[4], 4, (what, "planes4"))
    return ref


@pytest.mark.parametrize("w,h,n", CASES, ids=[f"{w}x{h}x{n}" for w, h, n in CASES])
def test_every_source_in_every_layout(enc, dec, w, h, n):
    truth = _frames(w, h, n)
    decoded = _roundtrip(enc, dec, truth)
    for kind in SOURCES:
        source = _source(kind, truth, decoded)
        ref = _all_layouts(dec, decoded, source, (w, h, n, kind))
        if kind == "self":
            got = dec.compare_batch_device(_torch().from_numpy(source).cuda())
            for g in got:
                assert g["sse"] == g["sad"] == g["n_diff"] == g["max_abs"] == [0] * 4
                assert g["psnr_db"] == [math.inf] * 4 and g["psnr_db_all"] == math.inf
        if kind == "adversarial":
            assert all(min(r["max_abs"]) >= 128 and r["n_diff"] == [w * h] * 4 for r in ref[4])
        if kind == "true" and w * h >= 256:                                # the round trip of 'mixed' frames is lossy, and not absurdly so
            assert any(sum(r["sse"]) > 0 for r in ref[3])
            print(f"{w} x {h} x {n}: round-trip PSNR (RGB) per frame:", [round(psnr_db(sum(r['sse']), 3 * w * h), 2) for r in ref[3]][:4])


def test_thirty_three_frames_of_several_workgroups(enc, dec):
    """1040 x 520 x 33: partials[f * groups + workgroup] with a partial last workgroup in every one of many frames; one source, one layout"""
    w, h, n = 1040, 520, 33
    truth = _frames(w, h, n, seed=4)
    decoded = _roundtrip(enc, dec, truth)
    _same(dec.compare_batch_device(_torch().from_numpy(truth).cuda(), tile_map=True), _refs(decoded, truth, 4), 4, (w, h, n))


def test_sources_that_are_not_on_the_device_are_refused(enc, dec):
    """a host address must never reach the kernel: a CPU tensor or a numpy array is a ValueError before any library call"""
    torch = _torch()
    w, h, n = 40, 24, 2
    truth = _frames(w, h, n, seed=12)
    decoded = _roundtrip(enc, dec, truth)
    cpu = torch.from_numpy(truth)                                           # the .cuda() forgotten
    planes_cpu = torch.from_numpy(np.ascontiguousarray(np.moveaxis(truth, -1, 1)).astype(np.int32))
    calls = [lambda: dec.compare_batch_device(cpu), lambda: dec.compare_batch_device(truth),
             lambda: dec.compare_batch_device(cpu.permute(0, 3, 1, 2).contiguous(), planar=True),
             lambda: dec.compare_device(cpu[0]), lambda: dec.compare_device(truth[0]), lambda: dec.compare_device(cpu[0].permute(2, 0, 1).contiguous(), planar=True),
             lambda: dec.compare_planes(planes_cpu), lambda: dec.compare_planes(planes_cpu.numpy()), lambda: dec.compare_planes(planes_cpu[0])]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match="must be a torch tensor on cuda:0"):
            call()
    _same(dec.compare_batch_device(cpu.cuda(), tile_map=True), _refs(decoded, truth, 4), 4, "usable after the refusals")


def _strided(flat, offset, shape, strides):
    return _torch().as_strided(flat, shape, strides, storage_offset=offset)


@pytest.mark.parametrize("offset", [1, 2, 3])
def test_padded_pitches_and_odd_base_addresses(enc, dec, offset):
    torch = _torch()
    w, h, n = 72, 40, 2
    truth = _frames(w, h, n, seed=offset)
    decoded = _roundtrip(enc, dec, truth)
    source = _source("random", truth, decoded, seed=offset)
    ref = {ch: _refs(decoded, source, ch) for ch in (3, 4)}
    for C_src in (3, 4):                                                    # HWC: rows of w * C bytes at a pitch of w * C + 13, frames 29 bytes further apart
        row, frame = w * C_src + 13, (w * C_src + 13) * h + 29
        flat = torch.full((offset + n * frame + 64,), 0xEE, dtype=torch.uint8, device="cuda")
        view = _strided(flat, offset, (n, h, w, C_src), (frame, row, C_src, 1))
        view.copy_(torch.from_numpy(np.ascontiguousarray(source[..., :C_src])).cuda())
        assert view.data_ptr() % 4 == (flat.data_ptr() + offset) % 4
        for ch in ((3,) if C_src == 3 else (3, 4)):
            _same(dec.compare_batch_device(view, channels=ch, tile_map=True), ref[ch], ch, ("hwc", C_src, ch, offset))
        dec.select_frame(1)
        _same([dec.compare_device(view[1], channels=3, tile_map=True)], ref[3][1:], 3, ("hwc single", C_src, offset))
        dec.select_frame(0)
    row, plane = w + 5, (w + 5) * h + 3                                     # CHW: padded rows, planes and frames
    frame = 4 * plane + 11
    flat = torch.full((offset + n * frame + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    view = _strided(flat, offset, (n, 4, h, w), (frame, plane, row, 1))
    view.copy_(torch.from_numpy(np.ascontiguousarray(np.moveaxis(source, -1, 1))).cuda())
    for ch in (3, 4):
        _same(dec.compare_batch_device(view, channels=ch, planar=True, tile_map=True), ref[ch], ch, ("chw", ch, offset))
    _same(dec.compare_batch_device(view[:, :3], planar=True), ref[3], 3, ("chw view of three planes", offset))
    dec.select_frame(1)
    _same([dec.compare_device(view[1], channels=4, planar=True, tile_map=True)], ref[4][1:], 4, ("chw single", offset))
    dec.select_frame(0)


def test_single_image_with_its_alpha_plane(enc, dec):
    """channels = 4 against the plane decompress_alpha left; channels = 3 on the same RGBA source skips the fourth byte"""
    torch = _torch()
    w, h = 72, 40
    truth = _frames(w, h, 1, seed=11)[0]
    enc.set_image_u8(torch.from_numpy(truth[:, :, :3].copy()).cuda())
    enc.encode(3, False, False)
    dec.begin(w, h)
    dec.decode_from_encoder(enc)
    pay = np.random.default_rng(4).integers(0, 256, 40 * 24, dtype=np.uint8)
    plane = dec.decompress_alpha(6, (16, 8, 40, 24), pay)                   # IS_8_BIT_FULL in an inner box, 0 around it
    decoded = dec.image().reshape(h, w, 4)
    assert np.array_equal(decoded[:, :, 3], plane)
    src = torch.from_numpy(truth).cuda()
    ref4, ref3 = Q.compare(decoded, truth), Q.compare(decoded[:, :, :3], truth[:, :, :3])
    _same([dec.compare_device(src, tile_map=True)], [ref4], 4, "default channels with a decoded plane")
    _same([dec.compare_device(src, channels=3, tile_map=True)], [ref3], 3, "rgb of an rgba source")
    _same([dec.compare_device(src.permute(2, 0, 1).contiguous(), channels=4, planar=True)], [ref4], 4, "chw")
    _same([dec.compare_planes(_planes_tensor(truth[None])[0], tile_map=True)], [ref4], 4, "planes")
    assert ref4["sse"][3] > 0 and ref4["sse"][:3] == ref3["sse"]


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def test_tile_map_extent_and_null_map(enc, dec):
    torch = _torch()
    w, h, n = 40, 24, 7
    truth = _frames(w, h, n, seed=2)
    decoded = _roundtrip(enc, dec, truth)
    ref = _refs(decoded, truth, 4)
    tiles = (w // 8) * (h // 8)
    src = torch.from_numpy(truth).cuda()
    buf = torch.full((n * tiles + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    out = (YkQuality * n)()
    torch.cuda.synchronize()
    rc = lib().yk_decode_compare_batch_device(dec._h, _ptr(src), w * 4, 0, w * h * 4, 4, 4, out, _ptr(buf))
    assert rc == 0
    got = buf.cpu().numpy()
    assert np.array_equal(got[:n * tiles].reshape(n, h // 8, w // 8), np.stack([r["tile_sse"] for r in ref]))   # fully overwritten inside its extent
    assert (got[n * tiles:] == SENTINEL).all()                                                                    # untouched beyond it
    _same([quality_dict(q, 4) for q in out], ref, 4, "c-abi")
    buf.fill_(SENTINEL)
    torch.cuda.synchronize()
    out2 = (YkQuality * n)()
    assert lib().yk_decode_compare_batch_device(dec._h, _ptr(src), w * 4, 0, w * h * 4, 4, 4, out2, None) == 0  # NULL map: statistics only
    assert bytes(out2) == bytes(out)                                                                            # ... and the same ones
    assert (buf.cpu().numpy() == SENTINEL).all()          # the earlier map buffer is not remembered (the kernel is not given its address here)
    # a caller's own map tensor is written in place
    mine = torch.full((n, h // 8, w // 8), SENTINEL, dtype=torch.int32, device="cuda")
    res = dec.compare_batch_device(src, tile_map=mine)
    assert res[3]["tile_sse"].data_ptr() == mine[3].data_ptr()
    assert np.array_equal(mine.cpu().numpy(), np.stack([r["tile_sse"] for r in ref]))


def test_selected_frame_equals_the_batch_entry_and_calls_repeat(enc, dec):
    torch = _torch()
    w, h, n = 72, 40, 7
    truth = _frames(w, h, n, seed=3)
    decoded = _roundtrip(enc, dec, truth)
    src = torch.from_numpy(truth).cuda()
    batch = dec.compare_batch_device(src, tile_map=True)
    _same(batch, _refs(decoded, truth, 4), 4, "batch")
    for f in (0, 3, 6):
        dec.select_frame(f)
        one = dec.compare_device(src[f], tile_map=True)
        assert {k: v for k, v in one.items() if k != "tile_sse"} == {k: v for k, v in batch[f].items() if k != "tile_sse"}, f
        assert torch.equal(one["tile_sse"], batch[f]["tile_sse"]), f
    dec.select_frame(0)
    strip = lambda rs: [{k: v for k, v in r.items() if k != "tile_sse"} for r in rs]
    for _ in range(4):                                                     # four calls in a row on the same handle and buffers
        assert strip(dec.compare_batch_device(src)) == strip(batch)


def test_one_handle_across_shapes_and_frame_counts(enc, dec):
    """the records buffer only grows: a large batch, then smaller and other shapes, then the large one again"""
    seen = {}
    for (w, h, n) in [(136, 8, 33), (8, 8, 1), (72, 40, 2), (16, 16, 7), (136, 8, 33)]:
        truth = _frames(w, h, n, seed=9)
        decoded = _roundtrip(enc, dec, truth)
        got = dec.compare_batch_device(_torch().from_numpy(truth).cuda(), tile_map=True)
        _same(got, _refs(decoded, truth, 4), 4, (w, h, n))
        key = [(g["sse"], g["sad"], g["n_diff"], g["max_abs"]) for g in got]
        assert seen.setdefault((w, h, n), key) == key


def test_nothing_decoded_compares_against_zeros(enc, dec):
    """the settle rule: after begin_batch with no chunk decoded, the output calls write zeros, so the comparison is against zeros"""
    torch = _torch()
    w, h, n = 72, 40, 2
    truth = _frames(w, h, n, seed=5)
    _roundtrip(enc, dec, truth)                                             # leaves content in the handle's planes
    dec.begin_batch(w, h, n)
    got = dec.compare_batch_device(torch.from_numpy(truth).cuda(), channels=3, tile_map=True)
    _same(got, _refs(np.zeros_like(truth), truth, 3), 3, "zeros")
    assert not dec.image_batch_device().any()


def test_sums_beyond_32_bits():
    """2048 x 2048 against the adversarial source: every sse is at least 2^22 x 128^2 = 2^36, so the u64 fold is exercised"""
    torch = _torch()
    from yaik_amd.synth import synth_planes_torch
    size = 2048
    e, d = HipTileEncoder(0), HipTileDecoder(0)
    try:
        px = synth_planes_torch(size, size, n_planes=3, seed=77, device="cuda").permute(1, 2, 0).to(torch.uint8).contiguous()
        e.set_image_u8(px)
        e.encode(3, False, False)
        d.begin(size, size)
        d.decode_from_encoder(e)
        decoded = d.image_device()
        adv = torch.where(decoded >= 128, 0, 255).to(torch.uint8)
        got = d.compare_device(adv, tile_map=True)
        ref = Q.compare(decoded.cpu().numpy(), adv.cpu().numpy())
        _same([got], [ref], 3, "2048")
        assert min(got["sse"]) > 1 << 36 and min(got["max_abs"]) >= 128
        true = d.compare_device(px)
        _same([true], [Q.compare(decoded.cpu().numpy(), px.cpu().numpy())], 3, "2048 true source")
        print("2048 x 2048 YAIK-synth round trip: PSNR per channel", [round(v, 2) for v in true["psnr_db"]], "max |err|", true["max_abs"])
    finally:
        e.close()
        d.close()


def test_one_stage_interval_per_call(enc, dec):
    torch = _torch()
    w, h, n = 40, 24, 2
    truth = _frames(w, h, n, seed=6)
    _roundtrip(enc, dec, truth)
    src = torch.from_numpy(truth).cuda()
    dec.stage_ms(YK_STAGE_DEC_COMPARE)                                     # read and reset
    dec.compare_batch_device(src)
    dec.compare_batch_device(src, channels=3, tile_map=True)
    dec.compare_device(src[0])
    dec.compare_planes(_planes_tensor(truth))
    ms, k = dec.stage_ms(YK_STAGE_DEC_COMPARE)
    assert k == 4 and ms > 0.0
    assert dec.stage_ms(YK_STAGE_DEC_COMPARE) == (0.0, 0)


def _refused(h, rc, code, text, out, out_before, maps):
    assert rc == code, (rc, code, text)
    msg = lib().yk_last_error(h).decode()
    assert text in msg, (text, msg)
    assert bytes(out) == out_before, text                                   # nothing written to out ...
    for m in maps:
        assert (m.cpu().numpy() == SENTINEL).all(), text                    # ... or to the map


def test_refusals(enc, dec):
    torch = _torch()
    L = lib()
    w, h, n = 40, 24, 2
    tiles = (w // 8) * (h // 8)
    truth = _frames(w, h, n, seed=8)
    out = (YkQuality * n)()
    C.memset(out, 0xEE, C.sizeof(out))
    before = bytes(out)
    tmap = torch.full((n * tiles,), SENTINEL, dtype=torch.int32, device="cuda")
    src = torch.from_numpy(truth).cuda()
    planes = _planes_tensor(truth, pad=0, high=False).contiguous()
    pp = lambda miss=(): (C.c_void_p * 4)(*[None if k in miss else planes.data_ptr() + k * w * h * 4 for k in range(4)])
    u8 = lambda **kw: L.yk_decode_compare_batch_device(fresh._h if kw.pop("fresh", False) else dec._h, kw.pop("src", _ptr(src)), kw.pop("row", w * 4), kw.pop("plane", 0),
                                                     kw.pop("frame", w * h * 4), kw.pop("sc", 4), kw.pop("ch", 4), kw.pop("out", out), _ptr(tmap))
    chk = lambda rc, code, text, hd=None: _refused((hd or dec)._h, rc, code, text, out, before, [tmap])
    # before any begin
    fresh = HipTileDecoder(0)
    try:
        chk(u8(fresh=True), YK_ERR_STATE, "yk_decode_begin_batch first", fresh)
        chk(L.yk_decode_compare_device(fresh._h, _ptr(src), w * 4, 0, 4, 3, out, _ptr(tmap)), YK_ERR_STATE, "yk_decode_begin first", fresh)
        chk(L.yk_decode_compare_planes_device(fresh._h, pp(), w, w * h * 4, 3, out, _ptr(tmap)), YK_ERR_STATE, "yk_decode_begin_batch first", fresh)
    finally:
        fresh.close()
    # a batch without alpha planes
    decoded3 = _roundtrip(enc, dec, truth, alpha=False)
    chk(u8(), YK_ERR_STATE, "channels = 4 needs the decoded alpha")
    chk(L.yk_decode_compare_device(dec._h, _ptr(src), w * 4, 0, 4, 4, out, _ptr(tmap)), YK_ERR_STATE, "channels = 4 needs the decoded alpha")
    chk(L.yk_decode_compare_planes_device(dec._h, pp(), w, w * h * 4, 4, out, _ptr(tmap)), YK_ERR_STATE, "channels = 4 needs the decoded alpha")
    _same(dec.compare_batch_device(src, channels=3), _refs(decoded3, truth, 3), 3, "usable after the refusals")
    # with alpha planes: the argument errors
    decoded = _roundtrip(enc, dec, truth)
    chk(u8(src=None), YK_ERR_BAD_ARG, "devSrc is NULL")
    chk(u8(out=None), YK_ERR_BAD_ARG, "out is NULL")
    for ch in (0, 2, 5):
        chk(u8(ch=ch), YK_ERR_BAD_ARG, "channels must be 3 or 4")
    for sc in (2, 5):
        chk(u8(sc=sc, ch=3), YK_ERR_BAD_ARG, "srcChannels must be 3 or 4")
    chk(u8(sc=3, ch=4, row=w * 3, frame=w * h * 3), YK_ERR_BAD_ARG, "at least channels")
    chk(u8(row=w * 4 - 1), YK_ERR_BAD_ARG, "row or plane pitch too small")                       # HWC
    chk(u8(sc=3, ch=3, row=w * 3 - 1), YK_ERR_BAD_ARG, "row or plane pitch too small")
    chk(u8(row=w - 1, plane=w * h), YK_ERR_BAD_ARG, "row or plane pitch too small")              # CHW
    chk(u8(row=w, plane=w * h - 1), YK_ERR_BAD_ARG, "row or plane pitch too small")
    chk(u8(frame=w * h * 4 - 1), YK_ERR_BAD_ARG, "frame stride too small")                       # more than one frame
    chk(u8(row=w, plane=w * h, frame=w * h * 4 - 1), YK_ERR_BAD_ARG, "frame stride too small")
    chk(L.yk_decode_compare_device(dec._h, None, w * 4, 0, 4, 4, out, _ptr(tmap)), YK_ERR_BAD_ARG, "devSrc is NULL")
    chk(L.yk_decode_compare_device(dec._h, _ptr(src), w * 4 - 1, 0, 4, 4, out, _ptr(tmap)), YK_ERR_BAD_ARG, "row or plane pitch too small")
    chk(L.yk_decode_compare_device(dec._h, _ptr(src), w * 4, 0, 4, 4, None, _ptr(tmap)), YK_ERR_BAD_ARG, "out is NULL")
    chk(L.yk_decode_compare_planes_device(dec._h, None, w, w * h * 4, 4, out, _ptr(tmap)), YK_ERR_BAD_ARG, "frame0Planes is NULL")
    chk(L.yk_decode_compare_planes_device(dec._h, pp(miss=(2,)), w, w * h * 4, 3, out, _ptr(tmap)), YK_ERR_BAD_ARG, "a plane the comparison needs is NULL")
    chk(L.yk_decode_compare_planes_device(dec._h, pp(miss=(3,)), w, w * h * 4, 4, out, _ptr(tmap)), YK_ERR_BAD_ARG, "a plane the comparison needs is NULL")
    chk(L.yk_decode_compare_planes_device(dec._h, pp(), w - 1, w * h * 4, 4, out, _ptr(tmap)), YK_ERR_BAD_ARG, "strideElems is smaller than the width")
    chk(L.yk_decode_compare_planes_device(dec._h, pp(), w, w * h * 4, 6, out, _ptr(tmap)), YK_ERR_BAD_ARG, "channels must be 3 or 4")
    chk(L.yk_decode_compare_planes_device(dec._h, pp(), w, w * h * 4, 4, None, _ptr(tmap)), YK_ERR_BAD_ARG, "out is NULL")
    # a missing fourth plane is fine when three channels are compared; the handle is correct after all of the above
    torch.cuda.synchronize()
    assert L.yk_decode_compare_planes_device(dec._h, pp(miss=(3,)), w, w * h * 4, 3, out, None) == 0
    _same([quality_dict(q, 3) for q in out], _refs(decoded, truth, 3), 3, "planes, three of four")
    _same(dec.compare_batch_device(src, tile_map=True), _refs(decoded, truth, 4), 4, "usable after the refusals")
