"""Decode into 8-bit RGB(A) pixels in device memory (yk_decode_output_device behind HipTileDecoder.image_device, YAIK_DecodeImageToDevice in
C++): every device output must equal, byte for byte, the host output of the same decode (image(), YAIK_DecodeImage) -- HWC as it is, CHW as
the HWC result transposed -- and nothing outside the pixel bytes of the destination may change."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle.refrun import parse_blobs
from tests import alpha_ref as R
from tests.ragged import oracle_streams, source
from yaik_amd._lib import YaikError, lib
from yaik_amd.decoder import HipTileDecoder
from yaik_amd.encoder import HipTileEncoder
from yaik_amd.synth import synth_planes_torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yaik_amd", "host")
YK_ERR_BAD_ARG, YK_ERR_STATE, YK_STAGE_DEC_DETILE = -2, -4, 5
YAIK_DECIMG_INVALIDCTX = 9
SENTINEL = 0xA5

SHAPES = [(8, 8), (24, 16), (264, 136), (1920, 1080), (2048, 2048), (8192, 8192)]
ORACLE_SHAPES = [(8, 8), (24, 16), (264, 136)]


@pytest.fixture(scope="module")
def dec():
    d = HipTileDecoder(0)
    yield d
    d.close()


@pytest.fixture(scope="module")
def enc():
    e = HipTileEncoder(0)
    yield e
    e.close()


def _torch():
    import torch
    return torch


def _decode_oracle(dec, w, h):
    passes, typ, pix = oracle_streams(source(w, h, "mixed"))
    dec.begin(w, h)
    for sx, sy, cnt, bm, rgb in passes:
        if cnt:
            dec.decompress_gradient(sx, sy, bm, rgb)
    dec.decompress_1d(typ, pix)


def _decode_encoder(dec, enc, w, h, seed=12345):
    torch = _torch()
    planes = synth_planes_torch(w, h, n_planes=3, seed=seed, device="cuda")
    enc.set_image_u8(planes.permute(1, 2, 0).to(torch.uint8).contiguous())
    enc.encode(3, False, False)
    dec.begin(w, h)
    dec.decode_from_encoder(enc)


def _alpha_plane(dec, w, h, seed=3):
    """an 'ALPM' plane in HBM: 8-bit values in an inner box (0 outside it); returns the plane as the host reads it"""
    bw, bh = max(8, w // 2 // 8 * 8), max(8, h // 2)
    bx, by = (w - bw) // 2, (h - bh) // 2
    pay = np.random.default_rng(seed).integers(0, 256, bw * bh, dtype=np.uint8)
    assert dec.decompress_alpha(R.IS_8_BIT_FULL, (bx, by, bw, bh), pay, to_host=False) is None
    plane = np.zeros((h, w), np.uint8)
    plane[by:by + bh, bx:bx + bw] = pay.reshape(bh, bw)
    return plane


def _host_hwc(dec, channels, alpha):
    """image() with the same alpha: [h, w, C] uint8 on the host"""
    h, w = dec.h, dec.w
    if channels == 3:
        img = np.empty((h, w * 3), np.uint8)
        dec.image_into(img)                                                  # RGB rows also when an 'ALPM' plane was decoded
    elif alpha is None:
        img = dec.image()
    else:
        img = dec.image(alpha=np.full((h, w), alpha, np.uint8))
    return np.ascontiguousarray(img).reshape(h, w, channels)


def _check_all_forms(dec):
    """RGB, RGBA from the plane (when there is one), RGBA with a constant; HWC and CHW; each against the host output"""
    torch = _torch()
    cases = [(3, None)] + ([(4, None)] if dec._has_alpha else []) + [(4, 77)]
    for channels, alpha in cases:
        want = torch.from_numpy(_host_hwc(dec, channels, alpha)).cuda()
        got = dec.image_device(channels=channels, alpha=alpha)
        assert got.shape == (dec.h, dec.w, channels) and got.dtype == torch.uint8
        assert torch.equal(got, want), (channels, alpha, "HWC")
        got = dec.image_device(channels=channels, alpha=alpha, planar=True)
        assert got.shape == (channels, dec.h, dec.w)
        assert torch.equal(got, want.permute(2, 0, 1)), (channels, alpha, "CHW")


@pytest.mark.parametrize("w,h", ORACLE_SHAPES)
def test_oracle_streams_device_equals_host(dec, oracle_built, w, h):
    _decode_oracle(dec, w, h)
    _check_all_forms(dec)
    _alpha_plane(dec, w, h)
    _check_all_forms(dec)


@pytest.mark.parametrize("w,h", SHAPES, ids=[f"{w}x{h}" for w, h in SHAPES])
def test_encoder_streams_device_equals_host(dec, enc, w, h):
    _decode_encoder(dec, enc, w, h)
    _check_all_forms(dec)
    plane = _alpha_plane(dec, w, h)
    _check_all_forms(dec)
    assert np.array_equal(dec.image_device(channels=4)[..., 3].cpu().numpy(), plane)


def test_defaults_follow_the_alpha_plane(dec, enc):
    w, h = 264, 136
    _decode_encoder(dec, enc, w, h)
    assert dec.image_device().shape == (h, w, 3)
    assert (dec.image_device(channels=4)[..., 3] == 255).all()                  # RGB file -> opaque RGBA8888
    _alpha_plane(dec, w, h)
    assert dec.image_device().shape == (h, w, 4)
    assert dec.image_device(planar=True).shape == (4, h, w)


def _stage_intervals(dec):
    return dec.stage_ms(YK_STAGE_DEC_DETILE)[1]


def test_stage_timer_records_the_device_detile(dec, enc):
    _decode_encoder(dec, enc, 256, 256)
    _stage_intervals(dec)
    dec.image_device()
    dec.image_device(planar=True)
    assert _stage_intervals(dec) == 2


# ---- pitches, alignment, sentinels -----------------------------------------------------------------------------------------------------------
def _strided(buf, offset, shape, strides):
    torch = _torch()
    return torch.as_strided(buf, shape, strides, offset)


def _footprint(n, offset, shape, strides):
    """bool mask over a buffer of n bytes: the bytes the view covers"""
    torch = _torch()
    m = torch.zeros(n, dtype=torch.bool, device="cuda")
    _strided(m, offset, shape, strides).fill_(True)
    return m


PITCHES = {"tight": 0, "padded": 48, "odd": 5}


@pytest.mark.parametrize("w,h", [(264, 136), (1920, 1080)])
@pytest.mark.parametrize("planar", [False, True], ids=["hwc", "chw"])
@pytest.mark.parametrize("channels,alpha", [(3, None), (4, None), (4, 200)], ids=["rgb", "rgba_plane", "rgba_const"])
def test_pitches_and_offsets_leave_every_other_byte(dec, enc, w, h, planar, channels, alpha):
    torch = _torch()
    _decode_encoder(dec, enc, w, h, seed=w + h)
    _alpha_plane(dec, w, h)
    want = torch.from_numpy(_host_hwc(dec, channels, alpha)).cuda()
    if planar:
        want = want.permute(2, 0, 1)
    for pname, extra in PITCHES.items():
        for offset in (0, 1, 2, 3):
            row = (w if planar else w * channels) + extra
            if planar:
                plane = row * h + (0 if extra == 0 else 7)
                shape, strides, n = (channels, h, w), (plane, row, 1), offset + plane * channels + 64
            else:
                shape, strides, n = (h, w, channels), (row, channels, 1), offset + row * h + 64
            buf = torch.full((n,), SENTINEL, dtype=torch.uint8, device="cuda")
            out = _strided(buf, offset, shape, strides)
            dec.image_device(out, channels=channels, alpha=alpha, planar=planar)
            assert torch.equal(out, want), (pname, offset)
            rest = buf[~_footprint(n, offset, shape, strides)]
            assert (rest == SENTINEL).all(), (pname, offset, "a byte outside the pixels changed")


def test_destination_beyond_4gib(dec, enc):
    """8192 rows at a pitch above 512 KiB: the last rows lie more than 4 GiB past the base"""
    torch = _torch()
    w, h, pitch = 64, 8192, 600064
    assert (h - 1) * pitch > 1 << 32
    _decode_encoder(dec, enc, w, h)
    _alpha_plane(dec, w, h)
    want = torch.from_numpy(_host_hwc(dec, 4, None)).cuda()
    buf = torch.full((pitch * h,), SENTINEL, dtype=torch.uint8, device="cuda")
    out = _strided(buf, 0, (h, w, 4), (pitch, 4, 1))
    dec.image_device(out)
    assert torch.equal(out, want)
    pad = _strided(buf, w * 4, (h, 256), (pitch, 1))                  # the first bytes of every row's padding
    assert (pad == SENTINEL).all()
    del buf, out, pad
    torch.cuda.empty_cache()


def test_batch_of_frames(dec, enc):
    """eight different images into frames[f] of one [8, h, w, 4] tensor, each equal to its own host decode"""
    torch = _torch()
    w, h = 264, 136
    frames = torch.full((8, h, w, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    wants = []
    for f in range(8):
        _decode_encoder(dec, enc, w, h, seed=100 + f)
        alpha = None
        if f % 2 == 0:
            _alpha_plane(dec, w, h, seed=f)
        else:
            alpha = 30 * f
        dec.image_device(frames[f], channels=4, alpha=alpha)
        wants.append(_host_hwc(dec, 4, alpha))
    for f in range(8):
        assert np.array_equal(frames[f].cpu().numpy(), wants[f]), f


def test_ordered_with_torch_streams_without_a_host_fence(enc):
    """torch fills out, image_device writes it, a torch clone on the current stream reads it; alternating images into one tensor"""
    torch = _torch()
    w, h = 2048, 2048
    decs = [HipTileDecoder(0), HipTileDecoder(0)]
    try:
        wants = []
        for i, d in enumerate(decs):
            _decode_encoder(d, enc, w, h, seed=7 + i)
            _alpha_plane(d, w, h, seed=i)
            wants.append(torch.from_numpy(_host_hwc(d, 4, None)).cuda())
        out = torch.empty((h, w, 4), dtype=torch.uint8, device="cuda")
        big = torch.empty((64 << 20,), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        snaps = []
        for rep in range(6):
            big.fill_(rep)                                             # queue work ahead on torch's stream so a missing wait shows
            out.fill_(rep)
            decs[rep % 2].image_device(out)
            snaps.append(out.clone())
        torch.cuda.synchronize()
        for rep, s in enumerate(snaps):
            assert torch.equal(s, wants[rep % 2]), rep
    finally:
        for d in decs:
            d.close()


# ---- refusals: nothing is written ------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(enc):
    torch = _torch()
    L = lib()
    w, h = 64, 32
    buf = torch.full((4 * w * h + 4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    d = HipTileDecoder(0)
    try:
        def rc(*args):
            r = L.yk_decode_output_device(d._h, *args)
            torch.cuda.synchronize()
            d.synchronize()
            assert (buf == SENTINEL).all(), args
            return r
        assert rc(p, w * 3, 0, 3, 0) == YK_ERR_STATE                             # before yk_decode_begin
        _decode_encoder(d, enc, w, h)
        assert rc(None, w * 3, 0, 3, 0) == YK_ERR_BAD_ARG
        for ch in (0, 1, 2, 5):
            assert rc(p, w * 4, 0, ch, 0) == YK_ERR_BAD_ARG, ch
        assert rc(p, w * 3 - 1, 0, 3, 0) == YK_ERR_BAD_ARG
        assert rc(p, w * 4 - 1, 0, 4, 255) == YK_ERR_BAD_ARG
        assert rc(p, w - 1, (w - 1) * h, 3, 0) == YK_ERR_BAD_ARG                  # CHW row shorter than w
        assert rc(p, w, w * h - 1, 4, 255) == YK_ERR_BAD_ARG                      # CHW plane shorter than rowBytes * h
        for a in (-2, 256, 1000):
            assert rc(p, w * 4, 0, 4, a) == YK_ERR_BAD_ARG, a
        assert rc(p, w * 4, 0, 4, -1) == YK_ERR_STATE                             # no 'ALPM' plane decoded
        with pytest.raises(YaikError):
            d.image_device(channels=4, alpha=-1)
        with pytest.raises(ValueError):
            d.image_device(torch.empty((h, w, 3), dtype=torch.uint8))            # a host tensor
        with pytest.raises(ValueError):
            d.image_device(torch.empty((h, w + 8, 3), dtype=torch.uint8, device="cuda"))
        with pytest.raises(ValueError):
            d.image_device(torch.empty((h, w, 4), dtype=torch.uint8, device="cuda"), channels=3)
        assert (buf == SENTINEL).all()
        # alpha is ignored with three channels
        assert L.yk_decode_output_device(d._h, p, w * 3, 0, 3, 1000) == 0
        torch.cuda.synchronize(); d.synchronize()
        want = torch.from_numpy(_host_hwc(d, 3, None)).cuda()
        assert torch.equal(buf[: w * h * 3].view(h, w, 3), want)
    finally:
        d.close()


# ---- the C++ drop-in: YAIK_DecodeImageToDevice -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drivers():
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL)
    return True


def _encode_file(planes, emit, tmp):
    n, h, w = planes.shape
    fin, fy = os.path.join(tmp, "in.bin"), os.path.join(tmp, f"out{int(emit)}.yaik")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", w, h, n)); f.write(np.ascontiguousarray(planes, np.int32).tobytes())
    subprocess.run([os.path.join(HOST, "alpha_driver"), "enc", fin, fy, "1" if emit else "0"], check=True, stdout=subprocess.DEVNULL)
    return fy


def test_decode_image_to_device_equals_decode_image(drivers, tmp_path):
    rng = np.random.default_rng(77)
    h, w = 96, 128
    a = np.zeros((h, w), np.int32)
    a[10:70, 20:100] = rng.integers(0, 256, (60, 80))
    a[10, 20] = 255
    planes = np.stack([rng.integers(0, 256, (h, w), dtype=np.int32) for _ in range(3)] + [a])
    files = [_encode_file(planes, False, str(tmp_path)), _encode_file(planes, True, str(tmp_path))]
    out = str(tmp_path / "dev.blobs")
    subprocess.run([os.path.join(HOST, "host_driver"), "decode_device", out] + files, check=True, stdout=subprocess.DEVNULL)
    b = parse_blobs(out)
    for i, bpp in enumerate((3, 4)):
        info = np.frombuffer(b[f"dev_info_{i}"], np.int32)
        assert list(info[:7]) == [1, 0, 1, 0, w, h, bpp], info
        host, dev = b[f"host_image_{i}"], b[f"dev_image_{i}"]
        assert len(host) == w * h * bpp and host == dev, i
        assert (info[7], info[8]) == (0, YAIK_DECIMG_INVALIDCTX)                  # a custom builder is refused
    img = np.frombuffer(b["dev_image_1"], np.uint8).reshape(h, w, 4)
    assert np.array_equal(img[..., 3], a.astype(np.uint8))
