"""One window of each of n `.yaik` files: YAIK_DecodeImagesWindowsToDevice through yaik_amd/files.py (decode_files_windows_device) against the crops
of YAIK_DecodeImagesToDevice (decode_files_device) on the same streams -- RGB streams, RGBA streams with 8-bit 'ALPM', RGBA streams in the 6-bit mask
mode, and a mix of batchable streams with one fallback stream.  Every comparison is bit-exact and over every byte of the destination.

The fallback stream: tests/golden holds chunk blobs, no whole .yaik stream, so the stream is made here from the image of the golden fixture
pp_planemix128_rgb (tests/golden/make_golden.py PARTIAL): encoded like the others, then its 4x4 'GTIL' chunk re-labelled as an R+G chunk
(HeaderGradientTile::plane = 3), which makes it a plane-subset stream the batch planner hands to the single-image chain."""
import ctypes as C
import struct

import numpy as np
import pytest

from tests import batch_window_cases as BC
from tests.images import edge_image

pytestmark = pytest.mark.gpu
SENTINEL = 0xA5
TAG_ALPM, TAG_GTIL = 0x4D504C41, 0x4C495447
W, H, N = 136, 264, 3


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def files():
    from yaik_amd import files as F
    F.set_device_palette(False)
    yield F
    F.set_device_palette(False)


def _chunks(data):
    out, p = [], 12
    while p + 8 <= len(data):
        tag, ln = struct.unpack_from("<II", data, p)
        if tag == 0xDEADBEEF:
            break
        out.append((p, tag, ln))
        p += 8 + ln
    return out


def _alpha_mode(stream):
    p = next(c[0] for c in _chunks(stream) if c[1] == TAG_ALPM)
    return stream[p + 8 + 17] & 7


def _analog_alpha(w, h, rng):
    """non-zero samples that fill whole 16x16 tiles of a box inside the image: a 'MIPM' chunk with every tile of its box kept, so the 6-bit mask
    mode can take it"""
    a = np.zeros((h, w), np.uint8)
    a[16:80, 32:112] = rng.integers(1, 256, (64, 80))
    return a


def _frames(w, h, kind, n, alpha):
    rng = np.random.default_rng(w + h + n)
    out = []
    for f in range(n):
        rgb = edge_image(w, h, kind, 3, seed=BC.frame_seed(w, h, f)).astype(np.uint8)
        planes = np.concatenate([rgb, _analog_alpha(w, h, rng)[None]]) if alpha else rgb
        out.append(np.ascontiguousarray(planes.transpose(1, 2, 0)))
    return np.stack(out)


@pytest.fixture(scope="module")
def streams(files):
    """kind -> N streams of W x H: "rgb", "alpha8" (8-bit 'ALPM'), "alpha6" (the 6-bit mask mode)"""
    out = {"rgb": files.encode_files_device(_frames(W, H, "mixed", N, False)),
           "alpha8": files.encode_files_device(_frames(W, H, "mixed", N, True), emit_alpha=True),
           "alpha6": files.encode_files_device(_frames(W, H, "mixed", N, True), emit_alpha=True, alpha_6bit=True)}
    assert not any(files.has_alpha_chunk(s) for s in out["rgb"])
    assert [_alpha_mode(s) for s in out["alpha8"]] == [6] * N and [_alpha_mode(s) for s in out["alpha6"]] == [3] * N
    return out


def _padded(torch, n, wh, ww, c, planar):
    row = (ww if planar else c * ww) + 7
    plane = row * wh + 13
    frame = (c * plane if planar else row * wh) + 29
    buf = torch.full((3 + n * frame + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    shape, strides = ((n, c, wh, ww), (frame, plane, row, 1)) if planar else ((n, wh, ww, c), (frame, row, c, 1))
    mask = torch.zeros(buf.numel(), dtype=torch.bool, device="cuda")
    torch.as_strided(mask, shape, strides, 3).fill_(True)
    return buf, torch.as_strided(buf, shape, strides, 3), mask


def _check(F, strs, origins, size, fallbacks=0):
    torch = _torch()
    n, (ww, wh) = len(strs), size
    whole = F.decode_files_device(strs, channels=4)
    assert F.last_batch_info()["fallbacks"] == fallbacks
    want = torch.stack([whole[f, y0:y0 + wh, x0:x0 + ww] for f, (x0, y0) in enumerate(origins)])
    for channels in (3, 4):
        for planar in (False, True):
            exp = want[..., :channels].permute(0, 3, 1, 2) if planar else want[..., :channels]
            got = F.decode_files_windows_device(strs, origins, size, channels=channels, planar=planar)
            assert F.last_batch_info()["fallbacks"] == fallbacks
            assert torch.equal(got, exp), (channels, planar)
            buf, view, mask = _padded(torch, n, wh, ww, channels, planar)
            assert F.decode_files_windows_device(strs, origins, size, out=view, channels=channels, planar=planar) is view
            assert torch.equal(view, exp) and (buf[~mask] == SENTINEL).all(), (channels, planar, "padded")
    return want


@pytest.mark.parametrize("kind", ["rgb", "alpha8", "alpha6"])
def test_windows_equal_the_crops_of_the_batch_decode(files, streams, kind):
    for name, size, origins in BC.window_sets(W, H):
        want = _check(files, streams[kind], origins, size)
        if kind != "rgb" and name == "whole":
            assert (want[..., 3] != 255).any()                               # the alpha of the streams is really read
    # origins as an array, one thread, and the batch of one
    got = files.decode_files_windows_device(streams[kind][:1], np.array([[56, 120]]), (32, 32), channels=4, threads=1)
    assert _torch().equal(got[0], files.decode_files_device(streams[kind][:1], channels=4)[0, 120:152, 56:88])


def _plane_subset(stream):
    stream = bytearray(stream)
    bodies = [p + 8 for p, tag, _ in _chunks(stream) if tag == TAG_GTIL and stream[p + 8 + 26] & 7 == 2 and (stream[p + 8 + 26] >> 3) & 7 == 2]
    assert len(bodies) == 1 and stream[bodies[0] + 27] == 7                  # the one 4x4 chunk, all three planes
    stream[bodies[0] + 27] = 3
    return bytes(stream)


def test_a_mix_with_one_fallback_stream(files):
    from tests.golden.make_golden import PARTIAL
    w = h = 128
    rng = np.random.default_rng(128)
    fixture = np.ascontiguousarray(PARTIAL["pp_planemix128_rgb"]().astype(np.uint8).transpose(1, 2, 0))
    rgb = _frames(w, h, "mixed", 2, False)
    rgba = np.stack([np.concatenate([rgb[f], _analog_alpha(w, h, rng)[..., None]], axis=2) for f in range(2)])
    fallback = _plane_subset(files.encode_file_device(fixture))
    strs = [files.encode_file_device(rgb[0]), fallback, files.encode_file_device(rgba[1], emit_alpha=True),
            files.encode_file_device(rgba[0], emit_alpha=True, alpha_6bit=True)]
    assert [files.has_alpha_chunk(s) for s in strs] == [False, False, True, True] and _alpha_mode(strs[3]) == 3
    for size, origins in (((32, 32), [(8, 8), (56, 56), (96, 96), (0, 64)]), ((128, 8), [(0, 0), (0, 64), (0, 120), (0, 56)]), ((128, 128), [(0, 0)] * 4)):
        _check(files, strs, origins, size, fallbacks=1)
    # the fallback stream alone, and first
    _check(files, [fallback, strs[0]], [(56, 56), (8, 8)], (24, 16), fallbacks=1)


def test_a_bad_window_fails_with_the_documented_code_and_writes_nothing(files, streams):
    torch = _torch()
    from yaik_amd.files import ERROR_NAMES, YaikFileError
    strs = streams["alpha8"]
    size = (32, 32)
    good = [(56, 56), (56, 120), (56, 184)]
    out = torch.full((N, 32, 32, 4), SENTINEL, dtype=torch.uint8, device="cuda")
    for f in range(N):                                                       # one stream's window outside the image, the others valid
        for bad in ((W - 24, 0), (0, H - 24), (W, 0), (0, H)):
            o = list(good)
            o[f] = bad
            with pytest.raises(YaikFileError) as e:
                files.decode_files_windows_device(strs, o, size, out=out, channels=4)
            assert ERROR_NAMES[e.value.code] == "YAIK_DECIMG_INVALIDCTX", (f, bad)
    with pytest.raises(YaikFileError) as e:
        files.decode_files_windows_device(strs, good, (W + 8, 8), out=torch.full((N, 8, W + 8, 4), SENTINEL, dtype=torch.uint8, device="cuda"), channels=4)
    assert ERROR_NAMES[e.value.code] == "YAIK_DECIMG_INVALIDCTX"
    # what Python lets through is refused by the library with the same code: an origin or size off the 8-pixel grid, a NULL table
    L, lib = files.host_lib(), files.library()
    bufs = [np.frombuffer(s, np.uint8) for s in strs]
    ptrs, lens = (C.c_void_p * N)(*[b.ctypes.data for b in bufs]), (C.c_uint32 * N)(*[b.size for b in bufs])
    failed = C.c_int32(0)
    for xy, ww, wh in (([4, 0, 0, 0, 0, 0], 32, 32), ([0, 0, 0, 0, 0, 0], 12, 32), ([0, 0, 0, 0, 0, 0], 32, 0), ([-8, 0, 0, 0, 0, 0], 32, 32), (None, 32, 32)):
        tab = (C.c_int * 6)(*xy) if xy else None
        assert not L.YAIK_DecodeImagesWindowsToDevice(lib, ptrs, lens, N, out.data_ptr(), 32 * 4, 0, 32 * 32 * 4, 4, 16, C.byref(failed), tab, ww, wh)
        assert ERROR_NAMES[L.YAIK_GetErrorCode()] == "YAIK_DECIMG_INVALIDCTX" and failed.value == -1
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()
    # ... and Python refuses them, and a wrong count or `out`, before any library call
    for bad_o, bad_size, exc in (([(4, 0)] + good[1:], size, ValueError), (good, (12, 32), ValueError), (good[:2], size, ValueError), (good, (32,), TypeError),
                                 ([(0.5, 0)] + good[1:], size, TypeError)):
        with pytest.raises(exc):
            files.decode_files_windows_device(strs, bad_o, bad_size, out=out, channels=4)
    with pytest.raises(ValueError):
        files.decode_files_windows_device(strs, good, size, out=out[:, :24], channels=4)
    with pytest.raises(ValueError):
        files.decode_files_windows_device(strs, good, size, out=out, channels=3)
    assert (out == SENTINEL).all()
    # the slot was released every time: the next call succeeds
    got = files.decode_files_windows_device(strs, good, size, out=out, channels=4)
    whole = files.decode_files_device(strs, channels=4)
    assert all(torch.equal(got[f], whole[f, y0:y0 + 32, x0:x0 + 32]) for f, (x0, y0) in enumerate(good))
