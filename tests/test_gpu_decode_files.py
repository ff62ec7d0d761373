"""`.yaik` files as a batch: YAIK_DecodeImagesToDevice through yaik_amd/files.py (decode_files_device) against YAIK_DecodeImageToDevice
(decode_file_device) on the same streams.  The files are written by ConvertHotPath (alpha_driver enc): RGB, RGBA with emitAlpha off, RGBA with
8-bit alpha, with binary alpha, and with alpha6 (mode 3 through the 'MIPM' mask).  Every comparison is bit-exact and over every pixel."""
import os
import struct
import subprocess

import numpy as np
import pytest

from tests.images import edge_image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADRV = os.path.join(ROOT, "yaik_amd", "host", "alpha_driver")
TAG_MIPM, TAG_ALPM, TAG_GTIL = 0x4D50494D, 0x4D504C41, 0x4C495447
SENTINEL = 0xA5
YAIK_INVALID_HEADER = 7
KINDS = ["rgb", "rgba_off", "alpha8", "binary", "alpha6"]


def _torch():
    import torch
    return torch


def _chunks(data):
    out, p = [], 12
    while p + 4 <= len(data):
        tag = struct.unpack_from("<I", data, p)[0]
        if tag == 0xDEADBEEF:
            break
        ln = struct.unpack_from("<I", data, p + 4)[0]
        out.append((p, tag, ln))
        p += 8 + ln
    return out


def _alpha(kind, w, h, rng):
    """an alpha plane whose non-zero samples fill whole 16x16 tiles of a box inside the image: a 'MIPM' chunk, every tile of its box kept"""
    a = np.zeros((h, w), np.int32)
    y0, y1, x0, x1 = (16, 80, 32, 112) if w == 128 else (0, 32, 16, 64)
    if kind == "binary":
        a[y0:y1, x0:x1] = 255 * rng.integers(0, 2, (y1 - y0, x1 - x0))
        a[y0, x0] = a[y1 - 1, x1 - 1] = 255
    else:
        a[y0:y1, x0:x1] = rng.integers(0, 256, (y1 - y0, x1 - x0))
        a[y0, x0] = a[y1 - 1, x1 - 1] = 200
    return a


def _encode(planes, tmp, emit, *opts):
    n, h, w = planes.shape
    fin, fy = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.yaik")
    with open(fin, "wb") as f:
        f.write(struct.pack("<3i", w, h, n)); f.write(np.ascontiguousarray(planes, np.int32).tobytes())
    subprocess.run([ADRV, "enc", fin, fy, "1" if emit else "0", *opts], check=True)
    with open(fy, "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """(w, kind) -> stream, written once"""
    subprocess.run(["make", "-C", os.path.join(ROOT, "yaik_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    tmp = str(tmp_path_factory.mktemp("yaik"))
    rng = np.random.default_rng(71)
    out = {}
    for w, h in ((128, 128), (72, 40)):
        rgb = edge_image(w, h, "mixed", 3)
        for kind in KINDS:
            if kind == "rgb":
                out[w, kind] = _encode(rgb, tmp, False)
                continue
            planes = np.concatenate([rgb, _alpha(kind, w, h, rng)[None]])
            out[w, kind] = _encode(planes, tmp, kind != "rgba_off", *(["alpha6"] if kind == "alpha6" else []))
    return out


@pytest.fixture(scope="module")
def files():
    from yaik_amd import files as F
    F.set_device_palette(False)
    yield F
    F.set_device_palette(False)


def _rgba(F, stream, cache, palette):
    """decode_file_device of the stream as [H, W, 4]: 255 added as alpha where the single call writes RGB"""
    key = (hash(stream), palette)
    if key not in cache:
        got = F.decode_file_device(stream).cpu().numpy()
        assert got.shape[2] == (4 if F.has_alpha_chunk(stream) else 3)
        if got.shape[2] == 3:
            got = np.concatenate([got, np.full(got.shape[:2] + (1,), 255, np.uint8)], axis=2)
        cache[key] = got
    return cache[key]


@pytest.fixture(scope="module")
def singles():
    return {}


def _check(F, streams, singles, palette=False, channels=4, planar=False, threads=16, padded=False, fallbacks=0):
    torch = _torch()
    want = np.stack([_rgba(F, s, singles, palette) for s in streams])[..., :channels]
    n, h, w, _ = want.shape
    if not padded:
        got = F.decode_files_device(streams, channels=channels, planar=planar, threads=threads)
        buf = None
    else:
        row = (w if planar else channels * w) + 7
        plane = row * h + 13
        frame = (channels * plane if planar else row * h) + 29
        buf = torch.full((3 + n * frame + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
        view = torch.as_strided(buf, (n, channels, h, w), (frame, plane, row, 1), 3) if planar else torch.as_strided(buf, (n, h, w, channels), (frame, row, channels, 1), 3)
        got = F.decode_files_device(streams, out=view, channels=channels, planar=planar, threads=threads)
    assert F.last_batch_info()["fallbacks"] == fallbacks
    g = got.cpu().numpy()
    np.testing.assert_array_equal(g.transpose(0, 2, 3, 1) if planar else g, want)
    if buf is not None:                                                       # row padding and the bytes between frames are never written
        exp = np.full(buf.numel(), SENTINEL, np.uint8)
        ev = np.lib.stride_tricks.as_strided(exp[3:], (n, channels, h, w), (frame, plane, row, 1)) if planar else \
            np.lib.stride_tricks.as_strided(exp[3:], (n, h, w, channels), (frame, row, channels, 1))
        ev[...] = want.transpose(0, 3, 1, 2) if planar else want
        np.testing.assert_array_equal(buf.cpu().numpy(), exp)
    return g


def test_the_files_are_what_their_names_say(made):
    for w in (128, 72):
        tags = {k: [t for _, t, _ in _chunks(made[w, k])] for k in KINDS}
        assert TAG_ALPM not in tags["rgb"] and TAG_ALPM not in tags["rgba_off"]
        modes = {}
        for k in ("alpha8", "binary", "alpha6"):
            p = next(c[0] for c in _chunks(made[w, k]) if c[1] == TAG_ALPM)
            modes[k] = made[w, k][p + 8 + 17] & 7
        assert modes == {"alpha8": 6, "binary": 1, "alpha6": 3}, (w, modes)
        assert tags["alpha6"][0] == TAG_MIPM and TAG_GTIL in tags["rgb"]


@pytest.mark.parametrize("palette", [False, True], ids=["host_palette", "device_palette"])
def test_mixed_batch_in_four_layouts(files, made, singles, palette):
    files.set_device_palette(palette)
    streams = [made[128, k] for k in ("rgb", "alpha6", "rgba_off", "alpha8", "binary", "alpha6")]
    for channels in (3, 4):
        for planar in (False, True):
            _check(files, streams, singles, palette, channels, planar, padded=True)
    files.set_device_palette(False)


def test_ragged_width_batch(files, made, singles):
    _check(files, [made[72, k] for k in ("alpha6", "rgb", "alpha8", "binary", "rgba_off")], singles)


def _swap_first_two_gtil(stream):
    gt = [c for c in _chunks(stream) if c[1] == TAG_GTIL]
    (a, _, la), (b, _, lb) = gt[0], gt[1]
    assert b == a + 8 + la
    return stream[:a] + stream[b:b + 8 + lb] + stream[a:a + 8 + la] + stream[b + 8 + lb:]


def test_one_fallback_stream(files, made, singles):
    swapped = _swap_first_two_gtil(made[128, "alpha8"])
    streams = [made[128, "rgb"], swapped, made[128, "alpha6"], made[128, "binary"]]
    for channels, planar in ((4, False), (3, True)):
        _check(files, streams, singles, channels=channels, planar=planar, fallbacks=1)


def test_batch_of_one(files, made, singles):
    _check(files, [made[128, "alpha6"]], singles)
    _check(files, [made[72, "rgb"]], singles, channels=3)


def test_threads_do_not_change_the_bytes(files, made, singles):
    streams = [made[128, k] for k in KINDS]
    a = _check(files, streams, singles, threads=1)
    b = _check(files, streams, singles, threads=16)
    np.testing.assert_array_equal(a, b)


def test_a_truncated_stream_fails_like_the_single_call(files, made, singles):
    cut = made[128, "alpha8"][:len(made[128, "alpha8"]) * 2 // 3]
    with pytest.raises(files.YaikFileError) as one:
        files.decode_file_device(cut)
    streams = [made[128, "rgb"], made[128, "alpha6"], cut, made[128, "binary"], cut]
    with pytest.raises(files.YaikFileError) as many:
        files.decode_files_device(streams, channels=4)
    assert many.value.index == 2 and many.value.code == one.value.code and one.value.code != 0
    _check(files, streams[:2] + streams[3:4], singles)                       # the next call on the same library succeeds


def test_a_stream_of_another_size_is_an_invalid_header(files, made, singles):
    with pytest.raises(files.YaikFileError) as e:
        files.decode_files_device([made[128, "rgb"], made[128, "alpha8"], made[72, "rgb"]], channels=3)
    assert e.value.code == YAIK_INVALID_HEADER and e.value.index == 2
    _check(files, [made[128, "rgb"]], singles, channels=3)
