"""Frames in device memory to .yaik streams as one batch: YAIK_EncodeImagesFromDevice (yaik_amd.files.encode_files_device).  The reference of every
comparison at level 0 is the file EncoderContext::ConvertHotPath writes for the frame alone (`alpha_driver enc`, a process per file, made once per
module); level 3 is compared with level 0 chunk by chunk, payload by payload, and through the batch decoder."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle.refrun import parse_blobs
from yaik_amd import files
from yaik_amd.synth import synth_planes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yaik_amd", "host")
DRIVER = os.path.join(HOST, "alpha_driver")
TOOL = os.path.join(HOST, "encode_frame_tool")
CHILD_TIMEOUT = 120                                                          # seconds: a child process takes a second or two
TAGS = {"MIPM": 0x4D50494D, "ALPM": 0x4D504C41, "GTIL": 0x4C495447, "1DTL": 0x4C544431}


def _torch():
    import torch
    return torch


def _alpha(kind, w, h):
    y, x = np.mgrid[0:h, 0:w]
    a = np.zeros((h, w), np.int32)
    x0, y0, x1, y1 = w // 4 + 3, h // 4 + 1, w - 9, h - 5                     # a box inside the image, on no tile edge
    if kind == "analog":
        a[y0:y1, x0:x1] = ((x * 3 + y * 5) % 251 + 4)[y0:y1, x0:x1]
    elif kind == "binary":
        a[y0:y1, x0:x1] = 255 * (((x >> 2) + (y >> 1)) & 1)[y0:y1, x0:x1]
        a[y0, x0] = a[y1 - 1, x1 - 1] = 255
    elif kind == "all255":
        a[:] = 255
    elif kind == "holes":                                                    # kept tiles all round, rejected tiles inside the box
        a[8:h - 8, 8:w - 24] = ((x * 7 + y * 3) % 200 + 30)[8:h - 8, 8:w - 24]
        a[48:80, 32:80] = 0
    else:
        raise ValueError(kind)
    return a


def _planes(w, h, kind, seed):
    rgb = synth_planes(w, h, n_planes=3, seed=seed)
    return rgb if kind == "rgb" else np.concatenate([rgb, _alpha(kind, w, h)[None]])


# name -> (w, h, kind, seed, emitAlpha): the eight reference files
CASES = {
    "rgb128": (128, 128, "rgb", 11, 0), "rgb72": (72, 40, "rgb", 12, 0),
    "analog128_off": (128, 128, "analog", 13, 0), "analog128": (128, 128, "analog", 13, 1),
    "binary128": (128, 128, "binary", 14, 1), "all255_128": (128, 128, "all255", 15, 1), "holes128": (128, 128, "holes", 16, 1),
    "analog72": (72, 40, "analog", 17, 1),
}


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """name -> (u8 frame [h, w, c], the file ConvertHotPath writes for it)"""
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL, timeout=600)
    assert len(CASES) <= 8
    d = tmp_path_factory.mktemp("refs")
    out = {}
    for name, (w, h, kind, seed, emit) in CASES.items():
        planes = _planes(w, h, kind, seed)
        src, dst = str(d / f"{name}.bin"), str(d / f"{name}.yaik")
        with open(src, "wb") as f:
            f.write(struct.pack("<3i", w, h, planes.shape[0]))
            f.write(np.ascontiguousarray(planes, np.int32).tobytes())
        subprocess.run([DRIVER, "enc", src, dst, str(emit)], check=True, timeout=CHILD_TIMEOUT, stdout=subprocess.DEVNULL)
        out[name] = (np.ascontiguousarray(planes.transpose(1, 2, 0)).astype(np.uint8), open(dst, "rb").read())
    return out


def _chunk_list(stream):
    out, p = [], 12
    while True:
        tag = struct.unpack_from("<I", stream, p)[0]
        if tag == 0xDEADBEEF:
            assert p + 4 == len(stream)
            return out
        length = struct.unpack_from("<I", stream, p + 4)[0]
        out.append((tag, p, 8 + length))
        p += 8 + length


def _batch(refs, names):
    torch = _torch()
    return torch.from_numpy(np.stack([refs[n][0] for n in names])).cuda(), [refs[n][1] for n in names]


RGBA7 = ["analog128", "binary128", "all255_128", "holes128", "binary128", "analog128", "holes128"]


def test_reference_files_are_what_their_names_say(refs):
    tags = {n: [t for t, _, _ in _chunk_list(s)] for n, (_, s) in refs.items()}
    for n, t in tags.items():
        assert t == sorted(t, key=list(TAGS.values()).index) and TAGS["GTIL"] in t, n
    assert TAGS["MIPM"] not in tags["rgb128"] and TAGS["ALPM"] not in tags["rgb128"]
    assert TAGS["MIPM"] in tags["analog128_off"] and TAGS["ALPM"] not in tags["analog128_off"]
    for n in ("analog128", "binary128", "holes128", "analog72"):
        assert tags[n][:2] == [TAGS["MIPM"], TAGS["ALPM"]], n
    assert TAGS["MIPM"] not in tags["all255_128"] and TAGS["ALPM"] not in tags["all255_128"]
    mode = {n: refs[n][1][_chunk_list(refs[n][1])[1][1] + 8 + 17] for n in ("analog128", "binary128", "holes128")}   # AlphaHeader::parameters
    assert mode == {"analog128": 6, "binary128": 1, "holes128": 6}
    _, at, size = _chunk_list(refs["holes128"][1])[0]                        # rejected tiles inside the box: a zero bit between set bits
    bits = np.unpackbits(np.frombuffer(refs["holes128"][1][at + 8 + 16:at + size], np.uint8), bitorder="little")
    assert struct.unpack_from("<4h", refs["holes128"][1], at + 8) == (0, 0, 7, 8) and int(bits[:56].sum()) == 50 and not bits[56:].any()


def test_rgb_and_mixed_rgba_batches_equal_the_single_files(refs):
    frames, want = _batch(refs, ["rgb128"] * 7)
    got = files.encode_files_device(frames)
    assert got == want
    frames, want = _batch(refs, RGBA7)
    got = files.encode_files_device(frames, emit_alpha=True)
    for f, (g, w) in enumerate(zip(got, want)):
        assert g == w, (f, RGBA7[f], len(g), len(w))
    assert got == files.encode_files_device(frames, emit_alpha=True, threads=1)          # no byte depends on the workers
    info = files.last_encode_info()
    assert info["total_ms"] > 0 and info["total_ms"] >= info["entropy_ms"] > 0 and info["device_ms"] > 0 and info["gather_ms"] > 0
    frames, want = _batch(refs, ["analog128_off"] * 2)                       # RGBA with the 'ALPM' opt-in off
    assert files.encode_files_device(frames, emit_alpha=False) == want
    frames, want = _batch(refs, ["analog72", "analog72", "analog72"])        # part tiles on both edges
    assert files.encode_files_device(frames, emit_alpha=True) == want
    frames, want = _batch(refs, ["rgb72"])
    assert files.encode_files_device(frames) == want


def test_padded_row_and_frame_pitches(refs):
    torch = _torch()
    frames, want = _batch(refs, RGBA7)
    n, h, w, c = frames.shape
    for pad_rows, pad_px, off in ((3, 5, 0), (1, 1, 4)):
        buf = torch.full((off + n * (h + pad_rows) * (w + pad_px) * c,), 0x5A, dtype=torch.uint8, device="cuda")
        view = torch.as_strided(buf, (n, h, w, c), ((h + pad_rows) * (w + pad_px) * c, (w + pad_px) * c, c, 1), off)
        view.copy_(frames)
        assert files.encode_files_device(view, emit_alpha=True) == want
    assert files.encode_files_device(np.stack([refs[k][0] for k in RGBA7]), emit_alpha=True) == want       # numpy: uploaded through torch


def test_a_batch_of_one(refs):
    torch = _torch()
    for name, emit in (("rgb128", False), ("holes128", True), ("analog72", True), ("all255_128", True)):
        assert files.encode_file_device(torch.from_numpy(refs[name][0]).cuda(), emit_alpha=emit) == refs[name][1], name


def _encode_with(e, frames, emit, level=0, threads=4):
    """the C entry points on a given encoder"""
    torch = _torch()
    L = files.host_lib()
    n, h, w, c = frames.shape
    failed = C.c_int32(99)
    torch.cuda.synchronize()
    ok = L.YAIK_EncodeImagesFromDevice(e, frames.data_ptr(), w * c, h * w * c, c, w, h, n, int(emit), level, threads, C.byref(failed))
    assert ok and failed.value == -1, L.YAIK_EncoderLastError(e)
    out = []
    for f in range(n):
        data, nb = C.c_void_p(), C.c_uint32()
        assert L.YAIK_EncodedStream(e, f, C.byref(data), C.byref(nb))
        out.append(C.string_at(data.value, nb.value))
    return out


def test_three_calls_on_one_encoder_equal_fresh_encoders(refs):
    L = files.host_lib()
    calls = [(["analog128", "holes128", "binary128", "all255_128", "analog128"], 1), (["analog72", "analog72"], 1), (["rgb128"], 0)]
    one = L.YAIK_EncoderCreate(0)
    assert one
    try:
        for names, emit in calls:
            frames, want = _batch(refs, names)
            got = _encode_with(one, frames, emit)
            fresh = L.YAIK_EncoderCreate(0)
            assert fresh
            try:
                assert got == _encode_with(fresh, frames, emit)
            finally:
                L.YAIK_EncoderRelease(fresh)
            assert got == want
    finally:
        L.YAIK_EncoderRelease(one)


def _parse(tmp_path, stream, tag):
    p = tmp_path / f"{tag}.yaik"
    p.write_bytes(stream)
    subprocess.run([TOOL, "parse", str(p), str(tmp_path / f"{tag}.blobs")], check=True, timeout=CHILD_TIMEOUT)
    return parse_blobs(str(tmp_path / f"{tag}.blobs"))


def test_level_3(refs, tmp_path):
    frames, want = _batch(refs, RGBA7)
    l0 = files.encode_files_device(frames, emit_alpha=True, level=0)
    l3 = files.encode_files_device(frames, emit_alpha=True, level=3)
    assert l0 == want and l3 == files.encode_files_device(frames, emit_alpha=True, level=3, threads=1)
    for f in range(4):                                                       # the four distinct frames
        a, b = l0[f], l3[f]
        assert a != b and a[:12] == b[:12]
        assert [t for t, _, _ in _chunk_list(a)] == [t for t, _, _ in _chunk_list(b)], f          # the same tags in the same order
        pa, pb = _parse(tmp_path, a, f"a{f}"), _parse(tmp_path, b, f"b{f}")
        assert list(pa) == list(pb) and len(pa) > 4
        for k in pa:                                                         # headers apart from compressed sizes, every decompressed payload
            if k.endswith("_pad"):
                n, ored = np.frombuffer(pb[k], np.int32).tolist()
                assert 0 <= n <= 3 and ored == 0
            else:
                assert bytes(pa[k]) == bytes(pb[k]), (f, k)
        assert np.frombuffer(pb["chunk_count_terminated_rest"], np.int32).tolist()[1:] == [1, 0]
    px0 = files.decode_files_device(l0, channels=4)
    assert files.last_batch_info()["fallbacks"] == 0
    px3 = files.decode_files_device(l3, channels=4)
    assert files.last_batch_info()["fallbacks"] == 0
    assert bool((px0 == px3).all())
    got = px3.cpu().numpy()
    src = frames.cpu().numpy()
    x0, y0, x1, y1 = 128 // 4 + 3, 128 // 4 + 1, 128 - 9, 128 - 5
    np.testing.assert_array_equal(got[0, y0:y1, x0:x1, 3], src[0, y0:y1, x0:x1, 3])     # 8-bit alpha comes back exactly inside its box


def test_refusals_leave_the_encoder_usable(refs):
    torch = _torch()
    L = files.host_lib()
    frames, want = _batch(refs, ["holes128", "binary128"])
    n, h, w, c = frames.shape
    e = files.encoder(0)
    assert _encode_with(e, frames, 1) == want
    failed = C.c_int32(99)
    torch.cuda.synchronize()
    args = dict(px=frames.data_ptr(), row=w * c, frame=h * w * c, c=c, w=w, h=h, n=n, emit=1, level=0, threads=4)

    def call(**kw):
        a = dict(args, **kw)
        failed.value = 99
        ok = L.YAIK_EncodeImagesFromDevice(e, a["px"], a["row"], a["frame"], a["c"], a["w"], a["h"], a["n"], a["emit"], a["level"], a["threads"], C.byref(failed))
        return ok, failed.value, L.YAIK_EncoderLastError(e).decode()

    for kw, word in ((dict(px=None), "devPixels"), (dict(n=0), "1..1024"), (dict(n=1025), "1..1024"), (dict(c=2), "channels"), (dict(w=100), "multiples of 8"),
                     (dict(row=w * c - 1), "rowBytes"), (dict(frame=h * w * c - 1), "frameBytes"), (dict(level=23), "zstdLevel"), (dict(level=-1), "zstdLevel"),
                     (dict(threads=0), "threads"), (dict(threads=17), "threads"), (dict(emit=2), "emitAlpha")):
        ok, idx, msg = call(**kw)
        assert not ok and idx == -1 and word in msg, (kw, idx, msg)
        data, nb = C.c_void_p(), C.c_uint32()
        assert not L.YAIK_EncodedStream(e, 0, C.byref(data), C.byref(nb)) and data.value is None and nb.value == 0   # nothing is handed out after a failure
    ok, idx, msg = call()
    assert ok and idx == -1
    assert _encode_with(e, frames, 1) == want                                # and the next call works
    data, nb = C.c_void_p(), C.c_uint32()
    assert not L.YAIK_EncodedStream(e, n, C.byref(data), C.byref(nb)) and not L.YAIK_EncodedStream(e, -1, C.byref(data), C.byref(nb))
    with pytest.raises(files.YaikEncodeError) as ei:
        files.encode_files_device(frames, level=23)
    assert ei.value.index == -1
    with pytest.raises(ValueError):
        files.encode_files_device(frames.cpu())
    with pytest.raises(ValueError):
        files.encode_files_device(frames[..., :2])
    assert files.encode_files_device(frames, emit_alpha=True) == want
    ms = (C.c_double * 4)()
    L.YAIK_LastEncodeStageMs(e, ms)
    assert ms[3] > 0
