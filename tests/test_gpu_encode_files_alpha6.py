"""Frames in device memory to .yaik streams with ConvertHotPath's alpha6Bit option: YAIK_EncodeImagesFromDeviceAlpha6
(yaik_amd.files.encode_files_device(alpha_6bit=True)).  The reference of every comparison at level 0 is the file EncoderContext::ConvertHotPath
writes for the frame alone with emitAlpha and alpha6Bit (`alpha_driver enc ... alpha6`, a process per file, made once per module)."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

from tests.test_gpu_encode_files import CHILD_TIMEOUT, DRIVER, HOST, TAGS, _alpha, _chunk_list, _parse
from yaik_amd import files
from yaik_amd.synth import synth_planes

pytestmark = pytest.mark.gpu
W = H = 128
BOX = (32, 16, 112, 80)                                                       # x0, y0, x1, y1 of "full6": whole tiles, not the image


def _torch():
    import torch
    return torch


def _alpha6(kind):
    y, x = np.mgrid[0:H, 0:W]
    if kind == "full6":                                                       # every tile of the 'MIPM' box kept: the 6-bit mask mode is taken
        a = np.zeros((H, W), np.int32)
        x0, y0, x1, y1 = BOX
        a[y0:y1, x0:x1] = ((x * 3 + y * 5) % 251 + 4)[y0:y1, x0:x1]
        return a
    if kind == "full6b":                                                      # the same rule on another box, with samples below 4 in it
        a = np.zeros((H, W), np.int32)
        a[48:128, 0:64] = ((x * 7 + y * 11) % 256)[48:128, 0:64]
        a[48:128:16, 0:64:16] = 77                                            # every tile holds a sample
        return a
    return _alpha(kind, W, H)                                                 # "holes": a rejected tile inside the box; "binary"; "all255"


# name -> (kind, seed, the 'ALPM' mode of the reference file, None = no chunk)
CASES = {"full6": ("full6", 21, 3), "full6b": ("full6b", 22, 3), "holes": ("holes", 16, 6), "binary": ("binary", 14, 1), "all255": ("all255", 15, None),
         "rgb": ("rgb", 11, None)}


def _planes(kind, seed):
    rgb = synth_planes(W, H, n_planes=3, seed=seed)
    return rgb if kind == "rgb" else np.concatenate([rgb, _alpha6(kind)[None]])


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    """name -> (u8 frame [h, w, c], the file ConvertHotPath writes for it with emitAlpha + alpha6Bit, the same without alpha6Bit)"""
    subprocess.run(["make", "-C", HOST], check=True, stdout=subprocess.DEVNULL, timeout=600)
    d = tmp_path_factory.mktemp("refs6")
    out = {}
    for name, (kind, seed, _) in CASES.items():
        planes = _planes(kind, seed)
        src = str(d / f"{name}.bin")
        with open(src, "wb") as f:
            f.write(struct.pack("<3i", W, H, planes.shape[0]))
            f.write(np.ascontiguousarray(planes, np.int32).tobytes())
        got = []
        for tag, opts in (("six", ["alpha6"]), ("eight", [])):
            if tag == "eight" and CASES[name][2] != 3:                        # the fallback writes the same file (tests/test_gpu_alpha_6bit.py pins it)
                got.append(got[0])
                continue
            dst = str(d / f"{name}_{tag}.yaik")
            subprocess.run([DRIVER, "enc", src, dst, "1", *opts], check=True, timeout=CHILD_TIMEOUT, stdout=subprocess.DEVNULL)
            got.append(open(dst, "rb").read())
        out[name] = (np.ascontiguousarray(planes.transpose(1, 2, 0)).astype(np.uint8), got[0], got[1])
    return out


def _alpm_mode(stream):
    for tag, at, _ in _chunk_list(stream):
        if tag == TAGS["ALPM"]:
            return stream[at + 8 + 17] & 7                                    # AlphaHeader::parameters
    return None


def _batch(refs, names, which=1):
    torch = _torch()
    return torch.from_numpy(np.stack([refs[n][0] for n in names])).cuda(), [refs[n][which] for n in names]


RGBA7 = ["full6", "holes", "binary", "full6b", "all255", "holes", "full6"]


def test_reference_files_are_what_their_names_say(refs):
    for name, (_, _, mode) in CASES.items():
        assert _alpm_mode(refs[name][1]) == mode, name
        assert _alpm_mode(refs[name][2]) == (6 if mode == 3 else mode), name
        assert (refs[name][1] == refs[name][2]) == (mode != 3), name            # alpha6Bit changes the file only where the 6-bit mode is taken


def test_batches_equal_the_single_files(refs):
    frames, want = _batch(refs, RGBA7)
    got = files.encode_files_device(frames, emit_alpha=True, alpha_6bit=True)
    for f, (g, w) in enumerate(zip(got, want)):
        assert g == w, (f, RGBA7[f], len(g), len(w))
    assert [_alpm_mode(s) for s in got] == [3, 6, 1, 3, None, 6, 3]
    assert got == files.encode_files_device(frames, emit_alpha=True, alpha_6bit=True, threads=1)         # no byte depends on the workers
    order = [3, 0, 6, 2, 5, 1, 4]                                             # the same frames in another order
    shuffled = files.encode_files_device(frames[order], emit_alpha=True, alpha_6bit=True)
    assert shuffled == [want[i] for i in order]
    for name in CASES:                                                        # and as batches of one
        if name != "rgb":
            assert files.encode_file_device(_torch().from_numpy(refs[name][0]).cuda(), emit_alpha=True, alpha_6bit=True) == refs[name][1], name
    frames, want = _batch(refs, ["rgb", "rgb"])                               # RGB: alpha6Bit has nothing to act on
    assert files.encode_files_device(frames, emit_alpha=True, alpha_6bit=True) == want


def test_alpha6_off_or_without_emit_alpha_changes_nothing(refs):
    frames, eight = _batch(refs, RGBA7, which=2)
    assert files.encode_files_device(frames, emit_alpha=True) == eight                                    # today's output
    assert files.encode_files_device(frames, emit_alpha=True, alpha_6bit=False) == eight
    off = files.encode_files_device(frames, emit_alpha=False)
    assert files.encode_files_device(frames, emit_alpha=False, alpha_6bit=True) == off
    assert all(_alpm_mode(s) is None for s in off)
    L = files.host_lib()                                                      # alpha6Bit = 0 on the new entry is the old entry
    e = files.encoder(0)
    n, h, w, c = frames.shape
    failed = C.c_int32(99)
    _torch().cuda.synchronize()
    assert L.YAIK_EncodeImagesFromDeviceAlpha6(e, frames.data_ptr(), w * c, h * w * c, c, w, h, n, 1, 0, 0, 4, C.byref(failed)) and failed.value == -1
    for f in range(n):
        data, nb = C.c_void_p(), C.c_uint32()
        assert L.YAIK_EncodedStream(e, f, C.byref(data), C.byref(nb)) and C.string_at(data.value, nb.value) == eight[f]
    for bad in (2, -1):                                                       # refused with its name, nothing handed out, the encoder usable
        failed.value = 99
        assert not L.YAIK_EncodeImagesFromDeviceAlpha6(e, frames.data_ptr(), w * c, h * w * c, c, w, h, n, 1, bad, 0, 4, C.byref(failed))
        assert failed.value == -1 and "alpha6Bit" in L.YAIK_EncoderLastError(e).decode()
        data, nb = C.c_void_p(), C.c_uint32()
        assert not L.YAIK_EncodedStream(e, 0, C.byref(data), C.byref(nb))
    assert not L.YAIK_EncodeImagesFromDeviceAlpha6(e, frames.data_ptr(), w * c, h * w * c, c, w, h, n, 2, 1, 0, 4, C.byref(failed))
    assert "emitAlpha" in L.YAIK_EncoderLastError(e).decode()                 # pinned: emitAlpha = 2 is refused as before
    assert files.encode_files_device(frames, emit_alpha=True, alpha_6bit=True) == [refs[k][1] for k in RGBA7]


def test_level_3_keeps_chunk_order_and_payloads(refs, tmp_path):
    names = ["full6", "holes", "binary", "full6b"]
    frames, want = _batch(refs, names)
    l0 = files.encode_files_device(frames, emit_alpha=True, level=0, alpha_6bit=True)
    l3 = files.encode_files_device(frames, emit_alpha=True, level=3, alpha_6bit=True)
    assert l0 == want and l3 == files.encode_files_device(frames, emit_alpha=True, level=3, threads=1, alpha_6bit=True)
    for f in range(len(names)):
        a, b = l0[f], l3[f]
        assert a != b and a[:12] == b[:12]
        assert [t for t, _, _ in _chunk_list(a)] == [t for t, _, _ in _chunk_list(b)], f
        pa, pb = _parse(tmp_path, a, f"a{f}"), _parse(tmp_path, b, f"b{f}")
        assert list(pa) == list(pb) and len(pa) > 4
        for k in pa:
            if k.endswith("_pad"):
                n, ored = np.frombuffer(pb[k], np.int32).tolist()
                assert 0 <= n <= 3 and ored == 0
            else:
                assert bytes(pa[k]) == bytes(pb[k]), (f, k)


def test_the_written_streams_decode_to_the_quantised_alpha(refs):
    frames, _ = _batch(refs, RGBA7)
    for level in (0, 3):
        streams = files.encode_files_device(frames, emit_alpha=True, level=level, alpha_6bit=True)
        got = files.decode_files_device(streams, channels=4).cpu().numpy()
        assert files.last_batch_info()["fallbacks"] == 0
        src = frames.cpu().numpy()
        for f, name in enumerate(RGBA7):
            a = src[f, ..., 3].astype(np.int32)
            if name.startswith("full6"):                                      # inside the value box (v >> 2 << 2) | (v >> 6), 0 outside
                ys, xs = np.nonzero(a >> 2)
                x0, x1, y0, y1 = (xs.min() >> 2) << 2, ((xs.max() + 4) >> 2) << 2, ys.min(), ys.max() + 1
                want = np.zeros((H, W), np.uint8)
                v = a[y0:y1, x0:x1]
                want[y0:y1, x0:x1] = ((v >> 2) << 2) | (v >> 6)
                np.testing.assert_array_equal(got[f, ..., 3], want, err_msg=f"{level} {f} {name}")
            elif name == "holes":                                             # the 8-bit fallback comes back exactly inside its box
                ys, xs = np.nonzero(a >> 2)
                np.testing.assert_array_equal(got[f, ys.min():ys.max() + 1, xs.min():xs.max() + 1, 3], a[ys.min():ys.max() + 1, xs.min():xs.max() + 1])
            elif name == "all255":
                assert bool((got[f, ..., 3] == 255).all())
