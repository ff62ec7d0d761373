"""CPU side of the batch file writer (YAIK_EncodeImagesFromDevice, yaik_amd/files.py) and of the two device calls under it: declarations, ctypes
tables and exported symbols agree; gather_layout on numpy; the HIP-free entropy stage and framing (encode_frame_tool) on the oracle's pass
outputs, against the product's chunk writer; the 'MIPM' bit rule as a numpy model against the decoder's mask."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from oracle.refrun import parse_blobs
from tests import alpha_ref as R
from tests import chunks
from tests import mip_ref as M
from yaik_amd.encoder import HipTileEncoder, _MipInfoC, gather_layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yaik_amd", "host")
TOOL = os.path.join(HOST, "encode_frame_tool")
NEW_HIP = {"yk_alpha_bitmaps_batch": 2, "yk_alpha_bitmap_device": 4, "yk_device_gather": 8}
NEW_HOST = {"YAIK_EncoderCreate": 1, "YAIK_EncoderRelease": 1, "YAIK_EncodeImagesFromDevice": 12, "YAIK_EncodedStream": 4, "YAIK_EncoderLastError": 1,
            "YAIK_LastEncodeStageMs": 2}
TAGS = {"MIPM": 0x4D50494D, "ALPM": 0x4D504C41, "GTIL": 0x4C495447, "1DTL": 0x4C544431}


def _arity(header_text, prefix):
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for name, args in re.findall(r"\b(%s[A-Za-z0-9_]+)\s*\(([^()]*)\)\s*;" % prefix, text):
        out[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return out


# ---- declarations -------------------------------------------------------------------------------------------------------------------------------
def test_hip_header_signature_table_and_library_agree():
    from yaik_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "yaik_hip.h")).read()
    declared = _arity(hdr, "yk_")
    for name, arity in NEW_HIP.items():
        assert declared.get(name) == arity, (name, declared.get(name))
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == arity and args[0] is C.c_void_p, name
    assert re.search(r"typedef struct yk_mip_info \{ int32_t hasChunk; int32_t bounds\[4\]; int32_t tileBBox\[4\]; uint32_t nBytes; \} yk_mip_info;", hdr)
    assert C.sizeof(_MipInfoC) == 40 and _MipInfoC.tileBBox.offset == 20 and _MipInfoC.nBytes.offset == 36
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)                                               # loading needs no device
    assert not [s for s in NEW_HIP if not hasattr(L, s)]


def test_host_header_ctypes_table_and_library_agree():
    from yaik_amd import files
    subprocess.run(["make", "-C", HOST, "libyaik_host.so"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(HOST, "yaik_encode.h")).read()
    assert 'extern "C"' in text
    declared = _arity(text, "YAIK_")
    assert declared == NEW_HOST
    assert sorted(files.ENC_SIGNATURES) == sorted(NEW_HOST)
    for name, (res, args) in files.ENC_SIGNATURES.items():
        assert len(args) == NEW_HOST[name], name
    out = subprocess.run(["nm", "-D", "--defined-only", files.HOST_LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(out.split())
    assert not [n for n in NEW_HOST if n not in exported]                   # C linkage: their own names
    L = files.host_lib()                                                    # loads without a device, every entry bound
    assert all(callable(getattr(L, name)) for name in NEW_HOST)
    assert L.YAIK_EncoderLastError(None) == b"null encoder"
    failed = C.c_int32(7)
    assert not L.YAIK_EncodeImagesFromDevice(None, None, 0, 0, 3, 8, 8, 1, 0, 0, 1, C.byref(failed)) and failed.value == -1
    assert files.last_encode_info() == {"device_ms": 0.0, "gather_ms": 0.0, "entropy_ms": 0.0, "total_ms": 0.0}


# ---- gather_layout ------------------------------------------------------------------------------------------------------------------------------
def test_gather_layout():
    lens = [0, 1, 15, 16, 17, 4095, 4096, 4097, 70001, 1000003]
    offs, total = gather_layout(lens)
    assert offs.dtype == np.int64 and offs.tolist() == [0, 0, 16, 32, 48, 80, 4176, 8272, 12384, 82400] and total == 82400 + 1000016
    end = 0
    for o, n in zip(offs.tolist(), lens):                                   # aligned, in order, nothing but the alignment gaps added
        assert o % 16 == 0 and end <= o < end + 16
        end = o + n
    assert total == (end + 15) // 16 * 16
    assert gather_layout([])[1] == 0 and gather_layout([]) [0].size == 0
    assert gather_layout(np.array([5], np.uint32)) [0].tolist() == [0] and gather_layout([5])[1] == 16
    assert gather_layout([0, 0, 0])[0].tolist() == [0, 0, 0] and gather_layout([0, 0, 0])[1] == 0
    big = gather_layout([(1 << 33) + 1, 7])
    assert big[0].tolist() == [0, (1 << 33) + 16] and big[1] == (1 << 33) + 32
    assert HipTileEncoder.gather_layout([3, 3])[0].tolist() == [0, 16]
    with pytest.raises(ValueError):
        gather_layout([4, -1])


# ---- the 'MIPM' bit rule --------------------------------------------------------------------------------------------------------------------------
def test_mip_bit_rule_against_the_decoder_mask():
    """bit y * tw + x, LSB first, is the keep flag of tile (bx0 + x, by0 + y): Decompress1BitTiled (tests/alpha_ref.py) must select exactly the kept
    tiles of the box"""
    rng = np.random.default_rng(8)
    for w, h in ((16, 16), (72, 40), (1040, 520), (208, 48)):
        mtw, mth = (w + 15) // 16, (h + 15) // 16
        for kind in M.KINDS:
            keep = M.keep_flags(M.alpha_plane(rng, h, w, kind))
            assert keep.shape == (mth, mtw)
            ys, xs = np.nonzero(keep)
            bounds = [9999999, 9999999, -1, -1] if ys.size == 0 else [int(xs.min()) * 16, int(ys.min()) * 16, int(xs.max()) * 16 + 16, int(ys.max()) * 16 + 16]
            has, tb, bits = M.mip_bits(keep, bounds, w, h)
            if ys.size == 0:
                assert has and bits.size == 0
                continue
            if bounds == [0, 0, w, h]:
                assert not has and bits.size == 0
                continue
            bx0, by0, tw, th = (int(v) for v in tb)
            assert has and bits.size == (tw * th + 7) // 8 and (bx0, by0, tw, th) == (int(xs.min()), int(ys.min()), int(np.ptp(xs)) + 1, int(np.ptp(ys)) + 1)
            mask = R.swizzled_mask(bits, tw, th).reshape(th, 2, tw, 16)
            np.testing.assert_array_equal(mask.min(axis=(1, 3)) == 255, keep[by0:by0 + th, bx0:bx0 + tw], err_msg=f"{w}x{h} {kind}")
            np.testing.assert_array_equal(mask.max(axis=(1, 3)) == 255, keep[by0:by0 + th, bx0:bx0 + tw])
            if (tw * th) & 7:                                               # the bits behind the last tile are zero
                assert bits[-1] >> ((tw * th) & 7) == 0
    # a row of bits that is never byte-aligned: byte i holds bits of two tile rows
    keep = np.zeros((33, 65), bool)
    keep[1, 64] = keep[2, 0] = True
    _, _, bits = M.mip_bits(keep, [0, 16, 1040, 48], 1040, 520)
    assert bits.tolist() == [0] * 8 + [3] + [0] * 8                             # bit 64 (row 0, x 64) and bit 65 (row 1, x 0) share byte 8


# ---- the entropy stage and framing ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tools():
    from oracle import pyoracle
    pyoracle.build()
    chunks.build_tool()
    subprocess.run(["make", "-C", HOST, "encode_frame_tool"], check=True, stdout=subprocess.DEVNULL)


def _rgba64():
    """64 x 64 RGBA: 8-bit analog alpha inside a box of kept tiles with a rejected tile in it"""
    from tests.images import synth_planes
    planes = np.concatenate([synth_planes(64, n_planes=3), np.zeros((1, 64, 64), np.int32)])
    y, x = np.mgrid[0:64, 0:64]
    planes[3, 18:62, 20:60] = ((x * 3 + y * 5) % 251 + 4)[18:62, 20:60]
    planes[3, 32:48, 32:48] = 0                                             # tile (2, 2): rejected, inside the box
    return planes


@pytest.fixture(scope="module")
def pieces(tools):
    """name -> (w, h, the oracle's pass outputs without the 'PLNT' blobs [+ the 'ALPM' pieces])"""
    from tests.images import edge_image, synth_planes
    images = {"synth64_rgb": synth_planes(64, n_planes=3), "ramp72x40_rgb": edge_image(72, 40, "ramp", 3), "twocolor64_rgb": edge_image(64, 64, "twocolor", 3),
              "box64_rgba": _rgba64()}
    out = {}
    for name, planes in images.items():
        st = {k: v for k, v in chunks.oracle_streams(planes).items() if not k.startswith("plnt_") and k != "bounds_post"}
        out[name] = (planes.shape[2], planes.shape[1], st)
    w, h, st = out["box64_rgba"]
    assert st["_mip_has_chunk"] == b"\x01" and np.frombuffer(st["_mip_tile_bbox"], np.int16).tolist() == [1, 1, 3, 3]
    assert np.frombuffer(st["_mip_bitmap"], np.uint8).tolist() == [0xEF, 0x01]                       # tile (1, 1) of the box is the rejected one
    from oracle.pyoracle import OracleEncoder
    enc = OracleEncoder(images["box64_rgba"]); enc.mip_prefilter()
    a = R.encode(images["box64_rgba"][3], enc.bounds(), None, True)
    assert a["mode"] == R.IS_8_BIT_FULL
    with_alpha = dict(st)
    with_alpha["alpha_mode"] = struct.pack("<i", a["mode"])
    with_alpha["alpha_bbox"] = np.array(a["bbox"], np.int32).tobytes()
    with_alpha["alpha_payload"] = a["payload"].tobytes()
    out["box64_rgba+alpm"] = (w, h, with_alpha)
    return out


def _encode(tmp_path, frames, level, threads=4, tag="e"):
    paths = []
    for i, st in enumerate(frames):
        p = str(tmp_path / f"{tag}{level}_{threads}_{i}.blobs")
        chunks.write_blobs(p, st)
        paths.append(p)
    prefix = str(tmp_path / f"{tag}{level}_{threads}_")
    r = subprocess.run([TOOL, "encode", str(level), str(threads), prefix] + paths, capture_output=True, text=True)
    if r.returncode:
        return r
    return [open(f"{prefix}{i}.yaik", "rb").read() for i in range(len(frames))]


def _parse(tmp_path, stream):
    p = tmp_path / "p.yaik"
    p.write_bytes(stream)
    subprocess.run([TOOL, "parse", str(p), str(tmp_path / "p.blobs")], check=True)
    return parse_blobs(str(tmp_path / "p.blobs"))


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


def test_level_0_is_the_chunk_writer_byte_for_byte(pieces, tmp_path):
    names = ["synth64_rgb", "ramp72x40_rgb", "twocolor64_rgb", "box64_rgba"]
    for name in names:
        w, h, st = pieces[name]
        (got,) = _encode(tmp_path, [st], 0)
        want = chunks.frame(st, with_file_header=True)
        assert got == want, name
        tags = [t for t, _, _ in _chunk_list(got)]
        assert tags == sorted(tags, key=[TAGS["MIPM"], TAGS["ALPM"], TAGS["GTIL"], TAGS["1DTL"]].index)
    assert [t for t, _, _ in _chunk_list(_encode(tmp_path, [pieces["box64_rgba"][2]], 0)[0])][0] == TAGS["MIPM"]
    assert TAGS["GTIL"] not in [t for t, _, _ in _chunk_list(_encode(tmp_path, [pieces["twocolor64_rgb"][2]], 0)[0])]


def test_alpm_chunk_sits_behind_mipm_and_the_rest_is_unchanged(pieces, tmp_path):
    w, h, st = pieces["box64_rgba+alpm"]
    (got,) = _encode(tmp_path, [st], 0)
    plain = chunks.frame(pieces["box64_rgba"][2], with_file_header=True)
    cl = _chunk_list(got)
    assert [t for t, _, _ in cl][:2] == [TAGS["MIPM"], TAGS["ALPM"]]
    _, at, size = cl[1]
    assert got[:at] + got[at + size:] == plain                              # the file without its 'ALPM' chunk is the file of emitAlpha = 0
    b = _parse(tmp_path, got)
    hdr = np.frombuffer(b["c1_hdr"], np.int32).tolist()
    a_bbox = np.frombuffer(st["alpha_bbox"], np.int32).tolist()
    assert hdr[:4] == a_bbox and hdr[4] == len(st["alpha_payload"]) and hdr[5] == 1 and hdr[6] == R.IS_8_BIT_FULL
    assert bytes(b["c1_alpha"]) == st["alpha_payload"]
    # the level-0 'ALPM' stream is writeAlpha's sweep: never larger than any single level of 5..21 taken alone up to the first growth
    z0 = struct.unpack_from("<I", got, at + 8 + 8)[0]
    z5 = struct.unpack_from("<I", _encode(tmp_path, [st], 5)[0], at + 8 + 8)[0]
    assert z0 <= z5


def test_level_3_keeps_order_headers_padding_and_payloads(pieces, tmp_path):
    for name in ("synth64_rgb", "ramp72x40_rgb", "box64_rgba+alpm"):
        st = pieces[name][2]
        (l0,), (l3,) = _encode(tmp_path, [st], 0), _encode(tmp_path, [st], 3)
        assert l0 != l3 and l0[:12] == l3[:12], name
        assert [t for t, _, _ in _chunk_list(l0)] == [t for t, _, _ in _chunk_list(l3)]
        b0, b3 = _parse(tmp_path, l0), _parse(tmp_path, l3)
        assert list(b0) == list(b3) and len(b0) > 4
        for k in b0:                                                        # how many padding bytes a chunk needs follows its compressed sizes
            assert k.endswith("_pad") or bytes(b0[k]) == bytes(b3[k]), (name, k)
        assert np.frombuffer(b0["chunk_count_terminated_rest"], np.int32).tolist()[1:] == [1, 0]
        for b in (b0, b3):                                                  # padding: up to a multiple of 4, at most 3 bytes, all zero
            for k in b:
                if k.endswith("_pad"):
                    n, ored = np.frombuffer(b[k], np.int32).tolist()
                    assert 0 <= n <= 3 and ored == 0


def test_bytes_do_not_depend_on_threads_or_on_the_batch(pieces, tmp_path):
    frames = [pieces[n][2] for n in ("synth64_rgb", "twocolor64_rgb", "synth64_rgb")]
    for level in (0, 3):
        alone = [_encode(tmp_path, [st], level, 1, "a")[0] for st in frames]
        for threads in (1, 2, 16):
            assert _encode(tmp_path, frames, level, threads, "b") == alone, (level, threads)
        assert alone[0] == alone[2]


def test_a_pass_with_colours_but_no_tile_fails_with_the_lowest_index(pieces, tmp_path):
    good = pieces["synth64_rgb"][2]
    bad = dict(good)
    bad["grad_bitmap_3"] = bytes(len(good["grad_bitmap_3"]))                # the tiles of pass 3 are gone, its colours are not
    assert len(good["grad_rgbraw_3"]) > 0
    r = _encode(tmp_path, [good, bad, bad], 3)
    assert r.returncode == 3 and "failed 1" in r.stderr and "a pass has colours but no tile" in r.stderr
    r = _encode(tmp_path, [good], 23)
    assert r.returncode == 2
