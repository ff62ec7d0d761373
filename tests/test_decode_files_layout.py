"""CPU side of the file-level batch decode (YAIK_DecodeImagesToDevice, yaik_amd/files.py) and of the mask modes of the batch 'ALPM' call:
declarations, ctypes tables and exported symbols agree; pack_alpha_batch with five-tuple entries; the HIP-free plan (batch_plan_tool) on files
made on the CPU; the tile-bitmap form of the mask bit against the decoder's swizzled mask."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import alpha_ref as R
from tests import chunks
from yaik_amd.decoder import pack_alpha_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yaik_amd", "host")
PLAN_TOOL = os.path.join(HOST, "batch_plan_tool")
NEW_HIP = {"yk_decode_alpha_mask_batch_device": 9, "yk_decode_alpha_batch_status": 2, "yk_device_upload": 4}
TAG_GTIL, TAG_END = 0x4C495447, 0xDEADBEEF


def _arity(header_text, prefix):
    text = re.sub(r"/\*.*?\*/", "", header_text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for name, args in re.findall(r"\b(%s[A-Za-z0-9_]+)\s*\(([^()]*)\)\s*;" % prefix, text):
        out[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return out


def test_hip_header_signature_table_and_library_agree():
    from yaik_amd import _lib
    declared = _arity(open(os.path.join(ROOT, "include", "yaik_hip.h")).read(), "yk_")
    for name, arity in NEW_HIP.items():
        assert declared.get(name) == arity, (name, declared.get(name))
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == arity and args[0] is C.c_void_p, name
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)                                               # loading needs no device
    assert not [s for s in NEW_HIP if not hasattr(L, s)]


def test_host_header_ctypes_table_and_library_agree():
    from yaik_amd import files
    declared = _arity(open(os.path.join(HOST, "yaik_decode.h")).read(), "YAIK_")
    for name, (res, args) in files.SIGNATURES.items():
        assert declared.get(name) == len(args), (name, declared.get(name), len(args))
    assert declared["YAIK_DecodeImagesToDevice"] == 11
    out = subprocess.run(["nm", "-D", "--defined-only", files.HOST_LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = set(out.split())
    for name in files.SIGNATURES:                                           # C++ linkage: the binding names the mangled symbols
        assert files.SYMBOLS[name] in exported and files.SYMBOLS[name].startswith("_Z%d%s" % (len(name), name)), name
    L = files.host_lib()                                                    # loads without a device, every entry bound
    assert all(callable(getattr(L, name)) for name in files.SIGNATURES)
    assert L.YAIK_LastBatchFallbacks() == 0
    assert C.sizeof(files.DecodedImage) == 72 and files.DecodedImage.outputImage.offset == 48 and files.DecodedImage.internalTag.offset == 64
    assert files.ERROR_NAMES.index("YAIK_INVALID_HEADER") == 7 and files.ERROR_NAMES.index("YAIK_INVALID_TAG_ID") == 20


def test_pack_five_tuples_at_aligned_offsets_and_three_tuples_as_before():
    rng = np.random.default_rng(5)
    pays = [rng.integers(0, 256, n, dtype=np.uint8) for n in (33, 0, 100, 7)]
    bits = [rng.integers(0, 256, n, dtype=np.uint8) for n in (1, 3)]
    ent = [(3, (4, 0, 40, 30), pays[0], bits[0], (1, 0, 3, 2)), None, (6, (0, 0, 10, 10), pays[2]), (2, (0, 16, 64, 8), pays[3], bits[1], (0, 1, 4, 5))]
    pk = pack_alpha_batch(ent)
    assert pk.modes.tolist() == [3, -1, 6, 2] and pk.nbytes.tolist() == [33, 0, 100, 7]
    assert pk.mip_boxes.dtype == np.int32 and pk.mip_boxes.tolist() == [[1, 0, 3, 2], [0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 4, 5]]
    assert pk.mip_nbytes.tolist() == [1, 0, 0, 3] and pk.mip_where[1] is None and pk.mip_where[2] is None
    spans = []
    for f, p in ((0, pays[0]), (2, pays[2]), (3, pays[3])):
        kind, off = pk.where[f]
        assert kind == "h" and off % 16 == 0
        np.testing.assert_array_equal(pk.staging[off:off + p.size], p)
        spans.append((off, p.size))
    for f, b in ((0, bits[0]), (3, bits[1])):
        off = pk.mip_where[f]
        assert off % 16 == 0
        np.testing.assert_array_equal(pk.staging[off:off + b.size], b)
        spans.append((off, b.size))
    spans.sort()
    assert all(a + n <= b for (a, n), (b, _) in zip(spans, spans[1:]))      # no overlap
    # three-tuple input: the pack of before, and no mask tables
    plain = [(6, (f, 2 * f, 8, 4), p) for f, p in enumerate(pays)]
    pk3 = pack_alpha_batch(plain)
    assert pk3.mip_where is None and pk3.mip_nbytes is None and pk3.mip_boxes is None
    assert [w for w in pk3.where] == [("h", 0), ("h", 48), ("h", 48), ("h", 160)] and pk3.staging.size == 176
    with pytest.raises(ValueError):
        pack_alpha_batch([(3, (0, 0, 4, 4), pays[0], bits[0], (0, 0, 1))])   # a tile box of three numbers
    with pytest.raises(ValueError):
        pack_alpha_batch([(3, (0, 0, 4, 4), 4096, bits[0], (0, 0, 1, 1))])   # a mask entry takes a host payload


def test_mask_bit_from_the_tile_bitmap_equals_the_swizzled_mask():
    """the batch kernels never expand the mask: bit `pos` of yk_dec_mask_kernel's output is the tile bit of u64 word q = pos >> 6"""
    rng = np.random.default_rng(6)
    for _ in range(60):
        bw, bh = int(rng.integers(1, 14)), int(rng.integers(1, 14))
        bits = np.packbits(rng.integers(0, 2, bw * bh).astype(np.uint8), bitorder="little")
        mask = R.swizzled_mask(bits, bw, bh)
        pos = np.arange(mask.size * 8 + 300)                                # past the end: those bits read 0
        q = pos >> 6
        valid = q < 4 * bw * bh
        ty, tx = q // (4 * bw), ((q % (4 * bw)) % (2 * bw)) >> 1
        i = np.where(valid, ty * bw + tx, 0)
        got = np.where(valid, (bits[i >> 3] >> (i & 7)) & 1, 0)
        want = np.zeros(pos.size, np.uint8)
        want[:mask.size * 8] = np.unpackbits(mask, bitorder="little")
        np.testing.assert_array_equal(got, want, err_msg=f"{bw} x {bh}")


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cpu_files():
    """name -> (stream, passes with corners): files framed on the CPU from the oracle's pass outputs.  The 'PLNT' blobs stay out: that chunk has
    no reader, the decoder's chunk loop takes it for an unknown tag (checked below)."""
    from oracle import pyoracle
    from tests.images import edge_image, synth_planes
    pyoracle.build()
    chunks.build_tool()
    subprocess.run(["make", "-C", HOST, "batch_plan_tool"], check=True, stdout=subprocess.DEVNULL)
    images = {"synth64_rgb": synth_planes(64, n_planes=3), "twocolor64_rgb": edge_image(64, 64, "twocolor", 3), "ramp72x40_rgb": edge_image(72, 40, "ramp", 3)}
    out = {}
    for name, planes in images.items():
        st = chunks.oracle_streams(planes)
        passes = [i for i in range(7) if len(st[f"grad_rgbraw_{i}"])]
        out[name] = (chunks.frame({k: v for k, v in st.items() if not k.startswith("plnt_")}, with_file_header=True), passes)
        out[name + "+plnt"] = (chunks.frame(st, with_file_header=True), passes)
    return out


def _plan(tmp_path, streams):
    paths = []
    for i, s in enumerate(streams):
        p = tmp_path / f"{i}.yaik"
        p.write_bytes(s)
        paths.append(str(p))
    lines = subprocess.run([PLAN_TOOL] + paths, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(lines) == len(streams)
    return [ln.split(" ", 4) for ln in lines]


def _chunk_list(stream):
    out, p = [], 12
    while True:
        tag, length = struct.unpack_from("<II", stream, p) if p + 8 <= len(stream) else (struct.unpack_from("<I", stream, p)[0], 0)
        if tag == TAG_END:
            return out, p
        out.append((p, tag, length))
        p += 8 + length


def test_plan_of_cpu_made_files(cpu_files, tmp_path):
    for name in ("synth64_rgb", "twocolor64_rgb", "ramp72x40_rgb"):
        stream, passes = cpu_files[name]
        (row,) = _plan(tmp_path, [stream])
        w, h = (72, 40) if name.startswith("ramp") else (64, 64)
        assert row[:4] == ["0", "batchable", str(w), str(h)], (name, row)
        fields = dict(kv.split("=") for kv in row[4].split())
        assert fields["passes"] == (",".join(map(str, passes)) or "-"), (name, fields, passes)
        assert fields["mip"] == "0" and fields["alpha"] == "-1"
        has_1d = any(tag == 0x4C544431 for _, tag, _ in _chunk_list(stream)[0])
        assert fields["d1"] == str(int(has_1d and bool(passes)))           # a '1DTL' in front of every 'GTIL' is ignored, as the single decoder does
    assert cpu_files["synth64_rgb"][1] == list(range(7)) and cpu_files["twocolor64_rgb"][1] == [] and 0 < len(cpu_files["ramp72x40_rgb"][1]) < 7


def test_plan_sends_broken_streams_to_the_fallback(cpu_files, tmp_path):
    good = cpu_files["synth64_rgb"][0]
    cl, end = _chunk_list(good)
    gt = [c for c in cl if c[1] == TAG_GTIL]
    assert len(gt) == 7
    (a, _, la), (b, _, lb) = gt[0], gt[1]
    swapped = good[:a] + good[b:b + 8 + lb] + good[a:a + 8 + la] + good[b + 8 + lb:]
    assert len(swapped) == len(good) and b == a + 8 + la
    plane3 = bytearray(good)
    assert plane3[gt[2][0] + 8 + 27] == 7                                   # HeaderGradientTile::plane
    plane3[gt[2][0] + 8 + 27] = 3
    truncated = good[:gt[4][0] + 20]
    unknown = bytearray(good)
    unknown[gt[6][0]:gt[6][0] + 4] = b"XXXX"
    no_end = good[:end]
    rows = _plan(tmp_path, [good, swapped, bytes(plane3), truncated, bytes(unknown), no_end, cpu_files["synth64_rgb+plnt"][0], cpu_files["ramp72x40_rgb"][0],
                            b"YAIK" + good[4:11]])
    assert rows[0][1] == "batchable"
    for i, why in ((1, "out of order"), (2, "plane-subset"), (3, "truncated"), (4, "unknown tag"), (5, "terminator"), (6, "unknown tag")):
        assert rows[i][1] == "fallback" and why in " ".join(rows[i][4:]), (i, rows[i])
    assert rows[7][:4] == ["7", "mismatch", "72", "40"]                     # a second header size
    assert rows[8][1] == "badheader"
