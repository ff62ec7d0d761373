"""CPU side of the round-trip quality calls: the three entry points are declared in include/yaik_hip.h, listed in yaik_amd/_lib.py with the same
arity and exported by the built library; yk_quality has the size and field order yaik_amd.quality.YkQuality binds; psnr_db on hand values; the
numpy restatement (tests/quality_ref.py) on a 16 x 8 case worked out by hand."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import quality_ref as Q
from yaik_amd.quality import YkQuality, psnr_db, quality_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"yk_decode_compare_device": 8, "yk_decode_compare_batch_device": 9, "yk_decode_compare_planes_device": 7}


def _header():
    hdr = open(os.path.join(ROOT, "include", "yaik_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def test_header_and_signature_table_agree_on_the_new_entry_points():
    from yaik_amd import _lib
    declared = {}
    for name, args in re.findall(r"\bint\s+(yk_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", _header()):
        declared[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    for name, arity in NEW.items():
        assert declared.get(name) == arity, (name, declared.get(name))
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == arity, (name, len(args))
        assert args[0] is C.c_void_p                                       # the handle
    assert re.search(r"YK_STAGE_DEC_COMPARE\s*=\s*8\b", _header())


def test_struct_matches_the_header():
    m = re.search(r"typedef\s+struct\s+yk_quality\s*\{(.*?)\}\s*yk_quality\s*;", _header(), flags=re.S)
    assert m, "yk_quality is not declared"
    fields = [(t, n, int(k)) for t, names in re.findall(r"(uint64_t|uint32_t)\s+([^;]+);", m.group(1))
              for n, k in re.findall(r"(\w+)(?:\[(\d+)\])?", names.replace(" ", "")) for k in [k or "1"]]
    assert fields == [("uint64_t", "sse", 4), ("uint64_t", "sad", 4), ("uint64_t", "nDiff", 4), ("uint32_t", "maxAbs", 4), ("uint64_t", "nSamples", 1)]
    ctype = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
    bound = [(n, t._type_, t._length_) if hasattr(t, "_length_") else (n, t, 1) for n, t in YkQuality._fields_]
    assert bound == [(n, ctype[t], k) for t, n, k in fields]
    assert C.sizeof(YkQuality) == 3 * 4 * 8 + 4 * 4 + 8 == 120
    assert YkQuality.maxAbs.offset == 96 and YkQuality.nSamples.offset == 112


def test_library_exports_the_new_entry_points():
    from yaik_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)                                               # loading needs no device
    assert not [s for s in NEW if not hasattr(L, s)]


def test_psnr_on_hand_values():
    assert psnr_db(0, 64) == math.inf
    assert psnr_db(65025, 1) == 0.0                                         # every sample off by 255
    assert psnr_db(65025 * 7, 7) == 0.0
    assert psnr_db(64, 64) == pytest.approx(20 * math.log10(255), abs=1e-12)     # mse 1: 48.1308 dB
    assert psnr_db(1, 100) == pytest.approx(10 * math.log10(6502500.0), abs=1e-12)
    big = psnr_db(255 * 255 << 30, 1 << 40)                                  # sums beyond 2^32 stay exact integers until the one division
    assert big == pytest.approx(10 * math.log10(1024.0), abs=1e-12)
    assert isinstance(psnr_db(np.uint64(5), np.int64(10)), float)
    for bad in [(-1, 4), (1, 0)]:
        with pytest.raises(ValueError):
            psnr_db(*bad)


def test_struct_to_dict():
    q = YkQuality()
    q.sse[:] = [64, 0, 65025 * 128, 9]
    q.sad[:] = [64, 0, 255 * 128, 3]
    q.nDiff[:] = [64, 0, 128, 1]
    q.maxAbs[:] = [1, 0, 255, 3]
    q.nSamples = 128
    d = quality_dict(q, 3)
    assert d["sse"] == [64, 0, 65025 * 128] and d["sad"] == [64, 0, 255 * 128] and d["n_diff"] == [64, 0, 128] and d["max_abs"] == [1, 0, 255]
    assert d["n_samples"] == 128 and d["channels"] == 3 and all(type(v) is int for k in ("sse", "sad", "n_diff", "max_abs") for v in d[k])
    assert d["psnr_db"][0] == psnr_db(64, 128) and d["psnr_db"][1] == math.inf and d["psnr_db"][2] == 0.0
    assert d["psnr_db_all"] == psnr_db(64 + 65025 * 128, 3 * 128)
    d4 = quality_dict(q, 4)
    assert d4["sse"][3] == 9 and d4["psnr_db_all"] == psnr_db(64 + 65025 * 128 + 9, 4 * 128)
    with pytest.raises(ValueError):
        quality_dict(q, 2)


def test_restatement_on_a_hand_made_case():
    """16 x 8 pixels = two tiles.  Left tile: R differs by 1 everywhere, one G sample by -3.  Right tile: B is 0 against 255 in one row, alpha equal."""
    dec = np.full((8, 16, 4), 100, np.uint8)
    src = dec.copy()
    src[:, :8, 0] = 101
    src[2, 5, 1] = 103
    dec[7, 8:, 2], src[7, 8:, 2] = 0, 255
    r = Q.compare(dec, src)
    assert r["n_samples"] == 128
    assert r["sse"] == [64, 9, 8 * 65025, 0] and r["sad"] == [64, 3, 8 * 255, 0]
    assert r["n_diff"] == [64, 1, 8, 0] and r["max_abs"] == [1, 3, 255, 0]
    assert r["tile_sse"].shape == (1, 2) and r["tile_sse"].tolist() == [[64 + 9, 8 * 65025]]
    r3 = Q.compare(dec[:, :, :3].astype(np.int32), src[:, :, :3])                # the sign of the difference does not matter, nor does the dtype
    assert r3["sse"] == r["sse"][:3] and r3["tile_sse"].tolist() == r["tile_sse"].tolist()
    assert Q.compare(src, dec)["sad"] == r["sad"]
    with pytest.raises(ValueError):
        Q.compare(dec, src[:, :8])
