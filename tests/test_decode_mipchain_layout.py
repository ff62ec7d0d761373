"""CPU side of the mip chain outputs: the three yk_decode_*mip* entry points are declared in include/yaik_hip.h, listed in
yaik_amd/_lib.py with the same arity and exported; YAIK_DecodeImageMipchainToDevice likewise in yaik_decode_mipchain.h, files.MIPCHAIN_SIGNATURES
and libyaik_host.so; and the Python methods check first, count, the list `out` and every shape before any library call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yaik_amd", "host")
NEW_HIP = {"yk_decode_mip_levels": 2, "yk_decode_output_mipchain_device": 6, "yk_decode_output_mipchain_batch_device": 6}
NEW_HOST = {"YAIK_DecodeImageMipchainToDevice": 7}


def _arity(text, prefix):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    out = {}
    for name, args in re.findall(r"\b(%s[A-Za-z0-9_]+)\s*\(([^()]*)\)\s*;" % prefix, text):
        out[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return out


def test_hip_header_signature_table_and_library_agree():
    from yaik_amd import _lib
    header = open(os.path.join(ROOT, "include", "yaik_hip.h")).read()
    declared = _arity(header, "yk_")
    for name, arity in NEW_HIP.items():
        assert declared.get(name) == arity, (name, declared.get(name))
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == arity, name
    S = _lib.SIGNATURES
    assert S["yk_decode_output_mipchain_device"] == S["yk_decode_output_mipchain_batch_device"]
    assert S["yk_decode_output_mipchain_device"][1] == [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int]
    # the level table: the header's struct and the ctypes one, field for field
    m = re.search(r"typedef struct \{ uint8_t\* devOut; size_t rowBytes, planeBytes, frameBytes; \} yk_mip_level;", header)
    assert m and [f[0] for f in _lib.MipLevel._fields_] == ["devOut", "rowBytes", "planeBytes", "frameBytes"]
    assert C.sizeof(_lib.MipLevel) == C.sizeof(C.c_void_p) + 3 * C.sizeof(C.c_size_t)
    assert re.search(r"#define YK_MIP_MAX_LEVELS 15\b", header) and _lib.YK_MIP_MAX_LEVELS == 15
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)                                               # loading needs no device
    assert not [s for s in NEW_HIP if not hasattr(L, s)]


def test_host_header_ctypes_table_and_library_agree():
    from yaik_amd import files
    subprocess.run(["make", "-C", HOST, "libyaik_host.so"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(HOST, "yaik_decode_mipchain.h")).read()
    assert 'extern "C"' in text
    assert _arity(text, "YAIK_") == NEW_HOST
    assert list(files.MIPCHAIN_SIGNATURES) == list(NEW_HOST)
    res, args = files.MIPCHAIN_SIGNATURES["YAIK_DecodeImageMipchainToDevice"]
    assert res is C.c_bool and args == files.SIGNATURES["YAIK_DecodeImageToDevice"][1] + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    out = subprocess.run(["nm", "-D", "--defined-only", files.HOST_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert not set(NEW_HOST) - set(out.split())                             # C linkage: its own name
    L = files.host_lib()                                                    # loads without a device
    assert callable(L.YAIK_DecodeImageMipchainToDevice)
    L.YAIK_GetErrorCode()                                                   # drop what an earlier test may have left
    assert not L.YAIK_DecodeImageMipchainToDevice(None, 0, None, 0, 1, None, None)     # no context: refused before anything is touched
    assert files.ERROR_NAMES[L.YAIK_GetErrorCode()] == "YAIK_DECIMG_INVALIDCTX"


def _bare_decoder(w=136, h=264, frames=1):
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder.__new__(HipTileDecoder)                              # no handle, no library: the checks come first
    d._h = None
    d.w, d.h, d.frames, d._window, d._has_alpha, d.device = w, h, frames, None, False, 0
    return d


def test_mip_levels_counts_the_chain():
    for (w, h), n in (((8, 8), 4), ((136, 264), 8), ((520, 264), 9), ((16384, 8), 4), ((16384, 16384), 15)):
        assert _bare_decoder(w, h).mip_levels() == n


def test_the_level_range_is_checked_before_any_library_call():
    from yaik_amd import files
    d = _bare_decoder()                                                      # 8 levels
    for call in (d.image_mipchain_device, d.image_mipchain_batch_device):
        for first, count in ((1.0, None), (True, None), (None, None), ("0", 1), (0, 2.0), (0, False), (np.float32(1), 1)):
            with pytest.raises(TypeError, match="first|count"):
                call(first, count)
        for first, count in ((-1, None), (8, None), (0, 0), (0, 9), (0, 16), (5, 4), (7, 2), (np.int64(8), 1)):
            with pytest.raises(ValueError, match="first|count"):
                call(first, count)
    for first, count in ((1.0, None), (0, 2.0), (True, 1)):
        with pytest.raises(TypeError, match="first|count"):
            files.decode_file_mipchain_device(b"", first, count)
    for first, count in ((-1, None), (0, 0)):
        with pytest.raises(ValueError, match="first|count"):
            files.decode_file_mipchain_device(b"", first, count)
    with pytest.raises(ValueError, match="alpha_from_planes"):
        d.image_mipchain_batch_device(channels=3, alpha_from_planes=True)
    for bad in (2, 5):
        with pytest.raises(ValueError, match="channels"):
            d.image_mipchain_device(channels=bad)


def test_the_list_out_and_every_shape_are_checked_before_any_library_call():
    import torch
    w, h = 136, 264
    d = _bare_decoder(w, h, frames=2)
    e = lambda *s: torch.empty(s, dtype=torch.uint8)
    with pytest.raises(TypeError, match="list"):
        d.image_mipchain_device(4, 1, out=e(h >> 4, w >> 4, 3))              # a tensor where a list belongs
    with pytest.raises(TypeError, match=r"out\[1\]"):
        d.image_mipchain_device(4, 2, out=[e(h >> 4, w >> 4, 3), None])
    with pytest.raises(ValueError, match="2 tensors"):
        d.image_mipchain_device(4, 3, out=[e(h >> 4, w >> 4, 3), e(h >> 5, w >> 5, 3)])
    with pytest.raises(ValueError, match=r"level 5 needs \(8, 4, 3\)"):
        d.image_mipchain_device(4, 2, out=[e(h >> 4, w >> 4, 3), e(h >> 4, w >> 4, 3)])
    with pytest.raises(ValueError, match=r"level 0 needs \(4, 264, 136\)"):
        d.image_mipchain_device(0, 1, out=[e(h, w, 4)], channels=4, alpha=9, planar=True)
    with pytest.raises(ValueError, match=r"level 7 needs \(2, 2, 1, 3\)"):
        d.image_mipchain_batch_device(7, 1, out=[e(2, 1, 3)])
    with pytest.raises(ValueError, match=r"level 6 needs \(2, 4, 4, 2\)"):
        d.image_mipchain_batch_device(6, None, out=[e(2, 4, 2, 4), e(2, 2, 1, 4)], channels=4, planar=True)
