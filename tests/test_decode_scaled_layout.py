"""CPU side of the reduced-resolution outputs: the three yk_decode_*_scaled_* entry points are declared in include/yaik_hip.h, listed in
yaik_amd/_lib.py with the same arity and exported; YAIK_DecodeImageScaledToDevice likewise in yaik_decode_scaled.h, files.SCALED_SIGNATURES and
libyaik_host.so; and the Python methods check level, windows and the shape of `out` before any library call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yaik_amd", "host")
NEW_HIP = {"yk_decode_output_scaled_device": 7, "yk_decode_output_scaled_batch_device": 8, "yk_decode_render_windows_scaled_device": 12}
NEW_HOST = {"YAIK_DecodeImageScaledToDevice": 4}
BAD_LEVELS = (-1, 4, 1.0, True, None)


def _arity(text, prefix):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
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
        assert res is C.c_int and len(args) == arity and args[0] is C.c_void_p and args[1] is C.c_int, name
    # the level, then the arguments of the full-size call
    S = _lib.SIGNATURES
    assert S["yk_decode_output_scaled_device"][1][2:] == S["yk_decode_output_device"][1][1:]
    assert S["yk_decode_output_scaled_batch_device"][1][2:] == S["yk_decode_output_batch_device"][1][1:]
    assert S["yk_decode_render_windows_scaled_device"][1][2:] == S["yk_decode_render_windows_device"][1][1:]
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)                                               # loading needs no device
    assert not [s for s in NEW_HIP if not hasattr(L, s)]


def test_host_header_ctypes_table_and_library_agree():
    from yaik_amd import files
    subprocess.run(["make", "-C", HOST, "libyaik_host.so"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(HOST, "yaik_decode_scaled.h")).read()
    assert 'extern "C"' in text
    assert _arity(text, "YAIK_") == NEW_HOST
    assert list(files.SCALED_SIGNATURES) == list(NEW_HOST)
    res, args = files.SCALED_SIGNATURES["YAIK_DecodeImageScaledToDevice"]
    assert res is C.c_bool and args == files.SIGNATURES["YAIK_DecodeImageToDevice"][1] + [C.c_int]
    out = subprocess.run(["nm", "-D", "--defined-only", files.HOST_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert not set(NEW_HOST) - set(out.split())                             # C linkage: its own name
    L = files.host_lib()                                                    # loads without a device
    assert callable(L.YAIK_DecodeImageScaledToDevice)
    L.YAIK_GetErrorCode()                                                   # drop what an earlier test may have left
    for level in (1, 4):
        assert not L.YAIK_DecodeImageScaledToDevice(None, 0, None, level)   # no context: refused before anything is touched
        assert files.ERROR_NAMES[L.YAIK_GetErrorCode()] == "YAIK_DECIMG_INVALIDCTX"


def _bare_decoder(w=136, h=264, frames=1):
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder.__new__(HipTileDecoder)                              # no handle, no library: the checks come first
    d._h = None
    d.w, d.h, d.frames, d._window, d._has_alpha, d.device = w, h, frames, None, False, 0
    return d


def _raises_for(level):
    return pytest.raises(TypeError if isinstance(level, (bool, float)) or level is None else ValueError, match="level")


def test_levels_are_checked_before_any_library_call():
    from yaik_amd import files
    d = _bare_decoder()
    for level in BAD_LEVELS:
        with _raises_for(level):
            d.image_scaled_device(level)
        with _raises_for(level):
            d.image_scaled_batch_device(level)
        with _raises_for(level):
            d.render_windows_scaled(level, [(0, 0)], 8, 8)
        with _raises_for(level):
            files.decode_file_scaled_device(b"", level)
    for level in (np.int64(5), 2.0, "1"):
        with pytest.raises((TypeError, ValueError), match="level"):
            d.image_scaled_device(level)


def test_windows_are_checked_before_any_library_call():
    d = _bare_decoder()
    for bad in ((4, 0, 8, 8), (0, 4, 8, 8), (0, 0, 12, 8), (0, 0, 8, 12), (0, 0, 0, 8), (-8, 0, 8, 8), (136, 0, 8, 8), (0, 264, 8, 8), (8, 0, 136, 8),
                (0, 8, 8, 264), (0, 0, 144, 8), (0, 0, 8, 272)):
        for level in (0, 1, 3):
            with pytest.raises(ValueError, match="window"):
                d.render_windows_scaled(level, [(0, 0), bad[:2]], bad[2], bad[3])
    for bad in ((0.0, 0, 8, 8), (0, 0, 8, "8"), (True, 0, 8, 8), (0, 0, None, 8)):
        with pytest.raises(TypeError, match="window"):
            d.render_windows_scaled(1, [bad[:2]], bad[2], bad[3])
    with pytest.raises(ValueError, match="window"):
        d.render_windows_scaled(1, [], 8, 8)
    with pytest.raises(ValueError, match="window"):
        d.render_windows_scaled(1, [(0, 0)] * 1025, 8, 8)
    with pytest.raises(ValueError, match="alpha_from_planes"):
        d.image_scaled_batch_device(1, channels=3, alpha_from_planes=True)


def test_an_out_tensor_of_the_full_size_shape_is_refused_before_any_library_call():
    import torch
    w, h = 136, 264
    d = _bare_decoder(w, h, frames=2)
    for level in (1, 2, 3):
        rw, rh = w >> level, h >> level
        with pytest.raises(ValueError, match=rf"needs \({rh}, {rw}, 3\)"):
            d.image_scaled_device(level, out=torch.empty((h, w, 3), dtype=torch.uint8))
        with pytest.raises(ValueError, match=rf"needs \(4, {rh}, {rw}\)"):
            d.image_scaled_device(level, out=torch.empty((4, h, w), dtype=torch.uint8), channels=4, alpha=9, planar=True)
        with pytest.raises(ValueError, match=rf"needs \(2, {rh}, {rw}, 3\)"):
            d.image_scaled_batch_device(level, out=torch.empty((2, h, w, 3), dtype=torch.uint8))
        with pytest.raises(ValueError, match=rf"needs \(2, {16 >> level}, {24 >> level}, 3\)"):
            d.render_windows_scaled(level, [(0, 0), (56, 56)], 24, 16, out=torch.empty((2, 16, 24, 3), dtype=torch.uint8))
    d._window = (56, 56, 24, 16)                                             # under a window it is the window that is reduced
    with pytest.raises(ValueError, match=r"window needs \(8, 12, 3\)"):
        d.image_scaled_device(1, out=torch.empty((16, 24, 3), dtype=torch.uint8))
    with pytest.raises(ValueError, match=r"window needs \(8, 12, 3\)"):
        d.image_scaled_device(1, out=torch.empty((rh, rw, 3), dtype=torch.uint8))
