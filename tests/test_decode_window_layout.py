"""CPU side of the window decode: yk_decode_set_window and yk_decode_output_window_device are declared in include/yaik_hip.h, listed in
yaik_amd/_lib.py with the same arity and exported by the built library; YAIK_DecodeImageWindowToDevice likewise in yaik_decode_window.h,
files.WINDOW_SIGNATURES and libyaik_host.so; HipTileDecoder.set_window and files.decode_file_window_device check their arguments before any
library call."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yaik_amd", "host")
NEW_HIP = {"yk_decode_set_window": 5, "yk_decode_output_window_device": 6}


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
        assert res is C.c_int and len(args) == arity and args[0] is C.c_void_p, name
    assert _lib.SIGNATURES["yk_decode_output_window_device"] == _lib.SIGNATURES["yk_decode_output_device"]
    assert _lib.SIGNATURES["yk_decode_set_window"][1][1:] == [C.c_int] * 4
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)                                               # loading needs no device
    assert not [s for s in NEW_HIP if not hasattr(L, s)]
    # no test hook was added for the feature
    hooks = _arity(open(os.path.join(ROOT, "include", "yaik_hip_test.h")).read(), "yk_")
    assert not [n for n in hooks if "window" in n]


def test_host_header_ctypes_table_and_library_agree():
    from yaik_amd import files
    subprocess.run(["make", "-C", HOST, "libyaik_host.so"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(HOST, "yaik_decode_window.h")).read()
    assert 'extern "C"' in text
    assert _arity(text, "YAIK_") == {"YAIK_DecodeImageWindowToDevice": 7}
    assert list(files.WINDOW_SIGNATURES) == ["YAIK_DecodeImageWindowToDevice"]
    res, args = files.WINDOW_SIGNATURES["YAIK_DecodeImageWindowToDevice"]
    assert res is C.c_bool and len(args) == 7
    assert args[:3] == files.SIGNATURES["YAIK_DecodeImageToDevice"][1] and args[3:] == [C.c_int] * 4
    out = subprocess.run(["nm", "-D", "--defined-only", files.HOST_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "YAIK_DecodeImageWindowToDevice" in set(out.split())             # C linkage: its own name
    L = files.host_lib()                                                    # loads without a device
    assert callable(L.YAIK_DecodeImageWindowToDevice)
    L.YAIK_GetErrorCode()                                                   # drop what an earlier test may have left
    # no context: refused like YAIK_DecodeImageToDevice, before anything is touched
    assert not L.YAIK_DecodeImageWindowToDevice(None, 0, None, 0, 0, 8, 8)
    assert files.ERROR_NAMES[L.YAIK_GetErrorCode()] == "YAIK_DECIMG_INVALIDCTX"


def test_set_window_arguments_are_checked_before_any_library_call():
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder.__new__(HipTileDecoder)                              # no handle, no library: the checks come first
    d._h = None
    d.w, d.h, d.frames, d._window = 136, 264, 1, None
    for bad in ((4, 0, 8, 8), (0, 4, 8, 8), (0, 0, 12, 8), (0, 0, 8, 12), (0, 0, 0, 8), (0, 0, 8, 0), (-8, 0, 8, 8), (0, -8, 16, 16), (0, 0, -8, -8),
                (136, 0, 8, 8), (0, 264, 8, 8), (8, 0, 136, 8), (0, 8, 8, 264), (0, 0, 144, 8), (0, 0, 8, 272)):
        with pytest.raises(ValueError, match="window"):
            d.set_window(*bad)
    for bad in ((0.0, 0, 8, 8), (0, 0, 8, "8"), (True, 0, 8, 8), (0, 0, None, 8)):
        with pytest.raises(TypeError, match="window"):
            d.set_window(*bad)
    assert d.window is None


def test_decode_file_window_device_checks_the_window_first():
    from yaik_amd import files
    for bad in ((0, 0, 8), (0, 0, 12, 8), (4, 0, 8, 8), (0, 0, 0, 0), (-8, 0, 8, 8), "0088", None):
        with pytest.raises((ValueError, TypeError), match="window"):
            files.decode_file_window_device(b"", bad)
