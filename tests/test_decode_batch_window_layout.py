"""CPU side of the batch-window decode: yk_decode_set_batch_windows and yk_decode_output_batch_windows_device are declared in
include/yaik_hip.h, listed in yaik_amd/_lib.py with the same arity and exported by the built library; YAIK_DecodeImagesWindowsToDevice likewise
in yaik_decode_batch_windows.h, files.BATCH_WINDOWS_SIGNATURES and libyaik_host.so; HipTileDecoder.set_batch_windows,
image_batch_windows_device and files.decode_files_windows_device check their arguments before any library call."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yaik_amd", "host")
NEW_HIP = {"yk_decode_set_batch_windows": 4, "yk_decode_output_batch_windows_device": 7}


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
    assert _lib.SIGNATURES["yk_decode_output_batch_windows_device"] == _lib.SIGNATURES["yk_decode_output_batch_device"]
    assert _lib.SIGNATURES["yk_decode_set_batch_windows"][1][2:] == [C.c_int] * 2
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
    text = open(os.path.join(HOST, "yaik_decode_batch_windows.h")).read()
    assert 'extern "C"' in text
    assert _arity(text, "YAIK_") == {"YAIK_DecodeImagesWindowsToDevice": 14}
    assert list(files.BATCH_WINDOWS_SIGNATURES) == ["YAIK_DecodeImagesWindowsToDevice"]
    res, args = files.BATCH_WINDOWS_SIGNATURES["YAIK_DecodeImagesWindowsToDevice"]
    assert res is C.c_bool and len(args) == 14
    assert args[:11] == files.SIGNATURES["YAIK_DecodeImagesToDevice"][1] and args[11:] == [C.c_void_p, C.c_int, C.c_int]
    out = subprocess.run(["nm", "-D", "--defined-only", files.HOST_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "YAIK_DecodeImagesWindowsToDevice" in set(out.split())           # C linkage: its own name
    L = files.host_lib()                                                    # loads without a device
    L.YAIK_GetErrorCode()                                                   # drop what an earlier test may have left
    # no library context, and no origin table: refused before anything is touched
    failed = C.c_int32(7)
    assert not L.YAIK_DecodeImagesWindowsToDevice(None, None, None, 1, None, 0, 0, 0, 3, 1, C.byref(failed), (C.c_int * 2)(0, 0), 8, 8)
    assert files.ERROR_NAMES[L.YAIK_GetErrorCode()] == "YAIK_INVALID_LIBRARYCTX" and failed.value == -1
    assert not L.YAIK_DecodeImagesWindowsToDevice(None, None, None, 1, None, 0, 0, 0, 3, 1, None, None, 8, 8)
    assert files.ERROR_NAMES[L.YAIK_GetErrorCode()] == "YAIK_DECIMG_INVALIDCTX"


def _decoder(frames=3):
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder.__new__(HipTileDecoder)                              # no handle, no library: the checks come first
    d._h = None
    d.device = 0
    d.w, d.h, d.frames, d._window, d._batch_windows = 136, 264, frames, None, None
    return d


def test_set_batch_windows_arguments_are_checked_before_any_library_call():
    d = _decoder()
    good = [(56, 56), (56, 120), (56, 184)]
    for origins, w, h in ((good[:2], 32, 32), (good + [(0, 0)], 32, 32), ([], 32, 32), ([(4, 0)] + good[1:], 32, 32), ([(0, 4)] + good[1:], 32, 32),
                          ([(-8, 0)] + good[1:], 32, 32), (good, 12, 32), (good, 32, 12), (good, 0, 32), (good, 32, 0), (good, -8, -8),
                          ([(112, 0)] + good[1:], 32, 32), (good[:2] + [(0, 240)], 32, 32), (good, 144, 8), (good, 8, 272)):
        with pytest.raises(ValueError):
            d.set_batch_windows(origins, w, h)
    for origins, w, h in (([(0.0, 0)] + good[1:], 32, 32), (good, 32.0, 32), (good, True, 32), ("abc", 32, 32), (None, 32, 32), ([(0, 0, 0)] + good[1:], 32, 32),
                          (np.zeros((3, 3), np.int64), 32, 32), (np.zeros((3, 2), np.float32), 32, 32), (np.zeros(6, np.int64), 32, 32)):
        with pytest.raises(TypeError):
            d.set_batch_windows(origins, w, h)
    assert d.batch_windows is None


def test_image_batch_windows_device_needs_windows_and_checks_its_arguments_first():
    d = _decoder()
    with pytest.raises(ValueError, match="set_batch_windows"):
        d.image_batch_windows_device()
    d._batch_windows = (np.array([[56, 56], [56, 120], [56, 184]], np.int32), 32, 32)
    got = d.batch_windows
    got[0][0, 0] = 0                                                        # a copy: the caller cannot move the windows by writing into it
    assert d.batch_windows[0][0, 0] == 56 and d.batch_windows[1:] == (32, 32)
    for kw in ({"channels": 5}, {"channels": 3, "alpha_from_planes": True}, {"channels": 4, "alpha": 256}, {"channels": 4, "alpha": -1}):
        with pytest.raises(ValueError):
            d.image_batch_windows_device(**kw)


def test_decode_files_windows_device_checks_origins_and_size_first():
    from yaik_amd import files
    files.host_lib()                                                        # loads without a device; no call below reaches a decode
    streams = [b"", b"", b""]
    good = [(56, 56), (56, 120), (56, 184)]
    for origins, size, exc in ((good[:2], (32, 32), ValueError), ([(4, 0)] + good[1:], (32, 32), ValueError), (good, (12, 32), ValueError), (good, (32, 0), ValueError),
                               (good, (32,), TypeError), (good, 32, TypeError), ([(0.5, 0)] + good[1:], (32, 32), TypeError), ("abcdef", (32, 32), TypeError)):
        with pytest.raises(exc):
            files.decode_files_windows_device(streams, origins, size)
    with pytest.raises(ValueError):
        files.decode_files_windows_device([], [], (32, 32))
    with pytest.raises(ValueError):
        files.decode_files_windows_device(streams, good, (32, 32), channels=5)
