"""CPU side of the pixel-window decode: yk_decode_set_window_px, yk_decode_render_windows_px_device and yk_decode_set_batch_windows_px
are declared in include/yaik_hip.h, listed in yaik_amd/_lib.py with the same arity and exported by the built library; the three host calls
likewise in yaik_decode_window_px.h, files.WINDOW_PX_SIGNATURES and libyaik_host.so; the cover and clip arithmetic of yaik_amd/csrc/yk_window_px.h
holds for every window of small images (window_px_tool, the functions the kernels run); and the Python methods check px windows before any
library call while px=False keeps today's checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import window_px_cases as PX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yaik_amd", "host")
TOOL = os.path.join(HOST, "window_px_tool")
NEW_HIP = {"yk_decode_set_window_px": 5, "yk_decode_render_windows_px_device": 11, "yk_decode_set_batch_windows_px": 4}
NEW_HOST = {"YAIK_DecodeImageWindowPxToDevice": 7, "YAIK_DecodeImageWindowsPxToDevice": 8, "YAIK_DecodeImagesWindowsPxToDevice": 14}


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
    # the arguments of the aligned namesakes
    assert _lib.SIGNATURES["yk_decode_set_window_px"] == _lib.SIGNATURES["yk_decode_set_window"]
    assert _lib.SIGNATURES["yk_decode_render_windows_px_device"] == _lib.SIGNATURES["yk_decode_render_windows_device"]
    assert _lib.SIGNATURES["yk_decode_set_batch_windows_px"] == _lib.SIGNATURES["yk_decode_set_batch_windows"]
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)                                               # loading needs no device
    assert not [s for s in NEW_HIP if not hasattr(L, s)]
    hooks = _arity(open(os.path.join(ROOT, "include", "yaik_hip_test.h")).read(), "yk_")
    assert not [n for n in hooks if "_px" in n]                             # no test hook was added for the feature


def test_host_header_ctypes_table_and_library_agree():
    from yaik_amd import files
    subprocess.run(["make", "-C", HOST, "libyaik_host.so"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(HOST, "yaik_decode_window_px.h")).read()
    assert 'extern "C"' in text
    assert _arity(text, "YAIK_") == NEW_HOST
    assert list(files.WINDOW_PX_SIGNATURES) == list(NEW_HOST)
    for name, arity in NEW_HOST.items():
        res, args = files.WINDOW_PX_SIGNATURES[name]
        assert res is C.c_bool and len(args) == arity, name
    out = set(subprocess.run(["nm", "-D", "--defined-only", files.HOST_LIB_PATH], check=True, capture_output=True, text=True).stdout.split())
    assert not [n for n in NEW_HOST if n not in out]                        # C linkage: their own names
    L = files.host_lib()                                                    # loads without a device
    L.YAIK_GetErrorCode()
    # no library context, and no origin table: refused before anything is touched
    failed = C.c_int32(7)
    assert not L.YAIK_DecodeImagesWindowsPxToDevice(None, None, None, 1, None, 0, 0, 0, 3, 1, C.byref(failed), (C.c_int * 2)(3, 5), 13, 11)
    assert files.ERROR_NAMES[L.YAIK_GetErrorCode()] == "YAIK_INVALID_LIBRARYCTX" and failed.value == -1
    assert not L.YAIK_DecodeImagesWindowsPxToDevice(None, None, None, 1, None, 0, 0, 0, 3, 1, None, None, 13, 11)
    assert files.ERROR_NAMES[L.YAIK_GetErrorCode()] == "YAIK_DECIMG_INVALIDCTX"
    info = files.DecodedImage()                                             # no decode slot behind it
    assert not L.YAIK_DecodeImageWindowPxToDevice(None, 0, C.byref(info), 3, 5, 13, 11)
    assert files.ERROR_NAMES[L.YAIK_GetErrorCode()] == "YAIK_DECIMG_INVALIDCTX"
    assert not L.YAIK_DecodeImageWindowsPxToDevice(None, 0, C.byref(info), 1, (C.c_int * 2)(3, 5), 13, 11, 0)
    assert files.ERROR_NAMES[L.YAIK_GetErrorCode()] == "YAIK_DECIMG_INVALIDCTX"


# ---- the arithmetic the kernels run, exhaustively on the CPU ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-C", HOST, "window_px_tool"], check=True, stdout=subprocess.DEVNULL)
    return TOOL


def _run(tool, *args):
    p = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True)
    return p.returncode, p.stdout.strip()


@pytest.mark.parametrize("w", [8, 16, 24, 72, 136])
def test_cover_and_clip_hold_for_every_window(tool, w):
    """the tool checks, for every valid (x0, ww): the single cover is minimal, 8-aligned, inside the image and contains the window; the shared
    cover's size depends on (w, ww) only, it contains the window and lies inside the image; over the tile columns of either cover the clip's
    destination columns are [0, ww), each once, from source columns inside the cover; and that the rule refuses every window just outside it"""
    rc, out = _run(tool, "check", w)
    assert rc == 0 and out == f"ok {w * (w + 1) // 2}", out                 # that many windows [x0, x0 + ww) lie inside [0, w)


@pytest.mark.parametrize("w", [8, 24, 72])
def test_tool_output_equals_an_independent_computation(tool, w):
    """... and what it prints for a window equals the same quantities worked out here, so a tool that checked nothing would show"""
    for ww in range(1, w + 1):
        for x0 in sorted({0, 1, 7, 8, 9, (w - ww) // 2, w - ww - 1, w - ww} & set(range(w - ww + 1))):
            rc, out = _run(tool, "show", w, x0, ww)
            assert rc == 0, (w, x0, ww)
            head, _, cols = out.partition(" :")
            cx, _, cw, _ = PX.cover((x0, 0, ww, 1))
            sx, _, sw, _ = PX.shared_cover((x0, 0, ww, 1), w, 8)
            assert [int(v) for v in head.split()] == [cx, cw, sx, sw], (w, x0, ww)
            got = [tuple(int(v) for v in c.split(",")) for c in cols.split()]
            assert [g[0] for g in got] == list(range(sw // 8))
            dst = []
            for j, src0, n, d in got:
                keep = [c for c in range(8) if x0 <= sx + 8 * j + c < x0 + ww]       # the columns of the segment inside the window
                assert n == len(keep), (w, x0, ww, j)
                if n:
                    assert src0 == keep[0] and d == sx + 8 * j + src0 - x0, (w, x0, ww, j)
                    dst += list(range(d, d + n))
            assert dst == list(range(ww)), (w, x0, ww)


def test_windows_outside_the_rule_are_refused(tool):
    for w, x0, ww in ((136, 0, 0), (136, 0, 137), (136, 1, 136), (136, 136, 1), (136, -1, 8), (136, 130, 7), (136, 0, -8), (136, 2 ** 31 - 1, 2), (8, 8, 1)):
        assert _run(tool, "show", w, x0, ww) == (3, "bad"), (w, x0, ww)
    assert _run(tool, "show", 136, 135, 1)[0] == 0 and _run(tool, "show", 136, 0, 136)[0] == 0
    assert _run(tool, "check", 12)[0] == 2 and _run(tool, "show", 136, 0)[0] == 2


# ---- the Python methods check px windows before any library call ---------------------------------------------------------------------------
def _decoder(frames=3):
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder.__new__(HipTileDecoder)                              # no handle, no library: the checks come first
    d._h = None
    d.device = 0
    d.w, d.h, d.frames, d._window, d._batch_windows = 136, 264, frames, None, None
    return d


def test_px_windows_are_checked_before_any_library_call():
    d = _decoder()
    for bad in ((-1, 0, 8, 8), (0, -1, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0), (130, 0, 7, 8), (0, 260, 8, 5), (0, 0, 137, 8), (0, 0, 8, 265), (136, 0, 1, 1), (0, 0, -3, -3)):
        with pytest.raises(ValueError):
            d.set_window(*bad, px=True)
        with pytest.raises(ValueError):
            d.render_windows([bad[:2]], bad[2], bad[3], px=True)
        with pytest.raises(ValueError):
            d.render_window(*bad, px=True)
        with pytest.raises(ValueError):
            d.set_batch_windows([bad[:2]] * 3, bad[2], bad[3], px=True)
    for bad in ((0.0, 0, 8, 8), (0, 0, 8.0, 8), (True, 0, 8, 8)):
        with pytest.raises(TypeError):
            d.set_window(*bad, px=True)
        with pytest.raises(TypeError):
            d.render_windows([bad[:2]], bad[2], bad[3], px=True)
    with pytest.raises(ValueError):
        d.set_batch_windows([(3, 5)] * 2, 13, 11, px=True)                  # two origins for three frames
    assert d.window is None and d.window_cover is None and d.batch_windows is None and d.batch_window_covers is None
    # the default keeps today's checks: an unaligned rectangle is refused before any library call
    for call in (lambda: d.set_window(3, 5, 13, 11), lambda: d.render_windows([(3, 5)], 13, 11), lambda: d.render_window(3, 5, 13, 11),
                 lambda: d.set_batch_windows([(3, 5)] * 3, 13, 11), lambda: d.set_window(8, 8, 13, 16), lambda: d.render_windows([(8, 8)], 16, 11)):
        with pytest.raises(ValueError, match="multiples of 8"):
            call()


def test_covers_follow_the_windows():
    d = _decoder()
    d._window = (3, 5, 13, 11)
    assert d.window_cover == (0, 0, 16, 16)
    d._window = (8, 16, 24, 32)
    assert d.window_cover == (8, 16, 24, 32)
    origins = np.array([[0, 0], [123, 253], [3, 5]], np.int32)
    d._batch_windows = (origins, 13, 11)
    o, w, h = d.batch_window_covers
    assert (w, h) == (24, 24) and o.tolist() == [[0, 0], [112, 240], [0, 0]]
    assert [tuple(c) + (w, h) for c in o.tolist()] == [PX.shared_cover((x0, y0, 13, 11), 136, 264) for x0, y0 in origins.tolist()]
    assert d.batch_windows[0].tolist() == origins.tolist()
    d._batch_windows = (np.array([[0, 0], [8, 16], [56, 56]], np.int32), 32, 32)      # all aligned: their own covers
    o, w, h = d.batch_window_covers
    assert (w, h) == (32, 32) and o.tolist() == [[0, 0], [8, 16], [56, 56]]


def test_file_calls_check_px_windows_first():
    from yaik_amd import files
    files.host_lib()                                                        # loads without a device; no call below reaches a decode
    for bad in ((-1, 0, 8, 8), (0, 0, 0, 8), (0, 0, 8, 0)):
        with pytest.raises(ValueError):
            files.decode_file_window_device(b"", bad, px=True)
        with pytest.raises(ValueError):
            files.decode_file_windows_device(b"", [bad[:2]], bad[2], bad[3], px=True)
        with pytest.raises(ValueError):
            files.decode_files_windows_device([b""], [bad[:2]], bad[2:], px=True)
    with pytest.raises(TypeError):
        files.decode_file_window_device(b"", (0.5, 0, 8, 8), px=True)
    # the default keeps today's checks
    with pytest.raises(ValueError, match="multiples of 8"):
        files.decode_file_window_device(b"", (3, 5, 13, 11))
    with pytest.raises(ValueError, match="multiples of 8"):
        files.decode_file_windows_device(b"", [(3, 5)], 13, 11)
    with pytest.raises(ValueError, match="multiples of 8"):
        files.decode_files_windows_device([b""], [(3, 5)], (13, 11))
