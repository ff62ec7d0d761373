"""CPU side of the prepared-image decode: yk_decode_prepare_device, yk_decode_render_windows_device and yk_decode_prepared_blocks are
declared in include/yaik_hip.h, listed in yaik_amd/_lib.py with the same arity and exported; YAIK_DecodeImageWindowsToDevice and
YAIK_LastWindowsPrepared likewise in yaik_decode_multiwindow.h, files.MULTIWINDOW_SIGNATURES and libyaik_host.so; the Python methods check their
windows before any library call; and the block list of a render call (yaik_amd/csrc/yk_window_blocks.h, through window_blocks_tool) equals its
numpy restatement -- a wrong block id would be an out-of-bounds access on the device, so this runs on the CPU before any launch is fed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import prepared_cases as PC
from tests import window_cases as WC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yaik_amd", "host")
TOOL = os.path.join(HOST, "window_blocks_tool")
NEW_HIP = {"yk_decode_prepare_device": 14, "yk_decode_render_windows_device": 11, "yk_decode_prepared_blocks": 3}
NEW_HOST = {"YAIK_DecodeImageWindowsToDevice": 8, "YAIK_LastWindowsPrepared": 0}


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
    # the gradient arguments of yk_decode_gradient_all_device, then the 1-D arguments of yk_decode_1d_device
    assert _lib.SIGNATURES["yk_decode_prepare_device"][1] == (_lib.SIGNATURES["yk_decode_gradient_all_device"][1] + _lib.SIGNATURES["yk_decode_1d_device"][1][1:])
    # the layout arguments of yk_decode_output_batch_device behind the window table
    assert _lib.SIGNATURES["yk_decode_render_windows_device"][1][5:] == _lib.SIGNATURES["yk_decode_output_batch_device"][1][1:]
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)                                               # loading needs no device
    assert not [s for s in NEW_HIP if not hasattr(L, s)]


def test_host_header_ctypes_table_and_library_agree():
    from yaik_amd import files
    subprocess.run(["make", "-C", HOST, "libyaik_host.so"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(HOST, "yaik_decode_multiwindow.h")).read()
    assert 'extern "C"' in text
    assert _arity(text, "YAIK_") == NEW_HOST
    assert list(files.MULTIWINDOW_SIGNATURES) == list(NEW_HOST)
    res, args = files.MULTIWINDOW_SIGNATURES["YAIK_DecodeImageWindowsToDevice"]
    assert res is C.c_bool and len(args) == 8
    assert args[:3] == files.SIGNATURES["YAIK_DecodeImageToDevice"][1] and args[3:] == [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_size_t]
    assert files.MULTIWINDOW_SIGNATURES["YAIK_LastWindowsPrepared"] == (C.c_int, [])
    out = subprocess.run(["nm", "-D", "--defined-only", files.HOST_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert not set(NEW_HOST) - set(out.split())                             # C linkage: their own names
    L = files.host_lib()                                                    # loads without a device
    assert callable(L.YAIK_DecodeImageWindowsToDevice) and callable(L.YAIK_LastWindowsPrepared)
    L.YAIK_GetErrorCode()                                                   # drop what an earlier test may have left
    xy = (C.c_int * 2)(0, 0)
    assert not L.YAIK_DecodeImageWindowsToDevice(None, 0, None, 1, xy, 8, 8, 192)   # no context: refused before anything is touched
    assert files.ERROR_NAMES[L.YAIK_GetErrorCode()] == "YAIK_DECIMG_INVALIDCTX"


def _bare_decoder(w=136, h=264):
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder.__new__(HipTileDecoder)                              # no handle, no library: the checks come first
    d._h = None
    d.w, d.h, d.frames, d._window, d._has_alpha, d.device = w, h, 1, None, False, 0
    return d


def test_render_window_arguments_are_checked_before_any_library_call():
    d = _bare_decoder()
    for bad in ((4, 0, 8, 8), (0, 4, 8, 8), (0, 0, 12, 8), (0, 0, 8, 12), (0, 0, 0, 8), (0, 0, 8, 0), (-8, 0, 8, 8), (0, -8, 16, 16), (0, 0, -8, -8),
                (136, 0, 8, 8), (0, 264, 8, 8), (8, 0, 136, 8), (0, 8, 8, 264), (0, 0, 144, 8), (0, 0, 8, 272), (0, 0, 0, 0)):
        with pytest.raises(ValueError, match="window"):
            d.render_window(*bad)
        with pytest.raises(ValueError, match="window"):
            d.render_windows([(0, 0), bad[:2]], bad[2], bad[3])
    for bad in ((0.0, 0, 8, 8), (0, 0, 8, "8"), (True, 0, 8, 8), (0, 0, None, 8)):
        with pytest.raises(TypeError, match="window"):
            d.render_window(*bad)
    with pytest.raises(ValueError, match="window"):
        d.render_windows([], 8, 8)
    with pytest.raises(ValueError, match="window"):
        d.render_windows([(0, 0)] * 1025, 8, 8)
    for bad in (None, 7, "0000", [(0, 0, 8)], [8, 8], [(0, 0), "ab"]):
        with pytest.raises(TypeError, match="window"):
            d.render_windows(bad, 8, 8)


def test_decode_file_windows_device_checks_the_windows_first():
    from yaik_amd import files
    for origins, w, h in (([(0, 0)], 12, 8), ([(4, 0)], 8, 8), ([(0, 0)], 0, 0), ([(-8, 0)], 8, 8), ([], 8, 8), ([(0, 0)] * 1025, 8, 8)):
        with pytest.raises(ValueError, match="window"):
            files.decode_file_windows_device(b"", origins, w, h)
    for origins, w, h in (("0088", 8, 8), (None, 8, 8), ([(0, 0, 8)], 8, 8), ([(0, 0)], 8.0, 8), ([(True, 0)], 8, 8)):
        with pytest.raises(TypeError, match="window"):
            files.decode_file_windows_device(b"", origins, w, h)


# ---- the block list ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-C", HOST, "window_blocks_tool"], check=True, stdout=subprocess.DEVNULL)
    return TOOL


def _run(tool, w, h, ww, wh, origins, done=(), calls=1):
    args = [tool, str(w), str(h), str(ww), str(wh)]
    if done:
        args += ["-d", ",".join(str(int(b)) for b in done)]
    if calls != 1:
        args += ["-r", str(calls)]
    args += [str(v) for o in origins for v in o]
    r = subprocess.run(args, capture_output=True, text=True)
    if r.returncode == 3:
        assert r.stdout.strip() == "bad"
        return None
    assert r.returncode == 0, r.stderr
    out = []
    for line in r.stdout.strip().split("\n"):
        head, _, ids = line.partition(":")
        rendered, total = (int(v) for v in head.split())
        out.append((rendered, total, np.array([int(v) for v in ids.split()], dtype=np.int64)))
    assert len(out) == calls
    return out


def _check(tool, w, h, ww, wh, origins, done=()):
    total = ((w + 63) // 64) * ((h + 63) // 64)
    want = PC.new_blocks(w, h, origins, ww, wh, done)
    first, second = _run(tool, w, h, ww, wh, origins, done, calls=2)
    rendered, tot, ids = first
    assert tot == total
    assert np.array_equal(ids, want), (w, h, ww, wh, origins, done)
    assert (np.diff(ids) > 0).all() and (ids.size == 0 or (ids[0] >= 0 and ids[-1] < total))      # sorted, distinct, in range
    assert not set(ids.tolist()) & set(done)
    assert rendered == len(set(done)) + ids.size
    assert second[0] == rendered and second[2].size == 0                     # the same windows again: nothing is left to render
    return ids


def test_block_list_empty_and_partly_filled_bitmap_duplicates_and_overlaps(tool):
    w, h = 520, 264
    ww, wh = PC.K8_SIZE
    ids = _check(tool, w, h, ww, wh, PC.K8_ORIGINS)
    assert ids.size < sum(PC.block_mask(w, h, [o], ww, wh).sum() for o in PC.K8_ORIGINS)      # windows share blocks: each listed once
    assert {8, 44, 39} <= set(ids.tolist())                                  # the partial right column, the last block, the partial bottom row
    some = ids[::2].tolist()
    left = _check(tool, w, h, ww, wh, PC.K8_ORIGINS, done=some)
    assert sorted(left.tolist() + some) == ids.tolist()
    assert _check(tool, w, h, ww, wh, PC.K8_ORIGINS, done=ids.tolist()).size == 0
    _check(tool, w, h, ww, wh, PC.K8_ORIGINS, done=list(range(45)))
    # every window of every image of the GPU tests, one by one and in one call per size
    for cw, ch, _ in WC.CASES:
        for win in PC.case_windows(cw, ch):
            _check(tool, cw, ch, win[2], win[3], [win[:2]])
            _check(tool, cw, ch, win[2], win[3], [win[:2], win[:2]], done=[0])


def test_block_list_partial_right_and_bottom_blocks(tool):
    # 136 x 264: 3 x 5 blocks, the right column 8 pixels wide, the bottom row 8 pixels high
    assert _check(tool, 136, 264, 8, 8, [(128, 256)]).tolist() == [14]
    assert _check(tool, 136, 264, 8, 8, [(128, 0), (0, 256)]).tolist() == [2, 12]
    assert _check(tool, 136, 264, 16, 16, [(120, 248)]).tolist() == [10, 11, 13, 14]
    assert _check(tool, 136, 264, 136, 264, [(0, 0)]).tolist() == list(range(15))
    assert _check(tool, 136, 264, 136, 8, [(0, 56), (0, 64)]).tolist() == [0, 1, 2, 3, 4, 5]
    assert _check(tool, 8, 8, 8, 8, [(0, 0)]).tolist() == [0]
    assert _check(tool, 8, 8, 8, 8, [(0, 0)], done=[0]).size == 0
    assert _check(tool, 32760, 32760, 8, 8, [(32752, 32752), (0, 0)]).tolist() == [0, 512 * 512 - 1]


def test_block_list_of_1024_windows(tool):
    rng = np.random.default_rng(1024)
    w, h, ww, wh = 2048, 1096, 72, 136
    origins = [(int(rng.integers(0, (w - ww) // 8 + 1)) * 8, int(rng.integers(0, (h - wh) // 8 + 1)) * 8) for _ in range(1024)]
    ids = _check(tool, w, h, ww, wh, origins)
    assert 0 < ids.size <= 32 * 18
    done = rng.choice(32 * 18, 200, replace=False).tolist()
    _check(tool, w, h, ww, wh, origins, done=done)
    assert _run(tool, w, h, ww, wh, origins + [(0, 0)]) is None               # 1025 windows


def test_block_list_tool_refuses_bad_windows(tool):
    for ww, wh, origins in ((8, 8, [(132, 0)]), (8, 8, [(136, 0)]), (8, 8, [(0, 264)]), (16, 8, [(128, 0)]), (8, 12, [(0, 0)]), (0, 8, [(0, 0)]),
                            (144, 8, [(0, 0)]), (8, 8, [(0, 0), (-8, 0)]), (8, 8, [(0, 0), (0, 260)])):
        assert _run(tool, 136, 264, ww, wh, origins) is None, (ww, wh, origins)


def test_the_scan_block_block_meets_the_window_condition(oracle_built):
    """(384, 64, 64, 64) on 520 x 264 holds a fully marked, an unmarked and a partly marked tile, and tiles of all three kinds precede it"""
    w, h, kind = 520, 264, "mixed"
    assert (w, h, kind) in WC.CASES
    ref = WC.reference(w, h, kind)
    assert WC.condition_failures(WC.tile_kinds(ref.tile4, w, h), PC.SCAN_BLOCK_BLOCK) == []
    x0, y0, ww, wh = PC.SCAN_BLOCK_BLOCK
    tiles = [(y0 // 8 + 7) * (w // 8) + x0 // 8 + k for k in range(8)]       # the block's last tile row
    assert tiles[0] == 1023 and tiles[1] == 1024                             # ... straddles two scan blocks of 1024 tiles
