"""CPU side of the batch 6-bit 'ALPM' encode: yk_alpha_values_mask_batch is declared in include/yaik_hip.h, listed in yaik_amd/_lib.py with the
same arity and exported by the built library; YAIK_EncodeImagesFromDeviceAlpha6 likewise in yaik_encode_alpha6.h, files.ENC6_SIGNATURES and
libyaik_host.so; the alpha6Bit fallback rule (files.alpha6_decodable) on hand-made bitmaps; the frames of tests/test_gpu_alpha6_batch.py give
the modes and the coverage that test relies on; the Python layer's argument checks, which call no library."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import alpha6_cases as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yaik_amd", "host")


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
    assert declared.get("yk_alpha_values_mask_batch") == 3
    res, args = _lib.SIGNATURES["yk_alpha_values_mask_batch"]
    assert res is C.c_int and len(args) == 3 and args[0] is C.c_void_p
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(C.CDLL(_lib.LIB_PATH), "yk_alpha_values_mask_batch")      # loading needs no device


def test_host_header_ctypes_table_and_library_agree():
    from yaik_amd import files
    subprocess.run(["make", "-C", HOST, "libyaik_host.so"], check=True, stdout=subprocess.DEVNULL)
    text = open(os.path.join(HOST, "yaik_encode_alpha6.h")).read()
    assert 'extern "C"' in text
    assert _arity(text, "YAIK_") == {"YAIK_EncodeImagesFromDeviceAlpha6": 13}
    assert list(files.ENC6_SIGNATURES) == ["YAIK_EncodeImagesFromDeviceAlpha6"]
    res, args = files.ENC6_SIGNATURES["YAIK_EncodeImagesFromDeviceAlpha6"]
    assert res is C.c_bool and len(args) == 13
    assert args[:9] == files.ENC_SIGNATURES["YAIK_EncodeImagesFromDevice"][1][:9]       # the same arguments up to emitAlpha, then alpha6Bit
    out = subprocess.run(["nm", "-D", "--defined-only", files.HOST_LIB_PATH], check=True, capture_output=True, text=True).stdout
    assert "YAIK_EncodeImagesFromDeviceAlpha6" in set(out.split())                    # C linkage: its own name
    L = files.host_lib()                                                    # loads without a device
    failed = C.c_int32(7)
    assert not L.YAIK_EncodeImagesFromDeviceAlpha6(None, None, 0, 0, 4, 8, 8, 1, 1, 1, 0, 1, C.byref(failed)) and failed.value == -1


def test_alpha6_decodable_rule():
    from yaik_amd.files import alpha6_decodable as rule
    full = np.array([0xFF, 0xFF, 0x07], np.uint8)                            # a 19-bit box: 3 used bits in the last byte
    assert rule(True, (1, 2, 19, 1), full)
    assert rule(1, np.array([0, 0, 19, 1], np.int32), full.tolist())
    assert rule(True, (0, 0, 4, 4), np.array([0xFF, 0xFF], np.uint8))
    for clear in (16, 17, 18, 0, 7, 8):                                      # one bit clear, in the last byte's used part and elsewhere
        bits = full.copy()
        bits[clear >> 3] &= ~(1 << (clear & 7)) & 0xFF
        assert not rule(True, (1, 2, 19, 1), bits), clear
    assert rule(True, (0, 0, 19, 1), np.array([0xFF, 0xFF, 0xFF], np.uint8))             # set padding bits do not count ...
    assert rule(True, (0, 0, 19, 1), np.array([0xFF, 0xFF, 0x07, 0x00], np.uint8))       # ... nor do whole bytes behind the box
    assert not rule(True, (0, 0, 19, 1), np.array([0x00, 0x00, 0xF8], np.uint8))         # set bits only in the padding beyond w * h
    assert not rule(True, (0, 0, 3, 1), np.array([0xF8], np.uint8))
    assert not rule(False, (1, 2, 19, 1), full)                              # no chunk
    assert not rule(True, (1, 2, 19, 1), np.zeros(0, np.uint8))              # empty bits
    assert not rule(True, (0, 0, 0, 5), full) and not rule(True, (0, 0, 5, 0), full)     # w * h = 0
    assert not rule(True, (0, 0, 19, 2), full)                               # fewer bits than the box has tiles
    assert rule(True, (0, 0, 19, 1), full) is True and rule(False, (0, 0, 19, 1), full) is False


def test_the_frames_of_the_gpu_test_give_the_modes_and_the_coverage():
    """ProcessAlpha(false) restated on the model of the alpha stage's bounds.  A rejected tile inside a box needs three tile columns and kept tiles
    spanning the image need sides that are multiples of 16 (the box of kept tiles ends on a tile edge, so on 72 x 40 and 1040 x 40 it never
    equals the image): 16 x 16 has only the second, 72 x 40 and 1040 x 40 only the first, 80 x 48 both in every batch of two or more."""
    for w, h in A.SHAPES:
        for n in A.COUNTS:
            kinds, frames = A.frames_of(w, h, n)
            assert len(kinds) == n and frames.shape == (n, 4, h, w)
            hole = span = 0
            for k, fr in zip(kinds, frames):
                a = fr[3]
                e6, e8 = A.want(a, A.model_bounds(a), False), A.want(a, A.model_bounds(a), True)
                assert (None if e6 is None else e6["mode"]) == A.KIND_MODE[k], (w, h, n, k)
                assert (None if e8 is None else e8["mode"]) == {3: 6}.get(A.KIND_MODE[k], A.KIND_MODE[k]), (w, h, n, k)
                hole += e6 is not None and e6["mode"] == 3 and A.has_rejected_tile_in_box(a)
                span += e6 is not None and e6["mode"] == 3 and A.spans_image(a)
            if (w, h) != (16, 16) and (n > 1 or (w, h) != (80, 48)):        # the batch of one at 80 x 48 is the spanning kind
                assert hole >= 1, (w, h, n)
            if (w, h) in ((16, 16), (80, 48)):
                assert span >= 1, (w, h, n)
    kinds, frames = A.frames_of(1040, 40, 2)
    x, y, bw, bh = A.want(frames[0, 3], A.model_bounds(frames[0, 3]), False)["bbox"]
    assert kinds[0] == "ring" and (x, bw) == (0, 1040)                       # the box spans all 65 tile columns
    low = A.frames_of(72, 40, 12)[1][10, 3]
    assert A.kinds_of(72, 40, 12)[10] == "low13" and low.max() == 3 and A.model_bounds(low)[2] > 0      # kept tiles, empty value box
    off = A.want(A.frames_of(72, 40, 12)[1][11, 3], A.model_bounds(A.frames_of(72, 40, 12)[1][11, 3]), False)
    assert off["bbox"][0] % 16 == 4 and off["bbox"][1] % 2 == 1


def test_force8bit_argument_is_checked_before_any_library_call():
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder.__new__(HipTileEncoder)                               # no handle, no library: the checks come first
    e.frames = 3
    assert e._force8bit_flags(None) is None
    assert e._force8bit_flags(True).tolist() == [1, 1, 1] and e._force8bit_flags(False).tolist() == [0, 0, 0]
    flags = e._force8bit_flags([0, True, np.bool_(False)])
    assert flags.dtype == np.uint8 and flags.tolist() == [0, 1, 0]
    for bad in ([1, 0], [1, 0, 1, 0], []):
        with pytest.raises(ValueError, match="3 frames"):
            e.alpha_values_mask_batch(bad)
        with pytest.raises(ValueError, match="3 frames"):
            e.alpha_mask_payloads_device(bad)
    e._h = None                                                              # __del__ -> close(): nothing to release


def test_pack_alpha_batch_takes_device_mask_entries():
    from yaik_amd.decoder import pack_alpha_batch
    pk = pack_alpha_batch([None, (3, (4, 5, 8, 2), 0x7F0000001000, 12, 0x7F0000002000, 2, (1, 0, 3, 4)), (6, (0, 0, 4, 1), 4096, 4, 0, 0, (0, 0, 0, 0))])
    assert pk.modes.tolist() == [-1, 3, 6] and pk.nbytes.tolist() == [0, 12, 4] and pk.staging.size == 0
    assert pk.where == [None, ("d", 0x7F0000001000), ("d", 4096)]
    assert pk.mip_where == [None, ("d", 0x7F0000002000), ("d", 0)] and pk.mip_nbytes.tolist() == [0, 2, 0]
    assert pk.mip_boxes.tolist() == [[0, 0, 0, 0], [1, 0, 3, 4], [0, 0, 0, 0]]
    with pytest.raises(ValueError):
        pack_alpha_batch([(3, (4, 5, 8, 2), np.zeros(12, np.uint8), 12, 4096, 2, (1, 0, 3, 4))])      # a host payload in a device entry
    with pytest.raises(ValueError):
        pack_alpha_batch([(3, (4, 5, 8, 2), 4096, 12, 4096, 2, (1, 0, 3))])
    with pytest.raises(ValueError):
        pack_alpha_batch([(3, (4, 5, 8, 2), 4096, 12, 4096, 2)])                                     # six fields
