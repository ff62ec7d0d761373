"""CPU side of the batch 'ALPM' calls: the five new entry points are declared in include/yaik_hip.h, listed in yaik_amd/_lib.py with the same
arity and exported by the built library; pack_alpha_batch (the staging layout HipTileDecoder.decompress_alpha_batch sends host payloads in) on
numpy: 16-byte aligned offsets, frames without a chunk, device pointers, refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from yaik_amd.decoder import pack_alpha_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"yk_alpha_values_batch": 3, "yk_alpha_payload_device": 4, "yk_alpha_payload": 5, "yk_decode_alpha_batch_device": 6,
       "yk_decode_output_batch_alpha_device": 5}


def _declared_arity():
    hdr = open(os.path.join(ROOT, "include", "yaik_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(yk_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
        out[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    return out


def test_header_and_signature_table_agree_on_the_new_entry_points():
    from yaik_amd import _lib
    declared = _declared_arity()
    for name, arity in NEW.items():
        assert declared.get(name) == arity, (name, declared.get(name))
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == arity, (name, len(args))
        assert args[0] is C.c_void_p                                       # the handle


def test_library_exports_the_new_entry_points():
    from yaik_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)                                               # loading needs no device
    assert not [s for s in NEW if not hasattr(L, s)]


def test_pack_host_payloads_at_aligned_offsets():
    rng = np.random.default_rng(3)
    sizes = [1, 16, 17, 0, 255, 4096, 33]
    pays = [rng.integers(0, 256, n, dtype=np.uint8) for n in sizes]
    ent = [(6, (f, 2 * f, 8, 4), p) for f, p in enumerate(pays)]
    pk = pack_alpha_batch(ent)
    assert pk.modes.dtype == np.int32 and pk.bboxes.dtype == np.int32 and pk.bboxes.shape == (len(ent), 4) and pk.bboxes.flags["C_CONTIGUOUS"]
    assert pk.modes.tolist() == [6] * len(ent) and pk.nbytes.tolist() == sizes
    assert pk.bboxes.tolist() == [[f, 2 * f, 8, 4] for f in range(len(ent))]
    end = 0
    for f, p in enumerate(pays):
        kind, off = pk.where[f]
        assert kind == "h" and off % 16 == 0 and off >= end                 # aligned, in order, no overlap
        np.testing.assert_array_equal(pk.staging[off:off + p.size], p)
        end = off + p.size
    assert pk.staging.dtype == np.uint8 and pk.staging.size >= end and pk.staging.size % 16 == 0
    assert pk.staging.size <= sum((n + 15) & ~15 for n in sizes)            # nothing but the alignment gaps is added


def test_pack_none_frames_device_pointers_and_stated_lengths():
    a = np.arange(40, dtype=np.uint8)
    pk = pack_alpha_batch([None, (1, (8, 0, 16, 3), a, 6), None, (4, [0, 0, 4, 1], 0x7F0000001230, 3), (5, np.array([4, 4, 8, 2]), C.c_void_p(4096), 12),
                           (6, (0, 0, 4, 4), a[::2])])
    assert pk.modes.tolist() == [-1, 1, -1, 4, 5, 6]
    assert pk.bboxes[0].tolist() == [0, 0, 0, 0] and pk.bboxes[2].tolist() == [0, 0, 0, 0] and pk.bboxes[4].tolist() == [4, 4, 8, 2]
    assert pk.nbytes.tolist() == [0, 6, 0, 3, 12, 20]
    assert pk.where[0] is None and pk.where[2] is None
    assert pk.where[1] == ("h", 0) and pk.where[3] == ("d", 0x7F0000001230) and pk.where[4] == ("d", 4096) and pk.where[5] == ("h", 16)
    np.testing.assert_array_equal(pk.staging[:6], a[:6])                    # only the stated length is staged
    np.testing.assert_array_equal(pk.staging[16:36], a[::2])                # a strided view is packed densely
    assert not pk.staging[6:16].any()
    empty = pack_alpha_batch([None, None])
    assert empty.staging.size == 0 and empty.modes.tolist() == [-1, -1] and empty.where == [None, None]
    assert pack_alpha_batch([]).modes.size == 0
    only_dev = pack_alpha_batch([(6, (0, 0, 1, 1), 4096, 1)])
    assert only_dev.staging.size == 0


def test_pack_refusals():
    a = np.zeros(10, np.uint8)
    with pytest.raises(ValueError, match="length"):
        pack_alpha_batch([(6, (0, 0, 4, 4), a, 11)])                         # a payload shorter than its stated length
    with pytest.raises(ValueError, match="length"):
        pack_alpha_batch([(6, (0, 0, 4, 4), a, -1)])
    with pytest.raises(ValueError, match="length"):
        pack_alpha_batch([(6, (0, 0, 4, 4), 4096)])                          # a device pointer without a length
    with pytest.raises(ValueError):
        pack_alpha_batch([(6, (0, 0, 4), a)])                                # a box of three numbers
    with pytest.raises(ValueError):
        pack_alpha_batch([(-1, (0, 0, 4, 4), a)])                            # None marks a frame without a chunk, not mode -1
    with pytest.raises(ValueError):
        pack_alpha_batch([(6, (0, 0, 4, 4))])
