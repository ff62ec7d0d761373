"""CPU side of PaletteCompressor on the GPU (yk_palette_*): the entry points are declared in include/yaik_hip.h, listed in yaik_amd/_lib.py with the
same arity and exported by the built library; the stage id; the Python methods refuse CPU tensors and bad chain values before any library call;
and the hand-made streams of tests/palette_streams.py make the CPU oracle alone produce every token kind (so that no kind hides behind inputs
that never reach it when tests/test_gpu_palette.py compares bytes)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import palette_streams as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"yk_palette_reset": 1, "yk_palette_compress_streams": 5, "yk_palette_compress": 1, "yk_palette_compress_batch": 1,
       "yk_palette_payload_device": 4, "yk_palette_payload": 5}


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
    assert re.search(r"YK_STAGE_PALETTE\s*=\s*9\b", _header())


def test_library_exports_the_new_entry_points():
    from yaik_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)                                               # loading needs no device
    assert not [s for s in NEW if not hasattr(L, s)]


class _NoCalls:
    """stands in for the library: any call through it fails the test"""
    def __getattr__(self, name):
        raise AssertionError(f"library call {name} before the arguments were checked")


def _bare_encoder():
    from yaik_amd.encoder import HipTileEncoder
    enc = HipTileEncoder.__new__(HipTileEncoder)                            # no handle: nothing below may reach the library
    enc._L, enc._h = _NoCalls(), None
    return enc


def test_methods_exist():
    from yaik_amd.encoder import HipTileEncoder
    for m in ("palette_reset", "palette_compress", "palette_compress_batch", "palette_compress_streams", "palette_payload", "palette_payload_device"):
        assert callable(getattr(HipTileEncoder, m))


def test_cpu_tensors_are_refused_before_any_library_call():
    import torch
    enc = _bare_encoder()
    with pytest.raises(ValueError, match="CPU tensor"):
        enc.palette_compress_streams([torch.zeros(9, dtype=torch.uint8)], 0)
    with pytest.raises(TypeError):
        enc.palette_compress_streams([np.zeros(9, np.uint8)], 0)
    with pytest.raises(ValueError):
        enc.palette_compress_streams([], 0)


@pytest.mark.parametrize("chain", [-1, 1.5, "7", None, True])
def test_bad_chain_values_are_refused_before_any_library_call(chain):
    import torch
    enc = _bare_encoder()
    with pytest.raises(ValueError, match="chain"):
        enc.palette_compress_streams([torch.zeros(9, dtype=torch.uint8)], chain)


def test_oracle_alone_produces_every_token_kind_on_the_hand_made_streams(oracle_built):
    """Token kinds counted in the oracle's own output over every hand-made case: each must occur, and so must books beyond 64 and 128 rows, a
    back-reference at every distance 0..63, and a hit on a STALE row (a row number at or above the stream's own row count)."""
    total = {}
    for name, streams, chain in PS.cases():
        for pay, stream in zip(PS.oracle_payloads(streams, chain), streams):
            if not stream.size:
                assert pay.size == 0
                continue
            k = PS.token_kinds(pay, stream.size // 3)
            for key, v in k.items():
                if isinstance(v, set):
                    total.setdefault(key, set()).update(v)
                else:
                    total[key] = max(total.get(key, 0), v) if key == "rows" else total.get(key, 0) + v
    for key in ("code", "backref", "explicit_delta", "explicit_abs", "stale_hit"):
        assert total[key] > 0, (key, total)
    assert total["rows"] == 128                                            # finalCount is capped
    assert total["distances"] == set(range(64)), sorted(set(range(64)) - total["distances"])
    assert total["masks_delta"] == set(range(1, 8)) and total["masks_abs"] == set(range(1, 8))
