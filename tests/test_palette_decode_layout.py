"""CPU side of PaletteDecompressor on the GPU (yk_palette_decompress_streams and friends): the entry points are declared in include/yaik_hip.h,
listed in yaik_amd/_lib.py with the same arity and exported by the built library; the stage id; the Python methods refuse CPU tensors and bad
arguments before any library call; and the ORACLE ALONE does on the corpus of tests/palette_payloads.py what tests/test_gpu_palette_decode.py
then demands of the device: it accepts every payload the corpus calls valid, rejects every one it calls malformed, decodes the compressor's
payloads back to their streams except for the few whose code index was resolved against a stale row, and has its truncation boundary where the
GPU test will look for it.  These oracle tests pass without the device decoder by design: they pin the reference behaviour."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import palette_payloads as PP
from tests import palette_streams as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"yk_palette_decompress_streams": 6, "yk_palette_decoded_device": 4, "yk_palette_decoded": 5, "yk_palette_decode_status": 2,
       "yk_decode_gradient_palette": 9}


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
    assert re.search(r"YK_STAGE_PALETTE_DEC\s*=\s*10\b", _header())


def test_library_exports_the_new_entry_points():
    from yaik_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)                                               # loading needs no device
    assert not [s for s in NEW if not hasattr(L, s)]


def test_chunk_sizes_are_those_of_the_kernels():
    src = open(os.path.join(ROOT, "yaik_amd", "csrc", "yk_palette_dec.hip")).read()
    assert int(re.search(r"#define\s+PD_CB\s+(\d+)", src).group(1)) == PP.CB
    assert int(re.search(r"#define\s+PD_CC\s+(\d+)", src).group(1)) == PP.CC


def _bare_decoder(monkeypatch):
    from yaik_amd import decoder

    def no_calls():
        raise AssertionError("library call before the arguments were checked")

    monkeypatch.setattr(decoder, "lib", no_calls)
    dec = decoder.HipTileDecoder.__new__(decoder.HipTileDecoder)            # no handle: nothing below may reach the library
    dec._h = None
    return dec


def test_methods_exist():
    from yaik_amd.decoder import HipTileDecoder
    for m in ("palette_decompress_streams", "palette_decoded", "palette_decoded_device", "palette_status"):
        assert callable(getattr(HipTileDecoder, m))


def test_cpu_tensors_and_bad_arguments_are_refused_before_any_library_call(monkeypatch):
    import torch
    dec = _bare_decoder(monkeypatch)
    pay = torch.zeros(9, dtype=torch.uint8)
    with pytest.raises(ValueError, match="CPU tensor"):
        dec.palette_decompress_streams([pay], [9])
    with pytest.raises(TypeError):
        dec.palette_decompress_streams([np.zeros(9, np.uint8)], [9])
    with pytest.raises(ValueError, match="payloads"):
        dec.palette_decompress_streams([], [])
    with pytest.raises(ValueError, match="output lengths"):
        dec.palette_decompress_streams([pay], [9, 9])
    for bad in (10, -3, 4.5, "9", None, True):
        with pytest.raises(ValueError, match="out_bytes"):
            dec.palette_decompress_streams([pay], [bad])
    for bad in (-1, 256, 1.0, "250", None, True):
        with pytest.raises(ValueError, match="remap_range"):
            dec.palette_decompress_streams([pay], [9], bad)


def test_oracle_accepts_every_valid_and_rejects_every_malformed_payload(oracle_built):
    items = PP.corpus()
    assert sum(it.valid for it in items) >= 40 and sum(not it.valid for it in items) >= 10
    assert len({it.name for it in items}) == len(items)
    for it in items:
        assert it.out_bytes % 3 == 0 and it.payload.dtype == np.uint8
        ok, out = PP.oracle_decode(it.payload, it.out_bytes)
        assert ok == it.valid, (it.name, ok)
        if ok:
            assert out.size == it.out_bytes
    # the shapes the GPU test relies on are really in there
    sizes = {it.out_bytes // 3 for it in items if it.valid}
    assert set(PP.COLOUR_COUNTS) <= sizes
    assert max(it.payload.size for it in items) > 4 * PP.CB


def test_corpus_reaches_every_token_kind_every_mask_and_every_distance():
    seen = {"delta": set(), "abs": set(), "dist": set(), "code": set(), "stack": 0}
    for it in PP.valid_items():
        p, n = it.payload, it.out_bytes // 3
        pos, written, run = 4 + 3 * int(p[0]), 1, 0
        while written < n and pos < p.size:
            b = int(p[pos])
            if b >= 0xC0:
                seen["dist"].add(b & 63); run += 1; pos += 1
                continue
            seen["stack"] = max(seen["stack"], run); run = 0
            if b < 0x80:
                seen["code"].add(b); pos += 1
            else:
                assert (b & 0xF0) == 0x80, (it.name, pos, b)
                seen["abs" if b & 8 else "delta"].add(b & 7); pos += 1 + bin(b & 7).count("1")
            written += 1
    assert seen["delta"] == set(range(8)) and seen["abs"] == set(range(8))
    assert seen["dist"] == set(range(64)) and seen["code"] == set(range(128)) and seen["stack"] >= 3


def test_compressor_payloads_decode_to_their_streams_except_a_few_stale_row_ones(oracle_built):
    """A code index the encoder resolved against a STALE row (a row of an earlier stream's book above this stream's own rows) is read by the
    decoder out of the bytes that follow this payload's header.  Reference behaviour; the device decoder reproduces it."""
    differ, total = [], 0
    for name, streams, chain in PS.cases():
        for i, (pay, stream) in enumerate(zip(PS.oracle_payloads(streams, chain), streams)):
            if not stream.size:
                continue
            total += 1
            ok, out = PP.oracle_decode(pay, stream.size, 250)
            assert ok, (name, i)
            if not np.array_equal(out, oracle_built.palette_remap(stream, 250)):
                differ.append((name, i))
    assert total > 300
    assert 1 <= len(differ) <= 6, differ
    assert {d[0] for d in differ} <= {"stale_chain", "empty_in_chain", "two_frames", "33_runs_of_7"}, differ


def test_truncation_boundary_of_the_header_only_payload(oracle_built):
    """Every colour beyond the first is a code token 0 read from the zero slack; tokens may start below n + 385."""
    assert PP.oracle_decode(PP.HEADER_ONLY, 3 * 2)[0]
    ok, out = PP.oracle_decode(PP.HEADER_ONLY, 3 * 385, 255)
    k = np.arange(1, 386, dtype=np.int64)[:, None]                          # with codeBookSize 0, "row 0" is the first colour's own bytes
    assert ok and np.array_equal(out.reshape(-1, 3), (k * PP.HEADER_ONLY[1:4].astype(np.int64)) & 255)
    b = PP.truncation_boundary()
    assert 385 <= b < 400
    assert PP.oracle_decode(PP.HEADER_ONLY, 3 * b)[0] and not PP.oracle_decode(PP.HEADER_ONLY, 3 * (b + 1))[0]
    assert not PP.oracle_decode(PP.HEADER_ONLY, 3 * (b + 2))[0]
    assert b == PP.HEADER_ONLY.size + 385 - 4 + 1                            # tokens at offsets 4 .. n + 384, plus the first colour
