"""batch_calls_from_table (yaik_amd/decoder.py): the decode_batch_streams call lists built from the rows of an encoder's stream table --
addresses and lengths only, so it is tested here on hand-made tables, without a GPU."""
import pytest

from yaik_amd.decoder import batch_calls_from_table
from yaik_amd.encoder import PASSES, FrameStreams

BM = [0x1000 + 0x100 * p for p in range(7)]
NBM = [2, 4, 4, 8, 16, 16, 32]


def _row(rgb=None, nrgb=None, pix=0x9000, npx=96, typ=0xA000, nty=18, bm=BM, nbm=NBM):
    rgb = [0x2000 + 0x400 * p for p in range(7)] if rgb is None else rgb
    nrgb = [3 * (p + 1) for p in range(7)] if nrgb is None else nrgb
    return FrameStreams(bm, nbm, rgb, nrgb, pix, npx, typ, nty)


def test_pass_order_and_fields():
    calls = batch_calls_from_table([_row(), _row(pix=0xB000, typ=0xC000)])
    assert len(calls) == 2 and all(len(c) == 8 for c in calls)
    for f, fr in enumerate(calls):
        for p, (sx, sy) in enumerate(PASSES):
            assert fr[p] == ("g", sx, sy, BM[p], NBM[p], 0x2000 + 0x400 * p, 3 * (p + 1)), (f, p)
    assert calls[0][7] == ("1", 0xA000, 18, 0x9000, 96)
    assert calls[1][7] == ("1", 0xC000, 18, 0xB000, 96)


def test_a_subset_of_passes_in_the_callers_order():
    passes = [PASSES[6], PASSES[0]]
    row = FrameStreams([0x100, 0x200], [32, 2], [0x300, 0], [6, 0], 0, 0, 0, 0)
    assert batch_calls_from_table([row], passes) == [[("g", 2, 2, 0x100, 32, 0x300, 6), ("g", 4, 4, 0x200, 2, 0, 0), ("1", 0, 0, 0, 0)]]


def test_empty_pass_keeps_its_bitmap_and_gets_a_null_stream():
    rgb = [0x2000, 0, 0x2800, 0x2C00, 0x3000, 0x3400, 0x3800]
    nrgb = [3, 0, 9, 12, 15, 18, 21]
    calls = batch_calls_from_table([_row(rgb, nrgb)])[0]
    assert calls[1] == ("g", 4, 3, BM[1], NBM[1], 0, 0)
    stale = list(rgb); stale[1] = 0x7777                                     # an address with no bytes behind it is not passed on
    assert batch_calls_from_table([_row(stale, nrgb)])[0][1] == ("g", 4, 3, BM[1], NBM[1], 0, 0)


def test_frame_without_1d_bytes():
    calls = batch_calls_from_table([_row(), _row(pix=0, npx=0, typ=0, nty=0), _row()])
    assert calls[1][7] == ("1", 0, 0, 0, 0)
    assert calls[0][7] == calls[2][7] == ("1", 0xA000, 18, 0x9000, 96)


def test_an_empty_table_gives_no_frames():
    assert batch_calls_from_table([]) == []


@pytest.mark.parametrize("bad", [
    dict(nrgb=[3, 3, 3, 3, 3, 3, 4]),                                        # not whole RGB triples
    dict(rgb=[0x2000, 0, 0x2800, 0x2C00, 0x3000, 0x3400, 0x3800]),            # a length with a NULL address
    dict(npx=95), dict(npx=32),                                              # not three planes of 16-byte cells
    dict(nty=17), dict(nty=6),                                               # not three planes of parameter triples
    dict(pix=0x9008),                                                        # read in place: 16-byte aligned
    dict(pix=0), dict(typ=0),                                                # lengths with NULL addresses
    dict(npx=0, pix=0), dict(nty=0, typ=0),                                  # one 1-D stream without the other
    dict(bm=BM[:6], nbm=NBM[:6]),                                            # not one bitmap per pass
    dict(bm=[0] + BM[1:]),                                                   # a pass without its bitmap
    dict(nbm=[0] + NBM[1:]),
    dict(nrgb=[-3, 3, 3, 3, 3, 3, 3]),
])
def test_wrong_lengths_are_rejected(bad):
    with pytest.raises(ValueError):
        batch_calls_from_table([_row(), _row(**bad)])


def test_frames_must_share_the_bitmap_lengths():
    with pytest.raises(ValueError):
        batch_calls_from_table([_row(), _row(nbm=NBM[:6] + [64])])


def test_rows_need_no_encoder_but_download_does():
    from yaik_amd._lib import YaikError
    with pytest.raises(YaikError):
        _row().download()


def test_header_signatures_and_record_agree():
    """include/yaik_hip.h declares the two entry points and the row layout that _lib.SIGNATURES and encoder._FrameStreamsC bind"""
    import ctypes as C
    import os
    import re

    from yaik_amd import _lib
    from yaik_amd.encoder import STREAMS_CORNERS, STREAMS_RANGE1D, _FrameStreamsC
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "yaik_hip.h")).read()
    assert re.search(r"int\s+yk_encode_streams_batch\(yk_ctx\*\s*c,\s*int\s+what\);", hdr)
    assert re.search(r"int\s+yk_batch_streams_table\(yk_ctx\*\s*c,\s*yk_frame_streams\*\s*out", hdr)
    assert re.search(r"YK_STREAMS_CORNERS\s*=\s*1,\s*YK_STREAMS_RANGE1D\s*=\s*2", hdr) and (STREAMS_CORNERS, STREAMS_RANGE1D) == (1, 2)
    assert _lib.SIGNATURES["yk_encode_streams_batch"] == (C.c_int, [C.c_void_p, C.c_int])
    assert _lib.SIGNATURES["yk_batch_streams_table"] == (C.c_int, [C.c_void_p, C.c_void_p])
    body = re.search(r"typedef struct yk_frame_streams \{(.*?)\} yk_frame_streams;", hdr, flags=re.S).group(1)
    fields = re.findall(r"(?:const uint8_t\*|size_t)\s+(\w+)(?:\[(\d)\])?;", body)
    assert [(n, int(k or 1)) for n, k in fields] == [(n, getattr(t, "_length_", 1)) for n, t in _FrameStreamsC._fields_]
    assert C.sizeof(_FrameStreamsC) == (4 * 7 + 4) * 8
    if os.path.exists(_lib.LIB_PATH):
        L = C.CDLL(_lib.LIB_PATH)
        assert hasattr(L, "yk_encode_streams_batch") and hasattr(L, "yk_batch_streams_table")
