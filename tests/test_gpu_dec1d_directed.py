"""The 1-D range decode kernels of yk_decode.hip (yk_dec1d_count / scan / body in its ALL, WIN and LIST forms, and the batch launches) on the
hand-built '1DTL' streams of tests/dec1d_cases.py, bit for bit against the model's planes and tile4x4Mask (tests/test_dec1d_cases.py shows, without
a GPU, that the model and the oracle agree on every case and that the cases hold what they claim).  Every case goes through

  host     decompress_1d = yk_decode_1d: the streams copied into the handle's scratch
  inplace  decode_streams = yk_decode_1d_device with 16-byte aligned pointers: the streams read where they lie
  off1     yk_decode_1d_device with both streams at offset 1 of a device buffer: the copy path
  off8     ... at offset 8

with the case's compressionRange; then windows (set_window, aligned and pixel), the batch call (whole frames, windows, rectangles), prepared images
(prepare + render_windows), the per-plane masks through a batch of one, stale scratch behind a shorter stream and one handle across two ranges.  A
failure names the case, the path, the first differing tile, its mask, its parameters and its place in the streams.
"""
import ctypes as C

import numpy as np
import pytest

from tests import dec1d_cases as DC
from tests import graddec_cases as GC

pytestmark = pytest.mark.gpu
PATHS = ("host", "inplace", "off1", "off8")


def _torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def dec(oracle_built):
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    yield d
    d.close()


_DEVICE = {}


def _dev(arr, key, off=0):
    """(address, length) of `arr` at offset `off` of a device buffer of its own (uploaded once per key, kept alive here; never an empty tensor)"""
    torch = _torch()
    if key not in _DEVICE:
        buf = np.zeros(off + arr.size + 16, dtype=np.uint8)
        buf[off:off + arr.size] = arr
        t = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        assert t.data_ptr() % 16 == 0
        _DEVICE[key] = t
    return _DEVICE[key].data_ptr() + off, int(arr.size)


def _call_1d(name, off=0):
    c = DC.case(name)
    return ("1",) + _dev(c["typ"], (name, "typ", off), off) + _dev(c["pix"], (name, "pix", off), off)


def _calls_g(name):
    """the case's 'GTIL' chunk in device memory as decode_streams / prepare take it: the raw stream (remap_range 250)"""
    g = DC.case(name)["gtil"]
    if g is None:
        return []
    (sx, sy, bm, raw), = g["chunks"]
    return [("g", sx, sy) + _dev(bm, (name, "bm")) + _dev(raw, (name, "raw"))]


def _marks(d, name):
    """the gradient phase through the host calls: the hand-built 4x4 chunk, or the plane-subset chunks with consistent marks"""
    c = DC.case(name)
    if c["gtil"] is not None:
        (sx, sy, bm, _), = c["gtil"]["chunks"]
        d.decompress_gradient(sx, sy, bm, GC.oracle_streams(c["gtil"])[0])
    for m, bm, stream in c["plane_chunks"]:
        d.decompress_gradient_planes(m, bm, stream, consistent_marks=True)


def _decode_1d(d, name, path):
    c = DC.case(name)
    if path == "host":
        d.decompress_1d(c["typ"], c["pix"], c["range"])
        return
    call = _call_1d(name, {"inplace": 0, "off1": 1, "off8": 8}[path])
    assert ((call[1] | call[3]) & 15 == 0) == (path == "inplace")
    d.decode_streams([call], compression_range=c["range"])


def _check(d, name, what):
    c, m = DC.case(name), DC.model(name)
    got = d.planes()
    assert np.array_equal(got, m["planes"]), f"{name} via {what}: planes differ; {DC.story(name, got, m['planes'])}"
    t4 = d.tile4x4(bool(c["plane_chunks"]))
    bad = np.flatnonzero(t4 != m["tile4"])
    assert not bad.size, f"{name} via {what}: tile4x4Mask differs first at byte {bad[0]}: {t4[bad[0]]:#04x} for {m['tile4'][bad[0]]:#04x}"
    return got


@pytest.mark.parametrize("name", DC.ALL_NAMES)
def test_case_equals_the_model_through_the_host_and_device_calls(dec, name):
    c = DC.case(name)
    got = {}
    for path in PATHS:
        dec.begin(c["w"], c["h"])
        _marks(dec, name)
        _decode_1d(dec, name, path)
        got[path] = _check(dec, name, path)
    for path in PATHS[1:]:
        assert np.array_equal(got[path], got["host"]), f"{name}: {path} and host disagree"


def _img(planes, w, h):
    """uint8 [h, w, 3] from 8x8-tiled planes"""
    return np.asarray(planes).reshape(3, h // 8, w // 8, 8, 8).transpose(1, 3, 2, 4, 0).reshape(h, w, 3)


def _assert_inside(name, got_planes, rect, what):
    c = DC.case(name)
    x0, y0, ww, wh = rect
    got = _img(got_planes, c["w"], c["h"])[y0:y0 + wh, x0:x0 + ww]
    want = _img(DC.model(name)["planes"], c["w"], c["h"])[y0:y0 + wh, x0:x0 + ww]
    bad = np.argwhere((got != want).any(axis=2))
    assert not bad.size, f"{name} {what}: {len(bad)} pixels differ inside {rect}, first at (x, y) = ({x0 + bad[0][1]}, {y0 + bad[0][0]})"


# aligned windows and pixel windows; on 520 x 264 tile 1024 is tile (49, 15): the first two windows hold it, with rows that end in one scan block and
# begin in the next; the third touches the right and bottom edges (the partial 64-blocks), the fourth lies inside block 0
WINDOWS = [("masks_136x72", (8, 8, 64, 32), False), ("masks_136x72", (72, 40, 64, 32), False), ("masks_136x72", (5, 3, 77, 41), True),
           ("blocks_520x264", (320, 96, 200, 64), False), ("blocks_520x264", (323, 99, 190, 61), True), ("blocks_520x264", (456, 200, 64, 64), False),
           ("blocks_520x264", (16, 8, 96, 40), False), ("blocks_520x264", (0, 0, 520, 264), True)]


@pytest.mark.parametrize("path", ["host", "inplace", "off1"])
@pytest.mark.parametrize("name,win,px", WINDOWS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_window_equals_the_model_inside_its_cover(dec, name, win, px, path):
    c = DC.case(name)
    if name == "blocks_520x264" and win[2] < 520:
        tx0, ty0, tx1, ty1 = win[0] >> 3, win[1] >> 3, (win[0] + win[2] + 7) >> 3, (win[1] + win[3] + 7) >> 3
        assert (tx0 <= 49 < tx1 and ty0 <= 15 < ty1) or ty1 <= 15 or ty0 > 15
    dec.begin(c["w"], c["h"])
    dec.set_window(*win, px=px)
    cover = dec.window_cover
    assert cover[0] <= win[0] and cover[1] <= win[1] and not (cover[0] | cover[1] | cover[2] | cover[3]) & 7
    _marks(dec, name)
    _decode_1d(dec, name, path)
    _assert_inside(name, dec.planes(), cover, f"window {win} via {path}")
    assert np.array_equal(dec.tile4x4(), DC.model(name)["tile4"]), f"{name} window {win} via {path}: the marks stay whole"
    got = dec.image_window_device().cpu().numpy()
    x0, y0, ww, wh = win
    assert np.array_equal(got, _img(DC.model(name)["planes"], c["w"], c["h"])[y0:y0 + wh, x0:x0 + ww]), f"{name} window {win} via {path}: the window's pixels"


def _batch_frames(names):
    frames = []
    for n in names:
        c = DC.case(n)
        (sx, sy, bm, raw), = c["gtil"]["chunks"]
        frames.append([("g", sx, sy, bm, bm.size, raw, raw.size), ("1", c["typ"], c["typ"].size, c["pix"], c["pix"].size)])
    return frames


BATCH_ORIGINS = [(8, 8), (72, 40), (32, 0)]                                       # 64 x 32 windows: inside, at the right and bottom edges, at the top
BATCH_RECTS = [(5, 3, 77, 41), (0, 0, 136, 72), (101, 50, 35, 22)]


@pytest.mark.parametrize("mode", ["whole", "windows", "rects"])
@pytest.mark.parametrize("key", list(DC.BATCHES))
def test_batch_equals_the_model_frame_by_frame(dec, key, mode):
    names = DC.BATCHES[key]
    c0 = DC.case(names[0])
    dec.begin_batch(c0["w"], c0["h"], 3)
    if mode == "windows":
        dec.set_batch_windows(BATCH_ORIGINS, 64, 32)
        covers = [(x, y, 64, 32) for x, y in BATCH_ORIGINS]
    elif mode == "rects":
        dec.set_batch_rects(BATCH_RECTS)
        covers = [(x & ~7, y & ~7, ((x + w + 7) & ~7) - (x & ~7), ((y + h + 7) & ~7) - (y & ~7)) for x, y, w, h in BATCH_RECTS]
    dec.decode_batch_streams(_batch_frames(names), remap_range=250, compression_range=c0["range"])
    for f, n in enumerate(names):
        dec.select_frame(f)
        if mode == "whole":
            _check(dec, n, f"batch {key} frame {f}")
        else:
            _assert_inside(n, dec.planes(), covers[f], f"batch {key} frame {f} with {mode}")
            assert np.array_equal(dec.tile4x4(), DC.model(n)["tile4"]), (key, f, mode)


PREPARED = [("masks_136x72", [(0, 0), (72, 8), (64, 40)], 64, 32),
            ("blocks_520x264", [(0, 0), (320, 96), (456, 200), (448, 0), (0, 200)], 64, 64)]      # the partial right and bottom 64-blocks of 520 x 264 included


@pytest.mark.parametrize("name,origins,ww,wh", PREPARED, ids=[p[0] for p in PREPARED])
def test_prepared_windows_equal_the_model(dec, name, origins, ww, wh):
    c = DC.case(name)
    w, h = c["w"], c["h"]
    want = _img(DC.model(name)["planes"], w, h)
    dec.begin(w, h)
    dec.prepare(_calls_g(name) + [_call_1d(name)], remap_range=250, compression_range=c["range"])
    got = dec.render_windows(origins[:2], ww, wh).cpu().numpy()
    got = np.concatenate([got, dec.render_windows(origins[2:], ww, wh).cpu().numpy()])
    for k, (x0, y0) in enumerate(origins):
        bad = np.argwhere((got[k] != want[y0:y0 + wh, x0:x0 + ww]).any(axis=2))
        assert not bad.size, f"{name} prepared window {k} at ({x0}, {y0}): {len(bad)} pixels differ, first at ({x0 + bad[0][1]}, {y0 + bad[0][0]})"
    assert np.array_equal(dec.tile4x4(), DC.model(name)["tile4"]), name
    if name == "blocks_520x264":
        assert any(x0 + ww > 512 for x0, _ in origins) and any(y0 + wh > 256 for _, y0 in origins)
        px = dec.render_windows([(323, 99)], 190, 61, px=True).cpu().numpy()[0]      # rows across tile 1024, any offset
        assert np.array_equal(px, want[99:160, 323:513]), f"{name} prepared pixel window"


def test_prepared_image_of_another_range(dec):
    """prepare hands compression_range on: 256 x 256 of range 7, every (delta, L) pair, through the LIST kernel"""
    name = "values_r7"
    c = DC.case(name)
    dec.begin(256, 256)
    dec.prepare([_call_1d(name)], compression_range=7)
    got = dec.render_windows([(0, 0), (192, 192), (64, 128)], 64, 64).cpu().numpy()
    want = _img(DC.model(name)["planes"], 256, 256)
    for k, (x0, y0) in enumerate([(0, 0), (192, 192), (64, 128)]):
        assert np.array_equal(got[k], want[y0:y0 + 64, x0:x0 + 64]), (name, k)


@pytest.mark.parametrize("name", DC.SPLIT_NAMES)
def test_per_plane_masks_through_a_batch_of_one(dec, name):
    """the dSplit hand-over of yk_decode_1d_batch_device: a batch of one behind plane-subset chunks takes the single-image path, plane after plane"""
    c = DC.case(name)
    for where in ("host arrays", "device"):
        dec.begin_batch(c["w"], c["h"], 1)
        _marks(dec, name)
        call = ("1", c["typ"], c["typ"].size, c["pix"], c["pix"].size) if where == "host arrays" else _call_1d(name)
        dec.decode_batch_streams([[call]], compression_range=c["range"])
        dec.select_frame(0)
        _check(dec, name, f"a batch of one, streams as {where}")


@pytest.mark.parametrize("path", ["host", "off1"])
@pytest.mark.parametrize("short", ["cut_pix_0", "cut_typ_0", "cut_pix_in0", "cut_typ_in0"])
def test_stale_scratch_does_not_show_behind_a_shorter_stream(path, short):
    """the copy paths keep the streams in a grow-only scratch buffer: a whole stream first, then the same image with a stream cut short"""
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    try:
        for k, name in enumerate(("masks_136x72", short, "masks_136x72")):
            c = DC.case(name)
            assert np.array_equal(c["full_pix"], DC.case("masks_136x72")["full_pix"])
            d.begin(c["w"], c["h"])
            _marks(d, name)
            _decode_1d(d, name, path)
            _check(d, name, f"{path}, image {k} of the handle")
    finally:
        d.close()


@pytest.mark.parametrize("path", PATHS)
def test_one_handle_across_ranges(path):
    """the range is the call's, not the handle's: two values cases back to back, then the first again"""
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    try:
        for k, name in enumerate(("values_r7", "values_r16", "values_r7")):
            d.begin(256, 256)
            _decode_1d(d, name, path)
            _check(d, name, f"{path}, image {k} of the handle")
    finally:
        d.close()


def test_a_range_of_zero_is_refused_and_the_next_decode_is_right(dec):
    from yaik_amd._lib import YaikError
    name = "tile_16x8_m6"
    c = DC.case(name)
    for call in (lambda: dec.decompress_1d(c["typ"], c["pix"], 0), lambda: dec.decode_streams([_call_1d(name)], compression_range=0)):
        dec.begin(c["w"], c["h"])
        _marks(dec, name)
        with pytest.raises(YaikError):
            call()
        _decode_1d(dec, name, "host")
        _check(dec, name, "host after a refused range 0")


# ---- a file whose '1DTL' header carries another compressionRange ---------------------------------------------------------------------------------
TAG_1DTL, TAG_GTIL_FILE = 0x4C544431, 0x4C495447
FW, FH = 136, 72


def _with_range(stream, rng):
    """the stream with the compressionRange byte of its '1DTL' header (Header1D, byte 17 of the chunk body) rewritten"""
    import struct
    stream, p, at = bytearray(stream), 12, []
    while p + 8 <= len(stream):
        tag, ln = struct.unpack_from("<II", stream, p)
        if tag == 0xDEADBEEF:
            break
        if tag == TAG_1DTL:
            at.append(p + 8 + 17)
        p += 8 + ln
    assert len(at) == 1 and stream[at[0]] == 15                               # what the encoder writes
    stream[at[0]] = rng
    return bytes(stream)


def _file_expected(stream):
    """[h, w, 3] of a stream: the oracle's gradient decode of the chunks tests/chunks.py parses out of it, then the model on its 1-D streams with
    the range its header carries"""
    from oracle.pyoracle import OracleDecoder
    from tests import chunks
    b = chunks.parse(stream, FW, FH)
    n = int(np.frombuffer(b["chunk_count_terminated"], np.int32)[0])
    od = OracleDecoder(FW, FH)
    one_d = None
    for i in range(n):
        tag = int(np.frombuffer(b[f"c{i}_tag"], np.uint32)[0])
        hdr = np.frombuffer(b[f"c{i}_hdr"], np.int32)
        if tag == TAG_GTIL_FILE:
            assert hdr[8] == 7 and one_d is None                              # all three planes, before the 1-D chunk
            od.gradient(int(hdr[7]) & 7, (int(hdr[7]) >> 3) & 7, np.frombuffer(b[f"c{i}_bitmap"], np.uint8), np.frombuffer(b[f"c{i}_rgb"], np.uint8))     # PaletteDecompressor's output: remapped already
        else:
            assert tag == TAG_1DTL
            one_d = {"name": "file", "w": FW, "h": FH, "range": int(hdr[3]), "typ": np.frombuffer(b[f"c{i}_type"], np.uint8), "pix": np.frombuffer(b[f"c{i}_pix"], np.uint8)}
    assert one_d is not None and one_d["typ"].size and one_d["pix"].size
    m = DC.model_decode(one_d, state={"planes": od.planes().copy(), "tile4": od.tile4x4().copy()})
    assert m["consumed"] == (one_d["typ"].size, one_d["pix"].size)            # a legal stream: the marks and the streams fit
    return _img(m["planes"], FW, FH), one_d["range"]


def test_files_whose_1dtl_header_carries_another_range(oracle_built):
    torch = _torch()
    from tests import chunks
    from tests.images import edge_image
    from yaik_amd import files as F
    chunks.build_tool()
    F.set_device_palette(False)
    frames = np.stack([np.ascontiguousarray(edge_image(FW, FH, "mixed", 3, seed=11 + f).astype(np.uint8).transpose(1, 2, 0)) for f in range(3)])
    r15 = F.encode_files_device(frames)
    r7, r0 = [_with_range(s, 7) for s in r15], [_with_range(s, 0) for s in r15]
    want15, want7 = [_file_expected(s) for s in r15], [_file_expected(s) for s in r7]
    assert [r for _, r in want15] == [15] * 3 and [r for _, r in want7] == [7] * 3
    assert all((a != b).any() for (a, _), (b, _) in zip(want15, want7))       # the range is seen in the pixels
    eq = lambda t, want, what: np.array_equal(t.cpu().numpy(), want) or pytest.fail(f"{what}: pixels differ from the oracle's gradient + the model")
    eq(F.decode_file_device(r7[0]), want7[0][0], "range 7 alone")
    got = F.decode_files_device(r7)
    assert F.last_batch_info()["fallbacks"] == 0
    for f in range(3):
        eq(got[f], want7[f][0], f"three files of range 7, frame {f}")
    got = F.decode_files_device([r15[0], r7[1], r15[2]])
    assert F.last_batch_info()["fallbacks"] == 1
    for f, w in enumerate((want15[0], want7[1], want15[2])):
        eq(got[f], w[0], f"ranges 15, 7, 15, frame {f}")
    # range 0: both entry points report an error and write nothing
    out = torch.full((3, FH, FW, 3), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(F.YaikFileError):
        F.decode_files_device(r0, out=out)
    assert (out == 0xA5).all()
    L, h = F.host_lib(), F.library()
    src = np.frombuffer(r0[0], np.uint8)
    info = F.DecodedImage()
    assert L.YAIK_DecodeImagePre(h, src.ctypes.data, src.size, C.byref(info))
    torch.cuda.synchronize()
    info.outputImage, info.outputImageStride = out[0].data_ptr(), FW * 3
    assert not L.YAIK_DecodeImageToDevice(src.ctypes.data, src.size, C.byref(info)) and L.YAIK_GetErrorCode() != 0
    torch.cuda.synchronize()
    assert (out == 0xA5).all()
    eq(F.decode_file_device(r7[2]), want7[2][0], "range 7 after a refused range 0")
    got = F.decode_files_device(r15)
    assert F.last_batch_info()["fallbacks"] == 0
    for f in range(3):
        eq(got[f], want15[f][0], f"three files of range 15 after a refused range 0, frame {f}")
