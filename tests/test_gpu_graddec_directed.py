"""The gradient decode kernels of yk_decode.hip on the hand-built chunks of tests/graddec_cases.py, bit for bit against the oracle's planes and
tile4x4Mask after the last chunk (tests/test_graddec_cases.py shows, without a GPU, that the oracle and the model agree on every case and that the
cases hold what they claim).  Every case goes through every entry point that takes it:

  host      decompress_gradient chunk by chunk (yk_dec_owner / corner / render_kernel), streams remapped on the host
  pp_raw    decode_streams(per_pass=True, remap_range=250): the same kernels behind yk_dec_remap_kernel
  pp_remap  decode_streams(per_pass=True, remap_range=0) on the remapped streams
  all_raw   decode_streams = yk_decode_gradient_all_device (yk_decall_owner / stream / scan / render_blocks), remap inside the emit launch
  all_remap the same with remap_range=0; `eight_chunks` takes its pass-after-pass fallback

then the batch call on the triples of group i, windows (set_window), prepared images (prepare + render_windows) and one handle reused across
images of different sizes.  A failure names the case, the path, the first differing 8x8 tile, the pass and tile that wrote it and what the
model's census says about that tile's corners.

Run time of the whole file on an MI355X: 3.9 s for 296 tests, the slowest 0.23 s (offsets_1024x512 through the host path).
"""
import numpy as np
import pytest

from tests import graddec_cases as GC
from tests import prepared_cases as PC

pytestmark = pytest.mark.gpu
PATHS = ("host", "pp_raw", "pp_remap", "all_raw", "all_remap")


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


def _calls(name, remapped):
    """the chunks of a case in device memory as the call list of decode_streams (uploaded once per case, kept alive here): raw streams, or remapped"""
    torch = _torch()
    if name not in _DEVICE:
        c = GC.case(name)
        keep, lists = [], ([], [])
        for (sx, sy, bm, raw), rm in zip(c["chunks"], GC.oracle_streams(c)):
            tb = torch.from_numpy(bm.copy()).cuda()
            keep.append(tb)
            for k, s in enumerate((raw, rm)):
                ts = torch.from_numpy(np.concatenate([s, np.zeros(1, np.uint8)])).cuda()       # never an empty tensor
                keep.append(ts)
                lists[k].append(("g", sx, sy, tb.data_ptr(), bm.size, ts.data_ptr(), s.size))
        torch.cuda.synchronize()
        _DEVICE[name] = (keep,) + lists
    return _DEVICE[name][2 if remapped else 1]


def _decode(d, name, path):
    c = GC.case(name)
    if path == "host":
        for (sx, sy, bm, _), rm in zip(c["chunks"], GC.oracle_streams(c)):
            d.decompress_gradient(sx, sy, bm, rm)
        return
    raw = path.endswith("_raw")
    if raw and not c["remap"]:
        pytest.fail("a case whose values are remapped already has no raw form")
    d.decode_streams(_calls(name, not raw), per_pass=path.startswith("pp_"), remap_range=c["remap"] if raw else 0)


def _check(d, name, what):
    o = GC.oracle_run(name)
    got = d.planes()
    assert np.array_equal(got, o["planes"]), f"{name} via {what}: planes differ; {GC.story(name, got, o['planes'])}"
    t4 = d.tile4x4()
    bad = np.flatnonzero(t4 != o["tile4"])
    assert not bad.size, f"{name} via {what}: tile4x4Mask differs first at byte {bad[0]}: {t4[bad[0]]:#04x} for {o['tile4'][bad[0]]:#04x}"


def _paths_of(name):
    return PATHS if GC.case(name)["remap"] else ("host", "pp_remap", "all_remap")


@pytest.mark.parametrize("name,path", [(n, p) for n in GC.ALL_NAMES for p in (PATHS if not n.startswith("interp_") else ("host", "pp_remap", "all_remap"))])
def test_case_equals_the_oracle(dec, name, path):
    assert path in _paths_of(name)
    c = GC.case(name)
    dec.begin(c["w"], c["h"])
    _decode(dec, name, path)
    _check(dec, name, path)


@pytest.mark.parametrize("key", list(GC.BATCHES))
@pytest.mark.parametrize("raw", [True, False], ids=["raw", "remap"])
def test_batch_equals_the_oracle_frame_by_frame(dec, key, raw):
    names = GC.BATCHES[key]
    cs = [GC.case(n) for n in names]
    frames = []
    for c in cs:
        streams = [ch[3] for ch in c["chunks"]] if raw else GC.oracle_streams(c)
        frames.append([("g", sx, sy, bm, bm.size, s, s.size) for (sx, sy, bm, _), s in zip(c["chunks"], streams)])
    dec.begin_batch(cs[0]["w"], cs[0]["h"], 3)
    dec.decode_batch_streams(frames, remap_range=250 if raw else 0)
    for f, n in enumerate(names):
        dec.select_frame(f)
        _check(dec, n, f"batch {key} frame {f} ({'raw' if raw else 'remapped'})")


def _crop(name, win):
    from oracle.pyoracle import image_builder
    c = GC.case(name)
    x0, y0, ww, wh = win
    return image_builder(GC.oracle_run(name)["planes"], c["w"], c["h"], c["w"] * 3).reshape(c["h"], c["w"], 3)[y0:y0 + wh, x0:x0 + ww]


# windows that cut through overlapping tiles, that hold no tile (no pixel of one, and a whole 64x64 block without one) and that touch the right and
# the bottom edge, partial 64-blocks included
WINDOWS = [("overlap_later_wins", (8, 0, 40, 24)), ("overlap_later_wins", (0, 8, 16, 8)), ("file_order_reversed", (56, 56, 16, 16)),
           ("file_order_reversed", (64, 64, 64, 64)), ("corner_tiles", (32, 24, 32, 32)), ("word_halves_192x128_00", (128, 0, 64, 64)),
           ("word_halves_192x128_10", (120, 56, 72, 72)), ("interp_16x16", (16, 16, 16, 16)), ("edge_80x48", (64, 0, 16, 48)), ("edge_72x40", (56, 32, 16, 8)),
           ("edge_8x8", (0, 0, 8, 8)), ("word_halves_192x192", (128, 128, 64, 64)), ("cap_under_496x256", (432, 192, 64, 64))]


@pytest.mark.parametrize("path", ["host", "all_remap"])
@pytest.mark.parametrize("name,win", WINDOWS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else v)
def test_window_equals_the_crop_and_the_marks_stay_whole(dec, name, win, path):
    c = GC.case(name)
    dec.begin(c["w"], c["h"])
    dec.set_window(*win)
    _decode(dec, name, path)
    got = dec.image_window_device().cpu().numpy()
    want = _crop(name, win)
    bad = np.argwhere((got != want).any(axis=2))
    assert not bad.size, f"{name} window {win} via {path}: first differing pixel of the window (x, y) = ({bad[0][1]}, {bad[0][0]})"
    assert np.array_equal(dec.tile4x4(), GC.oracle_run(name)["tile4"]), f"{name} window {win} via {path}: the marks outside the window are still owed"
    if name == "corner_tiles":
        assert not want.any()                                                    # the window that holds no tile reads as zeros


PREPARED = [("file_order_reversed", [(0, 0), (24, 24), (96, 96)], 32, 32), ("overlap_later_wins", [(0, 0), (8, 8), (48, 48)], 16, 16),
            ("offsets_1024x512", [(448, 192), (496, 248), (960, 448)], 64, 64), ("edge_72x40", [(0, 0), (8, 0), (64, 32)], 8, 8),
            ("word_halves_192x192", [(64, 64), (96, 96), (176, 176)], 16, 16)]


@pytest.mark.parametrize("name,origins,ww,wh", PREPARED, ids=[p[0] for p in PREPARED])
def test_prepared_windows_equal_the_crops(dec, name, origins, ww, wh):
    c = GC.case(name)
    w, h = c["w"], c["h"]
    total = ((w + 63) // 64) * ((h + 63) // 64)
    shared = PC.block_mask(w, h, origins[:2], ww, wh)
    assert (PC.block_mask(w, h, origins[:1], ww, wh) & PC.block_mask(w, h, origins[1:2], ww, wh)).any()     # the first two windows share a 64x64 block
    assert total == 1 or not (shared & PC.block_mask(w, h, origins[2:], ww, wh)).any()         # the third window is disjoint from the other two
    dec.begin(w, h)
    dec.prepare(_calls(name, False), remap_range=c["remap"])
    assert dec.prepared_blocks == (0, total)
    got = dec.render_windows(origins[:2], ww, wh).cpu().numpy()
    assert dec.prepared_blocks == (int(shared.sum()), total)
    got = np.concatenate([got, dec.render_windows(origins[2:], ww, wh).cpu().numpy()])
    assert dec.prepared_blocks == (int(PC.block_mask(w, h, origins, ww, wh).sum()), total)
    for k, (x0, y0) in enumerate(origins):
        assert np.array_equal(got[k], _crop(name, (x0, y0, ww, wh))), f"{name} prepared window {k} at ({x0}, {y0})"
    assert np.array_equal(dec.tile4x4(), GC.oracle_run(name)["tile4"]), name


@pytest.mark.parametrize("path", ["all_raw", "pp_raw", "host"])
def test_one_handle_across_images(path):
    """stale owner / loaded / blockSums state: a large over-the-cap image, a 64 x 64 one-chunk image, the large one again, on one fresh handle"""
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder(0)
    try:
        for k, name in enumerate(("cap_over_512x256", "single_chunk", "cap_over_512x256")):
            c = GC.case(name)
            assert name != "single_chunk" or (c["w"], c["h"]) == (64, 64)
            d.begin(c["w"], c["h"])
            _decode(d, name, path)
            _check(d, name, f"{path}, image {k} of the handle")
    finally:
        d.close()
