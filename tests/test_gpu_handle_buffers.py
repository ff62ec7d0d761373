"""One long-lived handle walked through shapes and frame counts of different sizes, across every stage that keeps device buffers: what the
handle hands out at each step must equal, byte for byte, what a FRESH handle gives for the same input (and, for the fused encode, what the
CPU oracle gives).  The logic under test is "needs more than before / less than before / more than ever / a shape seen before", so the
shapes are tiny.  Only documented call orders, and no allocation that is meant to fail."""
import numpy as np
import pytest

from oracle.pyoracle import PASSES, OracleEncoder
from tests.blobs import LUT_PASSES
from tests.images import edge_image
from tests.lutbank import lut_image
from tests.parity import compare_encode
from yaik_amd.synth import bank_patterns

pytestmark = pytest.mark.gpu

WALK = [(16, 16), (136, 72), (24, 8), (264, 136), (136, 72)]        # grows, shrinks, grows past the old maximum, a shape seen before
PIXEL_CACHE = [False, True, False, True, False]                     # the 1-D path behind the pixel cache at some shapes, from the planes at others


def _rgba(w, h, seed):
    """Mixed content (gradient tiles, noise, 1-D work) under an analog alpha plane with a transparent band on the left, a transparent block
    and, where the image has room for it, transparent 16x16 tiles along the right and bottom edges (the kept box then ends at least 16 pixels
    inside the image, which _oracle_padded needs)."""
    rgb = edge_image(w, h, "mixed", 3, seed)
    y, x = np.mgrid[0:h, 0:w]
    a = 40 + ((x * 3 + y * 5 + seed) % 200)
    a[:, : max(w // 8, 4)] = 0
    a[h // 2:, w // 2: w // 2 + 16] = 0
    if min(w, h) >= 48:
        a[:, (w - 16) // 16 * 16:] = 0
        a[(h - 16) // 16 * 16:, :] = 0
    return np.ascontiguousarray(np.concatenate([rgb, a[None]]).astype(np.int32))


def _same(got, want, where):
    """byte-for-byte equality of nested results (dicts, sequences, arrays, scalars, None)"""
    if isinstance(want, dict):
        assert isinstance(got, dict) and got.keys() == want.keys(), where
        for k in want:
            _same(got[k], want[k], f"{where}.{k}")
    elif isinstance(want, (list, tuple)):
        assert isinstance(got, (list, tuple)) and len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, f"{where}[{i}]")
    elif want is None:
        assert got is None, where
    else:
        g, w = np.asarray(got), np.asarray(want)
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), where


# ---- encoder, one image ---------------------------------------------------------------------------------------------------------------------
def _encoder_outputs(enc, planes, pixel_cache):
    out = {}
    enc.set_pixel_cache(pixel_cache)
    enc.set_image(planes)
    out["alpha"] = enc.mip_prefilter()                                              # alpha reject and finish
    enc.encode(3, False, True)                                                      # fused encode with wantDst
    out["bitmaps"] = [enc.gradient_bitmap(p) for p in range(7)]
    out["counts"] = enc.gradient_counts()
    out["coverage"] = enc.coverage()
    out["range"] = [enc.range_streams(p) for p in range(3)]
    out["dst"] = [enc.range_dst(p) for p in range(3)]
    out["corners"] = [enc.gradient_corners(p) for p in range(7)]
    out["edges"] = enc.gradient_corner_edges()
    out["1d"] = enc.dynamic_tile_compressor()
    out["alpha8"] = enc.alpha_values(True)
    out["alpha6"] = enc.alpha_values(False)
    enc.palette_reset()
    out["palette"] = [enc.palette_payload(i) for i in range(enc.palette_compress())]
    out["partial"] = enc.fitting_quad_smooth_planes(3, 2, 2)                        # one plane-subset pass: count, bitmap, corners
    out["partial_coverage"] = [enc.coverage_plane(p) for p in range(3)]
    return out


def _oracle_padded(planes, got):
    """RGBA that is no power-of-two square, where the oracle's MipPrefilter is not defined: the oracle on the planes zero-padded to the
    enclosing power-of-two square, as tests/test_gpu_event_chain.py does.  Padding adds rejected tiles only, so the box, the reject bitmap over it
    and -- the streams being row-major over the tile grid and the box ending 16 pixels inside the image -- the three planes' definition and nibble
    streams are those of the unpadded image; `got` holds what the handle gave for it."""
    n, h, w = planes.shape
    side = 16
    while side < max(h, w):
        side *= 2
    padded = np.zeros((n, side, side), np.int32)
    padded[:, :h, :w] = planes
    ora = OracleEncoder(padded)
    mo = ora.mip_prefilter()
    for k in ("has_chunk", "bounds", "remaining", "tile_bbox", "bitmap"):
        assert np.array_equal(np.asarray(got["alpha"][k]), np.asarray(mo[k])), k
    for sx, sy in PASSES:                                     # the oracle's range pass codes what its gradient passes left uncovered
        ora.fitting_quad_smooth(sx, sy)
    for p in range(3):
        defs, nib, nn, _ = ora.dynamic_tile_encode(p, False)
        d2, n2, nn2 = got["range"][p]
        assert nn2 == nn and np.array_equal(d2, defs) and np.array_equal(n2, nib), p


def test_encoder_walk(oracle_built):
    from yaik_amd.encoder import HipTileEncoder
    enc = HipTileEncoder(0)
    try:
        for step, ((w, h), cache) in enumerate(zip(WALK, PIXEL_CACHE)):
            planes = _rgba(w, h, 100 + step)
            # the oracle's MipPrefilter is defined for square power-of-two images only.  Elsewhere compare_encode takes the image's R, G, B
            # planes (every map, stream and corner) and the RGBA encode below goes against the oracle on the padded square, where the image has
            # room for the transparent edge that needs
            square = w == h and w & (w - 1) == 0
            assert compare_encode(planes if square else planes[:3], enc, False, True, check_corners=True) == [], (step, w, h)
            got = _encoder_outputs(enc, planes, cache)
            if not square and min(w, h) >= 48:
                _oracle_padded(planes, got)
            fresh = HipTileEncoder(0)
            try:
                want = _encoder_outputs(fresh, planes, cache)
            finally:
                fresh.close()
            _same(got, want, f"step{step}:{w}x{h}")
    finally:
        enc.close()


# ---- encoder, batches -----------------------------------------------------------------------------------------------------------------------
def _batch_outputs(enc, frames):
    out = {}
    enc.set_batch(frames)
    enc.encode_batch(3, False)
    out["streams"] = [s.download() for s in enc.streams_batch(corners=True, range1d=False)]
    out["streams_both"] = [s.download() for s in enc.streams_batch(corners=True, range1d=True)]
    table = enc.streams_table()
    out["table"] = [(t.bitmap_bytes, t.rgb_bytes, t.pix_bytes, t.type_bytes) for t in table]
    out["table_streams"] = [t.download() for t in table]
    out["alpha"] = enc.alpha_values_batch()
    out["palette"] = [enc.palette_payload(i) for i in range(enc.palette_compress_batch())]
    return out


def test_encoder_batch_walk():
    import torch
    from yaik_amd.encoder import HipTileEncoder
    w, h = 72, 40
    enc = HipTileEncoder(0)
    try:
        for step, n in enumerate((2, 5, 3)):
            frames = torch.from_numpy(np.stack([_rgba(w, h, 200 + 10 * step + f) for f in range(n)])).cuda().contiguous()
            got = _batch_outputs(enc, frames)
            fresh = HipTileEncoder(0)
            try:
                want = _batch_outputs(fresh, frames)
            finally:
                fresh.close()
            assert len(want["palette"]) == 7 * n and any(p.size for p in want["palette"])
            _same(got, want, f"step{step}:{n}frames")
    finally:
        enc.close()


# ---- decoder --------------------------------------------------------------------------------------------------------------------------------
def _pixels(planes_t):
    """torch int32 [..., 4, h, w] -> uint8 [..., h, w, 4] on the device"""
    import torch
    return planes_t.movedim(-3, -1).to(torch.uint8).contiguous()


def _decode_one(dec, enc, src, w, h, palette):
    import torch
    out = {}
    dec.begin(w, h)
    dec.decode_from_encoder(enc)                                                    # the gradient passes, then the 1-D chunk
    out["planes"], out["tile4"] = dec.planes(), dec.tile4x4()
    av = enc.alpha_values(True)
    if av is not None:
        out["alpha"] = dec.decompress_alpha(av["mode"], av["bbox"], av["payload"])  # the 'ALPM' chunk
    out["image"] = dec.image_device(channels=4).cpu().numpy()
    q = dec.compare_device(src, channels=4, tile_map=True)
    out["quality"] = {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in q.items() if not k.startswith("psnr")}   # the exact integers
    if palette:
        enc.palette_reset()
        pays = [enc.palette_payload_device(i) for i in range(enc.palette_compress())]
        lens = [int(enc.gradient_corners(p).size) for p in range(7)]
        n = dec.palette_decompress_streams(pays, lens, 250)
        out["palette_status"] = dec.palette_status()
        out["palette"] = [dec.palette_decoded(i) for i in range(n)]
    return out


def _decode_batch(dec, enc, src, w, h, n):
    out = {}
    dec.begin_batch(w, h, n)
    dec.decode_batch_from_encoder(enc, alpha=True)                                  # gradient passes, 1-D and 'ALPM' of every frame
    out["planes"] = []
    for f in range(n):
        dec.select_frame(f)
        out["planes"].append((dec.planes(), dec.tile4x4(), dec.alpha_plane()))
    out["image"] = dec.image_batch_device(channels=4, alpha_from_planes=True).cpu().numpy()
    qs = dec.compare_batch_device(src, channels=4)
    out["quality"] = [{k: np.asarray(v) for k, v in q.items() if not k.startswith("psnr")} for q in qs]
    return out


def test_decoder_walk():
    import torch
    from yaik_amd.decoder import HipTileDecoder
    from yaik_amd.encoder import HipTileEncoder
    steps = [(16, 16, 1), (136, 72, 1), (24, 8, 1), (136, 72, 4), (264, 136, 1)]
    dec, enc = HipTileDecoder(0), HipTileEncoder(0)
    try:
        for step, (w, h, n) in enumerate(steps):
            planes = torch.from_numpy(np.stack([_rgba(w, h, 300 + 10 * step + f) for f in range(n)])).cuda().contiguous()
            src = _pixels(planes)
            if n == 1:
                enc.set_image(planes[0])
                enc.mip_prefilter()
                enc.encode(3, False, False)
                run = lambda d: _decode_one(d, enc, src[0], w, h, palette=(step == 1))
            else:
                enc.set_batch(planes)
                enc.encode_batch(3, False)
                run = lambda d: _decode_batch(d, enc, src, w, h, n)
            got = run(dec)
            fresh = HipTileDecoder(0)
            try:
                want = run(fresh)
            finally:
                fresh.close()
            _same(got, want, f"step{step}:{w}x{h}x{n}")
    finally:
        dec.close()
        enc.close()


# ---- 3-D LUT search -------------------------------------------------------------------------------------------------------------------------
def _lut_outputs(enc, pats, planes, load):
    if load:
        enc.lut_clear()
        for k, p in enumerate(pats):
            assert enc.lut_load(p) == k
    enc.set_image(planes)
    enc.encode(3, False, False)
    enc.lut_start()
    out = {"matched": [enc.lut_search(sx, sy) for sx, sy in LUT_PASSES]}
    out["streams"] = enc.lut_streams()
    out["coverage"] = [enc.coverage_plane(p) for p in range(3)]
    return out


def test_lut_walk():
    from yaik_amd.encoder import HipTileEncoder
    pats = bank_patterns(2)
    enc = HipTileEncoder(0)
    try:
        # the bank is loaded at the first step and again, after yk_lut_clear, at the last
        for step, (w, h, load) in enumerate([(64, 64, True), (136, 72, False), (64, 64, False), (64, 64, True)]):
            planes = lut_image(w, h, pats, seed=400 + step)
            got = _lut_outputs(enc, pats, planes, load)
            fresh = HipTileEncoder(0)
            try:
                want = _lut_outputs(fresh, pats, planes, True)
            finally:
                fresh.close()
            assert sum(want["matched"]) > 0, (step, "the search matched nothing")
            _same(got, want, f"step{step}:{w}x{h}")
    finally:
        enc.close()
