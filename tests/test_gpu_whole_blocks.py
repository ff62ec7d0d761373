"""The fused encode kernel's instantiation for one whole image whose sides are multiples of 64 (WHOLE) against the
general instantiation in the same library and against the CPU oracle, byte for byte.

Every case is encoded three times: by the product library (the path yk_launch_encode2 selects by itself, pixel cache off), and by the test
build of the library with and without the hook that forces the general instantiation (yk_set_ablation 32; pixel cache on).  In front of each
encode the handle encodes noise of the same shape, so that nothing a path fails to store can survive from the run before it.  Compared:
everything bench.frame_outputs hands to a caller (the seven bitmaps with the 16x16 bytes folded in, corner streams, tile records and nibble
slots as the packed range streams, whose offsets are the run sums), the coverage words, and the live 1-D streams (with the cache on they are
made from the pixel cache the kernel filled).  The oracle is the reference wherever it has one: every RGB shape, and RGBA at 256x256 (its
alpha stage exists for square powers of two only).

Shapes: 64x64 (one block: the halo column's, the halo row's and the corner sample's clamp all act), 128x64, 64x128, 192x192 (interior and edge
blocks), 72x64 and 64x72 (the selector falls back: both runs take the general kernel and still agree with the oracle).  Content: noise, mild
noise (the range phase's input depends on the clamped halo through the gradient passes), ramp next to mild noise; rejectFactor 0, 3, 64.
Alpha planes at 256x256: see ALPHA_CASES (all sixteen keep patterns of a strip, a box that is the whole image, no alpha at all, boxes whose
edges cut strips, the zero-size quirk, strips with nothing to code); the case builder is checked on the CPU against the oracle's alpha stage,
with a model of the rule that sorts strips into scalar and per-lane liveness.  Boxes at 8-pixel steps: FORCED_BOXES at the end."""
import functools

import numpy as np
import pytest

SHAPES = ((64, 64), (128, 64), (64, 128), (192, 192), (72, 64), (64, 72))
CONTENTS = ("noise", "mild", "ramp_mild")
REJECT_FACTORS = (0, 3, 64)
SIDE = 256                                                                    # the alpha cases


def qualifies(w, h):
    return w % 64 == 0 and h % 64 == 0


@functools.lru_cache(maxsize=None)
def content(w, h, kind, seed=11):
    """[3, h, w] int32 in 0..255"""
    rng = np.random.default_rng(seed + 131 * w + h)
    y, x = np.mgrid[0:h, 0:w]
    ramp = np.stack([(255 * x) // w, (255 * y) // h, (255 * (x + y)) // (w + h)])
    mild = (ramp + rng.integers(0, 8, (3, h, w))) % 256
    if kind == "noise":
        out = rng.integers(0, 256, (3, h, w))
    elif kind == "mild":
        out = mild
    elif kind == "ramp_mild":                                                 # 32-pixel squares: every strip has ramp beside and above mild noise
        out = np.where((((x >> 5) + (y >> 5)) & 1).astype(bool)[None], mild, ramp)
    elif kind == "ramp_noise":                                                # left half ramp, right half noise
        out = np.where((x >= w // 2)[None], rng.integers(0, 256, (3, h, w)), ramp)
    else:
        raise ValueError(kind)
    out = np.ascontiguousarray(out, np.int32)
    out.setflags(write=False)
    return out


def _rect(x0, y0, x1, y1):
    a = np.zeros((SIDE, SIDE), np.int32)
    a[y0:y1, x0:x1] = 255
    return a


def _keep_patterns():
    """strip row s (16 of them), block column 0: macro-tile q kept when bit q of 15 - s is set -- all sixteen patterns of a strip's four keep
    bytes; block column 1 kept, column 2 kept in every other strip row, column 3 empty: the kept box (the alpha stage forms it from whole
    macro-tiles) is [0, 192) x [0, 256), not the whole image, so the keep bytes decide, and the strips of block column 3 lie outside it"""
    a = np.zeros((SIDE, SIDE), np.int32)
    for s in range(16):
        for q in range(4):
            if ((15 - s) >> q) & 1:
                a[16 * s:16 * s + 16, 16 * q:16 * q + 16] = 255
        a[16 * s:16 * s + 16, 64:128] = 255
        if s & 1:
            a[16 * s:16 * s + 16, 128:192] = 255
    return a


def _corners_only():
    a = np.zeros((SIDE, SIDE), np.int32)
    a[0, 0] = a[SIDE - 1, SIDE - 1] = 255
    return a


def _top_left():
    a = _rect(0, 0, 192, 128)
    a[255, 100] = 255                                                         # the box reaches the last row: [0, 192) x [0, 256)
    return a


# name -> (alpha plane, content kind)
ALPHA_CASES = {
    "keep_patterns": (_keep_patterns, "ramp_mild"),
    "discard": (_corners_only, "ramp_mild"),            # the kept box is the whole image: every reject is discarded, the keep bytes (nearly all zero) do not count
    "zero": (lambda: np.zeros((SIDE, SIDE), np.int32), "noise"),
    "cut_from_origin": (lambda: _rect(0, 0, 170, 200), "mild"),      # the box's right edge, [0, 176) x [0, 208), cuts the strips of block column 2
    "cut_all_round": (lambda: _rect(82, 40, 170, 200), "mild"),      # [80, 176) x [32, 208): both side edges cut strips, and the box is away from the origin
    "quirk": (lambda: _rect(128, 64, 192, 128), "mild"),             # a 64x64 box at (128, 64): tgx + 8 <= cw fails for every tile inside it
    "tails": (_top_left, "ramp_noise"),                 # kept strips a ramp covers completely; rejected strips of noise, nothing covered
}


@functools.lru_cache(maxsize=None)
def alpha_planes(name):
    make, kind = ALPHA_CASES[name]
    p = np.ascontiguousarray(np.concatenate([content(SIDE, SIDE, kind), make()[None]]), np.int32)
    p.setflags(write=False)
    return p


def strip_classes(bounds, alpha, w, h):
    """What the launcher's selector and the WHOLE kernel's scalar preamble decide for every strip, from the alpha stage's box: a model of
    the rule, not of the kernel.  Returns {(BX, stripRow): class}: 'discard' / 'inbox:<keep pattern>' / 'crossed' (some tile of the strip
    fails the box test: per-lane liveness) / 'quirk' (crossed only because of the zero-size rule's terms)."""
    b0, b1, b2, b3 = (int(v) for v in bounds[:4])
    discard = (b0, b1, b2, b3) == (0, 0, w, h)
    cx, cy = b0 >> 3 << 3, b1 >> 3 << 3
    cw, ch = ((b2 + 7) >> 3 << 3) - cx, ((b3 + 7) >> 3 << 3) - cy
    out = {}
    for sr in range(h // 16):
        for bx in range(w // 64):
            x0, y0 = 64 * bx, 16 * sr
            plain = x0 >= cx and x0 + 56 < cx + cw and y0 >= cy and y0 + 8 < cy + ch
            quirk = x0 + 64 <= cw and y0 + 16 <= ch
            if plain and quirk:
                keep = sum(1 << q for q in range(4) if alpha[y0:y0 + 16, x0 + 16 * q:x0 + 16 * q + 16].any())
                out[bx, sr] = "discard" if discard else f"inbox:{keep}"
            else:
                out[bx, sr] = "quirk" if plain else "crossed"
    return out


# ---- the case builder, on the CPU ---------------------------------------------------------------------------------------------------------
def test_case_builder_rgb():
    for w, h in SHAPES:
        for kind in CONTENTS:
            p = content(w, h, kind)
            assert p.shape == (3, h, w) and p.dtype == np.int32 and p.min() >= 0 and p.max() <= 255
    assert [qualifies(w, h) for w, h in SHAPES] == [True, True, True, True, False, False]
    p = content(64, 64, "ramp_mild")
    ramp = content(64, 64, "mild")                                            # the same generator state: mild = ramp + noise below 8
    assert not np.array_equal(p[:, :32, :32], ramp[:, :32, :32]) and np.array_equal(p[:, :32, 32:], ramp[:, :32, 32:])


def test_case_builder_alpha(oracle_built):
    from oracle.pyoracle import OracleEncoder
    got = {}
    for name in ALPHA_CASES:
        p = alpha_planes(name)
        a = OracleEncoder(p).mip_prefilter()
        got[name] = (a, strip_classes(np.asarray(a["bounds"]), p[3], SIDE, SIDE))
    cls = {name: set(c.values()) for name, (_, c) in got.items()}
    assert {f"inbox:{k}" for k in range(16)} <= cls["keep_patterns"] and "crossed" in cls["keep_patterns"]
    assert cls["discard"] == {"discard"}
    assert np.asarray(got["cut_from_origin"][0]["bounds"])[:4].tolist() == [0, 0, 176, 208]
    assert {"crossed"} <= cls["cut_from_origin"] and any(c.startswith("inbox") for c in cls["cut_from_origin"])
    assert np.asarray(got["cut_all_round"][0]["bounds"])[:4].tolist() == [80, 32, 176, 208] and "crossed" in cls["cut_all_round"]
    # the box's own four strips pass the plain test and fail the zero-size terms; nothing is in the box on the scalar path
    quirk = got["quirk"][1]
    assert [k for k, c in quirk.items() if c == "quirk"] == [(2, sr) for sr in range(4, 8)] and not any(c.startswith("inbox") for c in quirk.values())
    tails = got["tails"][1]
    assert tails[0, 0] == "inbox:15" and tails[2, 12] == "inbox:0"


# ---- on the GPU ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def encoders():
    from yaik_amd.encoder import HipTileEncoder
    product, hooked = HipTileEncoder(0), HipTileEncoder(0, hooks=True)
    hooked.set_pixel_cache(True)
    yield product, hooked
    from yaik_amd._lib import test_lib
    test_lib().yk_set_ablation(hooked._h, 0)
    product.close()
    hooked.close()


@functools.lru_cache(maxsize=None)
def _dirt(n, w, h):
    p = np.concatenate([content(w, h, "noise", seed=5), np.full((1, h, w), 255, np.int32)])[:n]
    return np.ascontiguousarray(p, np.int32)


def _outputs(enc, planes, rf, box=None):
    from bench import frame_outputs
    for p in (_dirt(*planes.shape[0:1], planes.shape[2], planes.shape[1]), planes):
        enc.set_image(p)
        if box is None or p is not planes:
            enc.mip_prefilter()
        else:                                                                 # a kept box handed in by the caller, as a stripe's is
            enc.alpha_reject()
            enc.alpha_finish(np.asarray(box, np.int32))
        enc.encode(rf, False, False)
    out = {k: np.array(v, copy=True) for k, v in frame_outputs(enc).items()}
    out["coverage"] = enc.coverage().copy()
    out["pix_1d"], out["type_1d"] = enc.dynamic_tile_compressor()
    return out


def _same(got, want, what):
    assert set(want) <= set(got), (what, sorted(set(want) - set(got)))
    for k, v in want.items():
        g, v = np.asarray(got[k]).ravel(), np.asarray(v).ravel()
        assert g.shape == v.shape, (what, k, g.shape, v.shape)
        if not np.array_equal(g, v):
            idx = np.nonzero(g != v)[0]
            raise AssertionError((what, k, "differs at", idx[:6].tolist(), "of", int(idx.size), "got", g[idx[:6]].tolist(), "reference", v[idx[:6]].tolist()))


def _three_ways(encoders, planes, rf, what, box=None):
    """the product library's own choice, the test build's own choice and the test build's general kernel: all outputs equal; returns them"""
    from yaik_amd._lib import test_lib
    product, hooked = encoders
    outs = []
    for enc, flag in ((product, None), (hooked, 0), (hooked, 32)):
        if flag is not None:
            assert test_lib().yk_set_ablation(enc._h, flag) == 0
        outs.append(_outputs(enc, planes, rf, box))
    _same(outs[1], outs[2], (what, "own choice against the forced general kernel"))
    _same(outs[0], outs[2], (what, "product library against the forced general kernel"))
    return outs[0]


@functools.lru_cache(maxsize=None)
def _oracle(key, rf):
    """the oracle's results under the names of bench.frame_outputs; key = (w, h, kind) or an alpha case's name"""
    from oracle.pyoracle import PASSES, OracleEncoder
    planes = alpha_planes(key) if isinstance(key, str) else content(*key)
    ora = OracleEncoder(planes)
    a = ora.mip_prefilter()
    out = {}
    if planes.shape[0] == 4:
        out = {"alpha_bounds": np.asarray(a["bounds"]), "alpha_has_chunk_remaining": np.array([int(a["has_chunk"]), a["remaining"]])}
        if a["has_chunk"]:
            out["alpha_bitmap"], out["alpha_tile_bbox"] = np.asarray(a["bitmap"]), np.asarray(a["tile_bbox"])
    counts = []
    for p, (sx, sy) in enumerate(PASSES):
        cnt, bm, rgb = ora.fitting_quad_smooth(sx, sy, rf)
        counts.append(cnt)
        out[f"gradient_bitmap_{p}"], out[f"gradient_corners_{p}"] = np.asarray(bm), np.asarray(rgb)
    out["gradient_counts"] = np.asarray(counts)
    for p in range(3):
        defs, nib, nn, _ = ora.dynamic_tile_encode(p, False)
        out[f"range_defs_{p}"], out[f"range_nibbles_{p}"], out[f"range_nibble_count_{p}"] = np.asarray(defs), np.asarray(nib), np.array([nn])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rf", REJECT_FACTORS)
@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_rgb_shapes(encoders, oracle_built, w, h, kind, rf):
    got = _three_ways(encoders, content(w, h, kind), rf, (w, h, kind, rf))
    _same(got, _oracle((w, h, kind), rf), (w, h, kind, rf, "against the oracle"))


@pytest.mark.gpu
@pytest.mark.parametrize("rf", REJECT_FACTORS)
@pytest.mark.parametrize("name", sorted(ALPHA_CASES))
def test_alpha_cases(encoders, oracle_built, name, rf):
    got = _three_ways(encoders, alpha_planes(name), rf, (name, rf))
    _same(got, _oracle(name, rf), (name, rf, "against the oracle"))
    if name == "tails" and rf == 3:
        # what the case is for: a kept strip the gradient tiles cover completely and a rejected strip with uncovered cells both have no valid lane
        cov = got["coverage"]
        assert cov[0:4, 0:16].all() and not cov[48:52, 32:48].any()


# The alpha stage's own box is made of whole macro-tiles, so its edges cut a strip at 16-pixel steps and never in y.  A box at 8-pixel steps in
# x and in y is handed in the way a stripe's caller hands in the combined box (alpha_finish); the oracle has no such entry, so these cases
# compare the two instantiations only.  The last one is a quirk box away from the origin whose edges are no macro-tile's.
FORCED_BOXES = ((72, 40, 184, 200), (8, 8, 248, 248), (0, 0, 184, 200), (136, 72, 184, 120))


@pytest.mark.gpu
@pytest.mark.parametrize("box", FORCED_BOXES)
def test_boxes_at_8_pixel_steps(encoders, box):
    planes = np.ascontiguousarray(np.concatenate([content(SIDE, SIDE, "mild"), _rect(*box)[None]]), np.int32)
    _three_ways(encoders, planes, 3, ("forced box", box), box=box)
