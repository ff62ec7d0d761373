"""What every strip of the fused encode kernel does whatever its content -- the unit decode by multiply and shift (yk_udiv.h), the bitmap
words and run sums placed through the output table (yk_out_table_fill), the alpha stage's box and keep bytes read with the pixels, the run
sums of strips with nothing to code -- bit for bit, in every output bench.frame_outputs hands to a caller.

The reference is the CPU oracle wherever it has one.  Its alpha stage (MipPrefilter) exists for square images whose side is a power of two
only (the reference's recursion reads out of bounds otherwise), so: RGB images of every shape and RGBA images 16, 32, 64, 128 and 256 square
are compared with the oracle; RGBA images of other shapes with the test suite's independent first-generation kernel
(tests/csrc/yk_encode_v1.hip, which shares no code with yk_encode2.hip) run on the same planes.

Shapes: widths 64, 72, 136, 200, 320 with heights 16, 24, 40, 136 (1 to 5 blocks a row, 1 to 3 block rows, right and bottom edges that end
inside a block, inside a 32-pixel block, tile grids that are no multiple of 8 wide: the atomics instead of the run sums, and macro-tile rows
of 5, 9 and 13: keep bytes at every alignment); a batch of three 136x40 frames (the frame division) and frames of it encoded again on their
own (the table's frame offset); two stripes of a 136x104 image (y0, full_h, one halo row); alpha planes all zero, all opaque, one kept
macro-tile in the far corner, kept and rejected macro-tiles side by side, and the bench frame's frame and holes at 256x256 (oracle) and
320x320; the pixel cache on and off; the replayed graph; both kernel generations wherever the oracle is the reference, as in
test_gpu_gradfit_directed."""
import functools

import numpy as np
import pytest

from tests.images import edge_image

pytestmark = pytest.mark.gpu

WIDTHS, HEIGHTS = (64, 72, 136, 200, 320), (16, 24, 40, 136)


def _alpha(w, h, kind):
    y, x = np.mgrid[0:h, 0:w]
    if kind == "zero":
        return np.zeros((h, w), np.int32)
    if kind == "opaque":
        return np.full((h, w), 255, np.int32)
    if kind == "corner":                                                      # one kept macro-tile, the last one (a part tile where the sides end inside it)
        return np.where((x >= (w - 1) // 16 * 16) & (y >= (h - 1) // 16 * 16), 255, 0).astype(np.int32)
    if kind == "checker":                                                     # kept and rejected macro-tiles side by side in every strip; the last
        keep = ((x >> 4) + (y >> 4)) % 3 != 0                                 # column and row rejected: the kept box starts at (0, 0) and is not the
        if w > 16:                                                            # whole image, so rejected tiles are not coded and the keep bytes decide
            keep &= x < (w - 1) // 16 * 16
        if h > 16:
            keep &= y < (h - 1) // 16 * 16
        return np.where(keep, 255, 0).astype(np.int32)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def _planes(w, h, alpha, kind="mixed", seed=7):
    if alpha == "bench":
        from yaik_amd.synth import synth_planes
        return np.ascontiguousarray(synth_planes(w, h, n_planes=4), np.int32)
    if alpha is None:
        return np.ascontiguousarray(edge_image(w, h, kind, 3, seed=seed), np.int32)
    p = np.ascontiguousarray(edge_image(w, h, kind, 4, seed=seed), np.int32)
    p[3] = _alpha(w, h, alpha)
    return p


def _oracle_has_alpha_stage(w, h):
    return w == h and w >= 16 and (w & (w - 1)) == 0


_v1 = []                                                                      # the first-generation kernel's encoder, made on first use


def _v1_encoder():
    if not _v1:
        from tests.parity import encoder_for_kernel_version
        _v1.append(encoder_for_kernel_version(1))
    return _v1[0]


@pytest.fixture(scope="module", autouse=True)
def _close_v1():
    yield
    while _v1:
        _v1.pop().close()


@functools.lru_cache(maxsize=None)
def _want(w, h, alpha, kind="mixed", seed=7):
    """the reference results for the image, under the names of bench.frame_outputs; computed once"""
    from oracle.pyoracle import PASSES, OracleEncoder
    if alpha is not None and not _oracle_has_alpha_stage(w, h):
        from bench import frame_outputs
        e = _v1_encoder()
        _encode_single(e, _planes(w, h, alpha, kind, seed))
        return {k: np.array(v, copy=True) for k, v in frame_outputs(e).items()}
    ora = OracleEncoder(_planes(w, h, alpha, kind, seed))
    a = ora.mip_prefilter()
    out = {}
    if alpha is not None:                                                     # as tests/parity.py compares them
        out = {"alpha_bounds": np.asarray(a["bounds"]), "alpha_has_chunk_remaining": np.array([int(a["has_chunk"]), a["remaining"]])}
        if a["has_chunk"]:
            out["alpha_bitmap"], out["alpha_tile_bbox"] = np.asarray(a["bitmap"]), np.asarray(a["tile_bbox"])
    counts = []
    for p, (sx, sy) in enumerate(PASSES):
        cnt, bm, rgb = ora.fitting_quad_smooth(sx, sy)
        counts.append(cnt)
        out[f"gradient_bitmap_{p}"], out[f"gradient_corners_{p}"] = np.asarray(bm), np.asarray(rgb)
    out["gradient_counts"] = np.asarray(counts)
    for p in range(3):
        defs, nib, nn, _ = ora.dynamic_tile_encode(p, False)
        out[f"range_defs_{p}"], out[f"range_nibbles_{p}"], out[f"range_nibble_count_{p}"] = np.asarray(defs), np.asarray(nib), np.array([nn])
    return out


def _same(enc, want, what):
    from bench import frame_outputs
    got = frame_outputs(enc)
    assert set(want) <= set(got), (what, sorted(set(want) - set(got)))
    for k, v in want.items():
        g, v = np.asarray(got[k]).ravel(), np.asarray(v).ravel()
        assert g.shape == v.shape, (what, k, g.shape, v.shape)
        if not np.array_equal(g, v):
            idx = np.nonzero(g != v)[0]
            raise AssertionError((what, k, "differs at", idx[:6].tolist(), "of", int(idx.size), "got", g[idx[:6]].tolist(), "reference", v[idx[:6]].tolist()))


@pytest.fixture(scope="module", params=[2, 1], ids=["fused2", "v1"])
def hip_gen(request):
    from tests.parity import encoder_for_kernel_version
    e = encoder_for_kernel_version(request.param)
    yield e
    e.close()


@pytest.fixture(scope="module")
def hip():
    from yaik_amd.encoder import HipTileEncoder
    e = HipTileEncoder(0)
    yield e
    e.close()


def _encode_single(e, planes):
    e.set_image(planes)
    e.mip_prefilter()
    e.encode(3, False, False)


@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_shapes_rgb_against_the_oracle(hip_gen, oracle_built, w, h):
    _encode_single(hip_gen, _planes(w, h, None))
    _same(hip_gen, _want(w, h, None), (w, h))


@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_shapes_with_kept_and_rejected_macro_tiles(hip, oracle_built, w, h):
    _encode_single(hip, _planes(w, h, "checker"))
    _same(hip, _want(w, h, "checker"), (w, h, "checker"))


SQUARES = [(s, a) for s in (16, 32, 64, 128) for a in ("zero", "opaque", "corner", "checker")] + [(256, "bench")]


@pytest.mark.parametrize("side,alpha", SQUARES)
def test_alpha_planes_against_the_oracle(hip_gen, oracle_built, side, alpha):
    assert _oracle_has_alpha_stage(side, side)
    _encode_single(hip_gen, _planes(side, side, alpha))
    _same(hip_gen, _want(side, side, alpha), (side, alpha))


@pytest.mark.parametrize("w,h,alpha", [(136, 40, "zero"), (136, 40, "opaque"), (136, 40, "corner"), (320, 136, "zero"), (320, 136, "corner"),
                                       (200, 136, "opaque"), (72, 136, "corner"), (320, 320, "bench")])
def test_alpha_planes_other_shapes(hip, oracle_built, w, h, alpha):
    _encode_single(hip, _planes(w, h, alpha))
    _same(hip, _want(w, h, alpha), (w, h, alpha))


BATCHES = {"rgb": (("mixed", None, 7), ("noise", None, 8), ("ramp", None, 9)), "rgba": (("mixed", "checker", 7), ("noise", "corner", 8), ("ramp", "zero", 9))}


@pytest.mark.parametrize("which", sorted(BATCHES))
def test_batch_of_three_and_a_frame_on_its_own(hip, oracle_built, which):
    import torch
    batch = BATCHES[which]
    frames = torch.from_numpy(np.ascontiguousarray(np.stack([_planes(136, 40, a, k, s) for k, a, s in batch]))).cuda()
    hip.set_batch(frames)
    hip.encode_batch(3, False)
    for f, (k, a, s) in enumerate(batch):
        hip.select_frame(f)
        _same(hip, _want(136, 40, a, k, s), (which, "batch", "frame", f))
    for f in (2, 1):                                                         # the single-frame launch on a frame other than the first
        hip.select_frame(f)
        hip.mip_prefilter()
        hip.encode(3, False, False)
        for g, (k, a, s) in enumerate(batch):
            hip.select_frame(g)
            _same(hip, _want(136, 40, a, k, s), (which, "frame", f, "encoded alone; frame", g))


def test_two_stripes(oracle_built):
    from yaik_amd import distributed as ykd
    from yaik_amd.encoder import HipTileEncoder
    W, H = 136, 104
    planes, want = _planes(W, H, "checker"), _want(W, H, "checker")
    encs, boxes = [], []
    try:
        for y0, h, halo in ((0, 64, 1), (64, 40, 0)):
            e = HipTileEncoder(0)
            encs.append(e)
            e.set_image(np.ascontiguousarray(planes[:, y0:y0 + h + halo, :]), full_h=H, y0=y0, halo_rows=halo)
            e.alpha_reject()
            boxes.append(e.stripe_bbox())
        gb = ykd.combine_bboxes(boxes)
        abits, remaining = None, 0
        for e in encs:
            e.alpha_finish(gb)
            ar = e.alpha_result()
            assert np.array_equal(ar["bounds"], want["alpha_bounds"])
            abits = ar["bitmap"] if abits is None else (abits | ar["bitmap"])
            remaining += ar["remaining"]
            e.encode(3, False, False)
        assert np.array_equal(abits, want["alpha_bitmap"]) and remaining == int(want["alpha_has_chunk_remaining"][1])
        for p in range(7):
            assert np.array_equal(np.concatenate([e.gradient_bitmap(p) for e in encs]), want[f"gradient_bitmap_{p}"]), ("bitmap", p)
        assert np.array_equal(sum(e.gradient_counts() for e in encs), want["gradient_counts"])
        merged = ykd.merge_corner_streams([[e.gradient_corners(p) for p in range(7)] for e in encs], [e.gradient_corner_edges() for e in encs])
        for p in range(7):
            assert np.array_equal(merged[p], want[f"gradient_corners_{p}"]), ("corner stream", p)
        for p in range(3):
            parts = [e.range_streams(p) for e in encs]
            assert np.array_equal(np.concatenate([d for d, _, _ in parts]), want[f"range_defs_{p}"]), ("defs", p)
            cat, total = ykd.concat_nibble_streams([n for _, n, _ in parts], [nn for _, _, nn in parts])
            assert total == int(want[f"range_nibble_count_{p}"][0]) and np.array_equal(cat, want[f"range_nibbles_{p}"]), ("nibbles", p)
    finally:
        for e in encs:
            e.close()


@pytest.mark.parametrize("w,h,alpha", [(200, 136, "checker"), (72, 24, "corner")])
def test_pixel_cache_on_and_off(hip, oracle_built, w, h, alpha):
    streams = {}
    for on in (False, True):
        hip.set_pixel_cache(on)
        try:
            _encode_single(hip, _planes(w, h, alpha))
            _same(hip, _want(w, h, alpha), (w, h, alpha, "pixel cache", on))
            streams[on] = hip.dynamic_tile_compressor()
        finally:
            hip.set_pixel_cache(False)
    for a, b in zip(streams[False], streams[True]):
        assert np.array_equal(a, b), (w, h, alpha, "1-D streams with and without the pixel cache")


@pytest.mark.parametrize("w,h,alpha", [(320, 320, "bench"), (136, 40, "corner")])
def test_graph_replay(hip, oracle_built, w, h, alpha):
    hip.set_image(_planes(w, h, alpha))
    for turn in range(2):                                                    # the second is a replay
        hip.encode_frame(3, False)
        _same(hip, _want(w, h, alpha), (w, h, alpha, "encode_frame", turn))
