"""8-bit interleaved RGB(A) pixels widened on the GPU (yk_upload_pixels_u8 / yk_load_device_pixels_u8 behind HipTileEncoder.set_image_u8 /
set_batch_u8, EncoderContext::LoadImagePixels in C++): every result must equal, exactly, the one of the same image fed as int32 planes through
the existing entry points (yk_upload_planes, yk_bind_device_planes, yk_bind_device_batch)."""
import ctypes as C
import os
import struct
import subprocess
import tempfile

import numpy as np
import pytest

from yaik_amd._lib import YaikError, lib
from yaik_amd.encoder import HipTileEncoder
from yaik_amd.synth import synth_planes, synth_planes_torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "yaik_amd", "host", "host_driver")
YK_ERR_BAD_ARG, YK_ERR_STATE, YK_STAGE_UNPACK = -2, -4, 7

KINDS = {"rgb": (3, 3, 3), "rgba": (4, 4, 4), "rgba3": (4, 4, 3)}      # planes of the image, bytes per pixel, planes loaded
# (extra bytes per row, or None = the row rounded up to 16 bytes + 32; byte offset of the first pixel)
LAYOUTS = {"tight": (0, 0), "padded": (None, 0), "offset1": (0, 1), "offset3": (5, 3)}


def _image(w, h, n, seed=12345):
    if w * h >= 1 << 22:
        return synth_planes_torch(w, h, n_planes=n, seed=seed, device="cuda").cpu().numpy()
    return synth_planes(w, h, n_planes=n, seed=seed)


def _pixels(planes, channels, layout):
    """int32 planes [n, h, w] -> (buffer, uint8 view [h, w, channels] into it); row padding and channels beyond n hold noise."""
    n, h, w = planes.shape
    pad, offset = LAYOUTS[layout]
    row = (w * channels + 15) // 16 * 16 + 32 if pad is None else w * channels + pad
    buf = np.random.default_rng(w + h).integers(0, 256, offset + row * h, dtype=np.uint8)
    view = np.ndarray((h, w, channels), np.uint8, buf, offset, (row, channels, 1))
    view[..., :n] = np.moveaxis(planes, 0, -1)
    return buf, view


def _source(buf, view, where):
    """the numpy view itself, or the same bytes in HBM as a torch view with the same offset and strides"""
    if where == "host":
        return view
    import torch
    off = view.ctypes.data - buf.ctypes.data
    return torch.as_strided(torch.from_numpy(buf).cuda(), view.shape, view.strides, off)


def _grab(out, name, fn):
    try:
        out[name] = fn()
    except YaikError as e:                                       # a refusal must be the same refusal on both paths
        out[name] = ("error", str(e).split(":")[0])


def _outputs(enc, n, full=True):
    """Everything the tile path produces from the bound planes."""
    out = {}
    enc.set_pixel_cache(False)
    if n == 4:
        _grab(out, "alpha", enc.mip_prefilter)
        if full:
            _grab(out, "alpha_values8", lambda: enc.alpha_values(True))
            _grab(out, "alpha_values6", lambda: enc.alpha_values(False))
    _grab(out, "encode", lambda: enc.encode(3, False, full))
    for i in range(7):
        _grab(out, f"bitmap{i}", lambda i=i: enc.gradient_bitmap(i))
    _grab(out, "counts", enc.gradient_counts)
    _grab(out, "coverage", enc.coverage)
    for p in range(3):
        _grab(out, f"range{p}", lambda p=p: enc.range_streams(p))
    if full:
        for p in range(3):
            _grab(out, f"dst{p}", lambda p=p: enc.range_dst(p))
        for i in range(7):
            _grab(out, f"corners{i}", lambda i=i: enc.gradient_corners(i))
        _grab(out, "d1", enc.dynamic_tile_compressor)
        enc.set_pixel_cache(True)                                # the 1-D path again, from the fused kernel's pixel cache
        _grab(out, "encode_cached", lambda: enc.encode(3, False, False))
        _grab(out, "d1_cached", enc.dynamic_tile_compressor)
        enc.set_pixel_cache(False)
    return out


def _maps(enc, n):
    """The tile maps of the last encode (no new encode)."""
    out = {}
    if n == 4:
        _grab(out, "alpha", enc.alpha_result)
    for i in range(7):
        _grab(out, f"bitmap{i}", lambda i=i: enc.gradient_bitmap(i))
    _grab(out, "counts", enc.gradient_counts)
    _grab(out, "coverage", enc.coverage)
    for p in range(3):
        _grab(out, f"range{p}", lambda p=p: enc.range_streams(p))
    return out


def _same(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray):
        return isinstance(b, np.ndarray) and a.shape == b.shape and np.array_equal(a, b)
    return a == b


def _diff(got, want):
    return [k for k in want if not _same(got.get(k), want[k])]


def _ran(want):
    """Every output of the int32 path is a result, not a refusal: an output refused on both paths would compare equal and test nothing."""
    refused = [k for k, v in want.items() if isinstance(v, tuple) and len(v) == 2 and isinstance(v[0], str) and v[0] == "error"]
    assert not refused, refused
    return want


def _reference(planes, n_planes, full=True):
    a = HipTileEncoder(0)
    try:
        a.set_image(np.ascontiguousarray(planes[:n_planes]))
        want = _outputs(a, n_planes, full)
    finally:
        a.close()
    return _ran(want)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("w,h", [(8, 8), (72, 40), (264, 136)])
def test_every_layout_and_source_equals_the_int32_path(w, h, kind):
    """RGB, RGBA, RGBA into 3 planes; tight rows, padded rows, bases at byte offsets 1 and 3; uploaded from the host and read in HBM."""
    n_img, ch, npl = KINDS[kind]
    planes = _image(w, h, n_img, seed=w * 7 + h)
    want = _reference(planes, npl)
    b = HipTileEncoder(0)
    try:
        for layout in LAYOUTS:
            buf, view = _pixels(planes, ch, layout)
            for src in ("host", "torch"):
                b.set_image_u8(_source(buf, view, src), n_planes=npl)
                bad = _diff(_outputs(b, npl), want)
                assert not bad, (layout, src, bad)
    finally:
        b.close()


@pytest.mark.parametrize("kind", list(KINDS))
def test_full_hd(kind):
    n_img, ch, npl = KINDS[kind]
    planes = _image(1920, 1080, n_img, seed=1080)
    want = _reference(planes, npl)
    b = HipTileEncoder(0)
    try:
        for layout in ("tight", "padded", "offset1"):
            buf, view = _pixels(planes, ch, layout)
            for src in ("host", "torch"):
                b.set_image_u8(_source(buf, view, src), n_planes=npl)
                bad = _diff(_outputs(b, npl), want)
                assert not bad, (layout, src, bad)
    finally:
        b.close()


@pytest.mark.parametrize("w,kind,layout,sources", [(4096, "rgba", "tight", ("host", "torch")), (4096, "rgb", "padded", ("torch",)),
                                                   (4096, "rgba3", "offset3", ("host",)), (8192, "rgba", "tight", ("host", "torch"))])
def test_large_images(w, kind, layout, sources):
    """4096^2 and 8192^2: alpha result, the seven bitmaps, counts, coverage and the range streams."""
    n_img, ch, npl = KINDS[kind]
    planes = _image(w, w, n_img, seed=w + 1)
    want = _reference(planes, npl, full=False)
    buf, view = _pixels(planes, ch, layout)
    del planes
    b = HipTileEncoder(0)
    try:
        for src in sources:
            b.set_image_u8(_source(buf, view, src), n_planes=npl)
            bad = _diff(_outputs(b, npl, full=False), want)
            assert not bad, (src, bad)
    finally:
        b.close()


@pytest.mark.parametrize("n_img", [4, 3])
def test_row_stripes_from_pixels_equal_the_whole_image(n_img):
    """Two row stripes (the first with its halo row), each loaded from a row-sliced view of one 8-bit image (no copy), concatenate to the
    whole image's int32 encode."""
    from yaik_amd import distributed as ykd
    planes = _image(512, 512, n_img, seed=99)
    n, H, W = planes.shape
    whole = HipTileEncoder(0)
    whole.set_image(planes)
    walpha = whole.mip_prefilter() if n == 4 else None
    whole.encode(3, False, False)
    wbm = [whole.gradient_bitmap(i) for i in range(7)]
    wcov, wrange, wcorners = whole.coverage(), [whole.range_streams(p) for p in range(3)], [whole.gradient_corners(i) for i in range(7)]
    whole.close()
    buf, view = _pixels(planes, n, "padded")
    encs, boxes = [], []
    for r in range(2):
        y0, h, halo = ykd.stripe_rows(H, 2, r)
        e = HipTileEncoder(0)
        src = _source(buf, view, "host" if r == 0 else "torch")
        e.set_image_u8(src[y0:y0 + h + halo], full_h=H, y0=y0, halo_rows=halo)
        if n == 4:
            e.alpha_reject()
            boxes.append(e.stripe_bbox())
        encs.append(e)
    gb = ykd.combine_bboxes(boxes) if n == 4 else None
    bitmaps, covs, defs, nibs, nns = [[] for _ in range(7)], [], [[], [], []], [[], [], []], [[], [], []]
    corner_streams, corner_edges, abits, remaining = [], [], None, 0
    for e in encs:
        if n == 4:
            e.alpha_finish(gb)
            ar = e.alpha_result()
            abits = ar["bitmap"] if abits is None else (abits | ar["bitmap"])
            remaining += ar["remaining"]
            assert np.array_equal(ar["bounds"], walpha["bounds"])
        e.encode(3, False, False)
        for i in range(7):
            bitmaps[i].append(e.gradient_bitmap(i))
        covs.append(e.coverage())
        corner_streams.append([e.gradient_corners(i) for i in range(7)])
        corner_edges.append(e.gradient_corner_edges())
        for p in range(3):
            d, nb, nn = e.range_streams(p)
            defs[p].append(d); nibs[p].append(nb); nns[p].append(nn)
        e.close()
    for i in range(7):
        assert np.array_equal(np.concatenate(bitmaps[i]), wbm[i]), f"bitmap {i}"
    assert np.array_equal(np.concatenate(covs, axis=0), wcov)
    for p in range(3):
        wd, wn, wnn = wrange[p]
        assert np.array_equal(np.concatenate(defs[p]), wd)
        cat, total = ykd.concat_nibble_streams(nibs[p], nns[p])
        assert total == wnn and np.array_equal(cat, wn)
    merged = ykd.merge_corner_streams(corner_streams, corner_edges)
    for i in range(7):
        assert np.array_equal(merged[i], wcorners[i]), f"corner stream {i}"
    if n == 4:
        assert np.array_equal(abits, walpha["bitmap"]) and remaining == walpha["remaining"]


@pytest.mark.parametrize("layout,kind", [("tight", "rgba"), ("padded", "rgb"), ("offset1", "rgba3")])
def test_batch_from_pixels_equals_set_batch(layout, kind):
    """F = 4 frames: set_batch_u8 (one unpack launch for every frame) == set_batch on int32 planes, frame by frame."""
    import torch
    F, w, h = 4, 256, 192
    n_img, ch, npl = KINDS[kind]
    host = [_image(w, h, n_img, seed=500 + f) for f in range(F)]
    a, b = HipTileEncoder(0), HipTileEncoder(0)
    try:
        a.set_batch(torch.from_numpy(np.stack([p[:npl] for p in host])).cuda())
        a.encode_batch(3, False)
        row_pad, frame_pad, offset = {"tight": (0, 0, 0), "padded": (48, 4096, 0), "offset1": (0, 0, 1)}[layout]
        row = w * ch + row_pad
        fstride = h * row + frame_pad
        buf = np.random.default_rng(3).integers(0, 256, offset + F * fstride, dtype=np.uint8)
        view = np.ndarray((F, h, w, ch), np.uint8, buf, offset, (fstride, row, ch, 1))
        for f in range(F):
            view[f, ..., :n_img] = np.moveaxis(host[f], 0, -1)
        frames = torch.as_strided(torch.from_numpy(buf).cuda(), view.shape, view.strides, offset)
        b.set_batch_u8(frames, n_planes=npl)
        b.encode_batch(3, False)
        for f in range(F):
            a.select_frame(f); b.select_frame(f)
            want, got = _ran(_maps(a, npl)), _maps(b, npl)
            for i in range(7):
                want[f"corners{i}"], got[f"corners{i}"] = a.gradient_corners(i), b.gradient_corners(i)
            bad = _diff(got, want)
            assert not bad, (f, bad)
    finally:
        a.close(); b.close()


@pytest.mark.parametrize("src", ["host", "torch"])
@pytest.mark.parametrize("n_img", [4, 3])
def test_encode_frame_replays_see_new_pixels(n_img, src):
    """Image A, encode_frame, image B of the same shape into the same handle, encode_frame: the owned planes keep their address, so the replayed
    graph must read B's pixels and give a fresh int32 encode of B."""
    A, B = _image(256, 256, n_img, seed=1), _image(256, 256, n_img, seed=2)
    ref = HipTileEncoder(0)
    e = HipTileEncoder(0)
    try:
        ref.set_image(B)
        ref.encode_frame(3, False)
        want = _ran(_maps(ref, n_img))
        bufA, viewA = _pixels(A, n_img, "tight")
        bufB, viewB = _pixels(B, n_img, "tight")
        e.set_image_u8(_source(bufA, viewA, src))
        e.encode_frame(3, False)
        assert _diff(_maps(e, n_img), want)                        # A's maps are not B's: the comparison below means something
        e.set_image_u8(_source(bufB, viewB, src))
        e.encode_frame(3, False)
        bad = _diff(_maps(e, n_img), want)
        assert not bad, bad
    finally:
        ref.close(); e.close()


def test_int32_and_8bit_entry_points_alternate_on_one_handle():
    imgs = {"A": _image(264, 136, 4, seed=11), "B": _image(264, 136, 4, seed=12), "C": _image(512, 192, 3, seed=13)}
    want = {k: _reference(v, v.shape[0]) for k, v in imgs.items()}
    e = HipTileEncoder(0)
    try:
        for k, how in (("A", "planes"), ("B", "host"), ("A", "torch"), ("C", "host"), ("B", "planes"), ("C", "torch"), ("A", "host")):
            planes = imgs[k]
            if how == "planes":
                e.set_image(planes)
            else:
                buf, view = _pixels(planes, planes.shape[0], "padded")
                e.set_image_u8(_source(buf, view, how))
            bad = _diff(_outputs(e, planes.shape[0]), want[k])
            assert not bad, (k, how, bad)
    finally:
        e.close()


@pytest.mark.parametrize("n_img", [3, 4])
def test_decode_from_the_8bit_encoder(n_img):
    from yaik_amd.decoder import HipTileDecoder
    planes = _image(256, 192, n_img, seed=7)
    a, b = HipTileEncoder(0), HipTileEncoder(0)
    images = []
    try:
        a.set_image(planes)
        b.set_image_u8(np.ascontiguousarray(np.moveaxis(planes, 0, -1).astype(np.uint8)))
        for e in (a, b):
            if n_img == 4:
                e.mip_prefilter()
            e.encode(3, False, False)
            d = HipTileDecoder(0)
            d.begin(256, 192)
            d.decode_from_encoder(e)
            images.append(d.image())
            d.close()
    finally:
        a.close(); b.close()
    assert np.array_equal(images[0], images[1])


def test_unpack_stage_is_timed():
    e = HipTileEncoder(0)
    try:
        e.stage_ms(YK_STAGE_UNPACK)
        buf, view = _pixels(_image(256, 256, 4), 4, "tight")
        e.set_image_u8(view)
        e.set_image_u8(_source(buf, view, "torch"))
        ms, n = e.stage_ms(YK_STAGE_UNPACK)
        assert n == 2 and ms > 0.0
    finally:
        e.close()


def test_refusals_leave_no_planes_bound():
    import torch
    L = lib()
    w = h = 64
    px4, px3 = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 3), np.uint8)
    d4 = torch.zeros((2, h, w, 4), dtype=torch.uint8, device="cuda")
    hp = lambda a: C.c_void_p(a.ctypes.data)
    dp = C.c_void_p(d4.data_ptr())
    e = HipTileEncoder(0)
    try:
        c = e._h
        assert L.yk_upload_pixels_u8(c, hp(px4), w * 4, 4) == YK_ERR_STATE                  # before yk_set_image
        assert L.yk_load_device_pixels_u8(c, dp, w * 4, 0, 4) == YK_ERR_STATE

        def bound():
            n = C.c_size_t()
            rc = L.yk_validate_planes(c, C.byref(n))
            assert rc in (0, YK_ERR_STATE)
            return rc == 0

        cases = [("null host", lambda: L.yk_upload_pixels_u8(c, None, w * 4, 4)),
                 ("null device", lambda: L.yk_load_device_pixels_u8(c, None, w * 4, 0, 4)),
                 ("2 channels", lambda: L.yk_upload_pixels_u8(c, hp(px4), w * 4, 2)),
                 ("5 channels", lambda: L.yk_load_device_pixels_u8(c, dp, w * 4, 0, 5)),
                 ("3 channels, 4 planes", lambda: L.yk_upload_pixels_u8(c, hp(px3), w * 3, 3)),
                 ("3 channels, 4 planes (device)", lambda: L.yk_load_device_pixels_u8(c, dp, w * 3, 0, 3)),
                 ("short rows", lambda: L.yk_upload_pixels_u8(c, hp(px4), w * 4 - 1, 4)),
                 ("short rows (device)", lambda: L.yk_load_device_pixels_u8(c, dp, w * 4 - 4, 0, 4))]
        for name, call in cases:
            e.set_image_u8(px4)
            assert bound(), name
            assert call() == YK_ERR_BAD_ARG, name
            assert not bound(), name
        # batches: the host entry refuses them, the device entry wants frames that do not overlap
        e.set_batch_u8(d4)
        assert bound()
        assert L.yk_upload_pixels_u8(c, hp(px4), w * 4, 4) == YK_ERR_STATE
        assert not bound()
        e.set_batch_u8(d4)
        assert L.yk_load_device_pixels_u8(c, dp, w * 4, w * 4 * h - 16, 4) == YK_ERR_BAD_ARG
        assert not bound()
        e.set_batch_u8(d4)                                                                # and a good call binds again
        assert bound()
    finally:
        e.close()


def _driver(planes, form):
    if not os.path.exists(DRIVER):
        subprocess.run(["make", "-C", os.path.dirname(DRIVER)], check=True)
    n, h, w = planes.shape
    with tempfile.TemporaryDirectory() as d:
        fin, fout, fy = os.path.join(d, "in.bin"), os.path.join(d, "out.blobs"), os.path.join(d, "out.yaik")
        with open(fin, "wb") as f:
            f.write(struct.pack("<3i", w, h, n)); f.write(np.ascontiguousarray(planes, np.int32).tobytes())
        subprocess.run([DRIVER, fin, fout, form, fy], check=True)
        from oracle.refrun import parse_blobs
        with open(fy, "rb") as f:
            return parse_blobs(fout), f.read()


@pytest.mark.parametrize("n_img", [4, 3])
def test_cpp_load_image_pixels_writes_the_same_file(n_img):
    """host_driver ... pixels (LoadImagePixels on padded 8-bit rows) writes the .yaik file and every blob of the default form, byte for byte."""
    planes = _image(256, 192, n_img, seed=21) if n_img == 4 else _image(128, 96, 3, seed=22)
    blobs0, yaik0 = _driver(planes, "0")
    blobs1, yaik1 = _driver(planes, "pixels")
    assert "pixels_unpack_intervals" not in blobs0
    # the pixels form ran, and its image went through the GPU unpack (one interval of the stage right after LoadImagePixels)
    assert np.frombuffer(bytes(blobs1.pop("pixels_unpack_intervals")), np.int32).tolist() == [1]
    assert len(yaik0) > 12 and yaik1 == yaik0
    assert blobs1.keys() == blobs0.keys()
    assert [k for k in blobs0 if bytes(blobs0[k]) != bytes(blobs1[k])] == []
