"""CPU side of the resampled outputs: the taps and blends the kernel runs (yaik_amd/csrc/yk_resample.h through resample_tool) against
the tool's own brute force and against tests/resample_ref.py, the identity and 2x properties, the derived bound against torch's CPU bilinear, the
checks that raise before any library call, random_resized_crop_rects, the declarations against the tables and libraries, and the proof that the
reference separates the mistakes a kernel can make on the very rectangle sets the GPU tests use."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import batch_window_cases as BW
from tests import resample_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yaik_amd", "host")
TOOL = os.path.join(HOST, "resample_tool")
BIG_PAIRS = [(16384, 1), (1, 16384), (16384, 16384), (16383, 224)]


@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-C", HOST, "resample_tool"], check=True, stdout=subprocess.DEVNULL)
    return TOOL


def _run(tool, *args):
    p = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True)
    return p.returncode, p.stdout.strip()


# ---- the tool: the header's functions against a 64-bit and rational brute force ---------------------------------------------------------------
def test_tool_against_brute_force(tool):
    rc, out = _run(tool, "check")
    assert rc == 0 and re.fullmatch(r"ok \d+", out), out
    # every output index of 40 x 40 pairs and of the four large pairs, and the blends, went through it
    assert int(out.split()[1]) > sum(no for _ in range(40) for no in range(1, 41)) + sum(no for _, no in BIG_PAIRS)


def test_tool_refuses_bad_arguments(tool):
    assert _run(tool, "check", 1)[0] == 2 and _run(tool, "taps", 0, 4) == (3, "bad") and _run(tool, "taps", 4, 16385) == (3, "bad")
    assert _run(tool, "blend", 0, 0, 0, 0, 256, 0) == (3, "bad")


def _tool_taps(tool, ns, no):
    rc, out = _run(tool, "taps", ns, no)
    assert rc == 0
    cols = [tuple(int(v) for v in c.split(",")) for c in out.split()]
    return cols[0], np.array(cols[1:], dtype=np.int64)


@pytest.mark.parametrize("ns,no", [(1, 1), (1, 7), (3, 7), (2, 3), (5, 3), (301, 13), (97, 11), (520, 56), (264, 40), (8, 8), (16, 8), (6, 56), (5, 40)] + BIG_PAIRS)
def test_reference_taps_equal_the_tools(tool, ns, no):
    (step, off), cols = _tool_taps(tool, ns, no)
    assert (step, off) == RR.axis(ns, no)
    i0, i1, f = RR.taps(ns, no)
    assert np.array_equal(cols[:, 0], i0) and np.array_equal(cols[:, 1], i1) and np.array_equal(cols[:, 2], f)
    assert i0.min() >= 0 and i1.max() <= ns - 1


def test_reference_blend_cover_and_rule_equal_the_tools(tool):
    rng = np.random.default_rng(29)
    for _ in range(40):
        a, b, c, d, fx, fy = (int(v) for v in rng.integers(0, 256, 6))
        src = np.array([[a, b], [c, d]], np.uint8)[..., None]
        # a 2 x 2 source and weights forced through the reference's own formula
        acc = (a * (256 - fx) + b * fx) * (256 - fy) + (c * (256 - fx) + d * fx) * fy + 32768
        assert _run(tool, "blend", a, b, c, d, fx, fy) == (0, str(acc >> 16))
        assert src.shape == (2, 2, 1)
    for rect in [(3, 5, 301, 97), (0, 0, 8, 8), (513, 257, 6, 5), (7, 7, 1, 1), (8, 16, 8, 8), (329, 105, 190, 37)]:
        assert _run(tool, "cover", *rect) == (0, ",".join(map(str, RR.cover(rect))))
    ok = lambda *v: _run(tool, "ok", *v)[1]
    assert ok(0, 0, 520, 264, 520, 264, 13, 11) == "1" and ok(519, 263, 1, 1, 520, 264, 1, 1) == "1" and ok(3, 5, 301, 97, 520, 264, 16384, 16384) == "1"
    for bad in [(-1, 0, 8, 8, 520, 264, 8, 8), (0, -1, 8, 8, 520, 264, 8, 8), (0, 0, 0, 8, 520, 264, 8, 8), (0, 0, 8, 0, 520, 264, 8, 8), (513, 0, 8, 8, 520, 264, 8, 8),
                (0, 257, 8, 8, 520, 264, 8, 8), (0, 0, 8, 8, 520, 264, 0, 8), (0, 0, 8, 8, 520, 264, 8, 16385), (0, 0, 16385, 8, 32760, 264, 8, 8),
                (0, 0, 8, 16385, 520, 32760, 8, 8), (2147483647, 0, 8, 8, 520, 264, 8, 8)]:
        assert ok(*bad) == "0", bad
    assert _run(tool, "words", 3, 5, 301, 97, 13, 11, 1) == (0, ",".join(map(str, (3, 5, 300, 96) + RR.axis(301, 13) + RR.axis(97, 11) + (1,))))


# ---- properties of the contract ----------------------------------------------------------------------------------------------------------------
def _noise(h, w, c=3, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, c), dtype=np.uint8)


def test_identity_and_two_times():
    img = _noise(41, 53, 4, seed=1)
    for rect in [(0, 0, 53, 41), (3, 5, 13, 11), (52, 40, 1, 1), (7, 0, 2, 41)]:
        x0, y0, sw, sh = rect
        crop = img[y0:y0 + sh, x0:x0 + sw]
        assert np.array_equal(RR.resample(img, rect, (sw, sh)), crop)
        assert np.array_equal(RR.resample(img, rect, (sw, sh), mirror=True), crop[:, ::-1])
    for rect in [(0, 0, 52, 40), (3, 5, 26, 22), (51, 39, 2, 2)]:
        x0, y0, sw, sh = rect
        s = img[y0:y0 + sh, x0:x0 + sw].astype(np.int64)
        box = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2                  # the level-1 box mean of §24: halves rounded up
        assert np.array_equal(RR.resample(img, rect, (sw // 2, sh // 2)), box.astype(np.uint8))


SHAPES = [((53, 41), (13, 11)), ((53, 41), (56, 40)), ((1, 1), (7, 3)), ((3, 2), (7, 3)), ((53, 41), (1, 1)), ((2, 3), (64, 48)), ((40, 40), (17, 39)), ((9, 31), (31, 9)),
          ((53, 41), (53, 41)), ((52, 40), (26, 20))]


@pytest.mark.parametrize("src,size", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_derived_bound_against_torch_bilinear(src, size):
    """|v - torch's float64 bilinear of the crop| <= 2 * 255/256 + 0.5 + 255 (ow + oh) / 65536: the weight truncation per axis, the final
    rounding and the accumulated truncation of step.  Derived, not measured."""
    import torch
    import torch.nn.functional as F
    (sw, sh), (ow, oh) = src, size
    img = _noise(sh + 9, sw + 11, 3, seed=sw * 31 + ow)
    rect = (5, 4, sw, sh)
    got = RR.resample(img, rect, size).astype(np.float64)
    crop = torch.from_numpy(img[4:4 + sh, 5:5 + sw].astype(np.float64)).permute(2, 0, 1)[None]
    want = F.interpolate(crop, size=(oh, ow), mode="bilinear", align_corners=False, antialias=False)[0].permute(1, 2, 0).numpy()
    bound = 2 * 255 / 256 + 0.5 + 255 * (ow + oh) / 65536
    worst = float(np.abs(got - want).max())
    print(f"{src} -> {size}: largest difference {worst:.3f}, bound {bound:.3f}")
    assert worst <= bound


# ---- the reference separates the mistakes a kernel can make, on the sets the GPU tests use ------------------------------------------------------
def _can_matter(variant, size):
    """With one output column and row the single tap sits at the rectangle's centre: pos = (sw << 15) - 32768 exactly, never clamped, its fraction
    0 or exactly one half, and the two taps of an even side are symmetric.  So a 1 x 1 output cannot show a wrong clamp, a rounded fraction or a
    mirrored source; the two remaining variants are asked of it."""
    return size != (1, 1) or variant in ("no_round", "no_half")


@pytest.mark.parametrize("w,h,kind,n", BW.BATCHES, ids=lambda v: str(v))
def test_reference_separates_the_mistakes(oracle_built, w, h, kind, n):
    refs = BW.batch_references(w, h, kind, n)
    flags = RR.FLAGS[:n]
    for name, rects in RR.rect_sets(w, h):
        for size in RR.SIZES:
            assert not all((r[2], r[3]) == size for r in rects)                                       # none of the sets is an identity
            good = [RR.resample(refs[f].rgb, rects[f], size, flags[f]) for f in range(n)]
            for variant in RR.VARIANTS:
                changed = False
                for f in range(n):
                    bound = RR.cover(rects[f]) if variant == "clamp_cover" else None
                    bad = RR.resample(refs[f].rgb, rects[f], size, flags[f], variant=variant, bound=bound)
                    changed = changed or not np.array_equal(bad, good[f])
                assert changed == _can_matter(variant, size), (name, size, variant)


# ---- random_resized_crop_rects -------------------------------------------------------------------------------------------------------------------
def test_random_resized_crop_rects():
    from yaik_amd.augment import random_resized_crop_rects, rect_table
    for w, h in [(512, 512), (2048, 2048), (520, 264), (8, 8), (32760, 8)]:
        r = random_resized_crop_rects(300, w, h, seed=0)
        assert r.dtype == np.int32 and r.shape == (300, 4)
        assert np.array_equal(rect_table(r, 300, w, h), r)                                            # every rectangle passes the library's rule
        assert np.array_equal(r, random_resized_crop_rects(300, w, h, seed=0))
        if h > 8:                                                                                     # (an 8-pixel side leaves few or no rectangles to choose from)
            assert not np.array_equal(r, random_resized_crop_rects(300, w, h, seed=1))
    r = random_resized_crop_rects(2000, 512, 512, seed=3).astype(np.float64)
    area, ratio = r[:, 2] * r[:, 3] / (512 * 512), r[:, 2] / r[:, 3]
    assert area.min() >= 0.08 * 0.98 and area.max() <= 1.0 and area.min() < 0.12 and area.max() > 0.9  # the scale range, up to the rounding of the sides
    assert ratio.min() >= 3 / 4 * 0.97 and ratio.max() <= 4 / 3 * 1.03 and ratio.min() < 0.8 and ratio.max() > 1.25
    assert abs(float(np.log(ratio).mean())) < 0.03                                                    # log-uniform: symmetric about 1
    assert len({(int(a), int(b)) for a, b in r[:, 2:]}) > 1000                                        # sizes differ from frame to frame
    # ten misses: a 1000 x 8 image has no crop with a ratio in 3/4 .. 4/3 and 50 % of the area; the centre fallback clamps the ratio
    r = random_resized_crop_rects(5, 1000, 8, scale=(0.5, 1.0), seed=0)
    assert (r == np.array([(1000 - 11) // 2, 0, 11, 8])).all()
    r = random_resized_crop_rects(5, 8, 1000, scale=(0.5, 1.0), seed=0)
    assert (r == np.array([0, (1000 - 11) // 2, 8, 11])).all()
    for bad in (dict(n=0), dict(w=0), dict(scale=(0.5, 0.1)), dict(ratio=(0.0, 1.0))):
        with pytest.raises(ValueError):
            random_resized_crop_rects(**{**dict(n=1, w=8, h=8), **bad})


# ---- the Python checks come before any library call ---------------------------------------------------------------------------------------------
def _decoder(frames=3):
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder.__new__(HipTileDecoder)                              # no handle, no library: the checks come first
    d._h = None
    d.device = 0
    d.w, d.h, d.frames, d._window, d._batch_windows, d._batch_rects, d._has_alpha = 136, 264, frames, None, None, None, False
    return d


BAD_RECTS = [[(0, 0, 8, 8)] * 2, [(0, 0, 8, 8)] * 4, [(-1, 0, 8, 8)] * 3, [(0, 0, 0, 8)] * 3, [(129, 0, 8, 8)] * 3, [(0, 257, 8, 8)] * 3, [(0, 0, 137, 8)] * 3]


def test_python_checks_raise_before_any_library_call():
    import torch
    d = _decoder()
    for bad in BAD_RECTS:
        with pytest.raises(ValueError):
            d.set_batch_rects(bad)
    for bad in ([(0, 0, 8)] * 3, [(0.0, 0, 8, 8)] * 3, "abc", 7, np.zeros((3, 4), np.float32), np.zeros((3, 3), np.int32), [(True, 0, 8, 8)] * 3):
        with pytest.raises(TypeError):
            d.set_batch_rects(bad)
    assert d.batch_rects is None
    for call in (d.image_resampled_batch_device, d.image_resampled_device):
        for bad in ((0, 8), (8, 0), (16385, 8), (8, 16385), (-1, -1)):
            with pytest.raises(ValueError, match="size"):
                call(bad)
        for bad in (8, (8,), (8, 8, 8), "88", (8.0, 8), (True, 8), None):
            with pytest.raises(TypeError):
                call(bad)
        for dt in (torch.float64, "int8"):
            with pytest.raises(TypeError):
                call((8, 8), dtype=dt)
        for dt in (None, torch.uint8, "uint8"):
            with pytest.raises(ValueError, match="uint8"):
                call((8, 8), dtype=dt, scale=1.0)
        with pytest.raises(ValueError, match="not both"):
            call((8, 8), dtype=torch.float16, scale=1.0, mean=0.0, std=1.0)
        with pytest.raises(ValueError):
            call((8, 8), dtype=torch.float32, bias=float("inf"))
        with pytest.raises(ValueError, match="channels"):
            call((8, 8), channels=5)
    with pytest.raises(ValueError, match="alpha"):
        d.image_resampled_batch_device((8, 8), channels=4, alpha=-1)
    with pytest.raises(ValueError, match="alpha_from_planes"):
        d.image_resampled_batch_device((8, 8), alpha_from_planes=True)
    with pytest.raises(ValueError, match="mirror"):
        d.image_resampled_batch_device((8, 8), mirror=[1, 0])
    with pytest.raises(ValueError, match="alpha"):
        d.image_resampled_device((8, 8), channels=4, alpha=256)
    for bad in ((-1, 0, 8, 8), (0, 0, 137, 8), (130, 260, 8, 8), (0, 0, 0, 0)):
        with pytest.raises(ValueError):
            d.image_resampled_device((8, 8), rect=bad)
    d._window = (8, 8, 24, 16)
    for bad in ((7, 8, 8, 8), (8, 7, 8, 8), (8, 8, 25, 16), (8, 8, 24, 17), (31, 23, 2, 1)):
        with pytest.raises(ValueError, match="window"):
            d.image_resampled_device((8, 8), rect=bad)
    d._window = None
    with pytest.raises(ValueError, match="replace"):
        d.decode_batch_from_encoder(None, windows=([(0, 0)] * 3, 8, 8), rects=[(0, 0, 8, 8)] * 3)


def test_file_call_checks_first():
    import torch
    from yaik_amd import files
    for bad in ((0, 8), (8, 16385)):
        with pytest.raises(ValueError, match="size"):
            files.decode_files_resampled_device([b""], bad)
    with pytest.raises(TypeError):
        files.decode_files_resampled_device([b""], 8)
    with pytest.raises(TypeError):
        files.decode_files_resampled_device([b""], (8, 8), dtype=torch.float64)
    with pytest.raises(ValueError, match="uint8"):
        files.decode_files_resampled_device([b""], (8, 8), mean=0.0, std=1.0)
    with pytest.raises(ValueError):
        files.decode_files_resampled_device([], (8, 8))
    with pytest.raises(ValueError, match="mirror"):
        files.decode_files_resampled_device([b""], (8, 8), mirror=[1, 0])
    with pytest.raises(ValueError):
        files.decode_files_resampled_device([b""], (8, 8), rects=[(-1, 0, 8, 8)])
    with pytest.raises(ValueError):
        files.decode_files_resampled_device([b"", b""], (8, 8), rects=[(0, 0, 8, 8)])
    with pytest.raises(ValueError):
        files.decode_files_resampled_device([b""], (8, 8), rects=[(0, 0, 16385, 8)])


# ---- declarations, tables, libraries -------------------------------------------------------------------------------------------------------------
def _arity(text, prefix):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return {name: args.count(",") + 1 for name, args in re.findall(r"\b(%s[A-Za-z0-9_]+)\s*\(([^()]*)\)\s*;" % prefix, text)}


def test_headers_signature_tables_and_libraries_agree():
    from yaik_amd import _lib, files
    from yaik_amd.augment import RS_MAX
    text = open(os.path.join(ROOT, "include", "yaik_hip.h")).read()
    declared = _arity(text, "yk_")
    for name, arity in (("yk_decode_set_batch_rects", 2), ("yk_decode_output_resampled_batch_device", 11), ("yk_decode_output_resampled_device", 11)):
        assert declared.get(name) == arity
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == arity
    pure = open(os.path.join(ROOT, "yaik_amd", "csrc", "yk_resample.h")).read()
    assert re.search(r"#define YK_RS_MAX %d\b" % RS_MAX, pure) and RS_MAX == RR.RS_MAX and "hip" not in re.sub(r"//[^\n]*", "", pure).lower()
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)                                               # loading needs no device
    assert all(hasattr(L, n) for n in ("yk_decode_set_batch_rects", "yk_decode_output_resampled_batch_device", "yk_decode_output_resampled_device"))
    subprocess.run(["make", "-C", HOST, "libyaik_host.so"], check=True, stdout=subprocess.DEVNULL)
    htext = open(os.path.join(HOST, "yaik_decode_resample.h")).read()
    assert 'extern "C"' in htext and _arity(htext, "YAIK_") == {"YAIK_DecodeImagesResampledToDevice": 16}
    res, args = files.RESAMPLE_SIGNATURES["YAIK_DecodeImagesResampledToDevice"]
    assert res is C.c_bool and len(args) == 16
    H = files.host_lib()                                                    # loads without a device
    failed = C.c_int32(7)
    assert not H.YAIK_DecodeImagesResampledToDevice(None, None, None, 1, None, 0, 0, 0, 3, 1, C.byref(failed), None, 8, 8, None, None)
    assert files.ERROR_NAMES[H.YAIK_GetErrorCode()] == "YAIK_INVALID_LIBRARYCTX" and failed.value == -1
    assert not H.YAIK_DecodeImagesResampledToDevice(None, None, None, 1, None, 0, 0, 0, 3, 1, None, None, 0, 8, None, None)          # no output size
    assert files.ERROR_NAMES[H.YAIK_GetErrorCode()] == "YAIK_DECIMG_INVALIDCTX"
