"""CPU side of the normalised outputs: the clip-and-mirror rule the kernel runs (yaik_amd/csrc/yk_window_mirror.h through
window_mirror_tool) against a brute-force enumeration, the reference of tests/norm_ref.py against torch's CPU conversions, norm_params, the
element-size-aware layout helper, the declarations against the signature tables and the built libraries, and the Python argument checks that raise
before any library call."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from tests import norm_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "yaik_amd", "host")
TOOL = os.path.join(HOST, "window_mirror_tool")


# ---- the clip-and-mirror rule ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tool():
    subprocess.run(["make", "-C", HOST, "window_mirror_tool"], check=True, stdout=subprocess.DEVNULL)
    return TOOL


def _run(tool, *args):
    p = subprocess.run([tool] + [str(a) for a in args], capture_output=True, text=True)
    return p.returncode, p.stdout.strip()


def test_clip_and_mirror_against_brute_force(tool):
    # the tool's own exhaustive check: every tile column, offset 0..23, window length 1..40, both mirror states
    assert _run(tool, "check", 23, 40) == (0, f"ok {24 * 40 * 2}")
    # and an enumeration made here, from the tool's table alone: where does every cover column land?
    for d in (0, 1, 7, 8, 9, 15, 16, 23):
        for ww in (1, 2, 7, 8, 9, 13, 16, 17, 40):
            for mirror in (0, 1):
                rc, out = _run(tool, "show", d, ww, mirror)
                assert rc == 0
                got = {}
                cols = [tuple(int(v) for v in col.split(",")) for col in out.split()]
                assert [c[0] for c in cols] == list(range((d + ww + 7) // 8))
                for j, src0, n, dst, rev0 in cols:
                    if n == 0:
                        continue
                    assert 0 <= src0 and src0 + n <= 8 and 0 <= dst and dst + n <= ww, (d, ww, mirror, j)
                    assert rev0 == (8 - src0 - n if mirror else src0)
                    for i in range(n):
                        to = dst + n - 1 - i if mirror else dst + i
                        assert to not in got
                        got[to] = 8 * j + src0 + i
                want = {(ww - 1 - x if mirror else x): d + x for x in range(ww)}
                assert got == want, (d, ww, mirror)


def test_clip_and_mirror_tool_refuses_bad_arguments(tool):
    assert _run(tool, "check", 23)[0] == 2 and _run(tool, "check", -1, 40)[0] == 2 and _run(tool, "show", 0, 0, 0) == (3, "bad")


def _f32_hex(v):
    return "%08x" % struct.unpack("<I", struct.pack("<f", v))[0]


def test_parameter_rule_of_the_library_and_of_python_agree(tool):
    from yaik_amd.encoder import check_norm
    good = [0.0, -0.0, 1.0, -1.0, 2.0 ** -100, -(2.0 ** -100), 2.0 ** 100, 1 / 255, 300.0, 0.0625]
    bad = [float("nan"), float("inf"), float("-inf"), 2.0 ** -101, -(2.0 ** -101), 2.0 ** 101, 1e-45, float(np.nextafter(np.float32(2.0 ** 100), np.float32(np.inf))),
           float(np.nextafter(np.float32(2.0 ** -100), np.float32(0)))]
    for v in good:
        assert _run(tool, "param", _f32_hex(v)) == (0, "1"), v
        check_norm(v, v)
    for v in bad:
        assert _run(tool, "param", _f32_hex(v)) == (0, "0"), v
        with pytest.raises(ValueError):
            check_norm(v, 0.0)
        with pytest.raises(ValueError):
            check_norm(1.0, [0.0, v, 0.0])
    for name, (s, b) in NR.parameter_sets().items():
        for v in list(s) + list(b):
            assert _run(tool, "param", _f32_hex(float(v))) == (0, "1"), name


# ---- the reference -----------------------------------------------------------------------------------------------------------------------------
ALL = np.arange(256, dtype=np.uint8).reshape(256, 1, 1).repeat(4, axis=2)        # every byte value in every channel


@pytest.mark.parametrize("name", list("ABCDEFG"))
def test_reference_conversions_equal_torch_cpu(name):
    import torch
    scale, bias = NR.parameter_sets()[name]
    f = NR.affine_f32(ALL, scale, bias)
    assert f.dtype == np.float32 and np.all(np.isfinite(f))
    # no fp32 intermediate is subnormal: the result does not depend on a denormal mode
    tiny = np.finfo(np.float32).tiny
    for a in (ALL.astype(np.float32) * scale, f):
        assert np.all((a == 0) | (np.abs(a) >= tiny))
    t = torch.from_numpy(f)
    assert np.array_equal(NR.convert_bits(f, "bfloat16"), NR.bits(t.to(torch.bfloat16))), name
    assert np.array_equal(NR.convert_bits(f, "float16"), NR.bits(t.to(torch.float16))), name
    assert np.array_equal(NR.convert_bits(f, "float32"), NR.bits(t)), name
    # the float32 product and sum are torch's too
    tt = torch.from_numpy(ALL).to(torch.float32) * torch.from_numpy(scale) + torch.from_numpy(bias)
    assert np.array_equal(NR.bits(tt), NR.convert_bits(f, "float32")), name


def test_parameter_sets_hit_what_they_are_meant_to_hit():
    P = NR.parameter_sets()
    # B: fused and unfused fp32 results differ for 124 to 158 of the 256 byte values in every channel, so the fp32 comparison catches an fma
    diff = (NR.affine_f32(ALL, *P["B"]).view(np.uint32) != NR.affine_fused_f32(ALL, *P["B"]).view(np.uint32)).reshape(256, 4).sum(axis=0)
    assert all(124 <= int(n) <= 158 for n in diff), diff
    # D: fp16 subnormals (non-zero, below the smallest normal 2^-14), kept
    h = NR.convert_bits(NR.affine_f32(ALL, *P["D"]), "float16")[:, 0, 0]
    assert np.all((h[1:64] & 0x7C00) == 0) and np.all((h[1:64] & 0x03FF) != 0) and np.all((h[64:] & 0x7C00) != 0)      # v 2^-20 < 2^-14 for v < 64
    assert h[1:64].tolist() == [v << 4 for v in range(1, 64)]                # v 2^-20 = (16 v) 2^-24: exact
    # E: fp16 goes to inf from v = 219
    h = NR.convert_bits(NR.affine_f32(ALL, *P["E"]), "float16")[:, 0, 0]
    assert np.all(h[219:] == 0x7C00) and np.all(h[:219] != 0x7C00)
    # F: every v >= 128 is a bf16 tie (v + 0.5 needs 9 bits, bf16 has 8), and both parities of the kept bit occur
    f = NR.affine_f32(ALL, *P["F"])[128:, 0, 0]
    u = f.view(np.uint32)
    assert np.all((u & 0xFFFF) == 0x8000) and set(((u >> 16) & 1).tolist()) == {0, 1}
    # G: every v >= 128 is an fp16 tie (v + 1/16 needs 12 bits, fp16 has 11)
    u = NR.affine_f32(ALL, *P["G"])[128:, 0, 0].view(np.uint32)
    assert np.all((u & 0x1FFF) == 0x1000)
    # ties go to even
    assert NR.bf16_bits(np.array([128.5, 129.5], np.float32)).tolist() == [0x4300, 0x4302]


def test_norm_ref_mirrors_and_converts():
    rng = np.random.default_rng(5)
    px = rng.integers(0, 256, (5, 7, 4)).astype(np.uint8)
    s, b = NR.parameter_sets()["B"]
    plain, flipped = NR.norm_ref(px, "float32", s, b), NR.norm_ref(px, "float32", s, b, mirror=True)
    assert plain.shape == (5, 7, 4) and np.array_equal(flipped, plain[:, ::-1]) and not np.array_equal(flipped, plain)
    assert np.array_equal(NR.norm_ref(px[..., :3], "bfloat16", s, b), NR.norm_ref(px, "bfloat16", s, b)[..., :3])


def test_norm_params():
    from yaik_amd.encoder import norm_params
    from yaik_amd import decoder
    assert decoder.norm_params is norm_params                                # public where the decoder lives
    s, b = norm_params([0.485 * 255, 0.456 * 255, 0.406 * 255], [0.229 * 255, 0.224 * 255, 0.225 * 255])
    assert s.dtype == b.dtype == np.float32 and s.shape == b.shape == (4,)
    for k, (m, sd) in enumerate(((0.485, 0.229), (0.456, 0.224), (0.406, 0.225))):
        assert s[k] == np.float32(1.0 / (sd * 255)) and b[k] == np.float32(-(m * 255) / (sd * 255))      # float64 first, one rounding
    assert s[3] == 1 and b[3] == 0                                           # three values leave alpha alone
    s, b = norm_params(127.5, 127.5)
    assert s.tolist() == [np.float32(1 / 127.5)] * 4 and b.tolist() == [-1.0] * 4
    s, b = norm_params([1, 2, 3, 4], [2, 4, 8, 16])
    assert s.tolist() == [0.5, 0.25, 0.125, 0.0625] and b.tolist() == [-0.5, -0.5, -0.375, -0.25]
    for bad in (([1, 2], [1, 2]), (0, 0), (0, [1, 0, 1]), (float("nan"), 1), (0, float("inf")), ([[1, 2, 3]], 1)):
        with pytest.raises(ValueError):
            norm_params(*bad)


# ---- the layout helper -------------------------------------------------------------------------------------------------------------------------
def test_elem_layout_on_cpu_tensors():
    import torch
    from yaik_amd.encoder import elem_layout
    for tdt, code, es in ((torch.float16, 1, 2), (torch.bfloat16, 2, 2), (torch.float32, 3, 4)):
        t = torch.zeros((11, 13, 3), dtype=tdt)
        assert elem_layout(t) == (code, es, 1, 3, 11, 13, 39 * es, 0, 11 * 39 * es)
        t = torch.zeros((4, 11, 13), dtype=tdt)
        assert elem_layout(t, planar=True) == (code, es, 1, 4, 11, 13, 13 * es, 143 * es, 4 * 143 * es)
        # padded views: row, plane and frame pitch, an odd element offset
        buf = torch.zeros(100000, dtype=tdt)
        v = torch.as_strided(buf, (2, 11, 13, 4), (700, 60, 4, 1), 3)
        assert elem_layout(v, batch=True) == (code, es, 2, 4, 11, 13, 60 * es, 0, 700 * es)
        v = torch.as_strided(buf, (2, 3, 11, 13), (900, 290, 24, 1), 5)
        assert elem_layout(v, planar=True, batch=True) == (code, es, 2, 3, 11, 13, 24 * es, 290 * es, 900 * es)
        assert elem_layout(v[1], planar=True) == (code, es, 1, 3, 11, 13, 24 * es, 290 * es, 3 * 290 * es)
        # a batch of one: the frame stride is the frame's own size
        assert elem_layout(torch.zeros((1, 8, 8, 3), dtype=tdt), batch=True).frame_bytes == 8 * 8 * 3 * es
        # inner stride != 1, pixel stride != C
        with pytest.raises(ValueError, match="contiguous"):
            elem_layout(torch.as_strided(buf, (11, 13, 3), (80, 6, 2), 0))
        with pytest.raises(ValueError, match="contiguous"):
            elem_layout(torch.as_strided(buf, (11, 13, 3), (80, 4, 1), 0))
        with pytest.raises(ValueError, match="contiguous"):
            elem_layout(torch.as_strided(buf, (3, 11, 13), (400, 30, 2), 0), planar=True)
        # overlapping rows, planes, frames
        with pytest.raises(ValueError, match="row stride"):
            elem_layout(torch.as_strided(buf, (11, 13, 3), (38, 3, 1), 0))
        with pytest.raises(ValueError, match="plane stride"):
            elem_layout(torch.as_strided(buf, (3, 11, 13), (142, 13, 1), 0), planar=True)
        with pytest.raises(ValueError, match="frame stride"):
            elem_layout(torch.as_strided(buf, (2, 11, 13, 3), (428, 39, 3, 1), 0), batch=True)
        with pytest.raises(ValueError):
            elem_layout(torch.zeros((11, 13, 5), dtype=tdt))
        with pytest.raises(ValueError):
            elem_layout(torch.zeros((11, 13, 3), dtype=tdt), batch=True)
    for bad in (torch.zeros((8, 8, 3), dtype=torch.uint8), torch.zeros((8, 8, 3), dtype=torch.float64), np.zeros((8, 8, 3), np.uint8)):
        with pytest.raises(TypeError):
            elem_layout(bad)
    assert elem_layout(np.zeros((8, 16, 3), np.float32)[:, :8]) == (3, 4, 1, 3, 8, 8, 16 * 3 * 4, 0, 8 * 16 * 3 * 4)
    # the uint8 helpers are what they were
    from yaik_amd.encoder import u8_pixel_layout
    with pytest.raises(TypeError):
        u8_pixel_layout(torch.zeros((8, 8, 3), dtype=torch.float16))


# ---- declarations, tables, libraries -------------------------------------------------------------------------------------------------------------
def _arity(text, prefix):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return {name: args.count(",") + 1 for name, args in re.findall(r"\b(%s[A-Za-z0-9_]+)\s*\(([^()]*)\)\s*;" % prefix, text)}


def test_headers_signature_tables_and_libraries_agree():
    from yaik_amd import _lib, files
    from yaik_amd.encoder import ELEM_DTYPES, NormC
    text = open(os.path.join(ROOT, "include", "yaik_hip.h")).read()
    declared = _arity(text, "yk_")
    for name, arity in (("yk_decode_output_norm_device", 8), ("yk_decode_output_norm_batch_device", 9)):
        assert declared.get(name) == arity
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == arity
    assert re.search(r"YK_ELEM_F16 = 1, YK_ELEM_BF16 = 2, YK_ELEM_F32 = 3", text)
    assert ELEM_DTYPES == {"float16": (1, 2), "bfloat16": (2, 2), "float32": (3, 4)}
    assert C.sizeof(NormC) == 36 and NormC.scale.offset == 4 and NormC.bias.offset == 20      # int32 dtype; float scale[4]; float bias[4]
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)                                               # loading needs no device
    assert hasattr(L, "yk_decode_output_norm_device") and hasattr(L, "yk_decode_output_norm_batch_device")
    hooks = open(os.path.join(ROOT, "include", "yaik_hip_test.h")).read()
    assert "norm" not in hooks                                              # no test hook was added for the feature
    subprocess.run(["make", "-C", HOST, "libyaik_host.so"], check=True, stdout=subprocess.DEVNULL)
    htext = open(os.path.join(HOST, "yaik_decode_norm.h")).read()
    assert 'extern "C"' in htext and _arity(htext, "YAIK_") == {"YAIK_DecodeImagesNormToDevice": 16}
    res, args = files.NORM_SIGNATURES["YAIK_DecodeImagesNormToDevice"]
    assert res is C.c_bool and len(args) == 16 and args[:14] == files.WINDOW_PX_SIGNATURES["YAIK_DecodeImagesWindowsPxToDevice"][1]
    out = set(subprocess.run(["nm", "-D", "--defined-only", files.HOST_LIB_PATH], check=True, capture_output=True, text=True).stdout.split())
    assert "YAIK_DecodeImagesNormToDevice" in out
    H = files.host_lib()                                                    # loads without a device
    H.YAIK_GetErrorCode()
    failed = C.c_int32(7)
    nrm = NormC(1, (C.c_float * 4)(1, 1, 1, 1), (C.c_float * 4)(0, 0, 0, 0))
    assert not H.YAIK_DecodeImagesNormToDevice(None, None, None, 1, None, 0, 0, 0, 3, 1, C.byref(failed), None, 0, 0, C.byref(nrm), None)
    assert files.ERROR_NAMES[H.YAIK_GetErrorCode()] == "YAIK_INVALID_LIBRARYCTX" and failed.value == -1
    assert not H.YAIK_DecodeImagesNormToDevice(None, None, None, 1, None, 0, 0, 0, 3, 1, None, None, 0, 0, None, None)      # no yk_norm
    assert files.ERROR_NAMES[H.YAIK_GetErrorCode()] == "YAIK_DECIMG_INVALIDCTX"


# ---- the Python checks come before any library call --------------------------------------------------------------------------------------------
def _decoder(frames=3):
    from yaik_amd.decoder import HipTileDecoder
    d = HipTileDecoder.__new__(HipTileDecoder)                              # no handle, no library: the checks come first
    d._h = None
    d.device = 0
    d.w, d.h, d.frames, d._window, d._batch_windows, d._has_alpha = 136, 264, frames, None, None, False
    return d


def test_python_checks_raise_before_any_library_call():
    import torch
    d = _decoder()
    for call in (d.image_norm_device, d.image_norm_batch_device):
        for dt in (torch.uint8, torch.float64, "int8", None):
            with pytest.raises(TypeError):
                call(dt)
        with pytest.raises(ValueError, match="not both"):
            call(torch.float16, scale=1.0, mean=0.0, std=1.0)
        with pytest.raises(ValueError, match="not both"):
            call(torch.float16, bias=0.0, mean=0.0, std=1.0)
        with pytest.raises(ValueError, match="together"):
            call(torch.float16, mean=0.0)
        with pytest.raises(ValueError):
            call(torch.float16, mean=0.0, std=0.0)
        for bad in (float("nan"), float("inf"), 2.0 ** 101, 2.0 ** -101, [1.0, 2.0], [1.0] * 5):
            with pytest.raises(ValueError):
                call(torch.float32, scale=bad)
            with pytest.raises(ValueError):
                call(torch.float32, bias=bad)
        with pytest.raises(ValueError, match="channels"):
            call(torch.float16, channels=5)
    with pytest.raises(ValueError, match="alpha"):
        d.image_norm_device(torch.float16, channels=4, alpha=256)
    with pytest.raises(ValueError, match="alpha"):
        d.image_norm_batch_device(torch.float16, channels=4, alpha=-1)
    with pytest.raises(ValueError, match="alpha_from_planes"):
        d.image_norm_batch_device(torch.float16, channels=3, alpha_from_planes=True)
    for bad in ([True, False], [1, 0, 1, 0], [[1, 0, 1]], [0.5, 0.0, 1.0], torch.zeros(2, dtype=torch.bool)):
        with pytest.raises(ValueError, match="mirror"):
            d.image_norm_batch_device(torch.float16, mirror=bad)


def test_file_call_checks_first():
    import torch
    from yaik_amd import files
    with pytest.raises(TypeError):
        files.decode_files_norm_device([b""], torch.uint8)
    with pytest.raises(ValueError, match="not both"):
        files.decode_files_norm_device([b""], torch.float16, scale=1.0, mean=0.0, std=1.0)
    with pytest.raises(ValueError):
        files.decode_files_norm_device([b""], torch.float16, scale=float("inf"))
    with pytest.raises(ValueError):
        files.decode_files_norm_device([], torch.float16)
    with pytest.raises(ValueError, match="together"):
        files.decode_files_norm_device([b""], torch.float16, origins=[(0, 0)])
    with pytest.raises(ValueError, match="mirror"):
        files.decode_files_norm_device([b""], torch.float16, mirror=[1, 0])
    with pytest.raises(ValueError):
        files.decode_files_norm_device([b""], torch.float16, origins=[(-1, 0)], size=(8, 8))
    with pytest.raises(ValueError):
        files.decode_files_norm_device([b"", b""], torch.float16, origins=[(0, 0)], size=(8, 8))
