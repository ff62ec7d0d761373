"""Python plumbing over the C-ABI (include/yaik_hip.h) for tests and bench.py.

The method names follow the reference's operator surface for this path
(``EncoderContext::MipPrefilter / FittingQuadSmooth / DynamicTileEncode``, encoder/EncoderContext.h:326-370):
one fused launch computes what the seven FittingQuadSmooth calls and the three DynamicTileEncode calls
compute; the per-call views below hand out the cached results.  The C++ mirror of the same surface lives in
yaik_amd/host/ (the reference is compiled C++, so that is the drop-in; this module only moves bytes).
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from ._lib import YaikError, lib

PASSES = [(4, 4), (4, 3), (3, 4), (3, 3), (3, 2), (2, 3), (2, 2)]   # EncoderContext.cpp:9057-9093


# handle -> the library build that created it (the product library, or the test-hooks build of the same sources: tests/csrc/libyaik_hip_test.so):
# a handle is only ever passed back to the build that owns it, error lookups included
_HANDLE_LIB: dict = {}


def _chk(h, rc: int, L=None):
    if rc != 0:
        owner = L or _HANDLE_LIB.get(getattr(h, "value", h)) or lib()
        msg = owner.yk_last_error(h)
        raise YaikError(f"yaik_hip error {rc}: {msg.decode() if msg else '?'}")


class PixelLayout(NamedTuple):
    """How the 8-bit entry points (yk_upload_pixels_u8 / yk_load_device_pixels_u8) read an interleaved array: u8_pixel_layout."""
    frames: int
    rows: int
    w: int
    channels: int           # bytes per pixel: 3 (RGB) or 4 (RGBA)
    n_planes: int           # planes filled: the first n_planes bytes of every pixel
    row_bytes: int          # row pitch
    frame_bytes: int        # frame stride (rows * row_bytes for a single image, where the library ignores it)


def u8_pixel_layout(pixels, n_planes: int | None = None, batch: bool = False) -> PixelLayout:
    """Layout of numpy or torch uint8 pixels [rows, w, C] (batch=True: [F, rows, w, C]), C = 3 or 4, n_planes (default C) <= C.  Row pitch and
    frame stride are the array's own strides, so padded or row-sliced views need no copy; the bytes of a row must be contiguous (channel
    stride 1, pixel stride C).  Reads only dtype, shape and strides."""
    if hasattr(pixels, "data_ptr"):
        import torch
        if pixels.dtype != torch.uint8:
            raise TypeError(f"8-bit pixels expected, got {pixels.dtype}")
        shape, strides = tuple(pixels.shape), tuple(pixels.stride())      # elements = bytes for uint8
    else:
        if pixels.dtype != np.uint8:
            raise TypeError(f"8-bit pixels expected, got {pixels.dtype}")
        shape, strides = pixels.shape, pixels.strides
    if len(shape) != (4 if batch else 3):
        raise ValueError(f"pixels must be [{'F, ' if batch else ''}rows, w, C], got shape {tuple(shape)}")
    rows, w, ch = shape[-3:]
    n = ch if n_planes is None else int(n_planes)
    if ch not in (3, 4) or n not in (3, 4) or n > ch:
        raise ValueError(f"C must be 3 (RGB) or 4 (RGBA) and n_planes 3 or 4, at most C; got C = {ch}, n_planes = {n}")
    if strides[-1] != 1 or strides[-2] != ch:
        raise ValueError(f"the bytes of a row must be contiguous (channel stride 1, pixel stride {ch}); got strides {tuple(strides)}")
    row_bytes = strides[-3]
    if row_bytes < w * ch:
        raise ValueError(f"row stride {row_bytes} is shorter than a row of {w * ch} bytes")
    frames, frame_bytes = (shape[0], strides[0]) if batch else (1, rows * row_bytes)
    if frames > 1 and frame_bytes < rows * row_bytes:
        raise ValueError(f"frame stride {frame_bytes} is shorter than a frame of {rows * row_bytes} bytes")
    return PixelLayout(frames, rows, w, ch, n, row_bytes, frame_bytes)


class PlanarLayout(NamedTuple):
    """How yk_decode_output_device writes a planar [C, rows, w] uint8 array: u8_planar_layout."""
    channels: int
    rows: int
    w: int
    row_bytes: int          # row pitch inside a plane
    plane_bytes: int        # plane stride


def u8_planar_layout(pixels) -> PlanarLayout:
    """Layout of numpy or torch uint8 pixels [C, rows, w], C = 3 or 4 (the [C, H, W] of torch image tensors).  Row pitch and plane stride are
    the array's own strides, so padded or sliced views need no copy; the bytes of a row must be contiguous (pixel stride 1), and rows and planes
    may not overlap.  Reads only dtype, shape and strides."""
    if hasattr(pixels, "data_ptr"):
        import torch
        if pixels.dtype != torch.uint8:
            raise TypeError(f"8-bit pixels expected, got {pixels.dtype}")
        shape, strides = tuple(pixels.shape), tuple(pixels.stride())
    else:
        if pixels.dtype != np.uint8:
            raise TypeError(f"8-bit pixels expected, got {pixels.dtype}")
        shape, strides = pixels.shape, pixels.strides
    if len(shape) != 3:
        raise ValueError(f"pixels must be [C, rows, w], got shape {tuple(shape)}")
    ch, rows, w = shape
    if ch not in (3, 4):
        raise ValueError(f"C must be 3 (RGB) or 4 (RGBA); got C = {ch}")
    if strides[2] != 1:
        raise ValueError(f"the bytes of a row must be contiguous (pixel stride 1); got strides {tuple(strides)}")
    row_bytes, plane_bytes = strides[1], strides[0]
    if row_bytes < w:
        raise ValueError(f"row stride {row_bytes} is shorter than a row of {w} bytes")
    if plane_bytes < rows * row_bytes:
        raise ValueError(f"plane stride {plane_bytes} is shorter than a plane of {rows * row_bytes} bytes")
    return PlanarLayout(ch, rows, w, row_bytes, plane_bytes)


class PlanarBatchLayout(NamedTuple):
    """How yk_decode_output_batch_device writes a planar batch [F, C, rows, w] uint8 array: u8_planar_batch_layout."""
    frames: int
    channels: int
    rows: int
    w: int
    row_bytes: int          # row pitch inside a plane
    plane_bytes: int        # plane stride inside a frame
    frame_bytes: int        # frame stride (channels * plane_bytes for a single frame, where the library ignores it)


def u8_planar_batch_layout(pixels) -> PlanarBatchLayout:
    """Layout of numpy or torch uint8 pixels [F, C, rows, w], C = 3 or 4 (the [N, C, H, W] of torch image batches): every frame as in
    u8_planar_layout, frames at the array's own stride.  Padded or sliced views need no copy; the bytes of a row must be contiguous, and rows,
    planes and frames may not overlap.  Reads only dtype, shape and strides."""
    if hasattr(pixels, "data_ptr"):
        import torch
        if pixels.dtype != torch.uint8:
            raise TypeError(f"8-bit pixels expected, got {pixels.dtype}")
        shape, strides = tuple(pixels.shape), tuple(pixels.stride())
    else:
        if pixels.dtype != np.uint8:
            raise TypeError(f"8-bit pixels expected, got {pixels.dtype}")
        shape, strides = pixels.shape, pixels.strides
    if len(shape) != 4:
        raise ValueError(f"pixels must be [F, C, rows, w], got shape {tuple(shape)}")
    if shape[0] < 1:
        raise ValueError("a batch holds at least one frame")
    lay = u8_planar_layout(pixels[0])
    frames, frame_bytes = shape[0], (strides[0] if shape[0] > 1 else lay.channels * lay.plane_bytes)
    if frame_bytes < lay.channels * lay.plane_bytes:
        raise ValueError(f"frame stride {frame_bytes} is shorter than a frame of {lay.channels * lay.plane_bytes} bytes")
    return PlanarBatchLayout(frames, lay.channels, lay.rows, lay.w, lay.row_bytes, lay.plane_bytes, frame_bytes)


class ElemLayout(NamedTuple):
    """How the normalised outputs (yk_decode_output_norm_device and its batch form) write a float16 / bfloat16 / float32 tensor: elem_layout.
    Every pitch is in BYTES and a multiple of elem_bytes."""
    dtype: int              # YK_ELEM_F16 = 1, YK_ELEM_BF16 = 2, YK_ELEM_F32 = 3
    elem_bytes: int
    frames: int
    channels: int
    rows: int
    w: int
    row_bytes: int
    plane_bytes: int        # 0: interleaved [rows, w, C]
    frame_bytes: int        # a whole frame's bytes for a single image, where the library ignores it


ELEM_DTYPES = {"float16": (1, 2), "bfloat16": (2, 2), "float32": (3, 4)}          # name -> (YK_ELEM_*, bytes)


def elem_layout(pixels, planar: bool = False, batch: bool = False) -> ElemLayout:
    """Layout of a torch (or, for float16 / float32, numpy) tensor [rows, w, C], or [C, rows, w] with planar=True, with a leading frame axis if
    batch=True; C = 3 or 4; dtype float16, bfloat16 or float32.  The element-size-aware sibling of u8_pixel_layout, u8_planar_layout and
    u8_planar_batch_layout: pitches are the tensor's own strides times the element size, so padded or sliced views need no copy; the elements
    of a row must be contiguous (inner stride 1, and pixel stride C when interleaved), and rows, planes and frames may not overlap.  Reads
    only dtype, shape and strides."""
    name = str(pixels.dtype).replace("torch.", "")
    if name not in ELEM_DTYPES:
        raise TypeError(f"float16, bfloat16 or float32 elements expected, got {pixels.dtype}")
    code, es = ELEM_DTYPES[name]
    if hasattr(pixels, "data_ptr"):
        shape, strides = tuple(pixels.shape), tuple(pixels.stride())      # in elements
    else:
        shape, strides = tuple(pixels.shape), tuple(s // es for s in pixels.strides)
    what = ("F, " if batch else "") + ("C, rows, w" if planar else "rows, w, C")
    if len(shape) != (4 if batch else 3):
        raise ValueError(f"pixels must be [{what}], got shape {shape}")
    if batch and shape[0] < 1:
        raise ValueError("a batch holds at least one frame")
    if planar:
        ch, rows, w = shape[-3:]
        inner_ok, row, plane = strides[-1] == 1, strides[-2], strides[-3]
    else:
        rows, w, ch = shape[-3:]
        inner_ok, row, plane = strides[-1] == 1 and strides[-2] == ch, strides[-3], 0
    if ch not in (3, 4):
        raise ValueError(f"C must be 3 (RGB) or 4 (RGBA); got C = {ch}")
    if not inner_ok:
        raise ValueError(f"the elements of a row must be contiguous (inner stride 1{'' if planar else f', pixel stride {ch}'}); got strides {strides}")
    if row < w * (1 if planar else ch):
        raise ValueError(f"row stride {row} is shorter than a row of {w * (1 if planar else ch)} elements")
    if planar and plane < rows * row:
        raise ValueError(f"plane stride {plane} is shorter than a plane of {rows * row} elements")
    whole = ch * plane if planar else rows * row
    frames, frame = (shape[0], strides[0] if shape[0] > 1 else whole) if batch else (1, whole)
    if frame < whole:
        raise ValueError(f"frame stride {frame} is shorter than a frame of {whole} elements")
    return ElemLayout(code, es, frames, ch, rows, w, row * es, plane * es, frame * es)


def resample_layout(pixels, planar: bool = False, batch: bool = False) -> ElemLayout:
    """elem_layout for the resampled outputs, which also write uint8: such a tensor goes through the uint8 layout functions and comes
    back as an ElemLayout of dtype 0 and one byte per element"""
    if str(pixels.dtype).replace("torch.", "") != "uint8":
        return elem_layout(pixels, planar=planar, batch=batch)
    if planar:
        lay = u8_planar_batch_layout(pixels) if batch else u8_planar_layout(pixels)
        frames, frame = (lay.frames, lay.frame_bytes) if batch else (1, lay.channels * lay.plane_bytes)
        return ElemLayout(0, 1, frames, lay.channels, lay.rows, lay.w, lay.row_bytes, lay.plane_bytes, frame)
    lay = u8_pixel_layout(pixels, batch=batch)
    return ElemLayout(0, 1, lay.frames, lay.channels, lay.rows, lay.w, lay.row_bytes, 0, lay.frame_bytes)


def norm_params(mean, std):
    """(scale, bias) as float32 arrays of four for the normalised outputs from a per-channel mean and std (scalars, or sequences of 3 or 4 in the
    units of the decoded bytes, 0..255): scale = fp32(1 / std), bias = fp32(-mean / std), both computed in float64 and rounded once.  Three
    values leave alpha at scale 1, bias 0.  The bit-exact contract of the outputs is on scale and bias; this is the convenience in front of it."""
    def four(v, fill, what):
        a = np.atleast_1d(np.asarray(v, dtype=np.float64))
        if a.ndim != 1 or a.size not in (1, 3, 4):
            raise ValueError(f"{what} must be a scalar or 3 or 4 values; got shape {a.shape}")
        return np.full(4, a[0]) if a.size == 1 else np.concatenate([a, np.full(4 - a.size, fill)])
    m, s = four(mean, 0.0, "mean"), four(std, 1.0, "std")
    if not np.all(np.isfinite(m)) or not np.all(np.isfinite(s)) or np.any(s == 0):
        raise ValueError(f"mean and std must be finite and std non-zero; got {mean!r}, {std!r}")
    return (1.0 / s).astype(np.float32), (-m / s).astype(np.float32)


def check_norm(scale, bias):
    """scale and bias of a normalised output as float32 arrays of four (a scalar serves every channel, three values leave alpha at 1, 0), checked
    against the library's rule before any library call: finite, and 0 or of magnitude in [2^-100, 2^100]."""
    out = []
    for v, fill, what in ((scale, 1.0, "scale"), (bias, 0.0, "bias")):
        a = np.atleast_1d(np.asarray(v, dtype=np.float32))
        if a.ndim != 1 or a.size not in (1, 3, 4):
            raise ValueError(f"{what} must be a scalar or 3 or 4 values; got shape {a.shape}")
        a = np.full(4, a[0], np.float32) if a.size == 1 else np.concatenate([a, np.full(4 - a.size, fill, np.float32)])
        mag = np.abs(a.astype(np.float64))
        if not np.all(np.isfinite(a)) or np.any((mag != 0) & ((mag < 2.0 ** -100) | (mag > 2.0 ** 100))):
            raise ValueError(f"{what} must be finite and 0 or of magnitude in [2^-100, 2^100]; got {a.tolist()}")
        out.append(a)
    return out[0], out[1]


class NormC(C.Structure):                         # yk_norm of include/yaik_hip.h
    _fields_ = [("dtype", C.c_int32), ("scale", C.c_float * 4), ("bias", C.c_float * 4)]


def norm_struct(dtype, scale=None, bias=None, mean=None, std=None) -> NormC:
    """dtype (a torch or numpy dtype, or its name) and the affine pair of a normalised output as the library's yk_norm: scale / bias (default 1, 0),
    or mean / std through norm_params; giving both pairs raises, like everything else here, before any library call."""
    name = str(dtype).replace("torch.", "")
    if name not in ELEM_DTYPES:
        raise TypeError(f"dtype must be float16, bfloat16 or float32; got {dtype!r}")
    if (mean is not None or std is not None) and (scale is not None or bias is not None):
        raise ValueError("give scale / bias or mean / std, not both")
    if (mean is None) != (std is None):
        raise ValueError("mean and std go together")
    if mean is not None:
        scale, bias = norm_params(mean, std)
    s, b = check_norm(1.0 if scale is None else scale, 0.0 if bias is None else bias)
    return NormC(ELEM_DTYPES[name][0], (C.c_float * 4)(*s.tolist()), (C.c_float * 4)(*b.tolist()))


def mirror_flags(mirror, n: int):
    """None, or the per-frame mirror flags of a normalised batch output as n contiguous uint8: a sequence, array or bool / integer tensor of n"""
    if mirror is None:
        return None
    m = mirror.detach().cpu().numpy() if hasattr(mirror, "detach") else np.asarray(mirror)
    if m.ndim != 1 or m.shape[0] != n or not (m.dtype == np.bool_ or np.issubdtype(m.dtype, np.integer)):
        raise ValueError(f"mirror must be None or {n} flags, one per frame; got {m.dtype} {m.shape}")
    return np.ascontiguousarray(m != 0, dtype=np.uint8)


def gather_layout(nbytes):
    """Where HipTileEncoder.gather (yk_device_gather) puts segments of these lengths: (offsets, total) -- offsets[0] = 0, every later offset the
    previous end rounded up to 16, total = the last end rounded up to 16.  Pure; int64 numpy offsets."""
    n = np.asarray(nbytes, dtype=np.int64).reshape(-1)
    if n.size and int(n.min()) < 0:
        raise ValueError("segment lengths must not be negative")
    ends = np.cumsum((n + 15) & ~np.int64(15))
    offsets = np.concatenate([np.zeros(1, np.int64), ends[:-1]]) if n.size else np.zeros(0, np.int64)
    return offsets, int(ends[-1]) if n.size else 0


class _MipInfoC(C.Structure):                     # yk_mip_info of include/yaik_hip.h
    _fields_ = [("hasChunk", C.c_int32), ("bounds", C.c_int32 * 4), ("tileBBox", C.c_int32 * 4), ("nBytes", C.c_uint32)]


class _FrameStreamsC(C.Structure):                # yk_frame_streams of include/yaik_hip.h
    _fields_ = [("bitmap", C.c_void_p * 7), ("bitmapBytes", C.c_size_t * 7), ("rgb", C.c_void_p * 7), ("rgbBytes", C.c_size_t * 7),
                ("pix", C.c_void_p), ("pixBytes", C.c_size_t), ("type", C.c_void_p), ("typeBytes", C.c_size_t)]


class FrameStreams:
    """One frame's row of yk_batch_streams_table: device addresses (int, 0 = NULL) and byte lengths of its seven tile bitmaps, its seven raw
    corner streams (CompressF(., 250) bytes, not remapped), its 1-D pixel stream and its 1-D parameter triples.  A stream that is empty or was
    not requested has address 0 and length 0.  The addresses point into the encoder's own buffers: they go stale with its next encode, set_image /
    set_batch or streams_batch."""
    __slots__ = ("bitmap", "bitmap_bytes", "rgb", "rgb_bytes", "pix", "pix_bytes", "type", "type_bytes", "_enc")

    def __init__(self, bitmap, bitmap_bytes, rgb, rgb_bytes, pix, pix_bytes, type, type_bytes, enc=None):
        self.bitmap, self.bitmap_bytes = [int(v or 0) for v in bitmap], [int(v) for v in bitmap_bytes]
        self.rgb, self.rgb_bytes = [int(v or 0) for v in rgb], [int(v) for v in rgb_bytes]
        self.pix, self.pix_bytes, self.type, self.type_bytes = int(pix or 0), int(pix_bytes), int(type or 0), int(type_bytes)
        self._enc = enc

    def download(self) -> dict:
        """{"rgb": [7 uint8 arrays], "pix": uint8 array, "type": uint8 array}: the frame's streams copied to the host (yk_device_download: on the
        encoder's stream, synchronises it).  For tests and file writers."""
        enc = self._enc
        if enc is None or not getattr(enc, "_h", None):
            raise YaikError("these FrameStreams belong to no live encoder")

        def get(ptr, n):
            out = np.empty(n, dtype=np.uint8)
            if n:
                _chk(enc._h, enc._L.yk_device_download(enc._h, out.ctypes.data, C.c_void_p(ptr), n))
            return out

        return {"rgb": [get(p, n) for p, n in zip(self.rgb, self.rgb_bytes)], "pix": get(self.pix, self.pix_bytes), "type": get(self.type, self.type_bytes)}


STREAMS_CORNERS, STREAMS_RANGE1D = 1, 2             # YK_STREAMS_* of include/yaik_hip.h


class HipTileEncoder:
    """One handle = one GPU = one image or one row stripe of an image."""

    def __init__(self, device: int = 0, hooks: bool = False):
        """hooks=True: a handle of the TEST build of the library (include/yaik_hip_test.h: self-tests, ablations, cross-check kernel) --
        test infrastructure; the product path never asks for it."""
        from ._lib import test_lib
        L = test_lib() if hooks else lib()
        self._L = L
        h = C.c_void_p()
        rc = L.yk_create(device, C.byref(h))
        if rc != 0:
            raise YaikError(f"yk_create failed ({rc}): no usable HIP device -- the product path has no CPU fallback")
        self._h = h
        _HANDLE_LIB[h.value] = L
        self._keepalive = None
        self._mip_boxes = None          # the tile boxes of the last yk_alpha_bitmaps_batch; whether its bits still hold is the library's to say
        self.w = self.h = self.n = 0
        self.frames = 1                 # images bound: 1, or the F of set_batch / set_batch_u8

    def close(self):
        if getattr(self, "_h", None):
            _HANDLE_LIB.pop(self._h.value, None)
            self._L.yk_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    # ---- EncoderContext::SetImageToEncode ----------------------------------------------------------
    def set_image(self, planes, full_h: int | None = None, y0: int = 0, halo_rows: int = 0):
        """planes: numpy int32 [n, rows, w] (uploaded) or torch int32 cuda tensor [n, rows, w] (bound in place).
        rows = owned rows + halo_rows."""
        L = self._L
        is_torch = hasattr(planes, "data_ptr")
        n, rows, w = planes.shape
        h = rows - halo_rows
        self.n, self.h, self.w, self.frames = n, h, w, 1
        self.full_h = full_h if full_h is not None else h
        self.y0 = y0
        _chk(self._h, L.yk_set_image(self._h, w, self.full_h, n, y0, h, halo_rows))
        if is_torch:
            import torch
            assert planes.dtype == torch.int32 and planes.is_cuda and planes.is_contiguous()
            base = planes.data_ptr()
            ptrs = (C.c_void_p * 4)(*[base + i * rows * w * 4 if i < n else None for i in range(4)])
            # The handle launches on its own non-blocking stream, which is not ordered against torch's streams (measured: a kernel
            # launched here right after a torch kernel reads stale planes).  The hand-over is therefore a host-side fence; results
            # handed back to torch are fenced the same way (every getter and yk_export_tile_maps synchronise the handle's stream).
            # (_lib.lib() brings torch's bundled HIP runtime up first, so that this library binds to the same runtime instance.)
            torch.cuda.current_stream(planes.device).synchronize()
            _chk(self._h, L.yk_bind_device_planes(self._h, ptrs, w))
        else:
            planes = np.ascontiguousarray(planes, dtype=np.int32)
            ptrs = (C.c_void_p * 4)(*[planes[i].ctypes.data if i < n else None for i in range(4)])
            _chk(self._h, L.yk_upload_planes(self._h, ptrs, w))
            _chk(self._h, L.yk_synchronize(self._h))
        self._keepalive = planes

    def set_image_u8(self, pixels, full_h: int | None = None, y0: int = 0, halo_rows: int = 0, n_planes: int | None = None):
        """8-bit interleaved pixels [rows, w, C] (C = 3 RGB or 4 RGBA; rows = owned rows + halo_rows), widened on the GPU into the handle's
        own int32 planes: numpy uint8 is uploaded (yk_upload_pixels_u8: one byte per sample crosses PCIe), a torch uint8 CUDA tensor is read
        where it lies (yk_load_device_pixels_u8).  n_planes defaults to C (RGBA into 3 planes drops the 4th byte).  The row pitch is the
        array's row stride (u8_pixel_layout): padded or row-sliced views need no copy."""
        L = self._L
        is_torch = hasattr(pixels, "data_ptr")
        if not is_torch:
            pixels = np.asarray(pixels)
        lay = u8_pixel_layout(pixels, n_planes)
        h = lay.rows - halo_rows
        self.n, self.h, self.w, self.frames = lay.n_planes, h, lay.w, 1
        self.full_h = full_h if full_h is not None else h
        self.y0 = y0
        _chk(self._h, L.yk_set_image(self._h, lay.w, self.full_h, lay.n_planes, y0, h, halo_rows))
        if is_torch:
            import torch
            assert pixels.is_cuda
            torch.cuda.current_stream(pixels.device).synchronize()          # hand-over fence, see set_image
            _chk(self._h, L.yk_load_device_pixels_u8(self._h, C.c_void_p(pixels.data_ptr()), lay.row_bytes, lay.frame_bytes, lay.channels))
        else:
            _chk(self._h, L.yk_upload_pixels_u8(self._h, C.c_void_p(pixels.ctypes.data), lay.row_bytes, lay.channels))
        self._keepalive = pixels

    def validate_planes(self) -> int:
        """Samples of the bound planes outside 0..255 (the precondition of the path; yk_upload_planes enforces it itself)."""
        n = C.c_size_t(0)
        _chk(self._h, self._L.yk_validate_planes(self._h, C.byref(n)))
        return int(n.value)

    # ---- EncoderContext::MipPrefilter ---------------------------------------------------------------
    def alpha_reject(self):
        _chk(self._h, self._L.yk_alpha_reject(self._h))

    def stripe_bbox(self) -> np.ndarray:
        b = np.zeros(4, dtype=np.int32)
        _chk(self._h, self._L.yk_get_stripe_bbox(self._h, b.ctypes.data))
        return b

    def alpha_finish(self, global_bbox: np.ndarray | None = None):
        if global_bbox is None:
            _chk(self._h, self._L.yk_alpha_finish(self._h, None))
        else:
            g = np.ascontiguousarray(global_bbox, dtype=np.int32)
            _chk(self._h, self._L.yk_alpha_finish(self._h, g.ctypes.data))

    def mip_prefilter(self) -> dict:
        """Whole-image EncoderContext::MipPrefilter: reject + finish + results."""
        if self.n == 4:
            self.alpha_reject()
            self.alpha_finish(None)
        return self.alpha_result()

    def alpha_result(self) -> dict:
        L = self._L
        b = np.zeros(4, dtype=np.int32); tb = np.zeros(4, dtype=np.int32)
        has, rem = C.c_int(), C.c_int()
        _chk(self._h, L.yk_alpha_result(self._h, b.ctypes.data, C.byref(has), C.byref(rem), tb.ctypes.data))
        out = np.zeros(((self.w + 15) // 16) * ((self.full_h + 15) // 16) // 8 + 8, dtype=np.uint8)   # a side of 8 mod 16 ends in a part tile
        nb = C.c_size_t()
        _chk(self._h, L.yk_alpha_bitmap(self._h, out.ctypes.data, out.size, C.byref(nb)))
        return {"has_chunk": bool(has.value), "bounds": b, "remaining": rem.value, "tile_bbox": tb, "bitmap": out[:nb.value].copy()}

    def alpha_values(self, force8bit: bool = True) -> dict | None:
        """EncoderContext::ProcessAlpha(force8bit) on the GPU (yk_alpha_values), after mip_prefilter(); force8bit=False gives analog alpha in the
        6-bit mask mode (3).  None when no 'ALPM' chunk is written, else
        {"mode": AlphaHeader::parameters, "bbox": (x, y, w, h), "payload": decompressed payload (u8)}."""

        class _Info(C.Structure):
            _fields_ = [("mode", C.c_int32), ("bbox", C.c_int32 * 4), ("rawSize", C.c_uint32)]

        info, n = _Info(), C.c_size_t()
        out = np.empty(self.w * self.full_h, dtype=np.uint8)       # the payload is at most one byte per pixel
        _chk(self._h, self._L.yk_alpha_values(self._h, int(force8bit), C.byref(info), out.ctypes.data, out.size, C.byref(n)))
        if info.mode < 0:
            return None
        return {"mode": int(info.mode), "bbox": tuple(int(v) for v in info.bbox), "payload": out[:n.value].copy()}

    def _alpha_values_batch(self) -> list:
        class _Info(C.Structure):
            _fields_ = [("mode", C.c_int32), ("bbox", C.c_int32 * 4), ("rawSize", C.c_uint32)]

        infos = (_Info * self.frames)()
        _chk(self._h, self._L.yk_alpha_values_batch(self._h, 1, infos))
        return [None if i.mode < 0 else (int(i.mode), tuple(int(v) for v in i.bbox), int(i.rawSize)) for i in infos]

    def alpha_values_batch(self) -> list:
        """ProcessAlpha(true) for every frame of the handle (yk_alpha_values_batch), after encode_batch() (or, for one frame, mip_prefilter()):
        per frame the dict of alpha_values(), or None where no 'ALPM' chunk is written.  Three launches and two read-backs for the whole batch;
        the payloads are then copied out frame by frame (alpha_payloads_device leaves them in HBM)."""
        out = []
        for f, e in enumerate(self._alpha_values_batch()):
            if e is None:
                out.append(None)
                continue
            pay, n = np.empty(e[2], dtype=np.uint8), C.c_size_t()
            _chk(self._h, self._L.yk_alpha_payload(self._h, f, pay.ctypes.data if pay.size else None, pay.size, C.byref(n)))
            out.append({"mode": e[0], "bbox": e[1], "payload": pay[:n.value]})
        return out

    def alpha_payloads_device(self) -> list:
        """alpha_values_batch() without copying the payloads out: per frame None or (mode, bbox, device pointer, nbytes), the entries
        HipTileDecoder.decompress_alpha_batch takes.  The payloads are written on this handle's stream (synchronize() or a stream hand-off before
        another stream reads them) and stay valid until the next encode, set_image / set_batch or alpha_values[_batch] of the handle."""
        out = []
        for f, e in enumerate(self._alpha_values_batch()):
            if e is None:
                out.append(None)
                continue
            dev, n = C.c_void_p(), C.c_size_t()
            _chk(self._h, self._L.yk_alpha_payload_device(self._h, f, C.byref(dev), C.byref(n)))
            out.append((e[0], e[1], int(dev.value or 0), int(n.value)))
        return out

    def _force8bit_flags(self, force8bit):
        """None (0 for every frame: NULL), a bool (every frame) or a sequence of `frames` bools -> the uint8 array yk_alpha_values_mask_batch
        takes, or None.  A wrong length raises ValueError: nothing has been called yet."""
        if force8bit is None:
            return None
        if isinstance(force8bit, (bool, np.bool_)):
            return np.full(self.frames, 1 if force8bit else 0, dtype=np.uint8)
        flags = np.array([1 if v else 0 for v in force8bit], dtype=np.uint8)
        if flags.size != self.frames:
            raise ValueError(f"{flags.size} force8bit flags for a batch of {self.frames} frames")
        return flags

    def _alpha_values_mask_batch(self, force8bit) -> list:
        class _Info(C.Structure):
            _fields_ = [("mode", C.c_int32), ("bbox", C.c_int32 * 4), ("rawSize", C.c_uint32)]

        flags = self._force8bit_flags(force8bit)
        infos = (_Info * self.frames)()
        _chk(self._h, self._L.yk_alpha_values_mask_batch(self._h, None if flags is None else flags.ctypes.data, infos))
        return [None if i.mode < 0 else (int(i.mode), tuple(int(v) for v in i.bbox), int(i.rawSize)) for i in infos]

    def alpha_values_mask_batch(self, force8bit=None) -> list:
        """ProcessAlpha(force8bit[f]) for every frame of the handle (yk_alpha_values_mask_batch), after encode_batch() (or, for one frame,
        mip_prefilter()): per frame the dict of alpha_values(force8bit[f]), or None where no 'ALPM' chunk is written.  force8bit is None (the
        6-bit mask mode for every analog frame), a bool, or one bool per frame.  At most six launches and three read-backs for the whole batch;
        the payloads are then copied out frame by frame (alpha_mask_payloads_device leaves them in HBM)."""
        out = []
        for f, e in enumerate(self._alpha_values_mask_batch(force8bit)):
            if e is None:
                out.append(None)
                continue
            pay, n = np.empty(e[2], dtype=np.uint8), C.c_size_t()
            _chk(self._h, self._L.yk_alpha_payload(self._h, f, pay.ctypes.data if pay.size else None, pay.size, C.byref(n)))
            out.append({"mode": e[0], "bbox": e[1], "payload": pay[:n.value]})
        return out

    def alpha_mask_payloads_device(self, force8bit=None) -> list:
        """alpha_values_mask_batch() without copying the payloads out: per frame None or (mode, bbox, device pointer, nbytes, 'MIPM' bits
        pointer, their length, tile box), the entries HipTileDecoder.decompress_alpha_batch takes for masked frames.  The bits are those of the
        last alpha_bitmaps_device() of this handle while yk_alpha_bitmap_device still hands them out (until the next encode, alpha_reject,
        set_image / set_batch), else pointer 0, length 0 and the box (0, 0, 0, 0) -- a mode-3 entry then cannot be decoded.  Validity as for alpha_payloads_device."""
        entries = self._alpha_values_mask_batch(force8bit)
        out = []
        for f, e in enumerate(entries):
            if e is None:
                out.append(None)
                continue
            dev, n = C.c_void_p(), C.c_size_t()
            _chk(self._h, self._L.yk_alpha_payload_device(self._h, f, C.byref(dev), C.byref(n)))
            # the library says whether the bits of yk_alpha_bitmaps_batch still hold (it refuses once they are gone): one validity rule
            bits, nbits = C.c_void_p(), C.c_size_t()
            have = self._mip_boxes is not None and self._L.yk_alpha_bitmap_device(self._h, f, C.byref(bits), C.byref(nbits)) == 0 and nbits.value
            out.append((e[0], e[1], int(dev.value or 0), int(n.value)) + ((int(bits.value), int(nbits.value), self._mip_boxes[f]) if have else (0, 0, (0, 0, 0, 0))))
        return out

    def _alpha_bitmaps_batch(self):
        infos = (_MipInfoC * self.frames)()
        _chk(self._h, self._L.yk_alpha_bitmaps_batch(self._h, infos))
        self._mip_boxes = [tuple(int(v) for v in i.tileBBox) for i in infos]       # alpha_mask_payloads_device hands them on with the bits
        return infos

    def alpha_bitmaps_device(self) -> list:
        """The 'MIPM' bitmaps of every frame (yk_alpha_bitmaps_batch: one launch and one read-back for the whole batch), left in HBM: per frame
        {"has_chunk", "bounds", "tile_bbox", "ptr", "nbytes"} (ptr 0 and nbytes 0 for a frame without bits).  After encode_batch() (or, with one
        frame, mip_prefilter()).  The bits are written on this handle's stream and stay valid until the next encode, alpha_reject, set_image /
        set_batch of the handle."""
        out = []
        for f, i in enumerate(self._alpha_bitmaps_batch()):
            dev, n = C.c_void_p(), C.c_size_t()
            _chk(self._h, self._L.yk_alpha_bitmap_device(self._h, f, C.byref(dev), C.byref(n)))
            out.append({"has_chunk": bool(i.hasChunk), "bounds": np.array(list(i.bounds), np.int32), "tile_bbox": np.array(list(i.tileBBox), np.int32),
                        "ptr": int(dev.value or 0), "nbytes": int(n.value)})
        return out

    def alpha_bitmaps_batch(self) -> list:
        """alpha_bitmaps_device() with the bits copied out: per frame the dict of alpha_result() without "remaining"."""
        out = []
        for e in self.alpha_bitmaps_device():
            bits = np.zeros(e["nbytes"], np.uint8)
            if bits.size:
                _chk(self._h, self._L.yk_device_download(self._h, bits.ctypes.data, C.c_void_p(e["ptr"]), bits.size))
            out.append({"has_chunk": e["has_chunk"], "bounds": e["bounds"], "tile_bbox": e["tile_bbox"], "bitmap": bits})
        return out

    gather_layout = staticmethod(gather_layout)

    def gather(self, ptrs, nbytes, out=None):
        """yk_device_gather: the segments (device addresses `ptrs`, lengths `nbytes`; a length of 0 may come with address 0) into `out`, a
        contiguous torch uint8 CUDA tensor whose address is a multiple of 16, at the offsets of gather_layout().  One launch on this handle's
        stream, no synchronisation: synchronize() (or a stream hand-off) before another stream reads `out`.  out=None is the size query.
        Returns (offsets, total)."""
        n = len(nbytes)
        src = (C.c_void_p * max(n, 1))(*[int(p) if p else None for p in ptrs])
        lens = (C.c_size_t * max(n, 1))(*[int(v) for v in nbytes])
        offs, total = (C.c_size_t * max(n, 1))(), C.c_size_t()
        if out is None:
            dst, cap = None, 0
        else:
            import torch
            assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
            torch.cuda.current_stream(out.device).synchronize()           # hand-over fence, see set_image
            dst, cap = C.c_void_p(out.data_ptr()), out.numel()
        _chk(self._h, self._L.yk_device_gather(self._h, src, lens, n, dst, cap, offs, C.byref(total)))
        return np.array(list(offs)[:n], np.int64), int(total.value)

    # ---- 7x FittingQuadSmooth + 3x DynamicTileEncode, one launch ---------------------------------------
    def encode(self, reject_factor: int = 3, mode3bit_only: bool = False, want_dst: bool = False, dst_fill: int = -1):
        L = self._L
        _chk(self._h, L.yk_set_dst_fill(self._h, dst_fill))
        _chk(self._h, L.yk_encode_tiles(self._h, reject_factor, int(mode3bit_only), int(want_dst)))

    def set_batch(self, frames):
        """frames: torch int32 cuda tensor [F, n, h, w] (contiguous): F equally shaped images bound in place (yk_set_batch)."""
        import torch
        L = self._L
        assert frames.dtype == torch.int32 and frames.is_cuda and frames.is_contiguous() and frames.dim() == 4
        F, n, h, w = frames.shape
        self.n, self.h, self.w, self.full_h, self.y0, self.frames = n, h, w, h, 0, F
        _chk(self._h, L.yk_set_image(self._h, w, h, n, 0, h, 0))
        _chk(self._h, L.yk_set_batch(self._h, F))
        torch.cuda.current_stream(frames.device).synchronize()          # hand-over fence, see set_image
        base = frames.data_ptr()
        ptrs = (C.c_void_p * 4)(*[base + i * h * w * 4 if i < n else None for i in range(4)])
        _chk(self._h, L.yk_bind_device_batch(self._h, ptrs, w, n * h * w))
        self._keepalive = frames

    def set_batch_u8(self, frames, n_planes: int | None = None):
        """frames: torch uint8 CUDA tensor [F, h, w, C]: F equally shaped 8-bit images widened, in one launch, into the handle's own planes
        (yk_set_batch + yk_load_device_pixels_u8).  Row pitch and frame stride come from the tensor's strides (u8_pixel_layout)."""
        import torch
        L = self._L
        lay = u8_pixel_layout(frames, n_planes, batch=True)
        assert frames.is_cuda
        self.n, self.h, self.w, self.full_h, self.y0, self.frames = lay.n_planes, lay.rows, lay.w, lay.rows, 0, lay.frames
        _chk(self._h, L.yk_set_image(self._h, lay.w, lay.rows, lay.n_planes, 0, lay.rows, 0))
        _chk(self._h, L.yk_set_batch(self._h, lay.frames))
        torch.cuda.current_stream(frames.device).synchronize()          # hand-over fence, see set_image
        _chk(self._h, L.yk_load_device_pixels_u8(self._h, C.c_void_p(frames.data_ptr()), lay.row_bytes, lay.frame_bytes, lay.channels))
        self._keepalive = frames

    def encode_batch(self, reject_factor: int = 3, mode3bit_only: bool = False):
        _chk(self._h, self._L.yk_encode_batch(self._h, reject_factor, int(mode3bit_only)))

    def streams_batch(self, corners: bool = True, range1d: bool = True) -> list:
        """The corner colour streams and / or the 1-D streams of EVERY frame of the handle (yk_encode_streams_batch + yk_batch_streams_table: one
        launch per kernel and one read-back for the whole batch), after encode_batch() -- or, with one frame bound, after encode() / encode_frame().
        Returns one FrameStreams per frame.  The streams lie packed in the encoder's HBM and are written on its stream: synchronize() (or a
        stream hand-off) before another stream reads them; they stay valid until the next encode, set_image / set_batch or streams_batch.
        select_frame and the single-image getters (gradient_corners, dynamic_tile_compressor) do not disturb them."""
        what = (STREAMS_CORNERS if corners else 0) | (STREAMS_RANGE1D if range1d else 0)
        _chk(self._h, self._L.yk_encode_streams_batch(self._h, what))
        tab = (_FrameStreamsC * self.frames)()
        _chk(self._h, self._L.yk_batch_streams_table(self._h, tab))
        return [FrameStreams(list(t.bitmap), list(t.bitmapBytes), list(t.rgb), list(t.rgbBytes), t.pix, t.pixBytes, t.type, t.typeBytes, self) for t in tab]

    def streams_table(self) -> list:
        """The FrameStreams of the last streams_batch() again (yk_batch_streams_table alone): nothing is launched, and the streams and the
        palette payloads made from them stay valid.  Refused by the library when there is no valid table."""
        tab = (_FrameStreamsC * self.frames)()
        _chk(self._h, self._L.yk_batch_streams_table(self._h, tab))
        return [FrameStreams(list(t.bitmap), list(t.bitmapBytes), list(t.rgb), list(t.rgbBytes), t.pix, t.pixBytes, t.type, t.typeBytes, self) for t in tab]

    # ---- PaletteCompressor (EncoderContext.cpp:3259-3502) on the GPU: the 'GTIL' colour payloads -----------------
    def palette_reset(self):
        """Forgets the 64 code-book rows that carry from call to call (PaletteResetCodeBook: a fresh process)."""
        _chk(self._h, self._L.yk_palette_reset(self._h))

    def palette_compress(self) -> int:
        """The seven corner streams of the selected frame through PaletteCompressor, continuing the handle's carried rows (yk_palette_compress),
        after encode().  Returns the number of payloads (7); palette_payload(p) / palette_payload_device(p) hand them out."""
        _chk(self._h, self._L.yk_palette_compress(self._h))
        self._palette_n = 7
        return 7

    def palette_compress_batch(self) -> int:
        """The corner streams of every frame after streams_batch(corners=True), every frame from a fresh book (yk_palette_compress_batch).
        Payload frame * 7 + pass.  Returns the number of payloads."""
        _chk(self._h, self._L.yk_palette_compress_batch(self._h))
        self._palette_n = 7 * self.frames
        return self._palette_n

    def palette_compress_streams(self, tensors, chain: int = 0) -> int:
        """PaletteCompressor over arbitrary colour streams in device memory: `tensors` is a sequence of 1-D contiguous uint8 CUDA tensors whose
        lengths are multiples of 3 (length 0: skipped, the book stays).  chain = K > 0: every run of K consecutive streams starts from a fresh
        book; chain = 0: the streams continue the handle's carried rows.  CPU tensors and bad chain values are refused before any library
        call.  Returns the number of payloads."""
        import torch
        if isinstance(chain, bool) or not isinstance(chain, int) or chain < 0:
            raise ValueError(f"chain must be an int >= 0 (0 = continue the carried book, K = run length); got {chain!r}")
        tensors = list(tensors)
        if not tensors:
            raise ValueError("at least one stream is needed")
        for i, t in enumerate(tensors):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"stream {i} is not a torch tensor")
            if not t.is_cuda:
                raise ValueError(f"stream {i} is a CPU tensor: the streams must lie in device memory")
            if t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous():
                raise ValueError(f"stream {i} must be a 1-D contiguous uint8 tensor")
            if t.numel() % 3:
                raise ValueError(f"stream {i} holds {t.numel()} bytes, not a multiple of 3")
        n = len(tensors)
        ptrs = (C.c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in tensors])
        lens = (C.c_size_t * n)(*[t.numel() for t in tensors])
        torch.cuda.current_stream(tensors[0].device).synchronize()          # hand-over fence, see set_image
        _chk(self._h, self._L.yk_palette_compress_streams(self._h, ptrs, lens, n, chain))
        self._palette_keepalive = tensors
        self._palette_n = n
        return n

    def palette_payload(self, i: int) -> np.ndarray:
        """Payload i of the last palette_compress* call, copied to the host (synchronises)."""
        n = C.c_size_t()
        _chk(self._h, self._L.yk_palette_payload(self._h, i, None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.uint8)
        if out.size:
            _chk(self._h, self._L.yk_palette_payload(self._h, i, out.ctypes.data, out.size, None))
        return out

    def palette_payload_device(self, i: int):
        """Payload i where it lies in HBM, as a uint8 tensor view of the handle's buffer (written on the handle's stream; stale after the next
        encode, set_image / set_batch, streams_batch or palette_compress*)."""
        import torch
        dev, n = C.c_void_p(), C.c_size_t()
        _chk(self._h, self._L.yk_palette_payload_device(self._h, i, C.byref(dev), C.byref(n)))
        if not n.value:
            return torch.empty(0, dtype=torch.uint8, device="cuda")

        class _View:                                                        # __cuda_array_interface__: a view, not a copy
            __cuda_array_interface__ = {"shape": (int(n.value),), "typestr": "|u1", "data": (int(dev.value), False), "version": 2}

        return torch.as_tensor(_View(), device="cuda")

    def order_fused_after(self, other: "HipTileEncoder"):
        """The next encode() of this handle starts its fused kernel after the fused kernel last launched on `other` has finished
        (device-side wait; see yk_order_fused_after)."""
        _chk(self._h, self._L.yk_order_fused_after(self._h, other._h))

    def set_pixel_cache(self, on: bool = True):
        """From the next encode() on, the fused kernel leaves the packed pixels of the cells it did not cover for the live 1-D path
        (dynamic_tile_compressor), which then reads 4 B per pixel from there instead of 12 B from the planes (yk_set_pixel_cache)."""
        _chk(self._h, self._L.yk_set_pixel_cache(self._h, 1 if on else 0))

    def select_frame(self, f: int):
        _chk(self._h, self._L.yk_select_frame(self._h, f))

    def encode_frame(self, reject_factor: int = 3, mode3bit_only: bool = False):
        """alpha reject + fused kernel + compaction as one replayed hipGraph launch (whole images; see yk_encode_frame)."""
        _chk(self._h, self._L.yk_encode_frame(self._h, reject_factor, int(mode3bit_only)))

    def synchronize(self):
        _chk(self._h, self._L.yk_synchronize(self._h))

    def gradient_bitmap(self, p: int) -> np.ndarray:
        L = self._L
        n = L.yk_gradient_bitmap_bytes(self._h, p)
        out = np.zeros(n, dtype=np.uint8)
        _chk(self._h, L.yk_gradient_bitmap(self._h, p, out.ctypes.data, n))
        return out

    def gradient_counts(self) -> np.ndarray:
        c = np.zeros(7, dtype=np.int32)
        _chk(self._h, self._L.yk_gradient_counts(self._h, c.ctypes.data))
        return c

    def coverage(self) -> np.ndarray:
        """[h/4, w/4] bool: 4x4 cell covered by an accepted gradient tile (smoothMap != 0)."""
        mtw, mth = (self.w + 15) // 16, (self.h + 15) // 16
        raw = np.zeros(mtw * mth, dtype=np.uint16)
        _chk(self._h, self._L.yk_coverage(self._h, raw.ctypes.data, raw.size))
        bits = (raw.reshape(mth, mtw, 1) >> np.arange(16, dtype=np.uint16)) & 1
        cells = bits.reshape(mth, mtw, 4, 4).transpose(0, 2, 1, 3).reshape(mth * 4, mtw * 4)
        return cells[: self.h // 4, : self.w // 4].astype(bool)

    def gradient_corners(self, p: int) -> np.ndarray:
        cap = (self.w // 4 + 1) * (self.h // 4 + 2) * 3 + 16
        out = np.zeros(cap, dtype=np.uint8)
        nb = C.c_size_t()
        _chk(self._h, self._L.yk_gradient_corners(self._h, p, out.ctypes.data, cap, C.byref(nb)))
        return out[:nb.value].copy()

    # ---- FittingQuadSmooth with NULL planes (EncoderContext.cpp:3710, call sites :9261-9415) ---------------
    def fitting_quad_smooth_planes(self, plane_bit: int, sx: int = 2, sy: int = 2, reject_factor: int = 3):
        """One more gradient pass over the planes of `plane_bit` (bit0/1/2 = R/G/B present), after encode_tiles().
        Returns (tiles accepted, swizzled bitmap bytes, corner stream bytes) like the reference's TileDone / pFillBitMap / rgbStream."""
        L = self._L
        n = C.c_int()
        _chk(self._h, L.yk_gradient_partial_pass(self._h, reject_factor, plane_bit, sx, sy, C.byref(n)))
        nb = C.c_size_t()
        _chk(self._h, L.yk_partial_bitmap(self._h, None, 0, C.byref(nb)))
        bm = np.zeros(nb.value, dtype=np.uint8)
        if bm.size:
            _chk(self._h, L.yk_partial_bitmap(self._h, bm.ctypes.data, bm.size, None))
        _chk(self._h, L.yk_partial_corners(self._h, None, 0, C.byref(nb)))
        cs = np.zeros(nb.value, dtype=np.uint8)
        if cs.size:
            _chk(self._h, L.yk_partial_corners(self._h, cs.ctypes.data, cs.size, None))
        return int(n.value), bm, cs

    def gradient_preview(self, passes=range(7)) -> np.ndarray:
        """FittingQuadSmooth's testOutput planes [3, h, w] int32 after the given passes (7 = the last plane-subset pass); INT32_MIN = untouched."""
        out = np.zeros((3, self.h, self.w), dtype=np.int32)
        for p in passes:
            _chk(self._h, self._L.yk_gradient_preview(self._h, int(p), out.ctypes.data, out.size))
        return out

    def coverage_plane(self, plane: int) -> np.ndarray:
        """[h/4, w/4] bool: 4x4 cell of `plane` covered by an accepted tile (mapSmoothTile[plane] != 0)."""
        mtw, mth = (self.w + 15) // 16, (self.h + 15) // 16
        raw = np.zeros(mtw * mth, dtype=np.uint16)
        _chk(self._h, self._L.yk_coverage_plane(self._h, plane, raw.ctypes.data, raw.size))
        bits = (raw.reshape(mth, mtw, 1) >> np.arange(16, dtype=np.uint16)) & 1
        cells = bits.reshape(mth, mtw, 4, 4).transpose(0, 2, 1, 3).reshape(mth * 4, mtw * 4)
        return cells[: self.h // 4, : self.w // 4].astype(bool)

    # ---- (f)4 3-D LUT tiles (Load3DPattern / StartCorrelationSearch / Correlation3DSearch) ----------------------------
    def lut_clear(self) -> None:
        _chk(self._h, self._L.yk_lut_clear(self._h))

    def lut_load(self, pattern: np.ndarray) -> int:
        """pattern: uint8 [count, 3] with 6-bit coordinates (one Bank3D .lut file).  Returns the pattern's number."""
        p = np.ascontiguousarray(pattern, dtype=np.uint8)
        r, g, b = (np.ascontiguousarray(p[:, k]) for k in range(3))
        idx = C.c_int()
        _chk(self._h, self._L.yk_lut_load_pattern(self._h, r.ctypes.data, g.ctypes.data, b.ctypes.data, len(p), C.byref(idx)))
        return int(idx.value)

    def lut_tables(self, k: int):
        fac = np.zeros((4, 3, 64), np.int16); dist = np.zeros(64 ** 3, np.uint16); pos = np.zeros((4, 64 ** 3), np.uint8)
        _chk(self._h, self._L.yk_lut_pattern_tables(self._h, k, fac.ctypes.data, dist.ctypes.data, pos.ctypes.data))
        return fac, dist, pos

    def lut_start(self) -> None:
        _chk(self._h, self._L.yk_lut_start(self._h))

    def lut_search(self, sx: int, sy: int) -> int:
        n = C.c_int()
        _chk(self._h, self._L.yk_lut_search(self._h, sx, sy, C.byref(n)))
        return int(n.value)

    def lut_streams(self) -> dict:
        L = self._L
        out = {}
        names = ["tileType", "color", "idx3", "idx4", "idx5", "idx6"] + [f"map{k}" for k in range(6)]
        for which, name in enumerate(names):
            nb = C.c_size_t()
            _chk(self._h, L.yk_lut_stream(self._h, which, None, 0, C.byref(nb)))
            buf = np.zeros(nb.value, np.uint8)
            if buf.size:
                _chk(self._h, L.yk_lut_stream(self._h, which, buf.ctypes.data, buf.size, None))
            out[name] = buf.view(np.uint16) if name == "tileType" else buf
        return out

    def gradient_corner_edges(self):
        """(keys[2, w/4+1], index[2, w/4+1]) of the stripe's first and last lattice rows (see yk_gradient_corner_edges)."""
        n = self.w // 4 + 1
        keys = np.zeros((2, n), dtype=np.uint32); idx = np.zeros((2, n), dtype=np.uint32)
        _chk(self._h, self._L.yk_gradient_corner_edges(self._h, keys.ctypes.data, idx.ctypes.data, 2 * n))
        return keys, idx

    def range_streams(self, plane: int):
        L = self._L
        nd, nn = C.c_size_t(), C.c_size_t()
        _chk(self._h, L.yk_range_sizes(self._h, plane, C.byref(nd), C.byref(nn)))
        defs = np.zeros(nd.value, dtype=np.uint16)
        nib = np.zeros((nn.value + 1) // 2, dtype=np.uint8)
        _chk(self._h, L.yk_range_streams(self._h, plane, defs.ctypes.data if defs.size else None, defs.size,
                                          nib.ctypes.data if nib.size else None, nib.size))
        return defs, nib, nn.value

    def range_dst(self, plane: int) -> np.ndarray:
        out = np.zeros((self.h, self.w), dtype=np.int32)
        _chk(self._h, self._L.yk_range_dst(self._h, plane, out.ctypes.data, out.size))
        return out

    # ---- 3x DynamicTileCompressor (live 1-D range path, '1DTL') -----------------------------------------
    def dynamic_tile_compressor(self):
        """Returns (pix_stream, type_stream) exactly as GenerateDynamicTileChunk receives them."""
        L = self._L
        _chk(self._h, L.yk_range1d_encode(self._h))
        npx, nty = C.c_size_t(), C.c_size_t()
        _chk(self._h, L.yk_range1d_streams(self._h, None, 0, C.byref(npx), None, 0, C.byref(nty)))
        pix = np.zeros(npx.value, dtype=np.uint8); typ = np.zeros(nty.value, dtype=np.uint8)
        _chk(self._h, L.yk_range1d_streams(self._h, pix.ctypes.data if pix.size else None, pix.size, None,
                                            typ.ctypes.data if typ.size else None, typ.size, None))
        return pix, typ

    def gradient_corners_run(self) -> None:
        """Builds the seven corner streams on the device (no copy to the host)."""
        _chk(self._h, self._L.yk_gradient_corners_run(self._h))

    def stage_ms(self, stage: int) -> tuple[float, int]:
        """(sum of the event-timed kernel intervals of a YK_STAGE_* since the last query, number of intervals)."""
        ms, n = C.c_float(), C.c_int()
        _chk(self._h, self._L.yk_stage_ms(self._h, stage, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def export_capacity(self) -> int:
        return int(self._L.yk_export_capacity(self._h))

    def export_tile_maps(self, dev_buffer) -> np.ndarray:
        """dev_buffer: torch uint8 cuda tensor of >= export_capacity() bytes. Returns the 15 section sizes."""
        sizes = np.zeros(15, dtype=np.uint64)
        # hand-over fence (see set_image): whatever torch still has queued on the buffer (its allocation fill, an earlier consumer) must be
        # done before the handle's own stream writes into it -- the two streams are not ordered against each other
        import torch
        torch.cuda.current_stream(dev_buffer.device).synchronize()
        _chk(self._h, self._L.yk_export_tile_maps(self._h, C.c_void_p(dev_buffer.data_ptr()), dev_buffer.numel(), sizes.ctypes.data))
        return sizes

    def export_tile_maps_async(self, dev_buffer, dev_meta16, consumer_stream: int = 0) -> None:
        """No host synchronisation: dev_meta16 (torch int64[16] cuda tensor) receives {total bytes, sizes[0..14]}; work queued
        afterwards on `consumer_stream` (a hipStream_t of the same runtime, 0 = null stream) sees buffer and table complete.
        The caller orders EARLIER work on the two buffers before the handle's stream itself (yk_stream_wait_for, or buffers that are idle)."""
        _chk(self._h, self._L.yk_export_tile_maps_async(self._h, C.c_void_p(dev_buffer.data_ptr()), dev_buffer.numel(),
                                                      C.c_void_p(dev_meta16.data_ptr()), C.c_void_p(consumer_stream)))

    def export_tile_maps_framed(self, dev_buffer, consumer_stream: int | None = 0) -> None:
        """The form the gather moves (yk_export_tile_maps_framed): dev_buffer[0:128] = header {payload bytes, sizes[0..14]}, the sections
        behind it; no host synchronisation.  Work queued afterwards on `consumer_stream` (0 = null stream; None = no hand-over) sees the
        buffer.  The caller orders EARLIER work on the buffer before the handle's stream (idle buffers, or yk_stream_wait_for)."""
        cs = C.c_void_p(-1 & 0xFFFFFFFFFFFFFFFF) if consumer_stream is None else C.c_void_p(consumer_stream)
        _chk(self._h, self._L.yk_export_tile_maps_framed(self._h, C.c_void_p(dev_buffer.data_ptr()), dev_buffer.numel(), cs))

    def kernel_ms(self) -> dict:
        e, a, p = C.c_float(), C.c_float(), C.c_float()
        _chk(self._h, self._L.yk_last_kernel_ms(self._h, C.byref(e), C.byref(a), C.byref(p)))
        return {"encode": e.value, "alpha": a.value, "pack": p.value}
