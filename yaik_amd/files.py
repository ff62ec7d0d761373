"""`.yaik` files to pixels on the GPU: a ctypes binding of the C++ drop-in decoder (yaik_amd/host/libyaik_host.so, yaik_decode.h).

decode_file_device(stream)    one stream through YAIK_DecodeImageToDevice: uint8 [H, W, 3], or [H, W, 4] when the stream has an 'ALPM' chunk
decode_file_window_device(stream, window)   a rectangle of it through YAIK_DecodeImageWindowToDevice: only the tiles the window needs are rendered
decode_file_windows_device(stream, origins, w, h)   K windows of one size through YAIK_DecodeImageWindowsToDevice: the map-sized work of the image
                              once, every 64x64 block the windows touch rendered once; uint8 [K, h, w, C]
decode_files_device(streams)  n streams of one shape through YAIK_DecodeImagesToDevice: ZStd on host workers, one upload, every kernel once over
                              the batch; uint8 [N, H, W, C] or [N, C, H, W]
decode_files_windows_device(streams, origins, size)   one window of each of them through YAIK_DecodeImagesWindowsToDevice: the same batch with
                              the pixel-sized work of a frame only inside its window; uint8 [N, h, w, C] or [N, C, h, w]
decode_files_norm_device(streams, dtype, ...)   the frames, or a pixel window of each, as normalised float16 / bfloat16 / float32 elements with a
                              mirror flag per stream through YAIK_DecodeImagesNormToDevice: converted in the de-tile store, no uint8 intermediate
decode_files_resampled_device(streams, size, rects=None, ...)   a rectangle of each stream (its own size and aspect), or the whole frame, resampled
                              to one size through YAIK_DecodeImagesResampledToDevice: uint8, or normalised elements with a mirror flag per stream
encode_files_device(frames)   the other direction (yaik_encode.h, YAIK_EncodeImagesFromDevice): uint8 [N, H, W, C] frames in device memory to N
                              streams, every kernel once over the batch, one gather and one download, ZStd and framing on host workers
encode_file_device(frame)     a batch of one

The process holds ONE decoder library (YAIK_Init allows one); it is created on first use with a single decode slot on `device()`.
"""
from __future__ import annotations

import ctypes as C
import os
import struct

import numpy as np

from ._lib import YaikError, lib

HERE = os.path.dirname(os.path.abspath(__file__))
HOST_LIB_PATH = os.environ.get("YK_HOST_LIB") or os.path.join(HERE, "host", "libyaik_host.so")

_ALLOC = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)
_FREE = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)


class MemAlloc(C.Structure):
    _fields_ = [("customAlloc", _ALLOC), ("customFree", _FREE), ("customContext", C.c_void_p)]


class DecodedImage(C.Structure):
    """YAIK_SDecodedImage"""
    _fields_ = [("width", C.c_uint16), ("height", C.c_uint16), ("hasAlpha", C.c_bool), ("customImageOutput", C.c_void_p),
                ("userContextCustomImage", C.c_void_p), ("userMemoryAllocator", MemAlloc), ("outputImage", C.c_void_p),
                ("outputImageStride", C.c_int32), ("hasAlpha1Bit", C.c_bool), ("internalTag", C.c_void_p)]


vp, u32 = C.c_void_p, C.c_uint32
# name -> (restype, argtypes): the declarations of yaik_decode.h this module calls
SIGNATURES = {
    "YAIK_Init": (vp, [C.c_uint8, vp]),
    "YAIK_Release": (None, [vp]),
    "YAIK_GetErrorCode": (C.c_int, []),
    "YAIK_SetDevice": (None, [C.c_int]),
    "YAIK_SetDevicePalette": (None, [C.c_int]),
    "YAIK_DecodeImagePre": (C.c_bool, [vp, vp, u32, vp]),
    "YAIK_DecodeImageToDevice": (C.c_bool, [vp, u32, vp]),
    "YAIK_DecodeImagesToDevice": (C.c_bool, [vp, vp, vp, C.c_int, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, vp]),
    "YAIK_LastBatchFallbacks": (C.c_int, []),
    "YAIK_LastBatchStageMs": (None, [vp]),
}
# yaik_decode.h repeats the reference's C++ header, so the library exports these with C++ linkage: their names under the Itanium ABI
SYMBOLS = {
    "YAIK_Init": "_Z9YAIK_InithP14YAIK_SMemAlloc",
    "YAIK_Release": "_Z12YAIK_ReleasePv",
    "YAIK_GetErrorCode": "_Z17YAIK_GetErrorCodev",
    "YAIK_SetDevice": "_Z14YAIK_SetDevicei",
    "YAIK_SetDevicePalette": "_Z21YAIK_SetDevicePalettei",
    "YAIK_DecodeImagePre": "_Z19YAIK_DecodeImagePrePvS_jP18YAIK_SDecodedImage",
    "YAIK_DecodeImageToDevice": "_Z24YAIK_DecodeImageToDevicePvjP18YAIK_SDecodedImage",
    "YAIK_DecodeImagesToDevice": "_Z25YAIK_DecodeImagesToDevicePvPKS_PKjiPhmmmiiPi",
    "YAIK_LastBatchFallbacks": "_Z23YAIK_LastBatchFallbacksv",
    "YAIK_LastBatchStageMs": "_Z21YAIK_LastBatchStageMsPd",
}
# yaik_encode.h: declared extern "C", bound under their own names
ENC_SIGNATURES = {
    "YAIK_EncoderCreate": (vp, [C.c_int]),
    "YAIK_EncoderRelease": (None, [vp]),
    "YAIK_EncodeImagesFromDevice": (C.c_bool, [vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
    "YAIK_EncodedStream": (C.c_bool, [vp, C.c_int, vp, vp]),
    "YAIK_EncoderLastError": (C.c_char_p, [vp]),
    "YAIK_LastEncodeStageMs": (None, [vp, vp]),
}
# yaik_encode_alpha6.h: the same library, C linkage
ENC6_SIGNATURES = {
    "YAIK_EncodeImagesFromDeviceAlpha6": (C.c_bool, [vp, vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, vp]),
}
# yaik_decode_window.h: the same library, C linkage
WINDOW_SIGNATURES = {
    "YAIK_DecodeImageWindowToDevice": (C.c_bool, [vp, u32, vp, C.c_int, C.c_int, C.c_int, C.c_int]),
}
# yaik_decode_multiwindow.h: the same library, C linkage
MULTIWINDOW_SIGNATURES = {
    "YAIK_DecodeImageWindowsToDevice": (C.c_bool, [vp, u32, vp, C.c_int, vp, C.c_int, C.c_int, C.c_size_t]),
    "YAIK_LastWindowsPrepared": (C.c_int, []),
}
# yaik_decode_batch_windows.h: the same library, C linkage
BATCH_WINDOWS_SIGNATURES = {
    "YAIK_DecodeImagesWindowsToDevice": (C.c_bool, [vp, vp, vp, C.c_int, vp, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_int, vp, vp, C.c_int, C.c_int]),
}
# yaik_decode_window_px.h: the same library, C linkage; the arguments of the aligned namesakes
WINDOW_PX_SIGNATURES = {
    "YAIK_DecodeImageWindowPxToDevice": WINDOW_SIGNATURES["YAIK_DecodeImageWindowToDevice"],
    "YAIK_DecodeImageWindowsPxToDevice": MULTIWINDOW_SIGNATURES["YAIK_DecodeImageWindowsToDevice"],
    "YAIK_DecodeImagesWindowsPxToDevice": BATCH_WINDOWS_SIGNATURES["YAIK_DecodeImagesWindowsToDevice"],
}
# yaik_decode_norm.h: the same library, C linkage; the arguments of YAIK_DecodeImagesWindowsPxToDevice, then yk_norm* and the mirror flags
NORM_SIGNATURES = {
    "YAIK_DecodeImagesNormToDevice": (C.c_bool, BATCH_WINDOWS_SIGNATURES["YAIK_DecodeImagesWindowsToDevice"][1] + [vp, vp]),
}
# yaik_decode_resample.h: the arguments of YAIK_DecodeImagesNormToDevice with rects, ow, oh in place of xy, ww, wh
RESAMPLE_SIGNATURES = {
    "YAIK_DecodeImagesResampledToDevice": NORM_SIGNATURES["YAIK_DecodeImagesNormToDevice"],
}
# yaik_decode_scaled.h: the same library, C linkage
SCALED_SIGNATURES = {
    "YAIK_DecodeImageScaledToDevice": (C.c_bool, [vp, u32, vp, C.c_int]),
}
# yaik_decode_mipchain.h: the same library, C linkage
MIPCHAIN_SIGNATURES = {
    "YAIK_DecodeImageMipchainToDevice": (C.c_bool, [vp, u32, vp, C.c_int, C.c_int, vp, vp]),
}
ERROR_NAMES = ["YAIK_NO_ERROR", "YAIK_INVALID_LIBRARYCTX", "YAIK_MALLOC_FAIL", "YAIK_INVALID_CONTEXT_COUNT", "YAIK_INIT_FAIL",
               "YAIK_RELEASE_EMPTY_LIBRARY", "YAIK_INVALID_STREAM", "YAIK_INVALID_HEADER", "YAIK_NO_EMPTYDECODE_SLOT", "YAIK_DECIMG_INVALIDCTX",
               "YAIK_DECIMG_DIFFSTREAM", "YAIK_DECIMG_BUFFERNOTSET", "YAIK_INVALID_CONTEXT_MEMALLOCATOR", "YAIK_INVALID_DECOMPRESSION",
               "YAIK_INVALID_LUT", "YAIK_DECOMPRESSION_CREATE_FAIL", "YAIK_INVALID_MIPMAP_LEVEL", "YAIK_ALPHA_FORMAT_IMPOSSIBLE",
               "YAIK_INVALID_ALPHA_FORMAT", "YAIK_ALPHA_UNSUPPORTED_YET", "YAIK_INVALID_TAG_ID", "YAIK_INVALID_PLANE_ID"]


class YaikFileError(YaikError):
    """A decode the library refused: .code = YAIK_ERROR_CODE (ERROR_NAMES[code]), .index = the lowest failing stream of a batch (or 0)."""

    def __init__(self, code: int, index: int = 0):
        name = ERROR_NAMES[code] if 0 <= code < len(ERROR_NAMES) else str(code)
        super().__init__(f"stream {index}: {name}")
        self.code, self.index = code, index


_host = None
_yaik = None
_device = 0
_encoders: dict = {}               # device index -> YAIK_ENC, created on first use
_last_encoder = None


def host_lib() -> C.CDLL:
    """libyaik_host.so.  torch and libyaik_hip.so are brought up first (yaik_amd._lib.lib()), so that the process holds one HIP runtime and the
    host library binds to the libyaik_hip.so already loaded."""
    global _host
    if _host is None:
        lib()
        if not os.path.exists(HOST_LIB_PATH):
            raise YaikError(f"{HOST_LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(HOST_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, SYMBOLS[name])
            fn.restype, fn.argtypes = res, args
            setattr(L, name, fn)
        for name, (res, args) in {**ENC_SIGNATURES, **ENC6_SIGNATURES, **WINDOW_SIGNATURES, **MULTIWINDOW_SIGNATURES, **BATCH_WINDOWS_SIGNATURES, **WINDOW_PX_SIGNATURES, **NORM_SIGNATURES, **RESAMPLE_SIGNATURES, **SCALED_SIGNATURES, **MIPCHAIN_SIGNATURES}.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _host = L
    return _host


def device() -> int:
    return _device


def library(dev: int = 0):
    """The process-wide decoder library (one decode slot), created on first use on HIP device `dev`."""
    global _yaik, _device
    if _yaik is None:
        L = host_lib()
        L.YAIK_SetDevice(int(dev))
        h = L.YAIK_Init(1, None)
        if not h:
            raise YaikFileError(L.YAIK_GetErrorCode())
        _yaik, _device = h, int(dev)
    return _yaik


def release() -> None:
    """Drops the decoder library and every cached encoder."""
    global _yaik
    if _yaik is not None:
        host_lib().YAIK_Release(_yaik)
        _yaik = None
    for e in _encoders.values():
        host_lib().YAIK_EncoderRelease(e)
    _encoders.clear()


def set_device_palette(on: bool) -> None:
    """YAIK_SetDevicePalette: where PaletteDecompressor runs for whole-RGB 'GTIL' chunks (False: host cores, True: the GPU)."""
    host_lib().YAIK_SetDevicePalette(1 if on else 0)


def has_alpha_chunk(stream: bytes) -> bool:
    """True when the chunk list of the stream holds an 'ALPM' chunk before its terminator (the default builder then writes RGBA rows)."""
    p, n = 12, len(stream)
    while p + 8 <= n:
        tag, length = struct.unpack_from("<II", stream, p)
        if tag == 0xDEADBEEF:
            return False
        if tag == 0x4D504C41:
            return True
        p += 8 + length
    return False


def _buffer(stream):
    a = np.frombuffer(stream, dtype=np.uint8)
    if a.size >= 1 << 32:
        raise ValueError("a stream must be shorter than 4 GB")
    return a


def decode_file_device(stream: bytes):
    """One stream through YAIK_DecodeImageToDevice: a torch.uint8 tensor [H, W, 3] on the GPU, or [H, W, 4] when the stream has an 'ALPM' chunk.
    Raises YaikFileError with the library's error code."""
    import torch
    L, h = host_lib(), library()
    src = _buffer(stream)
    info = DecodedImage()
    if not L.YAIK_DecodeImagePre(h, src.ctypes.data, src.size, C.byref(info)):
        raise YaikFileError(L.YAIK_GetErrorCode())
    dev = torch.device("cuda", _device)
    c = 4 if has_alpha_chunk(bytes(stream)) else 3
    out = torch.empty((info.height, info.width, c), dtype=torch.uint8, device=dev)
    torch.cuda.current_stream(dev).synchronize()                           # the library writes on its slot's own stream
    info.outputImage, info.outputImageStride = out.data_ptr(), info.width * c
    if not L.YAIK_DecodeImageToDevice(src.ctypes.data, src.size, C.byref(info)):
        raise YaikFileError(L.YAIK_GetErrorCode())
    return out


def _window_of(window, px: bool = False) -> tuple:
    """(x0, y0, ww, wh) as ints: multiples of 8, ww, wh >= 8, not negative -- with px any x0, y0 >= 0, ww, wh >= 1 (that it lies inside the image
    is the library's to check)"""
    if isinstance(window, (str, bytes)) or not hasattr(window, "__len__") or len(window) != 4:
        raise TypeError(f"window must be (x0, y0, w, h); got {window!r}")
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in window):
        raise TypeError(f"window must hold four ints; got {window!r}")
    x0, y0, ww, wh = (int(v) for v in window)
    if px:
        if x0 < 0 or y0 < 0 or ww < 1 or wh < 1:
            raise ValueError(f"window {(x0, y0, ww, wh)}: x0, y0 >= 0 and w, h >= 1 are needed")
    elif (x0 | y0 | ww | wh) & 7 or x0 < 0 or y0 < 0 or ww < 8 or wh < 8:
        raise ValueError(f"window {(x0, y0, ww, wh)}: x0, y0, w, h must be multiples of 8 with w, h >= 8")
    return x0, y0, ww, wh


def decode_file_window_device(stream: bytes, window, *, px: bool = False):
    """The rectangle window = (x0, y0, w, h) of one stream through YAIK_DecodeImageWindowToDevice: a torch.uint8 tensor [h, w, 3] on the GPU, or
    [h, w, 4] when the stream has an 'ALPM' chunk, equal to decode_file_device(stream)[y0:y0 + h, x0:x0 + w]; only the tiles the window needs are
    rendered.  x0, y0, w, h are multiples of 8 inside the image; with px=True any rectangle inside the image (YAIK_DecodeImageWindowPxToDevice: the
    window's 8-aligned cover is decoded and the de-tile clips it).  Raises YaikFileError with the library's error code (a window outside the image:
    YAIK_DECIMG_INVALIDCTX)."""
    import torch
    x0, y0, ww, wh = _window_of(window, px)
    L, h = host_lib(), library()
    src = _buffer(stream)
    info = DecodedImage()
    if not L.YAIK_DecodeImagePre(h, src.ctypes.data, src.size, C.byref(info)):
        raise YaikFileError(L.YAIK_GetErrorCode())
    dev = torch.device("cuda", _device)
    c = 4 if has_alpha_chunk(bytes(stream)) else 3
    out = torch.empty((wh, ww, c), dtype=torch.uint8, device=dev)
    torch.cuda.current_stream(dev).synchronize()                           # the library writes on its slot's own stream
    info.outputImage, info.outputImageStride = out.data_ptr(), ww * c
    if not (L.YAIK_DecodeImageWindowPxToDevice if px else L.YAIK_DecodeImageWindowToDevice)(src.ctypes.data, src.size, C.byref(info), x0, y0, ww, wh):
        raise YaikFileError(L.YAIK_GetErrorCode())
    return out


def window_origins(origins, w, h, px: bool = False) -> tuple:
    """((x0, y0), ...) and (w, h) as ints, (flat x0, y0 list, w, h): 1..1024 pairs, everything a multiple of 8, w, h >= 8, nothing negative.
    Shared with HipTileDecoder.render_windows, which adds the image's bounds; here that a window lies inside the image is the library's to check.
    px: pixel windows, nothing negative and w, h >= 1 is all that is asked."""
    if isinstance(origins, (str, bytes)) or not hasattr(origins, "__len__"):
        raise TypeError(f"window origins must be a sequence of (x0, y0) pairs; got {origins!r}")
    if not 1 <= len(origins) <= 1024:
        raise ValueError(f"1..1024 window origins are needed; got {len(origins)}")
    flat = []
    for o in origins:
        if isinstance(o, (str, bytes)) or not hasattr(o, "__len__") or len(o) != 2:
            raise TypeError(f"a window origin must be (x0, y0); got {o!r}")
        flat += list(o)
    if any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in flat + [w, h]):
        raise TypeError(f"window origins and the window size must be ints; got {origins!r}, {w!r}, {h!r}")
    flat, w, h = [int(v) for v in flat], int(w), int(h)
    if px:
        if any(v < 0 for v in flat) or w < 1 or h < 1:
            raise ValueError(f"windows {origins!r} of {w} x {h}: x0, y0 >= 0 and w, h >= 1 are needed")
    elif any(v & 7 or v < 0 for v in flat) or (w | h) & 7 or w < 8 or h < 8:
        raise ValueError(f"windows {origins!r} of {w} x {h}: x0, y0, w, h must be multiples of 8 with w, h >= 8")
    return flat, w, h


def decode_file_windows_device(stream: bytes, origins, w: int, h: int, *, px: bool = False):
    """K = len(origins) windows of w x h, window k at origins[k] = (x0, y0), of one stream through YAIK_DecodeImageWindowsToDevice: a torch.uint8
    tensor [K, h, w, 3] on the GPU, or [K, h, w, 4] when the stream has an 'ALPM' chunk; window k equals
    decode_file_device(stream)[y0:y0 + h, x0:x0 + w].  The map-sized work of the image runs once and every 64x64 block the windows touch is
    rendered once (last_windows_prepared() tells whether the stream could take that path).  px=True: windows at any pixel offset and size
    (YAIK_DecodeImageWindowsPxToDevice).  Raises YaikFileError with the library's error code (a
    window outside the image: YAIK_DECIMG_INVALIDCTX)."""
    import torch
    flat, ww, wh = window_origins(origins, w, h, px)
    k = len(flat) // 2
    L, lh = host_lib(), library()
    src = _buffer(stream)
    info = DecodedImage()
    if not L.YAIK_DecodeImagePre(lh, src.ctypes.data, src.size, C.byref(info)):
        raise YaikFileError(L.YAIK_GetErrorCode())
    dev = torch.device("cuda", _device)
    c = 4 if has_alpha_chunk(bytes(stream)) else 3
    out = torch.empty((k, wh, ww, c), dtype=torch.uint8, device=dev)
    torch.cuda.current_stream(dev).synchronize()                           # the library writes on its slot's own stream
    info.outputImage, info.outputImageStride = out.data_ptr(), ww * c
    xy = (C.c_int * (2 * k))(*flat)
    if not (L.YAIK_DecodeImageWindowsPxToDevice if px else L.YAIK_DecodeImageWindowsToDevice)(src.ctypes.data, src.size, C.byref(info), k, xy, ww, wh, wh * ww * c):
        raise YaikFileError(L.YAIK_GetErrorCode())
    return out


def decode_file_scaled_device(stream: bytes, level: int):
    """One stream through YAIK_DecodeImageScaledToDevice: the image at 1 / (1 << level) size (level 0..3) as a torch.uint8 tensor
    [H >> level, W >> level, 3] on the GPU, or [..., 4] when the stream has an 'ALPM' chunk.  Every pixel is the mean of its (1 << level)^2 box of
    decode_file_device(stream), halves rounded up, alpha included; no full-size image is written.  A level that is no int raises TypeError, one
    outside 0..3 ValueError, both before any library call.  Raises YaikFileError with the library's error code."""
    import torch
    if isinstance(level, bool) or not isinstance(level, (int, np.integer)):
        raise TypeError(f"level must be an int 0..3; got {level!r}")
    level = int(level)
    if not 0 <= level <= 3:
        raise ValueError(f"level must be 0..3 (1/1, 1/2, 1/4, 1/8 size); got {level}")
    L, h = host_lib(), library()
    src = _buffer(stream)
    info = DecodedImage()
    if not L.YAIK_DecodeImagePre(h, src.ctypes.data, src.size, C.byref(info)):
        raise YaikFileError(L.YAIK_GetErrorCode())
    dev = torch.device("cuda", _device)
    c = 4 if has_alpha_chunk(bytes(stream)) else 3
    out = torch.empty((info.height >> level, info.width >> level, c), dtype=torch.uint8, device=dev)
    torch.cuda.current_stream(dev).synchronize()                           # the library writes on its slot's own stream
    info.outputImage, info.outputImageStride = out.data_ptr(), (info.width >> level) * c
    if not L.YAIK_DecodeImageScaledToDevice(src.ctypes.data, src.size, C.byref(info), level):
        raise YaikFileError(L.YAIK_GetErrorCode())
    return out


def decode_file_mipchain_device(stream: bytes, first: int = 0, count: int | None = None):
    """One stream through YAIK_DecodeImageMipchainToDevice: levels first .. first + count - 1 of the image's mip chain (count=None: down to the
    last) as a list of torch.uint8 tensors on the GPU, level k [H >> k, W >> k, 3], or [..., 4] when the stream has an 'ALPM' chunk.  Every pixel of
    level k is the mean of its (1 << k)^2 box of decode_file_device(stream), halves rounded up, alpha included; the decoded planes are read once.
    A first or count that is no int raises TypeError, a range outside the chain ValueError, both before any chunk is decoded.  Raises
    YaikFileError with the library's error code."""
    import torch
    for name, v in (("first", first), ("count", count)):
        if (v is not None or name == "first") and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
            raise TypeError(f"{name} must be an int; got {v!r}")
    first = int(first)
    if first < 0 or (count is not None and int(count) < 1):
        raise ValueError(f"first must be >= 0 and count >= 1; got first = {first}, count = {count}")
    L, h = host_lib(), library()
    src = _buffer(stream)
    info = DecodedImage()
    if not L.YAIK_DecodeImagePre(h, src.ctypes.data, src.size, C.byref(info)):
        raise YaikFileError(L.YAIK_GetErrorCode())
    total = min(info.width, info.height).bit_length()
    n = total - first if count is None else int(count)
    if first >= total or n > total - first:
        info.outputImage = 0                                               # the call releases the slot and refuses before any chunk is decoded
        L.YAIK_DecodeImageMipchainToDevice(src.ctypes.data, src.size, C.byref(info), first, max(n, 1), None, None)
        L.YAIK_GetErrorCode()
        raise ValueError(f"levels {first}..{first + n - 1} are not inside the {total} levels of this {info.width} x {info.height} image")
    dev = torch.device("cuda", _device)
    c = 4 if has_alpha_chunk(bytes(stream)) else 3
    out = [torch.empty((info.height >> k, info.width >> k, c), dtype=torch.uint8, device=dev) for k in range(first, first + n)]
    torch.cuda.current_stream(dev).synchronize()                           # the library writes on its slot's own stream
    images = (C.c_void_p * n)(*[o.data_ptr() for o in out])
    strides = (C.c_uint32 * n)(*[(info.width >> k) * c for k in range(first, first + n)])
    if not L.YAIK_DecodeImageMipchainToDevice(src.ctypes.data, src.size, C.byref(info), first, n, images, strides):
        raise YaikFileError(L.YAIK_GetErrorCode())
    return out


def last_windows_prepared() -> bool:
    """Of the last decode_file_windows_device: True when the stream went through yk_decode_prepare_device, False when every window ran the
    single-window chain (a '3DTL' chunk, plane-subset chunks, a chunk order of its own)."""
    return bool(host_lib().YAIK_LastWindowsPrepared())


def decode_files_device(streams, out=None, channels: int = 3, planar: bool = False, threads: int = 16):
    """n (1..1024) streams of ONE width x height as a batch (YAIK_DecodeImagesToDevice): a torch.uint8 tensor [N, H, W, C], or [N, C, H, W] with
    planar=True, on the GPU.  channels 3 = RGB; 4 = RGBA with alpha from each frame's 'ALPM' chunk, 255 for a frame without one.  `out` may be
    any view with unit inner stride and any row, plane and frame pitch: only its pixel bytes are written.  The call returns once the pixels are
    in place.  Raises YaikFileError (.code, .index = the lowest failing stream); the frames' pixels are then unspecified."""
    import torch

    from .encoder import u8_pixel_layout, u8_planar_batch_layout
    L, h = host_lib(), library()
    streams = list(streams)
    n = len(streams)
    if not 1 <= n <= 1024:
        raise ValueError("1..1024 streams are needed")
    if channels not in (3, 4) or not 1 <= int(threads) <= 16:
        raise ValueError("channels must be 3 or 4 and threads 1..16")
    bufs = [_buffer(s) for s in streams]
    dev = torch.device("cuda", _device)
    W = H = 0
    if len(streams[0]) >= 12:
        tag, _, W, H, _ = struct.unpack_from("<IHHHH", streams[0], 0)
        if tag != 0x4B494159:                                              # not a .yaik header: the library says so, nothing is written
            W = H = 0
    if out is None:
        out = torch.empty((n, channels, H, W) if planar else (n, H, W, channels), dtype=torch.uint8, device=dev)
    elif not isinstance(out, torch.Tensor) or out.device != dev:
        raise ValueError(f"out must be a torch tensor on {dev}")
    if planar:
        lay = u8_planar_batch_layout(out)
        plane_bytes = lay.plane_bytes
    else:
        lay = u8_pixel_layout(out, batch=True)
        plane_bytes = 0
    if (lay.frames, lay.channels, lay.rows, lay.w) != (n, channels, H, W):        # the library writes H x W pixels per frame: never into a smaller view
        raise ValueError(f"out holds {lay.frames} frames of {lay.w} x {lay.rows} x {lay.channels}, the call needs {n} of {W} x {H} x {channels}")
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_uint32 * n)(*[b.size for b in bufs])
    failed = C.c_int32(-1)
    torch.cuda.current_stream(dev).synchronize()                           # the library writes on its slot's own stream
    ok = L.YAIK_DecodeImagesToDevice(h, ptrs, lens, n, out.data_ptr(), lay.row_bytes, plane_bytes, lay.frame_bytes, channels, int(threads),
                                     C.byref(failed))
    if not ok:
        raise YaikFileError(L.YAIK_GetErrorCode(), max(failed.value, 0))
    return out


def decode_files_windows_device(streams, origins, size, out=None, channels: int = 3, planar: bool = False, threads: int = 16, *, px: bool = False):
    """One window of each of n (1..1024) streams of ONE width x height (YAIK_DecodeImagesWindowsToDevice): origins[f] = (x0, y0) of stream f's
    window, size = (w, h) of every window; a torch.uint8 tensor [N, h, w, C], or [N, C, h, w] with planar=True, on the GPU, frame f equal to
    decode_files_device(streams)[f] cut to its window.  channels, `out` and threads follow decode_files_device, with the windows' size as the
    frame size.  A wrong number of origins, an origin or size that is no multiple of 8 and a wrong `out` raise before any library call; a window
    outside the image is the library's to refuse (YaikFileError, YAIK_DECIMG_INVALIDCTX; nothing is written).  px=True: windows at any pixel offset
    and size (YAIK_DecodeImagesWindowsPxToDevice)."""
    import torch

    from .encoder import u8_pixel_layout, u8_planar_batch_layout
    streams = list(streams)
    n = len(streams)
    if not 1 <= n <= 1024:
        raise ValueError("1..1024 streams are needed")
    if channels not in (3, 4) or not 1 <= int(threads) <= 16:
        raise ValueError("channels must be 3 or 4 and threads 1..16")
    if isinstance(size, (str, bytes)) or not hasattr(size, "__len__") or len(size) != 2:
        raise TypeError(f"size must be (w, h); got {size!r}")
    if isinstance(origins, np.ndarray):
        origins = origins.tolist() if origins.ndim == 2 and np.issubdtype(origins.dtype, np.integer) else origins
    flat, ww, wh = window_origins(origins, size[0], size[1], px)
    if len(flat) != 2 * n:
        raise ValueError(f"{len(flat) // 2} window origins for {n} streams")
    L, h = host_lib(), library()
    bufs = [_buffer(s) for s in streams]
    dev = torch.device("cuda", _device)
    if out is None:
        out = torch.empty((n, channels, wh, ww) if planar else (n, wh, ww, channels), dtype=torch.uint8, device=dev)
    elif not isinstance(out, torch.Tensor) or out.device != dev:
        raise ValueError(f"out must be a torch tensor on {dev}")
    if planar:
        lay = u8_planar_batch_layout(out)
        plane_bytes = lay.plane_bytes
    else:
        lay = u8_pixel_layout(out, batch=True)
        plane_bytes = 0
    if (lay.frames, lay.channels, lay.rows, lay.w) != (n, channels, wh, ww):      # the library writes wh x ww pixels per frame: never into a smaller view
        raise ValueError(f"out holds {lay.frames} frames of {lay.w} x {lay.rows} x {lay.channels}, the call needs {n} of {ww} x {wh} x {channels}")
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_uint32 * n)(*[b.size for b in bufs])
    xy = (C.c_int * (2 * n))(*flat)
    failed = C.c_int32(-1)
    torch.cuda.current_stream(dev).synchronize()                           # the library writes on its slot's own stream
    fn = L.YAIK_DecodeImagesWindowsPxToDevice if px else L.YAIK_DecodeImagesWindowsToDevice
    ok = fn(h, ptrs, lens, n, out.data_ptr(), lay.row_bytes, plane_bytes, lay.frame_bytes, channels, int(threads), C.byref(failed), xy, ww, wh)
    if not ok:
        raise YaikFileError(L.YAIK_GetErrorCode(), max(failed.value, 0))
    return out


def decode_files_norm_device(streams, dtype, scale=None, bias=None, mean=None, std=None, origins=None, size=None, mirror=None, out=None, channels: int = 3,
                             planar: bool = False, threads: int = 16):
    """n (1..1024) streams of ONE width x height as normalised elements (YAIK_DecodeImagesNormToDevice): a torch.float16 / bfloat16 /
    float32 tensor [N, h, w, C], or [N, C, h, w] with planar=True, on the GPU -- whole frames, or with origins and size=(w, h) stream f's pixel
    window at origins[f] (any rectangle inside the image, as with decode_files_windows_device(px=True)).  Every decoded byte v of channel k
    becomes fp32(v) * scale[k], then + bias[k], kept as fp32 or rounded to nearest even (HipTileDecoder.image_norm_device has the rule for scale /
    bias and mean / std); mirror: None, or n flags, a set one flips that stream's output horizontally.  channels 4 takes alpha from each frame's
    'ALPM' chunk, 255 for a frame without one, normalised like a colour.  `out`, threads and the errors follow decode_files_device."""
    import torch

    from .encoder import elem_layout, mirror_flags, norm_struct
    nrm = norm_struct(dtype, scale, bias, mean, std)
    streams = list(streams)
    n = len(streams)
    if not 1 <= n <= 1024:
        raise ValueError("1..1024 streams are needed")
    if channels not in (3, 4) or not 1 <= int(threads) <= 16:
        raise ValueError("channels must be 3 or 4 and threads 1..16")
    if (origins is None) != (size is None):
        raise ValueError("origins and size go together")
    flags = mirror_flags(mirror, n)
    xy = None
    if origins is not None:
        if isinstance(size, (str, bytes)) or not hasattr(size, "__len__") or len(size) != 2:
            raise TypeError(f"size must be (w, h); got {size!r}")
        if isinstance(origins, np.ndarray):
            origins = origins.tolist() if origins.ndim == 2 and np.issubdtype(origins.dtype, np.integer) else origins
        flat, ww, wh = window_origins(origins, size[0], size[1], True)
        if len(flat) != 2 * n:
            raise ValueError(f"{len(flat) // 2} window origins for {n} streams")
        xy = (C.c_int * (2 * n))(*flat)
    else:
        ww = wh = 0
        if len(streams[0]) >= 12:
            tag, _, W, H, _ = struct.unpack_from("<IHHHH", streams[0], 0)
            if tag == 0x4B494159:                                          # else: the library says so, nothing is written
                ww, wh = W, H
    L, h = host_lib(), library()
    bufs = [_buffer(s) for s in streams]
    dev = torch.device("cuda", _device)
    tdt = getattr(torch, str(dtype).replace("torch.", ""))
    if out is None:
        out = torch.empty((n, channels, wh, ww) if planar else (n, wh, ww, channels), dtype=tdt, device=dev)
    elif not isinstance(out, torch.Tensor) or out.device != dev:
        raise ValueError(f"out must be a torch tensor on {dev}")
    elif out.dtype != tdt:
        raise TypeError(f"out has dtype {out.dtype}, the call asks for {tdt}")
    lay = elem_layout(out, planar=planar, batch=True)
    if (lay.frames, lay.channels, lay.rows, lay.w) != (n, channels, wh, ww):      # the library writes wh x ww pixels per frame: never into a smaller view
        raise ValueError(f"out holds {lay.frames} frames of {lay.w} x {lay.rows} x {lay.channels}, the call needs {n} of {ww} x {wh} x {channels}")
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_uint32 * n)(*[b.size for b in bufs])
    failed = C.c_int32(-1)
    torch.cuda.current_stream(dev).synchronize()                           # the library writes on its slot's own stream
    ok = L.YAIK_DecodeImagesNormToDevice(h, ptrs, lens, n, out.data_ptr(), lay.row_bytes, lay.plane_bytes, lay.frame_bytes, channels, int(threads),
                                         C.byref(failed), xy, ww if xy is not None else 0, wh if xy is not None else 0, C.byref(nrm),
                                         None if flags is None else flags.ctypes.data)
    if not ok:
        raise YaikFileError(L.YAIK_GetErrorCode(), max(failed.value, 0))
    return out


def decode_files_resampled_device(streams, size, rects=None, dtype=None, scale=None, bias=None, mean=None, std=None, mirror=None, out=None, channels: int = 3,
                                  planar: bool = False, threads: int = 16):
    """n (1..1024) streams of ONE width x height, a rectangle of each resampled to size=(ow, oh) (YAIK_DecodeImagesResampledToDevice):
    [N, oh, ow, C], or [N, C, oh, ow] with planar=True, on the GPU.  rects: None (whole frames), or n rectangles (x0, y0, sw, sh), stream f's own,
    at any offset and of any size 1..16384 inside the image (yaik_amd.augment.random_resized_crop_rects samples them); only the tiles a
    rectangle needs are decoded.  dtype None gives torch.uint8; float16 / bfloat16 / float32 apply scale / bias (or mean / std) to the resampled
    byte as decode_files_norm_device does.  mirror: None, or n flags, a set one flips that stream's output horizontally.  Bilinear in 16.16 fixed
    point, taps clamped to the rectangle, no antialiasing filter (HipTileDecoder.image_resampled_batch_device has the rule).  channels 4 takes
    alpha from each frame's 'ALPM' chunk, 255 for a frame without one.  `out`, threads and the errors follow decode_files_device."""
    import torch

    from .augment import output_size, rect_table
    from .encoder import mirror_flags, norm_struct, resample_layout
    ow, oh = output_size(size)
    if dtype is None or str(dtype).replace("torch.", "") == "uint8":
        if any(v is not None for v in (scale, bias, mean, std)):
            raise ValueError("uint8 elements take no scale, bias, mean or std: give a float dtype")
        nrm, tdt = None, torch.uint8
    else:
        nrm, tdt = norm_struct(dtype, scale, bias, mean, std), getattr(torch, str(dtype).replace("torch.", ""))
    streams = list(streams)
    n = len(streams)
    if not 1 <= n <= 1024:
        raise ValueError("1..1024 streams are needed")
    if channels not in (3, 4) or not 1 <= int(threads) <= 16:
        raise ValueError("channels must be 3 or 4 and threads 1..16")
    flags = mirror_flags(mirror, n)
    tab = None
    if rects is not None:
        W = H = 1 << 30                                                    # without a readable header the library says so, nothing is written
        if len(streams[0]) >= 12:
            tag, _, w0, h0, _ = struct.unpack_from("<IHHHH", streams[0], 0)
            if tag == 0x4B494159:
                W, H = w0, h0
        tab = rect_table(rects, n, W, H)
    L, h = host_lib(), library()
    bufs = [_buffer(s) for s in streams]
    dev = torch.device("cuda", _device)
    if out is None:
        out = torch.empty((n, channels, oh, ow) if planar else (n, oh, ow, channels), dtype=tdt, device=dev)
    elif not isinstance(out, torch.Tensor) or out.device != dev:
        raise ValueError(f"out must be a torch tensor on {dev}")
    elif out.dtype != tdt:
        raise TypeError(f"out has dtype {out.dtype}, the call asks for {tdt}")
    lay = resample_layout(out, planar=planar, batch=True)
    if (lay.frames, lay.channels, lay.rows, lay.w) != (n, channels, oh, ow):      # the library writes oh x ow pixels per frame: never into a smaller view
        raise ValueError(f"out holds {lay.frames} frames of {lay.w} x {lay.rows} x {lay.channels}, the call needs {n} of {ow} x {oh} x {channels}")
    ptrs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_uint32 * n)(*[b.size for b in bufs])
    failed = C.c_int32(-1)
    torch.cuda.current_stream(dev).synchronize()                           # the library writes on its slot's own stream
    ok = L.YAIK_DecodeImagesResampledToDevice(h, ptrs, lens, n, out.data_ptr(), lay.row_bytes, lay.plane_bytes, lay.frame_bytes, channels, int(threads),
                                              C.byref(failed), None if tab is None else tab.ctypes.data, ow, oh, None if nrm is None else C.byref(nrm),
                                              None if flags is None else flags.ctypes.data)
    if not ok:
        raise YaikFileError(L.YAIK_GetErrorCode(), max(failed.value, 0))
    return out


def last_batch_info() -> dict:
    """Of the last decode_files_device or decode_files_windows_device: how many streams took the single-image chain, and the host clocks of its stages in ms."""
    L = host_lib()
    ms = (C.c_double * 3)()
    L.YAIK_LastBatchStageMs(ms)
    return {"fallbacks": L.YAIK_LastBatchFallbacks(), "expand_ms": ms[0], "upload_ms": ms[1], "decode_ms": ms[2]}


class YaikEncodeError(YaikError):
    """An encode the library refused: .index = the lowest frame that could not be framed, -1 for bad arguments and device errors."""

    def __init__(self, message: str, index: int = -1):
        super().__init__(message if index < 0 else f"frame {index}: {message}")
        self.index = index


def encoder(dev: int = 0):
    """The cached YAIK_ENC of HIP device `dev` (one per device, dropped by release())."""
    e = _encoders.get(int(dev))
    if e is None:
        e = host_lib().YAIK_EncoderCreate(int(dev))
        if not e:
            raise YaikError(f"YAIK_EncoderCreate({dev}) failed: no usable HIP device -- this path has no CPU fallback")
        _encoders[int(dev)] = e
    return e


def alpha6_decodable(has_chunk, tile_bbox, bits) -> bool:
    """The alpha6Bit fallback rule of ConvertHotPath and YAIK_EncodeImagesFromDeviceAlpha6 (yaik_amd/host/alpha6_rule.h) on numpy: True when the
    frame's 'MIPM' chunk exists, has bits, and every bit of its tile box (x, y, w, h), LSB first, is set.  Bits behind w * h do not count."""
    bits = np.asarray(bits, dtype=np.uint8).ravel()
    w, h = int(tile_bbox[2]), int(tile_bbox[3])
    if not has_chunk or bits.size == 0 or w <= 0 or h <= 0 or bits.size * 8 < w * h:
        return False
    return bool(np.unpackbits(bits, bitorder="little")[:w * h].all())


def encode_files_device(frames, emit_alpha: bool = False, level: int = 0, threads: int = 16, alpha_6bit: bool = False) -> list:
    """N (1..1024) frames of one shape as a batch (YAIK_EncodeImagesFromDevice): `frames` is a torch.uint8 CUDA tensor [N, H, W, C], C = 3 (RGB)
    or 4 (RGBA); stride(1) is the row pitch and stride(0) the frame pitch, the last two dims are dense.  A numpy array is uploaded through
    torch.  Returns N `bytes`, each a whole .yaik stream.  level 0: byte for byte the file ConvertHotPath writes for the frame alone (ZStd level
    18, 'ALPM' swept over levels 5..21); level 1..22: every stream at that ZStd level.  emit_alpha writes the 'ALPM' chunk of RGBA frames (8-bit
    or 1-bit values); alpha_6bit (with emit_alpha) is ConvertHotPath's alpha6Bit: analog alpha of a frame that satisfies alpha6_decodable takes the
    6-bit mask mode (YAIK_EncodeImagesFromDeviceAlpha6).  Raises YaikEncodeError (.index) when the library refuses."""
    global _last_encoder
    import torch

    from .encoder import u8_pixel_layout
    if not hasattr(frames, "data_ptr"):
        frames = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    if not frames.is_cuda:
        raise ValueError("frames must lie in device memory (or be a numpy array, which is uploaded)")
    lay = u8_pixel_layout(frames, batch=True)
    L = host_lib()
    dev = frames.device.index or 0
    e = encoder(dev)
    _last_encoder = e
    failed = C.c_int32(-1)
    torch.cuda.current_stream(frames.device).synchronize()                 # the library reads on its handle's own stream
    if alpha_6bit:
        ok = L.YAIK_EncodeImagesFromDeviceAlpha6(e, frames.data_ptr(), lay.row_bytes, lay.frame_bytes, lay.channels, lay.w, lay.rows, lay.frames,
                                                 int(bool(emit_alpha)), 1, int(level), int(threads), C.byref(failed))
    else:
        ok = L.YAIK_EncodeImagesFromDevice(e, frames.data_ptr(), lay.row_bytes, lay.frame_bytes, lay.channels, lay.w, lay.rows, lay.frames,
                                           int(bool(emit_alpha)), int(level), int(threads), C.byref(failed))
    if not ok:
        raise YaikEncodeError((L.YAIK_EncoderLastError(e) or b"?").decode(), failed.value)
    out = []
    for f in range(lay.frames):
        data, n = C.c_void_p(), C.c_uint32()
        if not L.YAIK_EncodedStream(e, f, C.byref(data), C.byref(n)):
            raise YaikEncodeError((L.YAIK_EncoderLastError(e) or b"?").decode())
        out.append(C.string_at(data.value, n.value))
    return out


def encode_file_device(frame, emit_alpha: bool = False, level: int = 0, threads: int = 16, alpha_6bit: bool = False) -> bytes:
    """One frame [H, W, C]: a batch of one."""
    return encode_files_device(frame[None], emit_alpha, level, threads, alpha_6bit)[0]


def last_encode_info() -> dict:
    """Of the last encode_files_device: the host clocks of its stages in ms (YAIK_LastEncodeStageMs)."""
    ms = (C.c_double * 4)()
    if _last_encoder is not None and _last_encoder in _encoders.values():
        host_lib().YAIK_LastEncodeStageMs(_last_encoder, ms)
    return {"device_ms": ms[0], "gather_ms": ms[1], "entropy_ms": ms[2], "total_ms": ms[3]}
