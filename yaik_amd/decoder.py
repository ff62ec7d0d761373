"""Python plumbing over the decode half of the C-ABI (include/yaik_hip.h): the loops behind
YAIK_DecodeImage's chunk switch (decoder/YAIK_API.cpp:731-1303), executed on the GPU.

Method names follow the reference: DecompressGradient*, Decompress1D, Decompress1BitTiled; decompress_alpha = the four
alpha value unpackers of decoder/YAIK_Alpha.cpp.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from ._lib import YaikError, lib
from .augment import output_size, rect_table
from .encoder import PASSES, NormC, _chk, elem_layout, mirror_flags, norm_params, norm_struct, resample_layout, u8_pixel_layout, u8_planar_batch_layout, u8_planar_layout  # noqa: F401  (norm_params: public here)
from .files import window_origins


class AlphaBatchPack(NamedTuple):
    """The tables of yk_decode_alpha_batch_device / yk_decode_alpha_mask_batch_device for a list of per-frame entries: pack_alpha_batch."""
    modes: np.ndarray       # int32 [N]: AlphaHeader::parameters & 7, -1 for a frame without a chunk
    bboxes: np.ndarray      # int32 [N, 4]: (x, y, w, h), zeros for a frame without a chunk
    nbytes: np.ndarray      # uint64 [N]: payload lengths
    where: list             # per frame ("h", offset into staging), ("d", device address) or None
    staging: np.ndarray     # uint8: every host payload at its offset, offsets are multiples of 16; empty when no entry is a host array
    mip_where: list = None  # only when an entry has a mask: per frame the offset of its 'MIPM' bitmap in staging, ("d", device address) or None
    mip_nbytes: np.ndarray = None   # uint64 [N]: bitmap lengths
    mip_boxes: np.ndarray = None    # int32 [N, 4]: the 'MIPM' box in 16-pixel tiles, zeros (w == 0) for a frame without one


def pack_alpha_batch(entries) -> AlphaBatchPack:
    """entries[f]: None (no 'ALPM' chunk), or (mode, bbox, payload[, nbytes]) with payload a numpy uint8 array (nbytes defaults to its size) or a
    device pointer (int / c_void_p; nbytes required), or (mode, bbox, payload, mip_bits, mip_box): a numpy payload with the frame's 'MIPM'
    bitmap (numpy uint8, 1 bit per tile as the file holds it) and its box (x, y, w, h) in 16-pixel tiles, which the mask modes 2 and 3 need,
    or (mode, bbox, payload ptr, nbytes, mip ptr, mip nbytes, mip_box): the same with payload and bitmap in device memory.
    Host payloads and bitmaps are laid out back to back in one staging array, each at a 16-byte aligned offset, so that they reach the device in
    one copy.  The mip_* fields stay None unless an entry has a mask.  Reads only the entries: no GPU."""
    n = len(entries)
    modes, bboxes, nbytes = np.full(n, -1, dtype=np.int32), np.zeros((n, 4), dtype=np.int32), np.zeros(n, dtype=np.uint64)
    where, chunks, size = [None] * n, [], 0
    mip_where, mip_nbytes, mip_boxes, masks = [None] * n, np.zeros(n, dtype=np.uint64), np.zeros((n, 4), dtype=np.int32), False
    for f, e in enumerate(entries):
        if e is None:
            continue
        if len(e) not in (3, 4, 5, 7):
            raise ValueError(f"entry {f}: (mode, bbox, payload[, nbytes]), (mode, bbox, payload, mip_bits, mip_box), "
                             "(mode, bbox, payload ptr, nbytes, mip ptr, mip nbytes, mip_box) or None expected")
        mode, bbox, pay = int(e[0]), np.asarray(e[1], dtype=np.int64).reshape(-1), e[2]
        if mode < 0 or bbox.size != 4:
            raise ValueError(f"entry {f}: a mode >= 0 and a box (x, y, w, h) expected (None marks a frame without a chunk)")
        if len(e) == 7 and (isinstance(pay, np.ndarray) or isinstance(e[4], np.ndarray) or np.asarray(e[6]).size != 4 or int(e[5]) < 0):
            raise ValueError(f"entry {f}: a device mask entry takes device pointers with their lengths and a tile box (x, y, w, h)")
        if len(e) == 5 and not (isinstance(pay, np.ndarray) and isinstance(e[3], np.ndarray) and np.asarray(e[4]).size == 4):
            raise ValueError(f"entry {f}: a mask entry takes numpy arrays for payload and 'MIPM' bitmap and a tile box (x, y, w, h)")
        modes[f], bboxes[f] = mode, bbox
        if isinstance(pay, np.ndarray):
            a = np.ascontiguousarray(pay, dtype=np.uint8).ravel()
            nb = a.size if len(e) != 4 else int(e[3])
            if nb < 0 or a.size < nb:
                raise ValueError(f"entry {f}: a payload of {a.size} bytes was given a length of {nb}")
            where[f] = ("h", size)
            chunks.append((size, a[:nb]))
            size = (size + nb + 15) & ~15
        else:
            if len(e) not in (4, 7):
                raise ValueError(f"entry {f}: a device payload needs its length")
            pay = pay.value if isinstance(pay, C.c_void_p) else pay
            nb = int(e[3])
            if nb < 0:
                raise ValueError(f"entry {f}: negative length")
            where[f] = ("d", int(pay) if pay else 0)
        nbytes[f] = nb
        if len(e) == 5:
            bits = np.ascontiguousarray(e[3], dtype=np.uint8).ravel()
            masks = True
            mip_where[f], mip_nbytes[f], mip_boxes[f] = size, bits.size, np.asarray(e[4], dtype=np.int64).reshape(4)
            chunks.append((size, bits))
            size = (size + bits.size + 15) & ~15
        if len(e) == 7:                                                    # the bits lie in device memory (HipTileEncoder.alpha_mask_payloads_device)
            mp = e[4].value if isinstance(e[4], C.c_void_p) else e[4]
            masks = True
            mip_where[f], mip_nbytes[f], mip_boxes[f] = ("d", int(mp) if mp else 0), int(e[5]), np.asarray(e[6], dtype=np.int64).reshape(4)
    staging = np.zeros(size, dtype=np.uint8)
    for off, a in chunks:
        staging[off:off + a.size] = a
    if not masks:
        return AlphaBatchPack(modes, bboxes, nbytes, where, staging)
    return AlphaBatchPack(modes, bboxes, nbytes, where, staging, mip_where, mip_nbytes, mip_boxes)


def batch_calls_from_table(table, passes=PASSES) -> list:
    """The call lists of HipTileDecoder.decode_batch_streams from the rows of an encoder's stream table (HipTileEncoder.streams_batch, or any
    objects with the attributes of encoder.FrameStreams): per frame ("g", sx, sy, bitmap, nbytes, rgb, nbytes) for every pass of `passes`, in
    that order, followed by ("1", type, nbytes, pix, nbytes) -- addresses and lengths only, nothing is copied.  A pass without tiles in a frame
    keeps its bitmap and gets the address 0 with length 0; a frame without 1-D bytes gets ("1", 0, 0, 0, 0).  Reads only the table: no GPU.
    Raises ValueError for a row whose lists do not match `passes`, frames whose bitmaps of a pass differ in length, a length with a NULL
    address, a corner stream that is not whole RGB triples, 1-D streams that are not three planes of whole cells / whole parameter triples,
    and a pixel stream that is not 16-byte aligned (yk_decode_1d_batch_device reads it in place)."""
    passes = list(passes)
    frames = []
    for f, t in enumerate(table):
        if not (len(t.bitmap) == len(t.bitmap_bytes) == len(t.rgb) == len(t.rgb_bytes) == len(passes)):
            raise ValueError(f"frame {f}: {len(t.bitmap)} bitmaps / {len(t.rgb)} corner streams for {len(passes)} passes")
        if frames and list(t.bitmap_bytes) != list(table[0].bitmap_bytes):
            raise ValueError(f"frame {f}: bitmap lengths {list(t.bitmap_bytes)} differ from frame 0's {list(table[0].bitmap_bytes)}")
        calls = []
        for p, (sx, sy) in enumerate(passes):
            bm, nbm, rgb, nrgb = int(t.bitmap[p] or 0), int(t.bitmap_bytes[p]), int(t.rgb[p] or 0), int(t.rgb_bytes[p])
            if nbm <= 0 or not bm:
                raise ValueError(f"frame {f} pass {p}: every pass needs its tile bitmap")
            if nrgb < 0 or nrgb % 3 or (nrgb and not rgb):
                raise ValueError(f"frame {f} pass {p}: a corner stream of {nrgb} bytes at address {rgb:#x}")
            calls.append(("g", sx, sy, bm, nbm, rgb if nrgb else 0, nrgb))
        typ, nty, pix, npx = int(t.type or 0), int(t.type_bytes), int(t.pix or 0), int(t.pix_bytes)
        if nty < 0 or nty % 9 or (nty and not typ):
            raise ValueError(f"frame {f}: a 1-D parameter stream of {nty} bytes at address {typ:#x} (three planes of triples expected)")
        if npx < 0 or npx % 48 or (npx and not pix) or (npx and pix & 15):
            raise ValueError(f"frame {f}: a 1-D pixel stream of {npx} bytes at address {pix:#x} (three planes of 16-byte cells, 16-byte aligned, expected)")
        if bool(nty) != bool(npx):
            raise ValueError(f"frame {f}: {nty} parameter bytes with {npx} pixel bytes")
        calls.append(("1", typ if nty else 0, nty, pix if npx else 0, npx))
        frames.append(calls)
    return frames


class HipTileDecoder:
    def __init__(self, device: int = 0):
        h = C.c_void_p()
        rc = lib().yk_create(device, C.byref(h))
        if rc != 0:
            raise YaikError(f"yk_create failed ({rc}): no usable HIP device -- the product path has no CPU fallback")
        self._h = h
        self.device = device
        self.w = self.h = 0
        self.frames = 1
        self._has_alpha = False
        self._alpha_batch = False        # decompress_alpha_batch left a plane per frame of the batch on the device
        self._batch_stage = None         # torch buffers a queued batch decode may still read: the staging tensor of host streams ...
        self._batch_streams = None       # ... and the copy of an encoder's per-handle streams (encoder_batch_streams)
        self._alpha_stage = None         # ... and the staging tensor of decompress_alpha_batch's host payloads
        self._window = None              # set_window: (x0, y0, w, h) of the image begun, None = the whole image
        self._batch_windows = None       # set_batch_windows: (origins [N, 2], w, h) of the batch begun, None = whole frames
        self._batch_rects = None         # set_batch_rects: int32 [N, 4] of (x0, y0, sw, sh), None = no rectangles

    def close(self):
        if getattr(self, "_h", None):
            lib().yk_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def begin(self, w: int, h: int):
        self.w, self.h, self.frames = w, h, 1
        self._has_alpha = self._alpha_batch = False
        self._window = None                                                # yk_decode_begin always clears the window
        self._batch_windows = None                                         # ... and the windows of a batch
        self._batch_rects = None
        _chk(self._h, lib().yk_decode_begin(self._h, w, h))

    # ---- windows: decode only the tiles a rectangle of the image needs (yk_decode_set_window) -----------------------------------
    @property
    def window(self):
        """(x0, y0, w, h) of the window set on the image begun, None when the decode is of the whole image (always after begin)."""
        return self._window

    @property
    def window_cover(self):
        """The 8-aligned rectangle (x0, y0, w, h) the chunk calls decode for the window set: the window itself, or with set_window(px=True) the
        smallest 8-aligned rectangle that contains it; planes() is exact inside it.  None without a window."""
        if self._window is None:
            return None
        x0, y0, w, h = self._window
        cx, cy = x0 & ~7, y0 & ~7
        return cx, cy, ((x0 + w + 7) & ~7) - cx, ((y0 + h + 7) & ~7) - cy

    def set_window(self, x0: int, y0: int, w: int, h: int, *, px: bool = False) -> None:
        """From here on the decode calls of this image owe only the pixels of the rectangle (x0, y0, w, h): the gradient render skips the 64x64
        blocks it does not touch and the 1-D chunk decodes its tiles only.  Call it right after begin(), before any chunk is decoded; x0, y0, w, h
        are multiples of 8 with w, h >= 8 inside the image; (0, 0, 0, 0) clears the window.  Read the result with image_window_device(); image(),
        image_device() and the compare calls raise the library's state error while a window is set, planes() is exact inside the window only,
        tile4x4() is whole and exact.  Bad arguments raise before any library call; a batch, or chunks decoded already, are the library's to
        refuse.  px=True (yk_decode_set_window_px): any rectangle inside the image, w, h >= 1; the chunk calls decode window_cover,
        image_window_device() writes exactly the rectangle, and image_scaled_device() at levels 1..3 is the library's to refuse."""
        v = (x0, y0, w, h)
        if any(isinstance(a, bool) or not isinstance(a, (int, np.integer)) for a in v):
            raise TypeError(f"window (x0, y0, w, h) must be four ints; got {v!r}")
        x0, y0, w, h = (int(a) for a in v)
        clear = w == 0 and h == 0 and x0 == 0 and y0 == 0
        if px:
            if not clear and (x0 < 0 or y0 < 0 or w < 1 or h < 1 or x0 + w > self.w or y0 + h > self.h):
                raise ValueError(f"window {(x0, y0, w, h)}: x0, y0 >= 0 and w, h >= 1 are needed, inside the {self.w} x {self.h} image")
            _chk(self._h, lib().yk_decode_set_window_px(self._h, x0, y0, w, h))
            self._window = None if clear else (x0, y0, w, h)
            return
        if not clear and ((x0 | y0 | w | h) & 7 or x0 < 0 or y0 < 0 or w < 8 or h < 8 or x0 + w > self.w or y0 + h > self.h):
            raise ValueError(f"window {(x0, y0, w, h)}: x0, y0, w, h must be multiples of 8 with w, h >= 8, inside the {self.w} x {self.h} image")
        _chk(self._h, lib().yk_decode_set_window(self._h, x0, y0, w, h))
        self._window = None if clear else (x0, y0, w, h)

    # ---- many windows of one image: prepare once, render 64x64 blocks on demand (yk_decode_prepare_device) ---------------------
    def prepare(self, calls: list, remap_range: int = 250, sync: bool = True, compression_range: int = 15) -> None:
        """The map-sized work of the image begun, once, from the call list of decode_streams (device-resident streams; at most one "1" entry, none
        for an image without a 1-D chunk): the corner lattice, the marks of every tile and the offsets into the 1-D streams.  No pixel is
        written.  From here on render_window / render_windows hand out windows, each paying only for the 64x64 blocks no earlier window needed
        and its own de-tile.  The tile bitmaps and 1-D streams are copied into the handle: with sync=True (or after synchronize()) every input
        may be freed or overwritten.  compression_range: the '1DTL' chunk header's compressionRange (15 is what the encoder writes).  Call it
        right after begin(); a window, a batch, chunks decoded already or a second prepare are the
        library's to refuse.  Until the next begin(), decode_streams, set_window, image(), image_device(), image_window_device() and the compare
        calls raise the library's state error; planes() is exact inside rendered blocks, tile4x4() is whole and exact."""
        L = lib()
        g = [c for c in calls if c[0] == "g"]
        d1 = [c for c in calls if c[0] == "1"]
        if len(d1) > 1 or len(g) + len(d1) != len(calls):
            raise ValueError('prepare takes ("g", ...) entries and at most one ("1", ...) entry')
        n = len(g)
        ptr = lambda v: v.value if isinstance(v, C.c_void_p) else v
        sx, sy = (C.c_int * n)(*[c[1] for c in g]), (C.c_int * n)(*[c[2] for c in g])
        bm, nb = (C.c_void_p * n)(*[ptr(c[3]) for c in g]), (C.c_size_t * n)(*[c[4] for c in g])
        rgb, nr = (C.c_void_p * n)(*[ptr(c[5]) for c in g]), (C.c_size_t * n)(*[c[6] for c in g])
        typ, nty, pix, npx = (ptr(d1[0][1]), d1[0][2], ptr(d1[0][3]), d1[0][4]) if d1 else (None, 0, None, 0)
        _chk(self._h, L.yk_decode_prepare_device(self._h, n, sx, sy, bm, nb, rgb, nr, remap_range, typ, nty, pix, npx, int(compression_range)))
        if sync:
            _chk(self._h, L.yk_synchronize(self._h))

    def prepare_from_encoder(self, enc, sync: bool = True) -> None:
        """prepare(encoder_streams(enc)): the streams where the encoder left them in HBM, remapped like decode_from_encoder."""
        self.prepare(self.encoder_streams(enc), 250, sync)

    @property
    def prepared_blocks(self) -> tuple:
        """(rendered, total): how many 64x64 blocks of the prepared image have been rendered, and how many it has (yk_decode_prepared_blocks)."""
        r, t = C.c_int(), C.c_int()
        _chk(self._h, lib().yk_decode_prepared_blocks(self._h, C.byref(r), C.byref(t)))
        return int(r.value), int(t.value)

    def _check_windows(self, origins, w, h, px: bool = False) -> list:
        """x0, y0 of every window, flat, after the checks of set_window on every one of them (raises before any library call)"""
        flat, w, h = window_origins(origins, w, h, px)
        for x0, y0 in zip(flat[::2], flat[1::2]):
            if x0 + w > self.w or y0 + h > self.h:
                raise ValueError(f"window {(x0, y0, w, h)} is not inside the {self.w} x {self.h} image")
        return flat

    def render_windows(self, origins, w: int, h: int, out=None, channels: int | None = None, alpha: int | None = None, planar: bool = False, *,
                       px: bool = False):
        """K = len(origins) windows of w x h of the prepared image, window k at origins[k] = (x0, y0), in ONE call (yk_decode_render_windows_device):
        a torch.uint8 tensor [K, h, w, C], or [K, C, h, w] with planar=True, window k equal to the same slice of the whole decode's
        image_device().  The blocks the windows touch that no earlier call rendered are rendered once, however many windows share them; a call
        that finds none only de-tiles.  channels and alpha are those of image_device (a decoded 'ALPM' plane is read at each window's offset);
        `out` follows the rules of image_batch_device: any view with unit inner stride and any row, plane and window pitch, only its pixel bytes
        are written.  1..1024 origins; x0, y0, w, h multiples of 8 inside the image: anything else raises before any library call.  px=True
        (yk_decode_render_windows_px_device): any rectangles inside the image, w, h >= 1; the blocks they touch are shared with the
        aligned and the scaled calls."""
        import torch
        flat = self._check_windows(origins, w, h, px)
        K, ww, wh = len(flat) // 2, int(w), int(h)
        C4 = channels if channels is not None else (4 if self._has_alpha else 3)
        a = (-1 if self._has_alpha else 255) if alpha is None else int(alpha)
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty((K, C4, wh, ww) if planar else (K, wh, ww, C4), dtype=torch.uint8, device=dev)
        elif not isinstance(out, torch.Tensor) or out.device != dev:
            raise ValueError(f"out must be a torch tensor on {dev}, got {getattr(out, 'device', type(out).__name__)}")
        if planar:
            lay = u8_planar_batch_layout(out)
            shape, plane_bytes = (lay.frames, lay.channels, lay.rows, lay.w), lay.plane_bytes
        else:
            lay = u8_pixel_layout(out, batch=True)
            shape, plane_bytes = (lay.frames, lay.rows, lay.w, lay.channels), 0
        want = (K, C4, wh, ww) if planar else (K, wh, ww, C4)
        if shape != want:
            raise ValueError(f"out has shape {shape}, the windows need {want}")
        L = lib()
        xy = (C.c_int * (2 * K))(*flat)
        cur = torch.cuda.current_stream(dev).cuda_stream
        _chk(self._h, L.yk_stream_wait_for(self._h, cur))                  # torch may have just allocated or written `out`
        fn = L.yk_decode_render_windows_px_device if px else L.yk_decode_render_windows_device
        _chk(self._h, fn(self._h, K, xy, ww, wh, out.data_ptr(), lay.row_bytes, plane_bytes, lay.frame_bytes, C4, a))
        _chk(self._h, L.yk_stream_handoff(self._h, cur))
        return out

    def render_window(self, x0: int, y0: int, w: int, h: int, out=None, channels: int | None = None, alpha: int | None = None, planar: bool = False, *,
                      px: bool = False):
        """One window of the prepared image: [h, w, C], or [C, h, w] with planar=True (render_windows with one origin; `out` of that shape)."""
        self._check_windows([(x0, y0)], w, h, px)
        if out is not None and hasattr(out, "unsqueeze"):
            self.render_windows([(x0, y0)], w, h, out.unsqueeze(0), channels, alpha, planar, px=px)
            return out
        return self.render_windows([(x0, y0)], w, h, out, channels, alpha, planar, px=px)[0]

    # ---- batches: n images of one shape, every kernel launched once over all of them (yk_decode_begin_batch) --------------------------------
    def begin_batch(self, w: int, h: int, n: int):
        """n (1..1024) images of w x h on this handle.  The single-image methods (decompress_gradient, decode_streams, decompress_1d, planes,
        tile4x4, image, image_device) then act on the frame select_frame chose (0 after begin_batch); begin() goes back to one image."""
        _chk(self._h, lib().yk_decode_begin_batch(self._h, w, h, n))
        self.w, self.h, self.frames = w, h, n
        self._has_alpha = self._alpha_batch = False
        self._window = None
        self._batch_windows = None                                         # yk_decode_begin_batch always clears the windows
        self._batch_rects = None                                           # ... and the rectangles

    def select_frame(self, f: int):
        _chk(self._h, lib().yk_decode_select_frame(self._h, f))

    # ---- a window of every frame of a batch: one size, one origin per frame (yk_decode_set_batch_windows) -----------------------
    @property
    def batch_windows(self):
        """(origins int32 [N, 2], w, h) of the windows set on the batch begun, None when the frames are decoded whole (always after begin_batch)."""
        if self._batch_windows is None:
            return None
        o, w, h = self._batch_windows
        return o.copy(), w, h

    @property
    def batch_window_covers(self):
        """(origins int32 [N, 2], w, h) of the 8-aligned rectangles the batch chunk calls decode: the windows themselves, or with
        set_batch_windows(px=True) every frame's cover of one shared size; planes() of a frame is exact inside its cover.  None
        without windows."""
        if self._batch_windows is None:
            return None
        o, w, h = self._batch_windows
        if not ((o | w | h) & 7).any():                                    # aligned windows are their own covers
            return o.copy(), w, h
        cw, ch = min(self.w, (w + 14) >> 3 << 3), min(self.h, (h + 14) >> 3 << 3)
        c = o & ~7
        c[:, 0] = np.minimum(c[:, 0], self.w - cw)
        c[:, 1] = np.minimum(c[:, 1], self.h - ch)
        return c.astype(np.int32), cw, ch

    def set_batch_windows(self, origins, w: int, h: int, *, px: bool = False) -> None:
        """From here on the batch decode calls owe frame f only the pixels of the rectangle (origins[f][0], origins[f][1], w, h): the gradient
        render skips the 64x64 blocks of a frame its window does not touch and the 1-D chunk decodes the window's tiles only.  `origins` is an
        [N, 2] integer array or a sequence of N (x0, y0) pairs, N = the frames of the batch.  Call it right after begin_batch(), before any
        chunk is decoded; everything is a multiple of 8 with w, h >= 8 and every rectangle inside the image; w = h = 0 clears the windows.  Read
        the result with image_batch_windows_device(); image_batch_device() and the other whole-frame outputs raise the library's state error
        while windows are set, planes() of a selected frame is exact inside its window only, tile4x4() is whole and exact.  Bad arguments raise
        before any library call; a handle begun with begin(), or chunks decoded already, are the library's to refuse.  px=True
        (yk_decode_set_batch_windows_px): any rectangles inside the image, w, h >= 1; the chunk calls decode batch_window_covers."""
        if isinstance(w, bool) or isinstance(h, bool) or not isinstance(w, (int, np.integer)) or not isinstance(h, (int, np.integer)):
            raise TypeError(f"the window size must be two ints; got {w!r}, {h!r}")
        if int(w) == 0 and int(h) == 0:
            _chk(self._h, lib().yk_decode_set_batch_windows(self._h, None, 0, 0))
            self._batch_windows = None
            self._batch_rects = None                                       # windows and rectangles replace each other, a clear included
            return
        if isinstance(origins, np.ndarray):
            if origins.ndim != 2 or origins.shape[1] != 2 or not np.issubdtype(origins.dtype, np.integer):
                raise TypeError(f"window origins must be an integer array [N, 2]; got {origins.dtype} {origins.shape}")
            origins = [(int(x), int(y)) for x, y in origins]
        flat = self._check_windows(origins, w, h, px)
        if len(flat) != 2 * self.frames:
            raise ValueError(f"{len(flat) // 2} window origins for a batch of {self.frames} frames")
        xy = (C.c_int * len(flat))(*flat)
        self._batch_windows = None
        _chk(self._h, (lib().yk_decode_set_batch_windows_px if px else lib().yk_decode_set_batch_windows)(self._h, xy, int(w), int(h)))
        self._batch_windows = (np.asarray(flat, dtype=np.int32).reshape(-1, 2), int(w), int(h))
        self._batch_rects = None                                           # windows replace rectangles

    def image_batch_windows_device(self, out=None, channels: int = 3, alpha: int = 255, planar: bool = False, alpha_from_planes: bool = False):
        """The window of every frame of the batch as 8-bit pixels in one torch.uint8 tensor on the handle's device
        (yk_decode_output_batch_windows_device, one launch): [N, h, w, C], or [N, C, h, w] with planar=True, of the windows' size; frame f equals
        image_batch_device()[f] of the whole decode cut to its window.  channels, alpha, alpha_from_planes (each frame's decoded 'ALPM' plane,
        read at its window's offset) and `out` follow image_batch_device; ordering against torch's current stream is the same: no host fence."""
        import torch
        if self._batch_windows is None and getattr(self, "_batch_rects", None) is not None:
            raise ValueError("rectangles are set on this batch (set_batch_rects): image_resampled_batch_device() writes them")
        if self._batch_windows is None:
            raise ValueError("no windows are set on this batch: set_batch_windows() first")
        if channels not in (3, 4):
            raise ValueError("channels must be 3 or 4")
        if alpha_from_planes and channels != 4:
            raise ValueError("alpha_from_planes needs channels=4")
        if not alpha_from_planes and not 0 <= int(alpha) <= 255:
            raise ValueError(f"alpha must be 0..255; got {alpha!r}")
        _, ww, wh = self._batch_windows
        dev = torch.device("cuda", self.device)
        N = self.frames
        if out is None:
            out = torch.empty((N, channels, wh, ww) if planar else (N, wh, ww, channels), dtype=torch.uint8, device=dev)
        elif not isinstance(out, torch.Tensor) or out.device != dev:
            raise ValueError(f"out must be a torch tensor on {dev}, got {getattr(out, 'device', type(out).__name__)}")
        if planar:
            lay = u8_planar_batch_layout(out)
            shape, plane_bytes = (lay.frames, lay.channels, lay.rows, lay.w), lay.plane_bytes
        else:
            lay = u8_pixel_layout(out, batch=True)
            shape, plane_bytes = (lay.frames, lay.rows, lay.w, lay.channels), 0
        want = (N, channels, wh, ww) if planar else (N, wh, ww, channels)
        if shape != want:
            raise ValueError(f"out has shape {shape}, the windows need {want}")
        L = lib()
        cur = torch.cuda.current_stream(dev).cuda_stream
        _chk(self._h, L.yk_stream_wait_for(self._h, cur))                  # torch may have just allocated or written `out`
        _chk(self._h, L.yk_decode_output_batch_windows_device(self._h, out.data_ptr(), lay.row_bytes, plane_bytes, lay.frame_bytes, channels,
                                                               -1 if alpha_from_planes else int(alpha)))
        _chk(self._h, L.yk_stream_handoff(self._h, cur))
        return out

    def decode_batch_streams(self, frames: list, sync: bool = True, remap_range: int = 250, compression_range: int = 15) -> None:
        """The gradient chunks + the 1-D chunk of every frame of the batch, one launch per kernel over all frames.  frames[f] is the call list
        of encoder_streams for frame f: ("g", sx, sy, bitmap, nbytes, rgb, nbytes) entries, the same passes in the same order in every frame (a
        pass without tiles in a frame: its all-zero bitmap and an empty stream), and at most one ("1", type, nbytes, pix, nbytes).  bitmap / rgb /
        type / pix are device pointers (int, c_void_p) or numpy uint8 arrays; all host arrays are packed, each 16-byte aligned, into one torch
        staging tensor that goes to the device in a single copy.  remap_range: PaletteFullRangeRemapping of the corner streams on the way in
        (250 for an encoder's streams, 0 for streams that are remapped already).  compression_range: the compressionRange of every frame's
        '1DTL' chunk (one value per batch; 15 is what the encoder writes)."""
        import torch
        L = lib()
        if len(frames) != self.frames:
            raise ValueError(f"{len(frames)} call lists for a batch of {self.frames} frames")
        g = [[c for c in fr if c[0] == "g"] for fr in frames]
        d1 = [[c for c in fr if c[0] == "1"] for fr in frames]
        shapes = [(c[1], c[2]) for c in g[0]]
        if any([(c[1], c[2]) for c in gf] != shapes for gf in g) or any(len(x) > 1 for x in d1):
            raise ValueError("every frame needs the same gradient passes in the same order, and at most one 1-D entry")
        chunks, size = [], 0

        def place(v, nbytes):
            nonlocal size
            if isinstance(v, np.ndarray):
                a = np.ascontiguousarray(v, dtype=np.uint8).ravel()
                if a.size < nbytes:
                    raise ValueError(f"a stream of {a.size} bytes was given a length of {nbytes}")
                chunks.append((size, a[:nbytes]))
                size = (size + nbytes + 15) & ~15
                return ("h", chunks[-1][0])
            v = v.value if isinstance(v, C.c_void_p) else v
            return ("d", int(v) if v else 0)

        bm = [[place(c[3], c[4]) for c in gf] for gf in g]
        rgb = [[place(c[5], c[6]) for c in gf] for gf in g]
        typ = [place(x[0][1], x[0][2]) if x else ("d", 0) for x in d1]
        pix = [place(x[0][3], x[0][4]) if x else ("d", 0) for x in d1]
        base = 0
        if chunks:
            buf = np.zeros(size + 16, dtype=np.uint8)
            for off, a in chunks:
                buf[off:off + a.size] = a
            dev = torch.device("cuda", self.device)
            if self._batch_stage is not None:
                _chk(self._h, L.yk_synchronize(self._h))                   # a decode queued with sync=False may still read the previous staging tensor
            stage = torch.from_numpy(buf).to(dev)
            base = stage.data_ptr()
            _chk(self._h, L.yk_stream_wait_for(self._h, torch.cuda.current_stream(dev).cuda_stream))
            self._batch_stage = stage
        addr = lambda e: (base + e[1] if e[0] == "h" else e[1]) or None
        n, P = self.frames, len(shapes)
        if P:
            sx, sy = (C.c_int * P)(*[s[0] for s in shapes]), (C.c_int * P)(*[s[1] for s in shapes])
            nb = (C.c_size_t * P)(*[min(gf[p][4] for gf in g) for p in range(P)])
            t_bm = (C.c_void_p * (n * P))(*[addr(bm[f][p]) for f in range(n) for p in range(P)])
            t_rgb = (C.c_void_p * (n * P))(*[addr(rgb[f][p]) if g[f][p][6] else None for f in range(n) for p in range(P)])
            t_nr = (C.c_size_t * (n * P))(*[g[f][p][6] for f in range(n) for p in range(P)])
            _chk(self._h, L.yk_decode_gradient_all_batch_device(self._h, P, sx, sy, t_bm, nb, t_rgb, t_nr, remap_range))
        if any(d1):
            nt = [x[0][2] if x else 0 for x in d1]
            npx = [x[0][4] if x else 0 for x in d1]
            t_ty = (C.c_void_p * n)(*[addr(typ[f]) if nt[f] else None for f in range(n)])
            t_px = (C.c_void_p * n)(*[addr(pix[f]) if npx[f] else None for f in range(n)])
            _chk(self._h, L.yk_decode_1d_batch_device(self._h, t_ty, (C.c_size_t * n)(*nt), t_px, (C.c_size_t * n)(*npx), int(compression_range)))
        if sync:
            _chk(self._h, L.yk_synchronize(self._h))

    def encoder_batch_streams(self, enc, per_frame: bool = False) -> list:
        """The call lists of decode_batch_streams for an encoder that ran encode_batch (same device).  Every pass is listed for every frame (a
        pass without tiles: all-zero bitmap, empty stream).
        Default: enc.streams_batch() builds the corner and 1-D streams of all frames with one launch per kernel and one read-back, and
        batch_calls_from_table lists them where they lie in the encoder's HBM: nothing is copied, no buffer is allocated here, the encoder is
        fenced once.  The corner and 1-D streams then go stale with the encoder's next encode, set_image / set_batch or streams_batch, like the
        bitmap pointers: decode (or copy) them before that.
        per_frame=True: the earlier form, kept as the cross-check and the baseline of profiles/encode_streams_batch.  Frame after frame:
        select_frame, the corner stage, yk_range1d_encode.  The corner and 1-D streams are ONE buffer per encoder handle, overwritten by the next
        frame's stages, so every frame's are copied device-to-device (on the encoder's stream) into one worst-case-sized torch buffer this decoder
        keeps alive until its next encoder_batch_streams; the lengths cost two read-backs per frame.  Only the bitmap pointers go stale with the
        encoder's next encode."""
        if not per_frame:
            _chk(self._h, lib().yk_synchronize(self._h))                       # a queued decode may still read streams the encoder's call replaces
            if (enc.w, enc.h, enc.frames) != (self.w, self.h, self.frames):
                raise ValueError(f"the encoder holds {enc.frames} frames of {enc.w} x {enc.h}, the decoder batch {self.frames} of {self.w} x {self.h}")
            frames = batch_calls_from_table(enc.streams_batch(), PASSES)
            enc.synchronize()
            self._batch_streams = None
            return frames
        import torch
        n = enc.frames
        _chk(self._h, lib().yk_synchronize(self._h))                           # a queued decode may still read the buffer this call replaces
        if (enc.w, enc.h, n) != (self.w, self.h, self.frames):
            raise ValueError(f"the encoder holds {n} frames of {enc.w} x {enc.h}, the decoder batch {self.frames} of {self.w} x {self.h}")
        EL = enc._L
        up = lambda v: (v + 15) & ~15
        lat3 = (self.w // 4 + 1) * (self.h // 4 + 1) * 3
        n_px, n_ty = 3 * self.w * self.h, 3 * (self.w // 8) * (self.h // 8) * 3          # the most the 1-D streams of a frame can hold
        per_frame = up(lat3) + 7 * 16 + up(n_px) + up(n_ty)
        dev = torch.device("cuda", self.device)
        keep = torch.empty(n * per_frame + 16, dtype=torch.uint8, device=dev)
        _chk(enc._h, EL.yk_stream_wait_for(enc._h, torch.cuda.current_stream(dev).cuda_stream))   # torch may still use the memory it just handed out
        frames = []
        for f in range(n):
            enc.select_frame(f)
            at, end, calls = keep.data_ptr() + f * per_frame, keep.data_ptr() + (f + 1) * per_frame, []
            for i, (sx, sy) in enumerate(PASSES):
                src, nb = C.c_void_p(), C.c_size_t()
                _chk(enc._h, EL.yk_gradient_corners_device(enc._h, i, C.byref(src), C.byref(nb)))
                if at + nb.value > end:
                    raise YaikError("the encoder's corner streams are longer than a frame can produce")
                _chk(enc._h, EL.yk_device_copy(enc._h, at, src, nb.value))
                calls.append(("g", sx, sy, EL.yk_gradient_bitmap_device(enc._h, i), EL.yk_gradient_bitmap_bytes(enc._h, i), at, nb.value))
                at += up(nb.value)
            _chk(enc._h, EL.yk_range1d_encode(enc._h))
            pix, npx, typ, nty = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
            _chk(enc._h, EL.yk_range1d_streams_device(enc._h, C.byref(pix), C.byref(npx), C.byref(typ), C.byref(nty)))
            if at + up(npx.value) + nty.value > end:
                raise YaikError("the encoder's 1-D streams are longer than a frame can produce")
            _chk(enc._h, EL.yk_device_copy(enc._h, at, pix, npx.value))
            _chk(enc._h, EL.yk_device_copy(enc._h, at + up(npx.value), typ, nty.value))
            calls.append(("1", at + up(npx.value), nty.value, at, npx.value))
            frames.append(calls)
        enc.synchronize()
        self._batch_streams = keep
        return frames

    def decode_batch_from_encoder(self, enc, sync: bool = True, alpha: bool = False, per_frame: bool = False, palette: bool = False,
                                  alpha_6bit: bool = False, windows=None, *, px: bool = False, rects=None) -> None:
        """decode_batch_streams of encoder_batch_streams(enc, per_frame); windows=(origins, w, h) first gives every frame its window
        (set_batch_windows, with px=True pixel windows; checked before anything else happens), so that the batch begun just before decodes those rectangles only; alpha=True also runs the encoder's alpha_values_batch and decodes every
        frame's 'ALPM' payload where the encoder left it in HBM (decompress_alpha_batch; frames without a chunk are opaque).  With sync=False on
        the default path the queued decode reads the encoder's own stream buffer: fence this decoder before the encoder's next encode.
        alpha_6bit=True (with alpha): the alpha goes through the encoder's alpha_bitmaps_device + alpha_mask_payloads_device and
        yk_decode_alpha_mask_batch_device, bits and payloads read where they lie in HBM: analog frames that have 'MIPM' bits are written and read
        in the 6-bit mask mode (3); a frame without bits has no mask to decode against and keeps the 8-bit mode.
        palette=True: the corner streams take the way of a file.  The payloads the CALLER made with enc.palette_compress_batch() (after
        enc.streams_batch(); this method does not touch the encoder's coder state) are decompressed on this handle
        (palette_decompress_streams, remap_range 250) and the gradient decode reads those outputs with remap off.  Only for streams that
        round-trip through the 'GTIL' coder: a payload PaletteDecompressor rejects raises YaikError (DESIGN §18 on payloads that decode to
        other bytes than their stream).  Without payloads of this batch on the encoder the call raises ValueError."""
        if windows is not None and rects is not None:
            raise ValueError("windows and rects replace each other: give one")
        if windows is not None:
            if not isinstance(windows, (tuple, list)) or len(windows) != 3:
                raise TypeError(f"windows must be (origins, w, h); got {windows!r}")
            self.set_batch_windows(*windows, px=px)
        if rects is not None:                                              # a rectangle per frame (set_batch_rects), checked before anything else happens
            self.set_batch_rects(rects)
        if palette:
            if per_frame:
                raise ValueError("palette=True needs the encoder's stream table (per_frame=False)")
            if not self._encoder_has_payloads(enc, 7 * enc.frames):
                raise ValueError("palette=True decodes the payloads of enc.palette_compress_batch(): call it first (after enc.streams_batch())")
            _chk(self._h, lib().yk_synchronize(self._h))
            if (enc.w, enc.h, enc.frames) != (self.w, self.h, self.frames):
                raise ValueError(f"the encoder holds {enc.frames} frames of {enc.w} x {enc.h}, the decoder batch {self.frames} of {self.w} x {self.h}")
            frames = batch_calls_from_table(enc.streams_table(), PASSES)     # the caller's table: building a new one would drop the payloads
            enc.synchronize()
            self._batch_streams = None
        else:
            frames = self.encoder_batch_streams(enc, per_frame)
        entries = None
        if alpha and alpha_6bit:
            entries = enc.alpha_mask_payloads_device([m["nbytes"] == 0 for m in enc.alpha_bitmaps_device()])
            enc.synchronize()
        elif alpha:
            entries = enc.alpha_payloads_device()
            enc.synchronize()                                              # the payloads are written on the encoder's stream
        if palette:
            frames = self._through_palette(enc, frames)
        self.decode_batch_streams(frames, sync and not alpha, 0 if palette else 250)
        if alpha:
            self.decompress_alpha_batch(entries, 255, sync)

    # ---- PaletteDecompressor (decoder/YAIK_GenericFunctions.cpp:139-241) on the GPU: 'GTIL' payloads back to colour streams -----------------
    def palette_decompress_streams(self, payload_tensors, out_bytes, remap_range: int = 250) -> int:
        """PaletteDecompressor over payloads in device memory: `payload_tensors` is a sequence of 1-D contiguous uint8 CUDA tensors, out_bytes[i]
        the decoded length of stream i (the chunk header's streamRGBSizeUncompressed, a multiple of 3; 0 skips the stream).  remap_range 1..255:
        PaletteFullRangeRemapping on the way out, 0: the bytes as decoded.  The call first waits for torch's current stream (the hand-over fence of
        the payload tensors, as in HipTileEncoder.palette_compress_streams); the library call behind it queues its launches and returns without
        waiting for them: palette_status() does.  CPU tensors
        and bad arguments are refused before any library call.  Returns the number of streams."""
        import torch
        if isinstance(remap_range, bool) or not isinstance(remap_range, int) or not 0 <= remap_range <= 255:
            raise ValueError(f"remap_range must be an int in 0..255; got {remap_range!r}")
        tensors, out_bytes = list(payload_tensors), list(out_bytes)
        if not tensors or len(tensors) > 65536:
            raise ValueError("1..65536 payloads are needed")
        if len(out_bytes) != len(tensors):
            raise ValueError(f"{len(out_bytes)} output lengths for {len(tensors)} payloads")
        for i, nb in enumerate(out_bytes):
            if isinstance(nb, bool) or not isinstance(nb, (int, np.integer)) or nb < 0 or nb % 3:
                raise ValueError(f"out_bytes[{i}] must be a non-negative multiple of 3; got {nb!r}")
        for i, (t, nb) in enumerate(zip(tensors, out_bytes)):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"payload {i} is not a torch tensor")
            if not t.is_cuda:
                raise ValueError(f"payload {i} is a CPU tensor: the payloads must lie in device memory")
            if t.dtype != torch.uint8 or t.dim() != 1 or not t.is_contiguous():
                raise ValueError(f"payload {i} must be a 1-D contiguous uint8 tensor")
            if nb and not t.numel():
                raise ValueError(f"payload {i} is empty but {nb} bytes are expected from it")
        n = len(tensors)
        ptrs = (C.c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in tensors])
        lens = (C.c_size_t * n)(*[t.numel() for t in tensors])
        outs = (C.c_size_t * n)(*[int(v) for v in out_bytes])
        torch.cuda.current_stream(tensors[0].device).synchronize()          # hand-over fence: the payloads are complete before this handle reads them
        _chk(self._h, lib().yk_palette_decompress_streams(self._h, ptrs, lens, outs, n, remap_range))
        self._palette_keepalive = tensors
        self._palette_n = n
        return n

    def palette_status(self) -> np.ndarray:
        """One int32 per stream of the last palette_decompress_streams: 0 = decoded, non-zero = PaletteDecompressor rejects the payload (synchronises)."""
        n = getattr(self, "_palette_n", 0)
        out = np.zeros(65536, dtype=np.int32)                               # the most streams a call can have: whatever the handle last decoded fits
        _chk(self._h, lib().yk_palette_decode_status(self._h, out.ctypes.data))
        return out[:n].copy()

    def palette_decoded(self, i: int) -> np.ndarray:
        """Output i of the last palette_decompress_streams, copied to the host (synchronises).  Unspecified bytes where palette_status()[i] != 0."""
        n = C.c_size_t()
        _chk(self._h, lib().yk_palette_decoded(self._h, i, None, 0, C.byref(n)))
        out = np.empty(n.value, dtype=np.uint8)
        if out.size:
            _chk(self._h, lib().yk_palette_decoded(self._h, i, out.ctypes.data, out.size, None))
        return out

    def palette_decoded_device(self, i: int):
        """Output i where it lies in HBM, as a uint8 tensor view of the handle's buffer (written on the handle's stream; stale after the next
        palette_decompress_streams or 'GTIL' payload decode of the handle)."""
        import torch
        dev, n = C.c_void_p(), C.c_size_t()
        _chk(self._h, lib().yk_palette_decoded_device(self._h, i, C.byref(dev), C.byref(n)))
        if not n.value:
            return torch.empty(0, dtype=torch.uint8, device="cuda")

        class _View:                                                        # __cuda_array_interface__: a view, not a copy
            __cuda_array_interface__ = {"shape": (int(n.value),), "typestr": "|u1", "data": (int(dev.value), False), "version": 2}

        return torch.as_tensor(_View(), device="cuda")

    @staticmethod
    def _encoder_has_payloads(enc, n: int) -> bool:
        """True when the encoder's library holds exactly n valid palette payloads (asked of the library: an encode since has dropped them)."""
        dev, nb = C.c_void_p(), C.c_size_t()
        return (enc._L.yk_palette_payload_device(enc._h, n - 1, C.byref(dev), C.byref(nb)) == 0
                and enc._L.yk_palette_payload_device(enc._h, n, C.byref(dev), C.byref(nb)) != 0)

    def _through_palette(self, enc, frames: list) -> list:
        """The call lists `frames` (one list per image) with every corner stream replaced by the decode of the encoder's 'GTIL' payload for it:
        payload number frame * 7 + pass of enc.palette_payload_device.  One palette_decompress_streams over all of them; raises on a rejected one."""
        index = {shape: p for p, shape in enumerate(PASSES)}
        where, pays, outs = [], [], []
        for f, calls in enumerate(frames):
            for k, c in enumerate(calls):
                if c[0] == "g" and c[6]:
                    where.append((f, k))
                    pays.append(enc.palette_payload_device(f * 7 + index[(c[1], c[2])]))
                    outs.append(int(c[6]))
        if not where:
            return frames
        self.palette_decompress_streams(pays, outs, 250)
        st = self.palette_status()
        if st.any():
            raise YaikError(f"PaletteDecompressor rejects the payload of {int(np.count_nonzero(st))} stream(s); first: frame, call {where[int(np.argmax(st != 0))]}")
        frames = [list(calls) for calls in frames]
        for i, (f, k) in enumerate(where):
            dev, n = C.c_void_p(), C.c_size_t()
            _chk(self._h, lib().yk_palette_decoded_device(self._h, i, C.byref(dev), C.byref(n)))
            c = frames[f][k]
            frames[f][k] = c[:5] + (dev.value, n.value)
        return frames

    def decompress_alpha_batch(self, entries, no_chunk_alpha: int = 255, sync: bool = True) -> None:
        """The 'ALPM' plane of every frame of the batch in one launch (yk_decode_alpha_batch_device).  entries[f] is None (no chunk: the plane is
        the constant no_chunk_alpha) or (mode, bbox, payload[, nbytes]) with the DECOMPRESSED payload as a numpy uint8 array or a device pointer
        with its length (HipTileEncoder.alpha_payloads_device); modes 1, 4, 5 and 6.  An entry (mode, bbox, payload, mip_bits, mip_box) carries the
        frame's 'MIPM' bitmap and tile box as well, and so does (mode, bbox, payload ptr, nbytes, mip ptr, mip nbytes, mip_box) with both in device
        memory (HipTileEncoder.alpha_mask_payloads_device); when any entry does, the call goes to yk_decode_alpha_mask_batch_device, which also decodes
        the mask modes 2 and 3 (three more launches over the masked frames; alpha_batch_status() tells whether a payload was shorter than its mask
        selects).  Host arrays are packed into one staging tensor (pack_alpha_batch) and sent in one copy.  The planes stay on the device for
        image_batch_device(alpha_from_planes=True) and, frame by frame, for image_device(alpha=-1) and alpha_plane()."""
        import torch
        L = lib()
        if len(entries) != self.frames:
            raise ValueError(f"{len(entries)} entries for a batch of {self.frames} frames")
        pk = pack_alpha_batch(entries)
        base = 0
        if pk.staging.size:
            dev = torch.device("cuda", self.device)
            if self._alpha_stage is not None:
                _chk(self._h, L.yk_synchronize(self._h))                   # a decode queued with sync=False may still read the previous staging tensor
            stage = torch.from_numpy(pk.staging).to(dev)
            base = stage.data_ptr()
            _chk(self._h, L.yk_stream_wait_for(self._h, torch.cuda.current_stream(dev).cuda_stream))
            self._alpha_stage = stage
        n = self.frames
        ptrs = (C.c_void_p * n)(*[None if w is None else ((base + w[1] if w[0] == "h" else w[1]) or None) for w in pk.where])
        sizes = (C.c_size_t * n)(*[int(v) for v in pk.nbytes])
        self._alpha_batch = False
        if pk.mip_where is None:
            _chk(self._h, L.yk_decode_alpha_batch_device(self._h, pk.modes.ctypes.data, np.ascontiguousarray(pk.bboxes).ctypes.data, ptrs, sizes,
                                                          int(no_chunk_alpha)))
        else:
            mptrs = (C.c_void_p * n)(*[None if o is None else ((o[1] or None) if isinstance(o, tuple) else base + o) for o in pk.mip_where])
            msizes = (C.c_size_t * n)(*[int(v) for v in pk.mip_nbytes])
            _chk(self._h, L.yk_decode_alpha_mask_batch_device(self._h, pk.modes.ctypes.data, np.ascontiguousarray(pk.bboxes).ctypes.data, ptrs, sizes,
                                                               mptrs, msizes, np.ascontiguousarray(pk.mip_boxes).ctypes.data, int(no_chunk_alpha)))
        self._alpha_batch = True
        if sync:
            _chk(self._h, L.yk_synchronize(self._h))

    def alpha_batch_status(self) -> np.ndarray:
        """One int32 per frame of the last decompress_alpha_batch: 1 = a mask-mode frame whose payload is shorter than its mask selects (the
        missing bytes were read as 0), 0 otherwise (yk_decode_alpha_batch_status; synchronises)."""
        out = np.zeros(self.frames, dtype=np.int32)
        _chk(self._h, lib().yk_decode_alpha_batch_status(self._h, out.ctypes.data))
        return out

    def alpha_plane(self) -> np.ndarray:
        """The decoded 'ALPM' plane [h, w] of the image, or of the selected frame of a batch, back on the host (yk_decode_alpha_plane)."""
        out = np.empty((self.h, self.w), dtype=np.uint8)
        _chk(self._h, lib().yk_decode_alpha_plane(self._h, out.ctypes.data, out.size))
        return out

    def image_batch_device(self, out=None, channels: int = 3, alpha: int = 255, planar: bool = False, alpha_from_planes: bool = False):
        """Every frame of the batch as 8-bit pixels in one torch.uint8 tensor on the handle's device (yk_decode_output_batch_device, one launch):
        [N, h, w, C], or [N, C, h, w] with planar=True; C = 3, or 4 with the constant alpha 0..255.  alpha_from_planes=True (channels=4 only)
        takes every frame's alpha from the planes decompress_alpha_batch left on the device instead (yk_decode_output_batch_alpha_device).  `out`
        may be any view with unit inner stride and any row, plane and frame pitch (u8_pixel_layout(batch=True) / u8_planar_batch_layout): only
        its pixel bytes are written.  Ordering against torch's current stream is that of image_device: no host fence."""
        import torch
        if alpha_from_planes and channels != 4:
            raise ValueError("alpha_from_planes needs channels=4")
        dev = torch.device("cuda", self.device)
        N = self.frames
        if out is None:
            out = torch.empty((N, channels, self.h, self.w) if planar else (N, self.h, self.w, channels), dtype=torch.uint8, device=dev)
        elif not isinstance(out, torch.Tensor) or out.device != dev:
            raise ValueError(f"out must be a torch tensor on {dev}, got {getattr(out, 'device', type(out).__name__)}")
        if planar:
            lay = u8_planar_batch_layout(out)
            shape, plane_bytes = (lay.frames, lay.channels, lay.rows, lay.w), lay.plane_bytes
        else:
            lay = u8_pixel_layout(out, batch=True)
            shape, plane_bytes = (lay.frames, lay.rows, lay.w, lay.channels), 0
        want = (N, channels, self.h, self.w) if planar else (N, self.h, self.w, channels)
        if shape != want:
            raise ValueError(f"out has shape {shape}, the batch needs {want}")
        L = lib()
        cur = torch.cuda.current_stream(dev).cuda_stream
        _chk(self._h, L.yk_stream_wait_for(self._h, cur))                  # torch may have just allocated or written `out`
        if alpha_from_planes:
            _chk(self._h, L.yk_decode_output_batch_alpha_device(self._h, out.data_ptr(), lay.row_bytes, plane_bytes, lay.frame_bytes))
        else:
            _chk(self._h, L.yk_decode_output_batch_device(self._h, out.data_ptr(), lay.row_bytes, plane_bytes, lay.frame_bytes, channels, int(alpha)))
        _chk(self._h, L.yk_stream_handoff(self._h, cur))
        return out

    # ---- normalised fp16 / bf16 / fp32 outputs with a per-frame mirror, converted in the de-tile store (yk_decode_output_norm_device) ----
    @staticmethod
    def _norm_args(dtype, scale, bias, mean, std) -> NormC:
        """dtype and the affine pair as the library's yk_norm; every check raises before any library call"""
        return norm_struct(dtype, scale, bias, mean, std)

    def image_norm_device(self, dtype, scale=None, bias=None, mean=None, std=None, mirror: bool = False, out=None, channels: int | None = None,
                          alpha: int | None = None, planar: bool = False):
        """What image_window_device() writes -- the image begun, or the window set on it by set_window (aligned or px=True) -- as a
        torch.float16 / bfloat16 / float32 tensor [h, w, C], or [C, h, w] with planar=True (yk_decode_output_norm_device, one launch, no uint8
        intermediate).  Every decoded byte v of channel k becomes fp32(v) * scale[k], then + bias[k] (two fp32 roundings, never an fma), kept
        as fp32 or rounded to nearest even; alpha counts as channel 3 whether it is the decoded plane or a constant.  scale / bias: a scalar
        for every channel, or 3 or 4 values (three leave alpha at 1, 0); finite and 0 or of magnitude in [2^-100, 2^100].  mean / std instead
        go through norm_params(); giving both pairs raises.  mirror=True flips horizontally: pixel x lands at column w - 1 - x.  channels,
        alpha, `out` (any view of `dtype` with unit inner stride and any pitch: elem_layout) and the stream hand-over follow image_device."""
        import torch
        nrm = self._norm_args(dtype, scale, bias, mean, std)
        window = self._window
        ww, wh = (window[2], window[3]) if window is not None else (self.w, self.h)
        C4 = channels if channels is not None else (4 if self._has_alpha else 3)
        if C4 not in (3, 4):
            raise ValueError("channels must be 3 or 4")
        a = (-1 if self._has_alpha else 255) if alpha is None else int(alpha)
        if not -1 <= a <= 255:
            raise ValueError(f"alpha must be None or 0..255; got {alpha!r}")
        dev = torch.device("cuda", self.device)
        tdt = getattr(torch, str(dtype).replace("torch.", ""))
        if out is None:
            out = torch.empty((C4, wh, ww) if planar else (wh, ww, C4), dtype=tdt, device=dev)
        elif not isinstance(out, torch.Tensor) or out.device != dev:
            raise ValueError(f"out must be a torch tensor on {dev}, got {getattr(out, 'device', type(out).__name__)}")
        elif out.dtype != tdt:
            raise TypeError(f"out has dtype {out.dtype}, the call asks for {tdt}")
        lay = elem_layout(out, planar=planar)
        shape = (lay.channels, lay.rows, lay.w) if planar else (lay.rows, lay.w, lay.channels)
        want = (C4, wh, ww) if planar else (wh, ww, C4)
        if shape != want:
            raise ValueError(f"out has shape {shape}, the {'window' if window is not None else 'image'} needs {want}")
        L = lib()
        cur = torch.cuda.current_stream(dev).cuda_stream
        _chk(self._h, L.yk_stream_wait_for(self._h, cur))                  # torch may have just allocated or written `out`
        _chk(self._h, L.yk_decode_output_norm_device(self._h, C.byref(nrm), 1 if mirror else 0, out.data_ptr(), lay.row_bytes, lay.plane_bytes, C4, a))
        _chk(self._h, L.yk_stream_handoff(self._h, cur))
        return out

    def image_norm_batch_device(self, dtype, scale=None, bias=None, mean=None, std=None, mirror=None, out=None, channels: int = 3, alpha: int = 255,
                                planar: bool = False, alpha_from_planes: bool = False):
        """image_norm_device for every frame of the batch in one launch (yk_decode_output_norm_batch_device): whole frames, or each frame's window
        if set_batch_windows (aligned or px=True) is set; [N, h, w, C], or [N, C, h, w] with planar=True.  mirror: None (no frame is flipped), or
        a sequence or bool tensor of N flags, one per frame.  channels, alpha, alpha_from_planes and `out` follow image_batch_windows_device, and
        so does the ordering against torch's current stream: no host fence."""
        import torch
        nrm = self._norm_args(dtype, scale, bias, mean, std)
        if channels not in (3, 4):
            raise ValueError("channels must be 3 or 4")
        if alpha_from_planes and channels != 4:
            raise ValueError("alpha_from_planes needs channels=4")
        if not alpha_from_planes and not 0 <= int(alpha) <= 255:
            raise ValueError(f"alpha must be 0..255; got {alpha!r}")
        N = self.frames
        flags = mirror_flags(mirror, N)
        if self._batch_windows is not None:
            _, ww, wh = self._batch_windows
        else:
            ww, wh = self.w, self.h
        dev = torch.device("cuda", self.device)
        tdt = getattr(torch, str(dtype).replace("torch.", ""))
        if out is None:
            out = torch.empty((N, channels, wh, ww) if planar else (N, wh, ww, channels), dtype=tdt, device=dev)
        elif not isinstance(out, torch.Tensor) or out.device != dev:
            raise ValueError(f"out must be a torch tensor on {dev}, got {getattr(out, 'device', type(out).__name__)}")
        elif out.dtype != tdt:
            raise TypeError(f"out has dtype {out.dtype}, the call asks for {tdt}")
        lay = elem_layout(out, planar=planar, batch=True)
        shape = (lay.frames, lay.channels, lay.rows, lay.w) if planar else (lay.frames, lay.rows, lay.w, lay.channels)
        want = (N, channels, wh, ww) if planar else (N, wh, ww, channels)
        if shape != want:
            raise ValueError(f"out has shape {shape}, the batch needs {want}")
        L = lib()
        cur = torch.cuda.current_stream(dev).cuda_stream
        _chk(self._h, L.yk_stream_wait_for(self._h, cur))                  # torch may have just allocated or written `out`
        _chk(self._h, L.yk_decode_output_norm_batch_device(self._h, C.byref(nrm), None if flags is None else flags.ctypes.data, out.data_ptr(), lay.row_bytes,
                                                           lay.plane_bytes, lay.frame_bytes, channels, -1 if alpha_from_planes else int(alpha)))
        _chk(self._h, L.yk_stream_handoff(self._h, cur))
        return out

    # ---- per-frame rectangles resampled to one output size: a random resized crop in the decoder (yk_decode_set_batch_rects) ------
    @property
    def batch_rects(self):
        """int32 [N, 4] of the source rectangles (x0, y0, sw, sh) set on the batch begun, None when there are none (always after begin_batch)."""
        return None if self._batch_rects is None else self._batch_rects.copy()

    def set_batch_rects(self, rects) -> None:
        """From here on the batch decode calls owe frame f only the pixels of its own rectangle rects[f] = (x0, y0, sw, sh): any offset, any size
        (1..16384) inside the image, a different size and aspect per frame.  The chunk calls decode the smallest 8-aligned rectangle round each;
        image_resampled_batch_device() resamples every rectangle to one output size.  Call it right after begin_batch(), before any chunk; None
        clears the rectangles.  Rectangles and windows (set_batch_windows) replace each other; while rectangles are set the whole-frame, window
        and normalised batch outputs raise the library's state error, planes() of a selected frame is exact inside its cover only, tile4x4() is
        whole and exact.  Bad rectangles raise before any library call."""
        if rects is None:
            _chk(self._h, lib().yk_decode_set_batch_rects(self._h, None))
            self._batch_rects = None
            self._batch_windows = None
            return
        tab = rect_table(rects, self.frames, self.w, self.h)
        _chk(self._h, lib().yk_decode_set_batch_rects(self._h, tab.ctypes.data))
        self._batch_rects = tab
        self._batch_windows = None                                         # rectangles replace windows

    @staticmethod
    def _resample_elem(dtype, scale, bias, mean, std):
        """(yk_norm or None, torch dtype) of a resampled output: dtype None is uint8, which takes no scale, bias, mean or std"""
        import torch
        if dtype is None or str(dtype).replace("torch.", "") == "uint8":
            if any(v is not None for v in (scale, bias, mean, std)):
                raise ValueError("uint8 elements take no scale, bias, mean or std: give a float dtype")
            return None, torch.uint8
        return norm_struct(dtype, scale, bias, mean, std), getattr(torch, str(dtype).replace("torch.", ""))

    def image_resampled_batch_device(self, size, dtype=None, scale=None, bias=None, mean=None, std=None, mirror=None, out=None, channels: int = 3,
                                     alpha: int = 255, planar: bool = False, alpha_from_planes: bool = False):
        """Every frame's rectangle (set_batch_rects; the whole frame if neither rectangles nor windows are set) resampled to size=(ow, oh) in one
        launch (yk_decode_output_resampled_batch_device): [N, oh, ow, C], or [N, C, oh, ow] with planar=True.  Bilinear in 16.16 fixed point with
        half-pixel centres and taps clamped to the rectangle -- "crop, then resize", torch's align_corners=False, antialias=False, within 2.5 grey
        levels of it and fully defined in integers; there is no antialiasing filter, so a rectangle more than twice the output size
        aliases.  dtype None gives torch.uint8; float16 / bfloat16 / float32 apply image_norm_batch_device's scale / bias (or mean / std) to the
        resampled byte.  mirror: None or N flags; a set one flips that frame's output horizontally.  channels, alpha, alpha_from_planes, `out`
        and the ordering against torch's current stream follow image_norm_batch_device."""
        import torch
        ow, oh = output_size(size)
        nrm, tdt = self._resample_elem(dtype, scale, bias, mean, std)
        if channels not in (3, 4):
            raise ValueError("channels must be 3 or 4")
        if alpha_from_planes and channels != 4:
            raise ValueError("alpha_from_planes needs channels=4")
        if not alpha_from_planes and not 0 <= int(alpha) <= 255:
            raise ValueError(f"alpha must be 0..255; got {alpha!r}")
        N = self.frames
        flags = mirror_flags(mirror, N)
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty((N, channels, oh, ow) if planar else (N, oh, ow, channels), dtype=tdt, device=dev)
        elif not isinstance(out, torch.Tensor) or out.device != dev:
            raise ValueError(f"out must be a torch tensor on {dev}, got {getattr(out, 'device', type(out).__name__)}")
        elif out.dtype != tdt:
            raise TypeError(f"out has dtype {out.dtype}, the call asks for {tdt}")
        lay = resample_layout(out, planar=planar, batch=True)
        if (lay.frames, lay.channels, lay.rows, lay.w) != (N, channels, oh, ow):
            raise ValueError(f"out holds {lay.frames} frames of {lay.w} x {lay.rows} x {lay.channels}, the call needs {N} of {ow} x {oh} x {channels}")
        L = lib()
        cur = torch.cuda.current_stream(dev).cuda_stream
        _chk(self._h, L.yk_stream_wait_for(self._h, cur))                  # torch may have just allocated or written `out`
        _chk(self._h, L.yk_decode_output_resampled_batch_device(self._h, None if nrm is None else C.byref(nrm), None if flags is None else flags.ctypes.data,
                                                                out.data_ptr(), ow, oh, lay.row_bytes, lay.plane_bytes, lay.frame_bytes, channels,
                                                                -1 if alpha_from_planes else int(alpha)))
        _chk(self._h, L.yk_stream_handoff(self._h, cur))
        return out

    def image_resampled_device(self, size, rect=None, dtype=None, scale=None, bias=None, mean=None, std=None, mirror: bool = False, out=None,
                               channels: int | None = None, alpha: int | None = None, planar: bool = False):
        """image_resampled_batch_device for the image begun, or the selected frame of a batch without rectangles or windows
        (yk_decode_output_resampled_device): rect = (x0, y0, sw, sh) inside the window set on the image (set_window, aligned or px=True), None for
        that window or the whole image, resampled to size=(ow, oh): [oh, ow, C], or [C, oh, ow] with planar=True.  channels, alpha and `out`
        follow image_norm_device."""
        import torch
        ow, oh = output_size(size)
        nrm, tdt = self._resample_elem(dtype, scale, bias, mean, std)
        rc = None
        if rect is not None:
            window = self._window
            bx, by, bw, bh = window if window is not None else (0, 0, self.w, self.h)
            rc = rect_table([rect], 1, self.w, self.h)
            x0, y0, sw, sh = (int(v) for v in rc[0])
            if x0 < bx or y0 < by or x0 + sw > bx + bw or y0 + sh > by + bh:
                raise ValueError(f"rectangle {tuple(int(v) for v in rc[0])} must lie inside the window {(bx, by, bw, bh)} set on this image")
        C4 = channels if channels is not None else (4 if self._has_alpha else 3)
        if C4 not in (3, 4):
            raise ValueError("channels must be 3 or 4")
        a = (-1 if self._has_alpha else 255) if alpha is None else int(alpha)
        if not -1 <= a <= 255:
            raise ValueError(f"alpha must be None or 0..255; got {alpha!r}")
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty((C4, oh, ow) if planar else (oh, ow, C4), dtype=tdt, device=dev)
        elif not isinstance(out, torch.Tensor) or out.device != dev:
            raise ValueError(f"out must be a torch tensor on {dev}, got {getattr(out, 'device', type(out).__name__)}")
        elif out.dtype != tdt:
            raise TypeError(f"out has dtype {out.dtype}, the call asks for {tdt}")
        lay = resample_layout(out, planar=planar)
        if (lay.channels, lay.rows, lay.w) != (C4, oh, ow):
            raise ValueError(f"out holds {lay.w} x {lay.rows} x {lay.channels}, the call needs {ow} x {oh} x {C4}")
        L = lib()
        cur = torch.cuda.current_stream(dev).cuda_stream
        _chk(self._h, L.yk_stream_wait_for(self._h, cur))                  # torch may have just allocated or written `out`
        _chk(self._h, L.yk_decode_output_resampled_device(self._h, None if rc is None else rc.ctypes.data, None if nrm is None else C.byref(nrm), 1 if mirror else 0,
                                                          out.data_ptr(), ow, oh, lay.row_bytes, lay.plane_bytes, C4, a))
        _chk(self._h, L.yk_stream_handoff(self._h, cur))
        return out

    def decompress_gradient(self, sx: int, sy: int, bitmap: np.ndarray, rgb_dq: np.ndarray):
        bitmap = np.ascontiguousarray(bitmap, dtype=np.uint8)
        rgb_dq = np.ascontiguousarray(rgb_dq, dtype=np.uint8)
        _chk(self._h, lib().yk_decode_gradient(self._h, sx, sy, bitmap.ctypes.data, bitmap.size,
                                               rgb_dq.ctypes.data if rgb_dq.size else None, rgb_dq.size))

    def encoder_streams(self, enc) -> list:
        """The device-resident streams of an encoder handle on the same device, as the argument lists of yk_decode_gradient_device (one per
        gradient pass with accepted tiles) and yk_decode_1d_device: tile bitmaps, corner streams and the 1-D streams where the encoder left
        them in HBM.  Runs the encoder's corner and 1-D stages if they have not run, and fences the encoder once (for the lengths)."""
        shapes = [(4, 4), (4, 3), (3, 4), (3, 3), (3, 2), (2, 3), (2, 2)]
        counts = enc.gradient_counts()
        calls = []
        for i, (sx, sy) in enumerate(shapes):
            dev, n = C.c_void_p(), C.c_size_t()
            _chk(enc._h, enc._L.yk_gradient_corners_device(enc._h, i, C.byref(dev), C.byref(n)))
            if counts[i]:
                calls.append(("g", sx, sy, enc._L.yk_gradient_bitmap_device(enc._h, i), enc._L.yk_gradient_bitmap_bytes(enc._h, i), dev, n.value))
        _chk(enc._h, enc._L.yk_range1d_encode(enc._h))
        pix, npx, typ, nty = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
        _chk(enc._h, enc._L.yk_range1d_streams_device(enc._h, C.byref(pix), C.byref(npx), C.byref(typ), C.byref(nty)))
        calls.append(("1", typ, nty.value, pix, npx.value))
        enc.synchronize()
        return calls

    def decode_streams(self, calls: list, sync: bool = True, per_pass: bool = False, remap_range: int = 250, compression_range: int = 15) -> None:
        """All gradient chunks + the 1-D chunk from device-resident streams (encoder_streams): the corner streams are remapped like
        PaletteFullRangeRemapping(250) on the way in; no PCIe hop, no host synchronisation between the passes.  The gradient chunks go through
        ONE yk_decode_gradient_all_device call (per_pass=True: one yk_decode_gradient_device call per chunk, same result).  remap_range=0 takes
        corner streams that are remapped already (the outputs of palette_decompress_streams).  compression_range: the '1DTL' chunk header's
        compressionRange (15 is what the encoder writes)."""
        L = lib()
        g = [c for c in calls if c[0] == "g"]
        if per_pass:
            for c in g:
                _chk(self._h, L.yk_decode_gradient_device(self._h, c[1], c[2], c[3], c[4], c[5], c[6], remap_range))
        elif g:
            n = len(g)
            ptr = lambda v: v.value if isinstance(v, C.c_void_p) else v
            sx, sy = (C.c_int * n)(*[c[1] for c in g]), (C.c_int * n)(*[c[2] for c in g])
            bm, nb = (C.c_void_p * n)(*[ptr(c[3]) for c in g]), (C.c_size_t * n)(*[c[4] for c in g])
            rgb, nr = (C.c_void_p * n)(*[ptr(c[5]) for c in g]), (C.c_size_t * n)(*[c[6] for c in g])
            _chk(self._h, L.yk_decode_gradient_all_device(self._h, n, sx, sy, bm, nb, rgb, nr, remap_range))
        for c in calls:
            if c[0] == "1":
                _chk(self._h, L.yk_decode_1d_device(self._h, c[1], c[2], c[3], c[4], int(compression_range)))
        if sync:
            _chk(self._h, L.yk_synchronize(self._h))

    def decode_from_encoder(self, enc, sync: bool = True, per_pass: bool = False, palette: bool = False) -> None:
        """decode_streams of encoder_streams(enc).  palette=True: the corner streams go through the payloads the CALLER made with
        enc.palette_compress() (and enc.palette_reset() before it where the image is to start from a fresh code book, like the first image of
        a file) and this handle's palette_decompress_streams first, like decode_batch_from_encoder(palette=True); only for streams that
        round-trip.  The encoder's coder state is not touched; without the seven payloads on the encoder the call raises ValueError."""
        calls = self.encoder_streams(enc)
        if palette:
            if not self._encoder_has_payloads(enc, 7):
                raise ValueError("palette=True decodes the payloads of enc.palette_compress(): call it first")
            calls = self._through_palette(enc, [calls])[0]
        self.decode_streams(calls, sync, per_pass, 0 if palette else 250)

    def decompress_gradient_planes(self, plane_bit: int, bitmap: np.ndarray, rgb_dq: np.ndarray, consistent_marks: bool = False):
        """DecompressGradient4x4 with planeBit 1..6; consistent_marks=False leaves tile4x4Mask as the reference's loops do (defects included)."""
        bitmap = np.ascontiguousarray(bitmap, dtype=np.uint8)
        rgb_dq = np.ascontiguousarray(rgb_dq, dtype=np.uint8)
        _chk(self._h, lib().yk_decode_gradient_planes(self._h, plane_bit, int(consistent_marks), bitmap.ctypes.data, bitmap.size,
                                                      rgb_dq.ctypes.data if rgb_dq.size else None, rgb_dq.size))

    def assign_lut(self, lut_file: np.ndarray) -> None:
        """YAIK_AssignLUT: the decoder's 3-D LUT file ('LUL0')."""
        lf = np.ascontiguousarray(lut_file, dtype=np.uint8)
        _chk(self._h, lib().yk_decode_assign_lut(self._h, lf.ctypes.data, lf.size))

    def decompress_lut3d(self, maps, tiles: np.ndarray, colors_dq: np.ndarray, idx) -> np.ndarray:
        """The '3DTL' chunk: Tile3D_16x8 .. Tile3D_4x4 on its streams (see yk_decode_lut3d).  Returns the bytes consumed per stream."""
        mp = [np.ascontiguousarray(m, dtype=np.uint8) for m in maps]
        ix = [np.ascontiguousarray(i, dtype=np.uint8) for i in idx]
        t = np.ascontiguousarray(tiles, dtype=np.uint16); cdq = np.ascontiguousarray(colors_dq, dtype=np.uint8)
        mptr = (C.c_void_p * 6)(*[m.ctypes.data if m.size else None for m in mp])
        msz = (C.c_size_t * 6)(*[m.size for m in mp])
        iptr = (C.c_void_p * 4)(*[i.ctypes.data if i.size else None for i in ix])
        isz = (C.c_size_t * 4)(*[i.size for i in ix])
        used = (C.c_size_t * 6)()
        _chk(self._h, lib().yk_decode_lut3d(self._h, mptr, msz, t.ctypes.data if t.size else None, t.size, cdq.ctypes.data if cdq.size else None, iptr, isz, used))
        return np.array(list(used), dtype=np.int64)

    def decompress_1d(self, type_stream: np.ndarray, pix_stream: np.ndarray, compression_range: int = 15):
        t = np.ascontiguousarray(type_stream, dtype=np.uint8)
        p = np.ascontiguousarray(pix_stream, dtype=np.uint8)
        if t.size == 0 and p.size == 0:
            return
        # one stream empty: the other is still decoded against it (missing bytes read as 0: no type bytes give zeros, no pixel bytes give color0)
        none = np.zeros(16, dtype=np.uint8)
        _chk(self._h, lib().yk_decode_1d(self._h, (t if t.size else none).ctypes.data, t.size, (p if p.size else none).ctypes.data, p.size, compression_range))

    def decompress_1bit_tiled(self, bits: np.ndarray, bw: int, bh: int) -> np.ndarray:
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        out = np.zeros(bw * bh * 32, dtype=np.uint8)
        _chk(self._h, lib().yk_decode_mask(self._h, bits.ctypes.data, bw, bh, out.ctypes.data, out.size))
        return out

    def decompress_alpha(self, mode: int, bbox, payload: np.ndarray, mask: np.ndarray | None = None, mask_bbox=None,
                         reference_1bit: bool = False, to_host: bool = True) -> np.ndarray | None:
        """'ALPM' chunk: the w x h alpha plane from the DECOMPRESSED payload (yk_decode_alpha).  mode = AlphaHeader::parameters & 7,
        bbox = (x, y, w, h) in pixels; the mask modes 2 / 3 take the decoded 'MIPM' mask (decompress_1bit_tiled) and its box in pixels.
        reference_1bit reproduces the reference's 1-bit row loop byte for byte.  The plane stays on the device for image() and
        image_device(); to_host=False skips its copy to the host and returns None."""
        p = np.ascontiguousarray(payload, dtype=np.uint8)
        b = np.ascontiguousarray(np.asarray(bbox, dtype=np.int32).reshape(4))
        m = np.ascontiguousarray(mask, dtype=np.uint8) if mask is not None else None
        mb = np.ascontiguousarray(np.asarray(mask_bbox, dtype=np.int32).reshape(4)) if mask_bbox is not None else None
        self._has_alpha = False
        _chk(self._h, lib().yk_decode_alpha(self._h, int(mode), b.ctypes.data, p.ctypes.data if p.size else None, p.size,
                                            m.ctypes.data if m is not None and m.size else None, m.size if m is not None else 0,
                                            mb.ctypes.data if mb is not None else None, 1 if reference_1bit else 0))
        self._has_alpha = True
        if not to_host:
            return None
        out = np.empty((self.h, self.w), dtype=np.uint8)
        _chk(self._h, lib().yk_decode_alpha_plane(self._h, out.ctypes.data, out.size))
        return out

    def planes(self) -> np.ndarray:
        n = (self.w // 8) * (self.h // 8) * 64
        out = np.zeros((3, n), dtype=np.uint8)
        _chk(self._h, lib().yk_decode_planes(self._h, out[0].ctypes.data, out[1].ctypes.data, out[2].ctypes.data, n))
        return out

    def image(self, alpha: np.ndarray | None = None, stride: int | None = None, fill: int = 0, reference_rgba: bool = False) -> np.ndarray:
        """internal_imageBuilderFunc: interleaved RGB ([h, stride] bytes, 3 B/pixel) or RGBA when an alpha plane is given.
        Bytes of a row beyond the pixels keep `fill` (the call never writes them).  reference_rgba selects the reference's own
        RGBA branch, defects included (yk_decode_output_reference_rgba).  Without an explicit alpha, the plane of the last
        decompress_alpha of this image (if any) is used on the device (yk_decode_output_alpha)."""
        if alpha is None and self._has_alpha and not reference_rgba:
            stride = stride or self.w * 4
            out = np.full((self.h, stride), fill, dtype=np.uint8)
            _chk(self._h, lib().yk_decode_output_alpha(self._h, out.ctypes.data, stride))
            return out
        bpp = 4 if alpha is not None else 3
        stride = stride or self.w * bpp
        out = np.full((self.h, stride), fill, dtype=np.uint8)
        a = np.ascontiguousarray(alpha, dtype=np.uint8) if alpha is not None else None
        fn = lib().yk_decode_output_reference_rgba if reference_rgba else lib().yk_decode_output
        _chk(self._h, fn(self._h, out.ctypes.data, stride, a.ctypes.data if a is not None else None, a.shape[1] if a is not None else 0))
        return out

    def image_into(self, out: np.ndarray) -> None:
        """RGB rows into a caller-owned [h, stride] uint8 array (no allocation per call)."""
        _chk(self._h, lib().yk_decode_output(self._h, out.ctypes.data, out.shape[1], None, 0))

    def image_window_device(self, out=None, channels: int | None = None, alpha: int | None = None, planar: bool = False):
        """image_device() for the window set by set_window (yk_decode_output_window_device): the window's pixels as a torch.uint8 tensor
        [wh, ww, C], or [C, wh, ww] with planar=True, equal to the same slice of the whole decode's image_device().  channels, alpha, `out`
        (any view with unit inner strides and any pitch, of the window's shape) and the stream hand-over are those of image_device; a decoded
        'ALPM' plane is read at the window's offset.  Without a window the call is image_device()."""
        return self._image_device(lib().yk_decode_output_window_device, self._window, out, channels, alpha, planar)

    def image_device(self, out=None, channels: int | None = None, alpha: int | None = None, planar: bool = False):
        """The decoded image as 8-bit pixels in a torch.uint8 tensor on the handle's device (yk_decode_output_device): [h, w, C], or
        [C, h, w] with planar=True.  channels defaults to 4 when an 'ALPM' plane was decoded, else 3 (as in image()).  With 4 channels,
        alpha=None takes the decoded plane when there is one and 255 otherwise; an int 0..255 is a constant alpha.  `out` may be any view with
        unit inner strides and any row or plane pitch (frames[f] of a batch, row-padded slices): only its pixel bytes are written.
        No host fence: the handle's stream waits for torch's current stream before the write, and torch's current stream waits for the
        write after it, so torch work queued afterwards sees the pixels.  Returns the tensor written.  Under a window (set_window) the library
        refuses with its state error: image_window_device() is the call."""
        return self._image_device(lib().yk_decode_output_device, None, out, channels, alpha, planar)

    def _image_device(self, fn, window, out, channels, alpha, planar, level=None):
        """image_device / image_window_device / image_scaled_device: the layout checks against the size written (the window's, or the image's, reduced
        by `level` when fn takes one), then fn between the hand-overs"""
        import torch
        ww, wh = (window[2], window[3]) if window is not None else (self.w, self.h)
        if level is not None:
            ww, wh = ww >> level, wh >> level
        C4 = channels if channels is not None else (4 if self._has_alpha else 3)
        a = (-1 if self._has_alpha else 255) if alpha is None else int(alpha)
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty((C4, wh, ww) if planar else (wh, ww, C4), dtype=torch.uint8, device=dev)
        elif not isinstance(out, torch.Tensor) or out.device != dev:
            raise ValueError(f"out must be a torch tensor on {dev}, got {getattr(out, 'device', type(out).__name__)}")
        if planar:
            lay = u8_planar_layout(out)
            shape, row_bytes, plane_bytes = (lay.channels, lay.rows, lay.w), lay.row_bytes, lay.plane_bytes
        else:
            lay = u8_pixel_layout(out)
            shape, row_bytes, plane_bytes = (lay.rows, lay.w, lay.channels), lay.row_bytes, 0
        want = (C4, wh, ww) if planar else (wh, ww, C4)
        if shape != want:
            raise ValueError(f"out has shape {shape}, the {'window' if window is not None else 'image'} needs {want}")
        L = lib()
        cur = torch.cuda.current_stream(dev).cuda_stream
        _chk(self._h, L.yk_stream_wait_for(self._h, cur))                  # torch may have just allocated or written `out`
        if level is None:
            _chk(self._h, fn(self._h, out.data_ptr(), row_bytes, plane_bytes, C4, a))
        else:
            _chk(self._h, fn(self._h, level, out.data_ptr(), row_bytes, plane_bytes, C4, a))
        _chk(self._h, L.yk_stream_handoff(self._h, cur))
        return out

    # ---- outputs at reduced resolution: 1/2, 1/4, 1/8 size box means straight from the de-tile kernel (yk_decode_output_scaled_device) ----
    @staticmethod
    def _check_level(level) -> int:
        """level as an int 0..3 (raises before any library call)"""
        if isinstance(level, bool) or not isinstance(level, (int, np.integer)):
            raise TypeError(f"level must be an int 0..3; got {level!r}")
        if not 0 <= int(level) <= 3:
            raise ValueError(f"level must be 0..3 (1/1, 1/2, 1/4, 1/8 size); got {level}")
        return int(level)

    @staticmethod
    def _check_out_shape(out, want, what: str) -> None:
        """an `out` of another shape than the reduced one (the full-size shape, say) is refused before anything else looks at it"""
        if out is not None and hasattr(out, "shape") and tuple(out.shape) != tuple(want):
            raise ValueError(f"out has shape {tuple(out.shape)}, the {what} needs {tuple(want)}")

    def image_scaled_device(self, level: int, out=None, channels: int | None = None, alpha: int | None = None, planar: bool = False):
        """The decoded image at 1 / (1 << level) size (level 0..3) as a torch.uint8 tensor on the handle's device: [h >> level, w >> level, C], or
        [C, h >> level, w >> level] with planar=True (yk_decode_output_scaled_device).  With a window set (set_window) it is the window that is
        reduced, otherwise the whole image; level 0 is image_window_device().  Every output pixel is the mean of its (1 << level)^2 box of the
        full-size decode, halves rounded up, computed from the full-size bytes inside the de-tile kernel: no full-size image is written.  Alpha
        is averaged like a colour channel (a constant stays that constant).  channels, alpha, `out` (of the reduced shape) and the stream
        hand-over are those of image_device.  level and the shape of `out` are checked before any library call."""
        level = self._check_level(level)
        win = self._window
        ww, wh = ((win[2], win[3]) if win is not None else (self.w, self.h))
        C4 = channels if channels is not None else (4 if self._has_alpha else 3)
        self._check_out_shape(out, (C4, wh >> level, ww >> level) if planar else (wh >> level, ww >> level, C4), "reduced window" if win is not None else "reduced image")
        return self._image_device(lib().yk_decode_output_scaled_device, win, out, channels, alpha, planar, level)

    def image_scaled_batch_device(self, level: int, out=None, channels: int = 3, alpha: int = 255, planar: bool = False, alpha_from_planes: bool = False):
        """image_batch_device() at 1 / (1 << level) size (yk_decode_output_scaled_batch_device, one launch): [N, h >> level, w >> level, C], or
        [N, C, h >> level, w >> level] with planar=True, every frame reduced by the rule of image_scaled_device.  alpha_from_planes=True
        (channels=4 only) averages the planes decompress_alpha_batch left on the device.  `out` follows image_batch_device at the reduced shape.
        level and the shape of `out` are checked before any library call."""
        import torch
        level = self._check_level(level)
        if alpha_from_planes and channels != 4:
            raise ValueError("alpha_from_planes needs channels=4")
        N, rw, rh = self.frames, self.w >> level, self.h >> level
        want = (N, channels, rh, rw) if planar else (N, rh, rw, channels)
        self._check_out_shape(out, want, "reduced batch")
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty(want, dtype=torch.uint8, device=dev)
        elif not isinstance(out, torch.Tensor) or out.device != dev:
            raise ValueError(f"out must be a torch tensor on {dev}, got {getattr(out, 'device', type(out).__name__)}")
        if planar:
            lay = u8_planar_batch_layout(out)
            plane_bytes = lay.plane_bytes
        else:
            lay = u8_pixel_layout(out, batch=True)
            plane_bytes = 0
        L = lib()
        cur = torch.cuda.current_stream(dev).cuda_stream
        _chk(self._h, L.yk_stream_wait_for(self._h, cur))                  # torch may have just allocated or written `out`
        _chk(self._h, L.yk_decode_output_scaled_batch_device(self._h, level, out.data_ptr(), lay.row_bytes, plane_bytes, lay.frame_bytes, channels,
                                                             -1 if alpha_from_planes else int(alpha)))
        _chk(self._h, L.yk_stream_handoff(self._h, cur))
        return out

    def render_windows_scaled(self, level: int, origins, w: int, h: int, out=None, channels: int | None = None, alpha: int | None = None, planar: bool = False):
        """render_windows() with reduced crops (yk_decode_render_windows_scaled_device): K windows of w x h FULL-RESOLUTION pixels at origins[k], each
        returned at 1 / (1 << level) size, [K, h >> level, w >> level, C] or [K, C, h >> level, w >> level] with planar=True, window k equal to the
        reduction (image_scaled_device's rule) of the same slice of the whole decode.  The blocks the windows touch are rendered at full size,
        once per prepared image, shared with render_windows: the two may be mixed freely.  level, the windows and the shape of `out` are checked
        before any library call."""
        import torch
        level = self._check_level(level)
        flat = self._check_windows(origins, w, h)
        K, ww, wh = len(flat) // 2, int(w), int(h)
        rw, rh = ww >> level, wh >> level
        C4 = channels if channels is not None else (4 if self._has_alpha else 3)
        a = (-1 if self._has_alpha else 255) if alpha is None else int(alpha)
        want = (K, C4, rh, rw) if planar else (K, rh, rw, C4)
        self._check_out_shape(out, want, "reduced windows")
        dev = torch.device("cuda", self.device)
        if out is None:
            out = torch.empty(want, dtype=torch.uint8, device=dev)
        elif not isinstance(out, torch.Tensor) or out.device != dev:
            raise ValueError(f"out must be a torch tensor on {dev}, got {getattr(out, 'device', type(out).__name__)}")
        if planar:
            lay = u8_planar_batch_layout(out)
            plane_bytes = lay.plane_bytes
        else:
            lay = u8_pixel_layout(out, batch=True)
            plane_bytes = 0
        L = lib()
        xy = (C.c_int * (2 * K))(*flat)
        cur = torch.cuda.current_stream(dev).cuda_stream
        _chk(self._h, L.yk_stream_wait_for(self._h, cur))                  # torch may have just allocated or written `out`
        _chk(self._h, L.yk_decode_render_windows_scaled_device(self._h, level, K, xy, ww, wh, out.data_ptr(), lay.row_bytes, plane_bytes, lay.frame_bytes, C4, a))
        _chk(self._h, L.yk_stream_handoff(self._h, cur))
        return out

    # ---- a full mip chain in one call: every level a box mean of level 0, the planes read once (yk_decode_output_mipchain_device) ----
    def mip_levels(self) -> int:
        """how many levels the image's chain has: floor(log2(min(w, h))) + 1, level k being (w >> k) x (h >> k)"""
        return min(self.w, self.h).bit_length()

    def _check_mip_range(self, first, count) -> tuple:
        """(first, count) as ints inside the chain (raises before any library call); count=None: every level from `first` down"""
        total = self.mip_levels()
        for name, v in (("first", first), ("count", count)):
            if (v is not None or name == "first") and (isinstance(v, bool) or not isinstance(v, (int, np.integer))):
                raise TypeError(f"{name} must be an int; got {v!r}")
        first = int(first)
        if not 0 <= first < total:
            raise ValueError(f"first must be a level 0..{total - 1} of this {self.w} x {self.h} image; got {first}")
        count = total - first if count is None else int(count)
        if not 1 <= count <= total - first:
            raise ValueError(f"count must be 1..{total - first} for first = {first} (the chain has {total} levels); got {count}")
        return first, count

    def _mipchain(self, fn, first, count, out, C4, a, planar, frames):
        """the two chain calls: the range, the list `out` and every shape first, then one table of the levels' layouts and fn between the hand-overs"""
        import torch
        from ._lib import MipLevel
        first, count = self._check_mip_range(first, count)
        if isinstance(C4, bool) or not isinstance(C4, (int, np.integer)):
            raise TypeError(f"channels must be 3 or 4; got {C4!r}")
        if C4 not in (3, 4):
            raise ValueError(f"channels must be 3 or 4; got {C4}")
        lead = () if frames is None else (frames,)
        wants = [lead + ((C4, self.h >> k, self.w >> k) if planar else (self.h >> k, self.w >> k, C4)) for k in range(first, first + count)]
        if out is not None:
            if not isinstance(out, (list, tuple)):
                raise TypeError(f"out must be a list of {count} tensors, one per level; got {type(out).__name__}")
            if len(out) != count:
                raise ValueError(f"out has {len(out)} tensors, levels {first}..{first + count - 1} need {count}")
            for k, (o, want) in enumerate(zip(out, wants), first):
                if not hasattr(o, "shape"):
                    raise TypeError(f"out[{k - first}] must be a torch tensor; got {type(o).__name__}")
                self._check_out_shape(o, want, f"level {k}")
        dev = torch.device("cuda", self.device)
        if out is None:
            out = [torch.empty(want, dtype=torch.uint8, device=dev) for want in wants]
        table = (MipLevel * count)()
        for i, o in enumerate(out):
            if not isinstance(o, torch.Tensor) or o.device != dev:
                raise ValueError(f"out[{i}] must be a torch tensor on {dev}, got {getattr(o, 'device', type(o).__name__)}")
            if planar:
                lay = u8_planar_layout(o) if frames is None else u8_planar_batch_layout(o)
                plane_bytes = lay.plane_bytes
            else:
                lay = u8_pixel_layout(o, batch=frames is not None)
                plane_bytes = 0
            table[i] = MipLevel(o.data_ptr(), lay.row_bytes, plane_bytes, 0 if frames is None else lay.frame_bytes)
        L = lib()
        cur = torch.cuda.current_stream(dev).cuda_stream
        _chk(self._h, L.yk_stream_wait_for(self._h, cur))                  # torch may have just allocated or written the levels
        _chk(self._h, fn(L)(self._h, first, count, table, C4, a))
        _chk(self._h, L.yk_stream_handoff(self._h, cur))
        return list(out)

    def image_mipchain_device(self, first: int = 0, count: int | None = None, out=None, channels: int | None = None, alpha: int | None = None, planar: bool = False):
        """Levels first .. first + count - 1 of the decoded image's mip chain (count=None: down to the last, mip_levels() - 1) as a list of torch.uint8
        tensors on the handle's device, level k [h >> k, w >> k, C], or [C, h >> k, w >> k] with planar=True (yk_decode_output_mipchain_device).
        Every pixel of level k is the mean of its (1 << k)^2 box of the full-size decode, halves rounded up, computed from the full-size bytes:
        levels 0..3 are image_device() and image_scaled_device(), the levels above ignore the columns and rows that fill no whole box.  One
        call reads the decoded planes once, however many levels it writes.  Alpha is averaged like a colour channel (a constant stays that
        constant).  channels, alpha and the stream hand-over are those of image_device; `out` is a list of views under image_device's stride
        rules, each of exactly its level's shape.  first, count, the length of `out` and every shape are checked before any library call."""
        C4 = channels if channels is not None else (4 if self._has_alpha else 3)
        a = (-1 if self._has_alpha else 255) if alpha is None else int(alpha)
        return self._mipchain(lambda L: L.yk_decode_output_mipchain_device, first, count, out, C4, a, planar, None)

    def image_mipchain_batch_device(self, first: int = 0, count: int | None = None, out=None, channels: int = 3, alpha: int = 255, planar: bool = False,
                                    alpha_from_planes: bool = False):
        """image_mipchain_device() for every frame of a batch in one call (yk_decode_output_mipchain_batch_device): a list of [N, h >> k, w >> k, C]
        tensors, or [N, C, h >> k, w >> k] with planar=True.  alpha_from_planes=True (channels=4 only) averages the planes decompress_alpha_batch
        left on the device.  `out` is a list of views under image_batch_device's stride rules."""
        if alpha_from_planes and channels != 4:
            raise ValueError("alpha_from_planes needs channels=4")
        return self._mipchain(lambda L: L.yk_decode_output_mipchain_batch_device, first, count, out, channels, -1 if alpha_from_planes else int(alpha), planar, self.frames)

    # ---- round-trip quality: the decode against a source that is already on the device (yk_decode_compare_*) --------------------------------
    def _compare_channels(self, channels, src_channels: int) -> int:
        if channels is None:
            return 4 if src_channels == 4 and (self._has_alpha or self._alpha_batch) else 3
        return int(channels)

    def _compare_tile_map(self, tile_map, n: int):
        """tile_map: False / None (no map), True (a new tensor) or a contiguous torch int32 tensor [n, h/8, w/8] on the device to write into"""
        import torch
        if tile_map is None or tile_map is False:
            return None
        dev, shape = torch.device("cuda", self.device), (n, self.h // 8, self.w // 8)
        if tile_map is True:
            return torch.empty(shape, dtype=torch.int32, device=dev)
        if not isinstance(tile_map, torch.Tensor) or tile_map.device != dev or tile_map.dtype not in (torch.int32, torch.uint32) \
                or tuple(tile_map.shape) != shape or not tile_map.is_contiguous():
            raise ValueError(f"tile_map must be True or a contiguous int32 tensor {shape} on {dev}")
        return tile_map

    def _compare_on_device(self, t, what: str):
        """the source's address goes to a kernel: anything but a torch tensor on the handle's device is refused here, before any library call"""
        import torch
        dev = torch.device("cuda", self.device)
        if not isinstance(t, torch.Tensor) or t.device != dev:
            raise ValueError(f"{what} must be a torch tensor on {dev}, got {getattr(t, 'device', type(t).__name__)}")

    def _compare_call(self, fn, args, n: int, channels: int, tmap) -> list:
        """the library call behind the stream hand-over, and its n structs as dicts"""
        import torch
        from .quality import YkQuality, quality_dict
        out = (YkQuality * n)()
        cur = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        _chk(self._h, lib().yk_stream_wait_for(self._h, cur))              # torch may have just written the source or allocated the map
        _chk(self._h, fn(self._h, *args, channels, out, tmap.data_ptr() if tmap is not None else None))
        res = [quality_dict(q, channels) for q in out]                      # the call has synchronised: the map is complete as well
        if tmap is not None:
            for f, r in enumerate(res):
                r["tile_sse"] = tmap[f]
        return res

    def compare_device(self, src, channels: int | None = None, planar: bool = False, tile_map=False) -> dict:
        """The decoded image -- or the selected frame of a batch -- against 8-bit source pixels in a torch.uint8 tensor on the handle's device,
        without moving a pixel to the host (yk_decode_compare_device): src is [h, w, C] (C = 3 or 4), or [C, h, w] with planar=True, any view with
        unit inner stride and any pitch or offset.  channels = 3 compares R, G, B (the 4th byte of an RGBA source is skipped), 4 also compares
        alpha against the decoded 'ALPM' plane; the default is 4 when the source has four channels and an alpha plane was decoded, else 3.
        Returns a dict of exact integers per channel -- sse, sad, n_diff, max_abs -- with psnr_db per channel and psnr_db_all over all compared
        samples (yaik_amd.quality).  tile_map=True adds tile_sse: an int32 tensor [h/8, w/8] on the device, the SSE of every 8x8 tile over the
        compared channels (or pass an int32 tensor [1, h/8, w/8] to write into).  What is compared is exactly what image_device() would write."""
        self._compare_on_device(src, "src")
        if planar:
            lay = u8_planar_layout(src)
            shape, row_bytes, plane_bytes = (lay.rows, lay.w), lay.row_bytes, lay.plane_bytes
        else:
            lay = u8_pixel_layout(src)
            shape, row_bytes, plane_bytes = (lay.rows, lay.w), lay.row_bytes, 0
        if shape != (self.h, self.w):
            raise ValueError(f"src is {shape[1]} x {shape[0]}, the image {self.w} x {self.h}")
        ch = self._compare_channels(channels, lay.channels)
        tmap = self._compare_tile_map(tile_map, 1)
        return self._compare_call(lib().yk_decode_compare_device, (src.data_ptr(), row_bytes, plane_bytes, lay.channels), 1, ch, tmap)[0]

    def compare_batch_device(self, src, channels: int | None = None, planar: bool = False, tile_map=False) -> list:
        """Every frame of the batch against its source in one call (yk_decode_compare_batch_device: two launches and one read-back whatever the
        frame count): src is [N, h, w, C], or [N, C, h, w] with planar=True, with any row, plane and frame pitch.  Returns one dict per frame as
        compare_device does; with tile_map=True (or an int32 tensor [N, h/8, w/8] to write into) frame f's dict holds tile_sse = map[f]."""
        self._compare_on_device(src, "src")
        if planar:
            lay = u8_planar_batch_layout(src)
            plane_bytes = lay.plane_bytes
        else:
            lay = u8_pixel_layout(src, batch=True)
            plane_bytes = 0
        if (lay.frames, lay.rows, lay.w) != (self.frames, self.h, self.w):
            raise ValueError(f"src holds {lay.frames} frames of {lay.w} x {lay.rows}, the batch {self.frames} of {self.w} x {self.h}")
        ch = self._compare_channels(channels, lay.channels)
        tmap = self._compare_tile_map(tile_map, self.frames)
        return self._compare_call(lib().yk_decode_compare_batch_device, (src.data_ptr(), lay.row_bytes, plane_bytes, lay.frame_bytes, lay.channels),
                                  self.frames, ch, tmap)

    def compare_planes(self, planes, channels: int | None = None, tile_map=False):
        """Every frame against int32 planes as the encoder binds them (yk_decode_compare_planes_device): a torch int32 tensor [P, h, w] on the
        device for a single image (returns a dict) or [N, P, h, w] for the batch (returns a list), P >= channels, unit inner stride and any row,
        plane and frame stride; the low byte of a sample is compared.  channels defaults to 4 when P == 4 and an alpha plane was decoded."""
        import torch
        self._compare_on_device(planes, "planes")
        if planes.dtype != torch.int32 or planes.dim() not in (3, 4):
            raise ValueError("planes must be a torch int32 tensor [P, h, w] or [N, P, h, w]")
        single = planes.dim() == 3
        p4 = planes[None] if single else planes
        n, P, h, w = p4.shape
        if (n, h, w) != (self.frames, self.h, self.w) or P not in (3, 4):
            raise ValueError(f"planes hold {n} frames of {P} planes of {w} x {h}; the decode holds {self.frames} frames of {self.w} x {self.h}")
        sf, sp, sr, sx = p4.stride()
        if sx != 1 or sr < w:
            raise ValueError(f"the samples of a row must be contiguous and rows may not overlap; got strides {tuple(planes.stride())}")
        ch = self._compare_channels(channels, P)
        if ch > P:
            raise ValueError(f"{ch} channels cannot be compared with {P} planes")
        tmap = self._compare_tile_map(tile_map, n)
        ptrs = (C.c_void_p * 4)(*[p4.data_ptr() + k * sp * 4 if k < P else None for k in range(4)])
        res = self._compare_call(lib().yk_decode_compare_planes_device, (ptrs, sr, sf if n > 1 else 0), n, ch, tmap)
        return res[0] if single else res

    def synchronize(self):
        _chk(self._h, lib().yk_synchronize(self._h))

    def stage_ms(self, stage: int) -> tuple[float, int]:
        ms, n = C.c_float(), C.c_int()
        _chk(self._h, lib().yk_stage_ms(self._h, stage, C.byref(ms), C.byref(n)))
        return float(ms.value), int(n.value)

    def tile4x4(self, all_planes: bool = False) -> np.ndarray:
        n = ((((self.w + 15) >> 4) << 2) * (((self.h + 7) >> 3) << 1)) >> 3
        out = np.zeros(n * (3 if all_planes else 1), dtype=np.uint8)
        fn = lib().yk_decode_tile4x4_planes if all_planes else lib().yk_decode_tile4x4
        _chk(self._h, fn(self._h, out.ctypes.data, out.size))
        return out
