/* yaik_hip.h — C-ABI of the MI355X (gfx950) implementation of the YAIK per-tile hot path.
 *
 * This is the drop-in boundary: plain C, opaque handle, caller-owned pointers and sizes, no C++ or
 * torch types.  Every entry point names the reference interface it replaces (paths relative to the
 * KLab/YAIK tree).  The reference has no FFI of its own — the passes are C++ member functions called
 * in-process — so the boundary sits exactly where `EncoderContext` touches pixels; the C++ mirror of
 * that class in yaik_amd/host/ (same method names and argument meaning) is a thin caller of these
 * functions, and INTEGRATION.md shows the binding a YAIK maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative yk_status on failure (first error text is kept
 *     in the handle: yk_last_error).  Nothing throws.  There is NO CPU fallback: without a usable
 *     HIP device yk_create fails.
 *   - one handle per host thread / GPU; handles are not thread-safe.
 *   - "device pointer" = HBM address valid on the handle's device (e.g. torch tensor data_ptr()).
 *   - planes are int32, row-major, values in [0,255]: the reference `Plane` layout
 *     (encoder/framework.h:74-127, idx = x + y*w).  Width and height must be multiples of 8
 *     (Image::LoadPNG enforces the same, encoder/Image.cpp:206).
 *   - all launches go to the handle's stream; getters that copy to host synchronise that stream.
 */
#ifndef YAIK_HIP_H
#define YAIK_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct yk_ctx yk_ctx;

enum yk_status {
    YK_OK = 0,
    YK_ERR_NO_DEVICE = -1,      /* no HIP device / runtime: the product path refuses to run */
    YK_ERR_BAD_ARG = -2,
    YK_ERR_HIP = -3,            /* a HIP call failed; see yk_last_error */
    YK_ERR_STATE = -4,          /* call order violated (e.g. encode before binding planes) */
    YK_ERR_RANGE = -5,          /* output buffer too small */
    YK_ERR_COMM = -6            /* RCCL missing or a RCCL call failed; see yk_last_error */
};

/* number of gradient passes and their (tileShiftX, tileShiftY) in the shipped order
 * 16x16,16x8,8x16,8x8,8x4,4x8,4x4 (encoder/EncoderContext.cpp:9057-9093) */
#define YK_NUM_PASSES 7

/* ---- lifetime ------------------------------------------------------------------------------ */
int         yk_create(int device, yk_ctx** out);
void        yk_destroy(yk_ctx* c);
const char* yk_last_error(const yk_ctx* c);
/* NULL = the handle's own non-blocking stream (the default).  That stream is NOT ordered against the null stream or any
 * other stream of the process: fence hand-overs of buffers on the host, or pass the producer's / consumer's stream here.
 * A stream handle is only meaningful inside the HIP runtime instance that created it (a process that loads this library
 * before a framework's bundled copy of the runtime ends up with two instances; load the framework first). */
/* The stream being replaced should still exist when this is called (the new stream is ordered behind what the old one holds); if it was
 * destroyed meanwhile the switch still happens, without that ordering. */
int         yk_set_stream(yk_ctx* c, void* hipStream);
int         yk_synchronize(yk_ctx* c);
/* Device-side ordering against another stream of the SAME runtime instance (0 = the null stream), instead of a host fence:
 * yk_stream_wait_for: everything queued on the handle's stream from now on waits for what `producerStream` holds now;
 * yk_stream_handoff:  everything queued on `consumerStream` from now on waits for what the handle's stream holds now. */
int         yk_stream_wait_for(yk_ctx* c, void* producerStream);
int         yk_stream_handoff(yk_ctx* c, void* consumerStream);
int         yk_device_count(void);                          /* no device initialisation side effects beyond hipGetDeviceCount */

/* ---- image binding:  EncoderContext::SetImageToEncode (encoder/EncoderContext.cpp:1227) ------
 * A handle works on one image or one row stripe of an image.  fullW/fullH are the whole image,
 * [y0, y0+h) the rows this handle owns (y0 and h multiples of 64 unless the stripe is the last one);
 * for a whole image pass y0 = 0, h = fullH.  The planes handed in must contain the owned rows plus
 * `haloRows` (0 or 1) further row: FittingQuadSmooth samples the BL/BR corners at y+T
 * (EncoderContext.cpp:3855-3856); the last stripe clamps like Plane::GetPixelValue instead. */
int yk_set_image(yk_ctx* c, int fullW, int fullH, int nPlanes, int y0, int h, int haloRows);
/* host planes -> HBM copy owned by the handle (strideElems = row pitch in int32 elements) */
int yk_upload_planes(yk_ctx* c, const int32_t* const hostPlanes[4], int strideElems);
/* zero-copy: planes already resident in HBM */
int yk_bind_device_planes(yk_ctx* c, const int32_t* const devPlanes[4], int strideElems);
/* The path is defined for samples in 0..255 held in int32 planes (the fused kernel keeps their low byte; the reference reads the whole int,
 * encoder/framework.h:116-121).  yk_upload_planes checks what it copied and fails with YK_ERR_BAD_ARG (no planes bound afterwards) when a sample
 * lies outside; callers that bind device memory and cannot vouch for its contents call yk_validate_planes: *nOutOfRange = samples outside 0..255
 * in the bound planes (all frames of a batch; one streaming pass, synchronises). */
int yk_validate_planes(yk_ctx* c, size_t* nOutOfRange);
/* 8-bit interleaved pixels (new; the pixels Image::LoadPNG widens on the host, encoder/Image.cpp:200-229): one kernel writes the handle's OWN
 * planes (the buffer yk_upload_planes fills, same layout) from rows of `channels` (3 = RGB, 4 = RGBA) bytes per pixel at a pitch of rowBytes:
 * plane p at (x, y) = pixels[y * rowBytes + x * channels + p] for p < nPlanes.  Four channels into 3 planes drop the 4th byte (RGBX).  For a
 * stripe the rows start at the stripe's first owned row and hold h + haloRows rows, as for planes.  Afterwards the handle is in the state
 * yk_upload_planes leaves (same flags reset): every consumer works unchanged.  There is no validation pass (8-bit samples are always in
 * range) and no allocation while the shape fits the buffers the handle already holds.  Any base address and pitch is accepted: a source
 * whose base and rowBytes (and frameBytes) are multiples of 16 is read through aligned pointers, any other one through byte pointers with no
 * alignment assumed (on gfx950 both read one 12- or 16-byte load per 4 pixels).
 * Errors: YK_ERR_BAD_ARG for a NULL pointer, channels not 3 or 4, channels < nPlanes, rowBytes < w * channels (and, for a batch, frameBytes
 * < rowBytes * fullH); YK_ERR_STATE before yk_set_image.  On any failure no planes are bound afterwards, as with yk_upload_planes' refusal.
 * yk_upload_pixels_u8: host pixels, one 2-D host-to-device copy into a grow-only 8-bit staging buffer of the handle, then the kernel.  Single
 * images and stripes only (YK_ERR_STATE for batches, like yk_upload_planes).  Returns when hostPixels may be reused. */
int yk_upload_pixels_u8(yk_ctx* c, const uint8_t* hostPixels, size_t rowBytes, int channels);
/* yk_load_device_pixels_u8: pixels in HBM on the handle's device; the kernel only, no host synchronisation.  With nFrames > 1 (yk_set_batch)
 * frame f starts at devPixels + f * frameBytes (frameBytes >= rowBytes * fullH); frameBytes is ignored for one frame.
 * ORDERING is the caller's, as for the yk_decode_*_device entry points: the source is read on THIS handle's stream, and nothing orders that
 * stream behind the producer's.  Order the producer first (yk_stream_wait_for(c, producerStream), or a host fence such as synchronising the
 * producer's stream), and leave the source unchanged until the handle's stream has passed the call (yk_stream_handoff(c, consumerStream),
 * yk_synchronize, or a getter that synchronises).  Unlike with yk_bind_device_planes, the source may be reused after that: the planes the
 * encode reads are the handle's own. */
int yk_load_device_pixels_u8(yk_ctx* c, const uint8_t* devPixels, size_t rowBytes, size_t frameBytes, int channels);

/* ---- a9  alpha tile-reject:  EncoderContext::MipPrefilter (EncoderContext.cpp:1257-1427) -----
 * stage 1 (per stripe): per aligned 16x16 block "all 256 alphas == 0" + bounding box of kept blocks. */
int yk_alpha_reject(yk_ctx* c);
/* bbox of kept blocks of THIS stripe in full-image pixels {x0,y0,x1,y1}; {9999999,9999999,-1,-1} if none. Synchronises. */
int yk_get_stripe_bbox(yk_ctx* c, int32_t bbox[4]);
/* stage 2: the image-wide bbox (min/max over stripes; for a whole image pass yk_get_stripe_bbox's result or NULL
 * to use the handle's own).  Applies the reference rule "bbox == whole image -> all rejects discarded, no chunk"
 * (:1294, :1400-1403) and fixes boundX0..Y1 for the range quantiser.  Images without alpha: call with NULL or skip. */
int yk_alpha_finish(yk_ctx* c, const int32_t globalBBox[4]);
/* results: bounds[4] = boundX0,boundY0,boundX1,boundY1; hasChunk; remainingPixels (this stripe);
 * tileBBox[4] = MipmapHeader.bbox in 16-px tiles (x,y,w,h).  Synchronises. */
int yk_alpha_result(yk_ctx* c, int32_t bounds[4], int* hasChunk, int* remainingPixels, int32_t tileBBox[4]);
/* 'MIPM' payload: 1 bit per 16x16 tile inside tileBBox, row-major, LSB first, 1 = kept (:1317-1327).
 * For a stripe: only the bits of the owned rows are set (OR the stripes' buffers). cap >= (w*h+7)/8 of tileBBox. */
int yk_alpha_bitmap(yk_ctx* c, uint8_t* hostOut, size_t cap, size_t* nBytes);
/* EncoderContext::ProcessAlpha(force8Bit) (encoder/EncoderContext.cpp:1429-1682): the alpha VALUES of a whole single image, after
 * yk_alpha_reject + yk_alpha_finish (the search region is their bounds, read on the device).  One kernel reduces the box of samples with
 * v >> 2 != 0; one kernel reads the box rounded to 4 once for the class flags and the 8-bit payload; binary alpha (only 0 / 255 in the box)
 * is packed again by a third kernel on the box re-aligned to 8 (make1BitStream, :317-355).  Two small readbacks (box, class) size the launches.
 * force8Bit = 0 (:1503-1565): analog alpha becomes IS_6_BIT_USEMIPMAPMASK_INVERSE, 63 - (v >> 2) of the box samples the mipmapMask selects
 * (every pixel of a kept 16x16 tile, or every pixel when the kept tiles span the image), four values in three bytes; three more kernels
 * (per-band tile prefixes from the keep flags, their scan, the pack from the u8 box) and a third readback (the selected count).
 * Binary, all-255 and empty alpha are the same for both values of force8Bit.
 * out->mode = -1 (no chunk: no alpha plane, empty box, all 255), 1 (IS_1_BIT_FULL), 3 (IS_6_BIT_USEMIPMAPMASK_INVERSE, force8Bit = 0) or
 * 6 (IS_8_BIT_FULL, force8Bit = 1); bbox = {x, y, w, h}; rawSize = the decompressed payload size (expectedDecompressionSize).
 * hostPayload may be NULL (size query); *n = rawSize.  Convert passes force8Bit = 1 (:9027-9028).  Synchronises. */
typedef struct yk_alpha_info { int32_t mode; int32_t bbox[4]; uint32_t rawSize; } yk_alpha_info;
int yk_alpha_values(yk_ctx* c, int force8Bit, yk_alpha_info* out, uint8_t* hostPayload, size_t cap, size_t* n);
/* yk_alpha_values(force8Bit = 1) for every frame of the handle (nFrames 1..1024), after the alpha stage of all frames: yk_encode_batch, or for a
 * batch of one yk_alpha_reject + yk_alpha_finish.  infos[f] is exactly what yk_alpha_values returns for frame f bound alone (mode -1 / 1 / 6, box,
 * rawSize) and the payload is byte-identical.  Whatever nFrames is, a call costs at most three kernel launches, two blocking read-backs and one
 * table upload: the box reduction over all frames (frame = a grid dimension) and the read-back of every box; the host lays the payload slots out
 * back to back in one buffer (slot = w * h bytes of the box rounded to 4, each offset rounded up to 16) and uploads one record per frame that has a
 * box; the class flags + 8-bit payload kernel over those frames (grid sized from the largest box) and the read-back of the flags; the 1-bit pack
 * over the frames classed binary, into the same slots (not launched when no frame is binary).  Frames without an alpha plane: mode -1 for all.
 * The payloads stay in HBM: yk_alpha_payload_device hands out frame's slot (*dev = NULL, *nBytes = 0 for a frame without a chunk) without a host
 * synchronisation -- read it on this handle's stream or behind yk_stream_handoff; valid until the next encode, yk_set_image or
 * yk_alpha_values[_batch] of the handle.  yk_alpha_payload copies it to the host (*nBytes = rawSize, also when hostOut is too small) and synchronises.
 * Refusals launch nothing and leave the handle usable: YK_ERR_BAD_ARG for NULL infos, and for force8Bit = 0 (the 6-bit mask mode is not batched: it
 * needs every frame's mask selection); YK_ERR_STATE before the alpha stage has finished, or on a stripe.  The getters: YK_ERR_BAD_ARG for a frame
 * out of range, YK_ERR_STATE before yk_alpha_values_batch, YK_ERR_RANGE for a short buffer. */
int yk_alpha_values_batch(yk_ctx* c, int force8Bit, yk_alpha_info* infos /* nFrames */);
int yk_alpha_payload_device(yk_ctx* c, int frame, const uint8_t** dev, size_t* nBytes);
int yk_alpha_payload(yk_ctx* c, int frame, uint8_t* hostOut, size_t cap, size_t* nBytes);
/* yk_alpha_values(force8Bit[f]) for every frame of the handle, the 6-bit mask mode included; force8Bit = NULL is 0 for every frame.  Valid in the
 * states of yk_alpha_values_batch.  infos[f] and frame f's payload are byte for byte what yk_alpha_values(c, force8Bit[f], ..) returns for that
 * frame bound alone: mode -1, 1, 3 or 6.  Box, class and 1-bit pack are yk_alpha_values_batch's; the frames classed analog whose force8Bit is 0 get
 * one record each (keep flags, bounds, the u8 box in the frame's 8-bit slot, a 6-bit slot of (bw / 4) * 3 * bh bytes on a multiple of 16 in a second
 * grow-only buffer) and three launches over all of them: band prefixes (one wave per tile band), one wave per record scanning its bands, the pack.
 * Whatever nFrames is: at most six launches, three blocking read-backs (boxes, class flags, selected counts) and two table uploads; when no frame
 * takes the 6-bit path the call costs what yk_alpha_values_batch costs.  A selected count beyond the box fails with YK_ERR_STATE.
 * The getters above hand out the 6-bit slot for mode 3 and the 8-bit slot for modes 1 and 6, under the same validity rule.
 * Refusals launch nothing and leave the handle and earlier published payloads usable: YK_ERR_BAD_ARG for NULL infos; YK_ERR_STATE before the alpha
 * stage has finished, on a stripe, without bound planes, and for a handle without keep flags.  No alpha plane: mode -1 for all, nothing launched. */
int yk_alpha_values_mask_batch(yk_ctx* c, const uint8_t* force8Bit /* nFrames, or NULL */, yk_alpha_info* infos /* nFrames */);
/* The 'MIPM' bitmaps of every frame of the handle (new), after the alpha stage of all frames: yk_encode_batch, or for a batch of one yk_alpha_reject +
 * yk_alpha_finish.  infos[f] and frame f's bytes are exactly what yk_select_frame(f) + yk_alpha_result + yk_alpha_bitmap give: hasChunk = 0 and
 * nBytes = 0 when the box is the whole image, nBytes = 0 when no tile is kept (bounds[2] < bounds[0]), otherwise bit y * tw + x of tileBBox, LSB
 * first; remainingPixels is not reported (no chunk needs it).  Whatever nFrames is, a call is ONE kernel launch (frame = a grid dimension; a thread
 * produces one output byte from the keep flags and the box of its frame, both read on the device) and ONE blocking read-back (the boxes).  Every
 * frame has a slot of (mtW * mtH + 7) / 8 bytes rounded up to 16 in a buffer of the handle that only grows; the kernel writes the whole slot (zeros
 * behind nBytes), so nothing is cleared.  A handle without an alpha plane launches nothing: hasChunk 0, the whole image as bounds, tileBBox 0.
 * yk_alpha_bitmap_device hands out frame's slot where it lies in HBM (*dev = NULL, *nBytes = 0 for a frame without bits) without a host
 * synchronisation; valid until the next encode, yk_alpha_reject, yk_set_image, yk_set_batch or (re)bind of the handle.  Neither call touches the
 * buffers of yk_alpha_values[_batch].
 * Refusals launch nothing and leave the handle usable: YK_ERR_BAD_ARG for NULL infos / result pointers and a frame out of range; YK_ERR_STATE on a
 * stripe, before yk_set_image, before the alpha stage has finished, and for yk_alpha_bitmap_device before yk_alpha_bitmaps_batch. */
typedef struct yk_mip_info { int32_t hasChunk; int32_t bounds[4]; int32_t tileBBox[4]; uint32_t nBytes; } yk_mip_info;
int yk_alpha_bitmaps_batch(yk_ctx* c, yk_mip_info* infos /* nFrames */);
int yk_alpha_bitmap_device(yk_ctx* c, int frame, const uint8_t** dev, size_t* nBytes);

/* ---- a6 + a10..a13  fused tile encode ----------------------------------------------------------
 * One launch does what 7x EncoderContext::FittingQuadSmooth(rejectFactor, R,G,B, .., sx, sy)
 * (EncoderContext.cpp:3710-4363) followed by DynamicTileEncode(mode3BitOnly, plane, dst, ..) for the three
 * planes (EncoderContext.cpp:4365-4602) compute, reading every input sample once.
 *   rejectFactor : the reference passes 3 (:9042)
 *   mode3BitOnly : DynamicTileEncode's first argument (Stats.startMode = 3, :4412)
 *   wantDst      : also produce the decoded-value planes `dst` (:4448-4457); costs 12 B/pixel of writes */
int yk_encode_tiles(yk_ctx* c, int rejectFactor, int mode3BitOnly, int wantDst);
/* The whole frame with ONE launch: alpha reject (RGBA) + fused kernel + stream compaction captured as a hipGraph the first
 * time and replayed afterwards (re-captured when the bound planes, the shape or the arguments change).  Same results as
 * yk_alpha_reject + yk_alpha_finish(NULL) + yk_encode_tiles(.., wantDst 0); for batches of small frames, where the ~8 stream
 * operations per frame cost more host time than the kernels take.  Whole images only (a stripe needs the host bbox step). */
int yk_encode_frame(yk_ctx* c, int rejectFactor, int mode3BitOnly);

/* ---- batches of equally shaped images (new; BASELINE config 4: 256 x 2048x2048 frames) --------------------------------
 * A frame of 2048x2048 is one round of waves: alone it cannot fill the chip.  A handle can hold nFrames images of one shape
 * (yk_set_image for the shape, then yk_set_batch) whose planes lie at frame0Planes[p] + f * frameStrideElems; yk_encode_batch
 * runs alpha reject + fused kernel + compaction over ALL frames with one launch per kernel (the grid simply spans
 * nFrames x strips), with the same per-frame results as yk_encode_frame.  yk_select_frame chooses the frame every getter,
 * yk_export_tile_maps and the single-image corner streams (yk_gradient_corners*) and 1-D path (yk_range1d_*) act on (default 0);
 * yk_encode_streams_batch below builds the corner and 1-D streams of ALL frames at once.  Whole images only, kernel version 2. */
int yk_set_batch(yk_ctx* c, int nFrames);
int yk_bind_device_batch(yk_ctx* c, const int32_t* const frame0Planes[4], int strideElems, size_t frameStrideElems);
int yk_encode_batch(yk_ctx* c, int rejectFactor, int mode3BitOnly);
int yk_select_frame(yk_ctx* c, int frame);

/* The corner colour streams and the live 1-D streams of every frame of the handle, one launch per kernel (new).
 * yk_encode_streams_batch(what = YK_STREAMS_CORNERS | YK_STREAMS_RANGE1D, 1..3) is valid after yk_encode_batch and, for a batch of one, after
 * yk_encode_tiles / yk_encode_frame on a whole image.  Frame f's results are byte-identical to yk_select_frame(f) followed by yk_gradient_corners
 * for the seven passes and by yk_range1d_encode + yk_range1d_streams.  Whatever nFrames (1..1024) is, the call makes at most seven kernel launches
 * and the lattice clear, ONE blocking read-back (nine uint32 per frame: the stream lengths) and one upload of a table of stream bases; the streams
 * are packed into one buffer in HBM, each at an offset that is a multiple of 16 (yk_decode_1d_batch_device reads pixel streams in place), with no
 * worst-case regions: the buffer is as large as the streams are and only grows.  The stripe edge index (yk_gradient_corner_edges) is not
 * produced and the pixel cache (yk_set_pixel_cache) is not used.  One interval of YK_STAGE_CORNERS (which spans the read-back), YK_STAGE_RANGE1D_PACK
 * and YK_STAGE_RANGE1D per call, each only when that stage is requested.
 * yk_batch_streams_table fills out[0..nFrames): bitmap[p] / bitmapBytes[p] are what yk_gradient_bitmap_device(p) / yk_gradient_bitmap_bytes(p) give
 * for that frame; rgb[p] is the corner stream of pass p (CompressF(., 250) bytes, not remapped), pix the 1-D pixel stream (planes R, G, B
 * appended), type the 1-D parameter triples; a stream that is empty or was not requested has a NULL pointer and length 0.  No synchronisation:
 * the emit kernels may still be running, so read the streams on this handle's stream or behind yk_stream_handoff (yk_synchronize on the host).
 * The batch's results live in buffers of their own: yk_select_frame and the single-image getters still work afterwards and do not disturb them.
 * The table and the streams stay valid until the next yk_encode_tiles / yk_encode_frame / yk_encode_batch, yk_set_image, yk_set_batch, (re)bind
 * or upload of planes or pixels, or yk_encode_streams_batch of the handle; yk_select_frame does not invalidate them.
 * Refusals launch nothing and leave the handle and an earlier valid table usable (the message: yk_last_error): YK_ERR_BAD_ARG for `what` outside
 * 1..3 or a NULL `out`; YK_ERR_STATE before an encode, on a stripe, with no planes bound, after a plane-subset pass (yk_gradient_partial_pass),
 * and for yk_batch_streams_table without a valid table. */
enum { YK_STREAMS_CORNERS = 1, YK_STREAMS_RANGE1D = 2 };
typedef struct yk_frame_streams {
    const uint8_t* bitmap[7]; size_t bitmapBytes[7];
    const uint8_t* rgb[7];    size_t rgbBytes[7];
    const uint8_t* pix;  size_t pixBytes;
    const uint8_t* type; size_t typeBytes;
} yk_frame_streams;
int yk_encode_streams_batch(yk_ctx* c, int what);
int yk_batch_streams_table(yk_ctx* c, yk_frame_streams* out /* nFrames */);

/* ---- PaletteCompressor on the GPU (new): the 'GTIL' colour payloads, byte-exact ---------------------------------------------------------
 * EncoderContext.cpp:3259-3502 (registerCodeBook :3231, FindCodeBook :3248): the delta / code-book coder the corner colour streams pass through
 * before ZStd.  Its output for a stream depends on the streams coded before it: FindCodeBook scans rows 0..63 of a table whose rows survive from
 * call to call, so the state that carries is exactly 64 rows (all (0,0,0) in a fresh process).  The handle keeps those rows in HBM.
 *   yk_palette_reset             forgets the carried rows: the next continuing call behaves like the first call of a fresh process.
 *   yk_palette_compress_streams  nStreams (1..65536) streams anywhere in the device's memory, nBytes[i] each a multiple of 3 (a colour is 3 bytes).
 *                                chain = K > 0: every run of K consecutive streams starts from the fresh rows and carries them through the run
 *                                (K = 7: one frame per run); the handle's carried rows are neither read nor written.  chain = 0: the streams
 *                                continue from the handle's carried rows, in order, and leave theirs behind.  A stream of length 0 is skipped and
 *                                leaves the rows alone, like a pass without a chunk; its payload is empty.
 *   yk_palette_compress          the seven corner streams of the selected frame (built first if needed, as by yk_gradient_corners_device), with
 *                                chain = 0.  Whole images; not after a plane-subset pass.
 *   yk_palette_compress_batch    the 7 x nFrames corner streams of a valid yk_encode_streams_batch table built with YK_STREAMS_CORNERS, chain = 7:
 *                                every frame like one image of a fresh process.  Does not touch the carried rows.
 * A call is eight kernel launches and two clears over all its streams, whatever their number, and ONE blocking read-back at its end (8 bytes per
 * stream: payload length and offset).  The payloads lie packed in one grow-only buffer of the handle, each at a multiple of 16.
 *   yk_palette_payload_device    payload `index` (the stream's number in the last call; frame * 7 + pass after the batch call) where it lies in HBM
 *                                and its length, which is what the chunk header's streamRGBSizeCustomCompressor holds; NULL / 0 for a skipped stream.
 *   yk_palette_payload           the same copied to the host (hostOut may be NULL: size query); synchronises.
 * The payloads stay valid under the rule of the streams table: until the next encode, yk_set_image, yk_set_batch, (re)bind or upload of planes or
 * pixels, yk_encode_streams_batch or yk_palette_compress* of the handle.  The input streams are read on the handle's stream: ORDERING against
 * their producer is the caller's, as for the yk_decode_*_device entry points.  Timed as one YK_STAGE_PALETTE interval per call.
 * Refusals launch nothing, leave earlier payloads, the carried rows and the handle usable, and set yk_last_error: YK_ERR_BAD_ARG for a NULL table,
 * nStreams outside 1..65536, chain < 0, a length that is not a multiple of 3 (plane-subset streams stay with the host coder), a length with a
 * NULL pointer, more than 2^28 colours in one call, a payload index out of range; YK_ERR_STATE on a stripe, before an encode, after a
 * plane-subset pass, without a valid table with corner streams (batch), and for the getters before any call; YK_ERR_RANGE for a short buffer. */
int yk_palette_reset(yk_ctx* c);
int yk_palette_compress_streams(yk_ctx* c, const uint8_t* const* devStreams, const size_t* nBytes, int nStreams, int chain);
int yk_palette_compress(yk_ctx* c);
int yk_palette_compress_batch(yk_ctx* c);
int yk_palette_payload_device(yk_ctx* c, int index, const uint8_t** dev, size_t* nBytes);
int yk_palette_payload(yk_ctx* c, int index, uint8_t* hostOut, size_t cap, size_t* nBytes);

/* ---- PaletteDecompressor on the GPU (new): 'GTIL' colour payloads back to colour streams, byte-exact -----------------------------------------
 * decoder/YAIK_GenericFunctions.cpp:139-241, as the project's CPU restatement (yko_palette_decompress) executes it.  A payload of n bytes is read as if
 * followed by zeros; a token may start at any offset below n + 385; byte 0 is codeBookSize and 1 + 3 * codeBookSize > n is an error; code index i
 * (0..127) reads the bytes at 1 + 3i .. 3 + 3i whatever codeBookSize says; outBytes / 3 colours are written and nothing behind the token that
 * writes the last one is looked at.
 *   yk_palette_decompress_streams  nStreams (1..65536) payloads anywhere in the device's memory.  outBytes[i] is the chunk header's
 *                                  streamRGBSizeUncompressed, a multiple of 3; 0 skips the stream (status 0, empty output).  remapRange 1..255
 *                                  applies PaletteFullRangeRemapping(range) to every output, 0 leaves the bytes as decoded (which is the encoder's
 *                                  corner stream whenever the round trip is clean).  Six kernel launches over all streams on the handle's stream
 *                                  and NO host synchronisation (the stream table travels through the pinned ring of the decode batch calls:
 *                                  a call waits only when the tables of four earlier calls are all still queued); ORDERING against the payloads' producer is the caller's, as for yk_decode_*_device.
 *                                  The outputs lie packed in one grow-only buffer of the handle, each at a multiple of 16, with 64 bytes the call
 *                                  never writes in front of the first and behind the last.
 *   yk_palette_decoded_device      output `index` where it lies in HBM and its length (NULL / 0 for a skipped stream).
 *   yk_palette_decoded             the same copied to the host (hostOut may be NULL: size query); synchronises.
 *   yk_palette_decode_status       synchronises and reads one word per stream back: 0 = decoded, non-zero = PaletteDecompressor rejects the payload.
 *                                  Only zero / non-zero is contract.  The bits say what was found at or before the token that writes the last
 *                                  colour: 1 header longer than the payload, 2 an extension code (1001xxxx, 101xxxxx), 4 input exhausted (a token
 *                                  at or beyond n + 385), 8 a back-reference before colour 0.
 * Malformed payloads are data, not bad arguments: the call returns YK_OK, the other streams are unaffected, the failed stream's slot holds
 * unspecified bytes and nothing outside a slot is written.  The outputs stay valid until the next yk_palette_decompress_streams or
 * yk_decode_gradient_palette of the handle.  Timed as one YK_STAGE_PALETTE_DEC interval per call.
 * Refusals launch nothing, leave earlier outputs and the handle usable and set yk_last_error: YK_ERR_BAD_ARG for a NULL table, nStreams outside
 * 1..65536, an outBytes that is not a multiple of 3 (plane-subset streams stay with the host coder), outBytes != 0 with payBytes == 0 or a NULL
 * pointer, more than 2^28 colours or 2^31 payload bytes in one call, remapRange outside 0..255, an index out of range; YK_ERR_STATE for the getters
 * and the status before any call; YK_ERR_RANGE for a short buffer.
 *   yk_decode_gradient_palette     yk_decode_gradient fed with the 'GTIL' payload instead of the colour stream (host pointers): uploads bitmap and
 *                                  payload, decompresses on the device with PaletteFullRangeRemapping(colorCompression) (0 behaves as 1, as in the
 *                                  reference), checks the status and decodes the pass.  A malformed payload gives YK_ERR_BAD_ARG and a message
 *                                  before anything of the image is touched. */
int yk_palette_decompress_streams(yk_ctx* c, const uint8_t* const* devPayloads, const size_t* payBytes, const size_t* outBytes, int nStreams, int remapRange);
int yk_palette_decoded_device(yk_ctx* c, int index, const uint8_t** dev, size_t* nBytes);
int yk_palette_decoded(yk_ctx* c, int index, uint8_t* hostOut, size_t cap, size_t* nBytes);
int yk_palette_decode_status(yk_ctx* c, int32_t* out /* nStreams */);
int yk_decode_gradient_palette(yk_ctx* c, int tileShiftX, int tileShiftY, const uint8_t* bitmap, size_t bitmapBytes,
                               const uint8_t* payload, size_t payloadBytes, size_t rgbBytes, int colorCompression);

/* ---- streams of frames on several handles (new) --------------------------------------------------------------------------
 * With two handles (two streams) in flight the HBM-bound alpha / compaction kernels of one frame run under the fused kernel of
 * the other.  Two fused kernels sharing the chip only slow each other down, so a caller that alternates handles can order them:
 * the NEXT yk_encode_tiles of c launches its fused kernel after the fused kernel most recently launched on `other` has finished
 * (one stream-wait on the event behind that kernel, queued on c's own stream where the fused kernel is launched; no host synchronisation; the
 * alpha stage and the compaction of c are not held back).  Same device.  `other` may be destroyed before that encode of c is issued:
 * the two handles share the ownership of the event.  A handle that has never encoded orders nothing.  The request is consumed by the next
 * yk_encode_tiles / yk_encode_batch / yk_encode_frame of c (the last one holds its whole replay back) and dropped by yk_set_image. */
int yk_order_fused_after(yk_ctx* c, const yk_ctx* other);

/* gradient results (valid after yk_encode_tiles) -------------------------------------------------
 * swizzled 1-bit tile bitmap of pass p, byte-exact `pFillBitMap` (:3775-3777, bit rule :3801-3805,:4026;
 * size = HeaderGradientTile::getBitmapSwizzleSize/8, include/YAIK_private.h:278-286) */
size_t yk_gradient_bitmap_bytes(const yk_ctx* c, int pass);
int    yk_gradient_bitmap(yk_ctx* c, int pass, uint8_t* hostOut, size_t cap);
const uint8_t* yk_gradient_bitmap_device(const yk_ctx* c, int pass);
/* accepted-tile count per pass = FittingQuadSmooth's return value (TileDone, :4362). Synchronises. */
int    yk_gradient_counts(yk_ctx* c, int32_t counts[YK_NUM_PASSES]);
/* coverage after the 7 passes: 1 bit per 4x4 cell, u16 per 16x16 macro-tile (bit = cellY*4+cellX), row-major
 * macro-tiles.  Equals smoothMap/mapSmoothTile != 0 sampled per cell (:4029-4037). */
int    yk_coverage(yk_ctx* c, uint16_t* hostOut, size_t capElems);
/* corner-colour stream of pass p = `rgbStream` (:4113-4132): CompressF(Round6(corner),250) bytes of every corner
 * not yet in `mappedRGB`, in scan order, de-duplicated across passes.  Call for p = 0..6 in order. */
int    yk_gradient_corners(yk_ctx* c, int pass, uint8_t* hostOut, size_t cap, size_t* nBytes);
/* pass's corner stream where it lies in HBM (valid until the handle's next encode) and its length; builds the streams on first use */
int yk_gradient_corners_device(yk_ctx* c, int pass, const uint8_t** dev, size_t* nBytes);
/* (re)builds the seven corner streams on the device without copying anything out (yk_gradient_corners does it on first use) */
int    yk_gradient_corners_run(yk_ctx* c);
/* Row stripes (new; SURVEY §8e "corner dedup across stripe-boundary lattice rows ... on the root"): a stripe handle
 * de-duplicates inside its own rows, but its first and last lattice rows (y = y0 and y = y0 + h) are shared with the
 * neighbouring stripes.  For those two rows, n = w/4 + 1 points each (first row, then last row): keys[i] = the stripe-local
 * first-toucher key pass << 27 | bitIndex << 2 | corner (0xFFFFFFFF = untouched), index[i] = position, in corners, of that
 * point's colour inside the stripe's stream of that pass.  The root drops the later of two emissions of one point:
 * yaik_amd/distributed.py::merge_corner_streams.  capElems >= 2 * (w/4 + 1). */
int    yk_gradient_corner_edges(yk_ctx* c, uint32_t* hostKeys, uint32_t* hostIndex, size_t capElems);

/* ---- a6 with nullable planes: EncoderContext::FittingQuadSmooth(rejectFactor, srcA, srcB, srcC, ..., tileShiftX, tileShiftY) where one or
 * two of the planes are NULL (EncoderContext.cpp:3710-4363; PlaneBit :3715; the reference's call sites are the six 4x4 passes RB, RG, GB, R,
 * G, B of Convert(), :9261-9415, all compiled out or under `if (0)`).  planeBit: bit0/1/2 = srcA/srcB/srcC present (7 = a plain RGB pass).
 * Runs ONE more pass after yk_encode_tiles, on the state the seven RGB passes left (further calls continue from each other):
 *   - a tile is tried when its top-left pixel is uncovered in every PRESENT plane (:3871-3875); absent planes read 0 and never reject;
 *   - accepted tiles paint the per-plane coverage of the present planes and the common coverage (smoothMap; :4029-4037), so yk_coverage
 *     grows and yk_coverage_plane(p) tells what plane p still has to code in the 1-D path - yk_range1d_encode uses the per-plane
 *     coverage from the first partial pass on, exactly like DynamicTileCompressor(.., mapSmoothTile->GetPlane(p), ..) (:9451-9460);
 *   - the corner stream holds one byte per PRESENT plane whose mappedRGB[p] has not seen the lattice point (:4001-4021, :4113-4132).
 * The 2-D tile maps of yk_encode_tiles are not touched (the reference's partial passes precede only the 1-D compressor).
 * Single images only (nFrames == 1, whole image: y0 == 0).  *tilesAccepted = the function's return value (TileDone).  Synchronises. */
int    yk_gradient_partial_pass(yk_ctx* c, int rejectFactor, int planeBit, int tileShiftX, int tileShiftY, int* tilesAccepted);
/* testOutput of FittingQuadSmooth (:3960-3971, :4096-4104): the tiles pass `pass` accepted (0..6 = the RGB passes, 7 = the last plane-subset
 * pass) write blendC6Exp - the rounded bilinear blend of their Round6P corners - into three int32 preview planes the handle keeps per
 * encode (INT32_MIN where no tile wrote yet).  Calls accumulate; hostOut (may be NULL) receives the three planes, w*h each.  A debugging
 * aid of the encoder, not what the decoder reconstructs.  Single whole images. */
int    yk_gradient_preview(yk_ctx* c, int pass, int32_t* hostOut, size_t capElems);
/* bitmap (swizzled like yk_gradient_bitmap, size :3770-3777) and corner stream of the LAST partial pass */
int    yk_partial_bitmap(yk_ctx* c, uint8_t* hostOut, size_t cap, size_t* nBytes);
int    yk_partial_corners(yk_ctx* c, uint8_t* hostOut, size_t cap, size_t* nBytes);
/* mapSmoothTile->GetPlane(plane) != 0 per 4x4 cell, same layout as yk_coverage (equal to it until the first partial pass) */
int    yk_coverage_plane(yk_ctx* c, int plane, uint16_t* hostOut, size_t capElems);

/* ---- (f)4  3-D LUT tiles: EncoderContext::Load3DPattern (EncoderContext.cpp:7851), EvalCtx3D::Set3DPointCloud (:4744),
 * StartCorrelationSearch (:7316), Correlation3DSearch (:6245) with computeValues3D (:5807).  Runs where Convert() runs it (:9117-9218):
 * after the gradient passes, before the 1-D compressor, whose per-plane maps it shrinks (a matched tile covers all three planes of
 * mapSmoothTile, not smoothMap: yk_coverage_plane grows, yk_coverage does not).
 * yk_lut_load_pattern: one pattern of the bank = the contents of one 'Bank3D' .lut file (u8 count, r[], g[], b[], 6-bit values), at most 64
 * points (more make the reference overrun its tables, :7907-7917) and 64 patterns; *index = its number.  The bank belongs to the handle
 * and survives yk_set_image (the first pattern reserves the whole bank's tables in HBM: 64 MB of nearest-entry tables + 0.3 MB).  yk_lut_start allocates and clears the streams; yk_lut_search runs ONE tile shape (shiftX, shiftY) in
 * {(4,3),(3,4),(3,3),(3,2),(2,3),(2,2)} - the reference calls them in that order - and appends to the streams; *matched = tiles taken.
 * yk_lut_stream(which): 0 = corr3D_tileStreamTileType (u16: orientation | pattern << 6 | bitMode << 14, :6559), 1 = corr3D_colorStream
 * (box lo RGB, hi RGB per tile, before EndCorrelationSearch's CompressF :7494), 2..5 = corr3D_stream3Bit..6Bit (entry numbers, before the
 * x 3 of :7526), 6..11 = the tile maps of 16x8, 8x16, 8x8, 8x4, 4x8, 4x4 (BitmapSwizzleMapSize bytes, :7310).  Single whole images. */
int yk_lut_clear(yk_ctx* c);
int yk_lut_load_pattern(yk_ctx* c, const uint8_t* r, const uint8_t* g, const uint8_t* b, int count, int* index);
int yk_lut_pattern_tables(yk_ctx* c, int pattern, int16_t* factors, uint16_t* distanceField, uint8_t* positions);
int yk_lut_start(yk_ctx* c);
int yk_lut_search(yk_ctx* c, int tileShiftX, int tileShiftY, int* matched);
int yk_lut_stream(yk_ctx* c, int which, uint8_t* hostOut, size_t cap, size_t* nBytes);

/* range-quantiser results per plane (valid after yk_encode_tiles) ---------------------------------
 * tileDefs = `streamTileDef` u16 EncodeTileType(type,range,base) of tiles with >= 1 valid pixel, LeftRightOrder
 * (:4419,:4434-4438); nibbles = `streamTileIdx`, low nibble first (:1180-1184), closed to a whole byte (:4525). */
int yk_range_sizes(yk_ctx* c, int plane, size_t* nDefs, size_t* nNibbles);        /* synchronises */
int yk_range_streams(yk_ctx* c, int plane, uint16_t* hostDefs, size_t capDefs, uint8_t* hostNibbles, size_t capBytes);
const uint16_t* yk_range_defs_device(const yk_ctx* c, int plane);
const uint8_t*  yk_range_nibbles_device(const yk_ctx* c, int plane);
/* `dst` plane (int32 w*h of this stripe; untouched where no valid pixel; pre-filled with `fill`) */
int yk_range_dst(yk_ctx* c, int plane, int32_t* hostOut, size_t capElems);
int yk_set_dst_fill(yk_ctx* c, int32_t fill);

/* ---- a15  live 1-D range path:  3x EncoderContext::DynamicTileCompressor(stream, plane, mapSmoothTile[plane], debug)
 * (EncoderContext.cpp:8398-8522, call sites :9451-9465) on what the gradient passes left uncovered.  Produces the two
 * streams GenerateDynamicTileChunk hands to ZStd (:8524-8576): pixel bytes (planes R,G,B appended, 1 B per pixel) and the
 * per-tile parameter bytes color0,minCol,delta (`streamType`, :8503-8505).  colorCompression1D = 255, rangeCompression1D = 15. */
int yk_range1d_encode(yk_ctx* c);
/* enable != 0: from the next yk_encode_tiles on, the fused kernel also leaves the packed pixels of every 4x4 cell it did not cover (4 bytes per
 * pixel, only those cells) in a cache the 1-D path reads instead of the int32 planes: every input sample is then read from HBM once on the whole
 * path.  Costs the fused kernel four 16-byte stores per lane of an uncovered cell, so it is off unless a caller runs the 1-D path
 * (EncoderContext::ConvertHotPath turns it on).  The results of yk_range1d_encode are the same either way.  Not for batches. */
int yk_set_pixel_cache(yk_ctx* c, int enable);
int yk_range1d_streams(yk_ctx* c, uint8_t* hostPix, size_t capPix, size_t* nPix, uint8_t* hostType, size_t capType, size_t* nType);
/* the two streams where they lie in HBM (valid until the handle's next yk_range1d_encode / yk_set_image) and their lengths; synchronises once for the lengths */
int yk_range1d_streams_device(yk_ctx* c, const uint8_t** devPix, size_t* nPix, const uint8_t** devType, size_t* nType);
/* where plane p's share of the two streams ends (bytes, cumulative): the cursor DynamicTileCompressor returns after plane p (:8521) and
 * the end of its streamType entries.  Equal thirds unless a partial-plane pass gave the planes different coverage. */
int yk_range1d_plane_ends(yk_ctx* c, size_t pixEnd[3], size_t typeEnd[3]);

/* ---- tile-map export for the multi-GPU gather (new; the reference is single-process) -----------------------
 * Packs this handle's results into ONE caller-owned HBM buffer (device-to-device copies on the handle's stream) so
 * that a single RCCL gather can concatenate the per-stripe / per-frame tile maps.  Layout, every section padded to
 * 16 bytes: 7 gradient bitmaps | keep flags (1 byte per 16x16 tile, RGBA only) | per plane: tile defs (u16), nibbles.
 * sizes[0..6] bitmap bytes, sizes[7] keep bytes, sizes[8+2p] = nDefs(p), sizes[9+2p] = nNibbles(p), sizes[14] = total
 * bytes written.  One kernel packs all sections; the call returns after the stream has been synchronised, i.e. the buffer
 * is complete and may be handed to another runtime instance / RCCL.  cap >= yk_export_capacity.  The buffer is WRITTEN on the handle's
 * stream: work other streams still have queued on it (its fill, a previous consumer) must have finished or be ordered before that stream
 * (yk_stream_wait_for) -- the handle's stream is not ordered against any other. */
size_t yk_export_capacity(const yk_ctx* c);
int    yk_export_tile_maps(yk_ctx* c, void* devDst, size_t cap, uint64_t sizes[15]);
/* The same without a host synchronisation, for pipelines that keep the size table on the device: devMeta16 (device, 16 x u64)
 * receives {total payload bytes, sizes[0..14]}; work queued afterwards on `consumerStream` (same runtime instance, 0 = null
 * stream; e.g. the stream a RCCL collective is enqueued behind) sees the finished buffer and table (yk_stream_handoff). */
int    yk_export_tile_maps_async(yk_ctx* c, void* devDst, size_t cap, void* devMeta16, void* consumerStream);
/* The framed form the gather moves: devDst[0..127] = 16 x u64 header {payload bytes, sizes[0..14]}, the sections behind it (cap >= 128 +
 * yk_export_capacity).  A receiver needs nothing but the buffer: the size table travels inside it, and the length to transfer for a LATER
 * payload of the same rank is agreed from this header on both sides -- no second collective.  No host synchronisation; work queued
 * afterwards on consumerStream (0 = null stream, (void*)-1 = no hand-over: the gather then goes to the handle's own stream) sees the buffer. */
#define YK_EXPORT_HEADER_BYTES 128
int    yk_export_tile_maps_framed(yk_ctx* c, void* devDst, size_t cap, void* consumerStream);

/* ---- the multi-GPU gather of the tile maps (SURVEY 8(b) `yk_gather_maps`, 8(e); new: the reference is one process,
 * include/YAIK.h:42-47) ------------------------------------------------------------------------------------------------
 * Row stripes / frames are independent given their pixels; the only exchange is the concatenation of the per-rank tile maps on a root.
 * RCCL over xGMI, bound at run time (librccl.so.1); communicators are opaque pointers owned by the caller.  A gather is ONE grouped launch
 * of point-to-point transfers (every sender uses its own direct link into the root) on the handles' streams, behind the kernels that
 * produced the payloads: nothing is synchronised, the host never waits for the frame it just queued.
 *   one process per GPU:  id on rank 0 (yk_comm_unique_id), passed to the others by the launcher's own means, yk_comm_init_rank on
 *                         every rank, then yk_gather_maps per image / frame;
 *   one process, n GPUs:  yk_comm_init_all over n handles (one per device), then yk_gather_maps_all. */
/* HBM scratch for hosts that do not link the HIP runtime themselves (the C++ mirror is plain g++): buffers on the handle's device;
 * yk_device_download copies to the host on the handle's stream and synchronises it; yk_device_upload copies from the host (pageable or pinned)
 * on the handle's stream and returns when `host` may be reused; yk_device_copy queues a device-to-device copy on the
 * handle's stream and does not synchronise (both buffers on the handle's device; e.g. an encoder's per-handle streams into a buffer that
 * outlives its next yk_select_frame). */
int  yk_device_alloc(yk_ctx* c, size_t bytes, void** dev);
void yk_device_free(yk_ctx* c, void* dev);
int  yk_device_download(yk_ctx* c, void* host, const void* dev, size_t bytes);
int  yk_device_upload(yk_ctx* c, void* dev, const void* host, size_t bytes);
int  yk_device_copy(yk_ctx* c, void* devDst, const void* devSrc, size_t bytes);
/* yk_device_copy for a list of segments (new): nSeg (1..262144) pieces of device memory into ONE buffer, so that what a batch left in several
 * handle buffers crosses to the host with one download.  Segment i lands at devDst + offsets[i]: offsets[0] = 0, offsets[i + 1] = offsets[i] +
 * nBytes[i] rounded up to 16, *total = the end of the last segment rounded up to 16.  devDst == NULL is a size query (offsets and *total only; devSrc
 * is then not looked at and may be NULL).  One kernel launch on the handle's stream and one table upload (through the pinned ring of the batch tables), no host
 * synchronisation.  The grid follows the bytes moved: a workgroup of 256 lanes copies one 4 KB piece of one segment, 16 bytes per lane, and finds its
 * segment by a binary search over the per-segment piece counts.  A source may have any alignment (sources that are not 16-byte aligned are read
 * through byte pointers); devDst must be a multiple of 16.  Only the segments' own bytes are written: the gaps between them and everything from
 * *total on keep their contents.  A segment of length 0 is skipped and its pointer may be NULL.  ORDERING against the sources' producers is the
 * caller's, as for the yk_decode_*_device entry points: they are read on this handle's stream.
 * Refusals launch nothing and write nothing: YK_ERR_BAD_ARG for a NULL nBytes / offsets / total (or devSrc with a destination), nSeg outside
 * 1..262144, a length with a NULL source, a devDst that is not a multiple of 16, 2^31 or more 4 KB pieces in one call; YK_ERR_RANGE for cap < *total
 * (offsets and *total are filled in). */
int  yk_device_gather(yk_ctx* c, const void* const* devSrc, const size_t* nBytes, int nSeg, void* devDst, size_t cap, size_t* offsets /* nSeg, out */, size_t* total);
int  yk_comm_available(void);                                           /* 1 when RCCL could be loaded */
int  yk_comm_unique_id(void* id128);                                    /* 128 bytes (ncclUniqueId) */
int  yk_comm_init_rank(yk_ctx* c, const void* id128, int nRanks, int rank, void** comm);
int  yk_comm_init_all(yk_ctx* const* ctxs, int n, void** comms);        /* comms[n] out */
int  yk_comm_ranks(void* comm, int* nRanks, int* rank);                 /* what RCCL reports for the communicator */
void yk_comm_destroy(void* comm);
/* Rank side (one process per GPU): every rank but `root` sends sendBytes from devSend; the root receives recvBytes[r] bytes of rank r at
 * devRecv + recvOffsets[r] (its own payload is copied there on the device; recvBytes / recvOffsets / devRecv may be NULL elsewhere).
 * Sender and root must name the same count for a rank: derive it on both sides from that rank's previous header. */
/* COUNTS MUST AGREE: rank r's sendBytes has to equal recvBytes[r] as the root posts it.  The library cannot check this across ranks, and an
 * ncclSend / ncclRecv pair with different counts is undefined in RCCL (a hang or a truncated payload).  Callers either exchange the sizes first
 * or use a fixed capacity per rank with the true length inside the payload (the framed export's 128-byte header carries it; that is what
 * yaik_amd/distributed.py and EncoderContext::ConvertHotPathStripes do). */
int  yk_gather_maps(yk_ctx* c, void* comm, int root, const void* devSend, size_t sendBytes,
                    void* devRecv, const size_t* recvBytes, const size_t* recvOffsets);
/* One process driving n devices: rank r's sendBytes[r] bytes land at devRecv + recvOffsets[r] on the root's device. */
int  yk_gather_maps_all(yk_ctx* const* ctxs, void* const* comms, int n, int root, void* const* devSend, const size_t* sendBytes,
                        void* devRecv, const size_t* recvOffsets);

/* ---- decode side: the loops behind YAIK_DecodeImage's chunk switch (decoder/YAIK_API.cpp:731-1303) ----
 * Buffers mirror YAIK_Instance (include/YAIK_private.h:26-54): planeR/G/B u8 in 8x8 tiles, mapRGB lattice,
 * tile4x4Mask.  Width/height: the sizes the encoder accepts, multiples of 8 from 8 to 32760.  At sides of 8 (mod 16) the decode follows the
 * project's consistent reading, not the reference's mis-strided loops (YAIK_Gradient.cpp:15): tiles that reach past the right or bottom
 * edge are skipped and consume nothing.  Other sizes fail with YK_ERR_BAD_ARG. */
int yk_decode_begin(yk_ctx* c, int w, int h);
/* DecompressGradient16x16 .. 4x4 (decoder/YAIK_Gradient.cpp:28,203,401,599,800,999,1208), planeBit 7.
 * bitmap = swizzled tile bitmap, rgb = corner stream AFTER PaletteDecompressor (0..255). Host pointers. */
int yk_decode_gradient(yk_ctx* c, int tileShiftX, int tileShiftY, const uint8_t* bitmap, size_t bitmapBytes,
                       const uint8_t* rgb, size_t rgbBytes);
/* The same with both streams already in HBM on the handle's device (e.g. straight from an encoder handle: yk_gradient_bitmap_device,
 * yk_gradient_corners_device) and no host synchronisation.  remapRange > 0 applies PaletteFullRangeRemapping(range) to the colour stream on
 * the way in (decoder/YAIK_GenericFunctions.cpp:128-137; the encoder's streams are CompressF(.., 250) values), 0 takes it as it is. */
/* ORDERING is the caller's: the yk_decode_*_device entry points read the given device memory on THIS handle's stream and nothing orders that
 * stream behind the producer's.  When the streams come from an encoder handle (yk_gradient_corners_device, yk_range1d_streams_device,
 * yk_gradient_bitmap_device), order the two first: yk_synchronize(producer) on the host, or a device-side wait (yk_stream_handoff(producer,
 * consumerStream) / yk_stream_wait_for(c, producerStream) with the streams the caller gave the handles through yk_set_stream).  The pointers go
 * stale with the producer's next encode / yk_set_image. */
int yk_decode_gradient_device(yk_ctx* c, int tileShiftX, int tileShiftY, const uint8_t* devBitmap, size_t bitmapBytes,
                              const uint8_t* devRgb, size_t rgbBytes, int remapRange);
/* All 'GTIL' chunks of a file at once, streams in HBM: the same result as yk_decode_gradient_device for pass 0 .. nPasses-1 in that order
 * (first toucher of every lattice point over ALL passes in one launch, one scan, one launch popping the colours, then ONE render launch
 * in which a workgroup owns a 64x64 block of the image and walks the passes in call order: one clear and 5 launches for seven passes
 * instead of 35 launches + 21 copies / clears).  Up to seven passes per call and 2^25 tile slots per pass; beyond that the call runs the
 * passes one after the other. */
int yk_decode_gradient_all_device(yk_ctx* c, int nPasses, const int* tileShiftX, const int* tileShiftY, const uint8_t* const* devBitmap,
                                  const size_t* bitmapBytes, const uint8_t* const* devRgb, const size_t* rgbBytes, int remapRange);
/* DecompressGradient4x4 with a plane subset (decoder/YAIK_Gradient.cpp:1208-1226 -> 4x4R / G / RG / B / RB / GB, :1420-2732): planeBit
 * 1..6 (bit 0 = R, 1 = G, 2 = B; 7 forwards to yk_decode_gradient).  Like YAIK_API.cpp:875-877 the masks are split per plane first
 * (UpdateTileAndRGBMask).  Only the 4x4 size has partial-plane loops in the reference.  consistentMarks = 0 reproduces what those loops
 * do to tile4x4Mask, defects included (the R / G / B loops never mark; GB / RB put the B marks at tile4x4Mask + (size >> 1), :1678,
 * :1924) -- byte-identical state to the reference decoder; 1 marks every present plane's own mask, which is what the ENCODER's
 * per-plane coverage and therefore the 1-D streams behind such passes assume (with 0 the reference's own Decompress1D runs off them). */
int yk_decode_gradient_planes(yk_ctx* c, int planeBit, int consistentMarks, const uint8_t* bitmap, size_t bitmapBytes,
                              const uint8_t* rgb, size_t rgbBytes);
/* UpdateTileAndRGBMask alone (decoder/YAIK_API.cpp:530-544): what a plane-subset chunk of any OTHER tile shape still does before its
 * decoder returns without work (YAIK_Gradient.cpp:29-36).  Idempotent. */
int yk_decode_split_masks(yk_ctx* c);
/* ---- (f)4 decode: YAIK_AssignLUT (decoder/YAIK_API.cpp:133-415) and the '3DTL' chunk, Tile3D_16x8 .. Tile3D_4x4 (decoder/YAIK_3DTile.cpp:244-2140,
 * chunk reader YAIK_API.cpp:1002-1270).  yk_decode_assign_lut takes the decoder's LUT file ('LUL0': LUTHeader + per depth 3..6 and pattern the
 * x, y, z entry lists) and lays out the 48 orientation tables per pattern and depth in HBM; it belongs to the handle until replaced.
 * yk_decode_lut3d runs the six tile shapes in chunk order on host streams: maps[k] / mapBytes[k] (16x8, 8x16, 8x8, 8x4, 4x8, 4x4; NULL or 0 =
 * absent), tiles (u16 per tile), colors (6 bytes per tile AFTER PaletteFullRangeRemapping), idx[f] / idxBytes[f] = the 3 / 4 / 5 / 6 bit index
 * streams as stored (entry number x 3).  Pixels of 4x4 cells tile4x4Mask already marks are skipped (and consume no index), every cell of a
 * decoded tile is marked afterwards.  consumed[6] = bytes used of tiles, colors and the four index streams.  Must come before '1DTL' /
 * plane-subset chunks (single-plane masks), like in the file. */
int yk_decode_assign_lut(yk_ctx* c, const uint8_t* lutFile, size_t lutBytes);
int yk_decode_lut3d(yk_ctx* c, const uint8_t* const maps[6], const size_t mapBytes[6], const uint16_t* tiles, size_t nTiles, const uint8_t* colors,
                    const uint8_t* const idx[4], const size_t idxBytes[4], size_t consumed[6]);
/* Decompress1D x3 planes (decoder/YAIK_3DTile.cpp:24-240) on the '1DTL' streams (type: 3 B/tile, pix: 1 B/pixel) */
int yk_decode_1d(yk_ctx* c, const uint8_t* typeStream, size_t typeBytes, const uint8_t* pixStream, size_t pixBytes,
                 int compressionRange);
/* streams already in HBM (yk_range1d_streams_device of an encoder handle on the same device), no host synchronisation */
int yk_decode_1d_device(yk_ctx* c, const uint8_t* devType, size_t typeBytes, const uint8_t* devPix, size_t pixBytes, int compressionRange);
/* Decompress1BitTiled (decoder/YAIK_Mipmap.cpp:23-154): 1 bit / 16x16 tile -> swizzled 1 bit / pixel mask */
int yk_decode_mask(yk_ctx* c, const uint8_t* bits, int tileBBoxW, int tileBBoxH, uint8_t* hostOut, size_t cap);
/* 8x8-tiled u8 planes exactly as YAIK_SCustomDataSource hands them to imageBuilderFunc (include/YAIK.h:205-224).  Under a decode window
 * (yk_decode_set_window, below) the planes are exact inside the window and unspecified outside it; yk_decode_tile4x4[_planes] stay whole-image
 * and exact. */
int yk_decode_planes(yk_ctx* c, uint8_t* hostR, uint8_t* hostG, uint8_t* hostB, size_t capEach);
const uint8_t* yk_decode_planes_device(yk_ctx* c, size_t* planeSize);
/* internal_imageBuilderFunc (decoder/YAIK_DefaultCallback.cpp:24-191): de-tile into interleaved rows at outputImageStride.
 * Only the pixel bytes of a row are written; the rest of each outputImageStride-sized row is left untouched, like the reference
 * (include/YAIK.h:190: the stride places the image inside a larger user buffer).
 * hostAlpha == NULL -> RGB, 3 B/pixel, byte-identical to the reference (pinned by the compiled reference: tests/golden, blob dec_rgb_out).
 * With a linear 8-bit alpha plane (strideA bytes per row) yk_decode_output writes RGBA 4 B/pixel as include/YAIK.h documents.
 * The reference's own RGBA branch does something else (:45-62: the alpha store never advances dst and the alpha row cursors are
 * not moved per tile row): rows of w RGB triples + one alpha byte.  yk_decode_output_reference_rgba reproduces exactly that
 * (blob dec_rgba_out) for callers that need byte identity with the reference's output rather than a usable RGBA image. */
int yk_decode_output(yk_ctx* c, uint8_t* hostOut, size_t outputImageStride, const uint8_t* hostAlpha, int strideA);
int yk_decode_output_reference_rgba(yk_ctx* c, uint8_t* hostOut, size_t outputImageStride, const uint8_t* hostAlpha, int strideA);
int yk_decode_tile4x4(yk_ctx* c, uint8_t* hostOut, size_t cap);
/* 'ALPM' alpha values (chunk reader decoder/YAIK_API.cpp:750-833, unpackers decoder/YAIK_Alpha.cpp): the full w x h 8-bit alpha plane of the
 * image begun by yk_decode_begin is written in HBM from the DECOMPRESSED payload (0 outside the box) and stays there for
 * yk_decode_output_alpha.  mode = AlphaHeader::parameters & 7: 1 = 1 bit (0 / 255; box width a multiple of 8), 4 / 5 = 6 bit (/ inverted;
 * width a multiple of 4), 6 = 8 bit, 2 / 3 = 6 bit (/ inverted) of the pixels the mipmap mask selects.  For 2 / 3, mask = the decoded
 * 'MIPM' mask exactly as yk_decode_mask returns it and maskBBox = its box in pixels (tile box << 4); like the reference it is read linearly
 * with stride maskBBox[2] from the alpha box's origin, and bits outside the buffer read 0.  bbox = {x, y, w, h} in pixels.
 * refQuirk = 1 reproduces the reference's 1-bit row loop byte for byte (`while (--cnt)`, YAIK_Alpha.cpp:76: w/8 - 1 bytes per row, each row
 * landing 8 pixels left of the previous one, the rest 0); 0 decodes what the encoder writes (w/8 bytes per row).
 * Errors: YK_ERR_BAD_ARG for a box outside the image or empty, mode 0 or 7, a misaligned width; YK_ERR_RANGE for a payload shorter than the
 * box (or the mask selection) needs.  Nothing is read or written out of bounds.  The mask modes synchronise once (the selected count). */
int yk_decode_alpha(yk_ctx* c, int mode, const int32_t bbox[4], const uint8_t* payload, size_t n, const uint8_t* mask, size_t maskBytes,
                    const int32_t maskBBox[4], int refQuirk);
int yk_decode_alpha_plane(yk_ctx* c, uint8_t* hostOut, size_t cap);                       /* the plane back to the host (tests, custom builders) */
/* yk_decode_output with the plane of yk_decode_alpha as alpha: RGBA 4 B/pixel; the alpha plane never leaves HBM */
int yk_decode_output_alpha(yk_ctx* c, uint8_t* hostOut, size_t outputImageStride);
/* The default builder's de-tile into DEVICE memory (on this handle's device): 8-bit pixels of the image begun by yk_decode_begin at any base
 * address and pitch, written by the kernel of yk_decode_output with no host copy and no host synchronisation.
 *   planeBytes == 0: HWC, pixel (x, y) channel k at devOut[y * rowBytes + x * channels + k] (the RGB888 / RGBA8888 rows of yk_decode_output);
 *   planeBytes >  0: CHW, at devOut[k * planeBytes + y * rowBytes + x] (the [C, H, W] layout of torch image tensors).
 * channels = 3 (RGB) or 4 (RGBA).  With 4, alpha = -1 takes the plane yk_decode_alpha left in HBM, 0..255 that constant (opaque RGBA from an
 * RGB file: 255); alpha is ignored with 3.  Only pixel bytes are written: row padding and the bytes between planes are never touched.
 * Refusals write nothing: YK_ERR_BAD_ARG for a NULL devOut, channels other than 3 / 4, rowBytes < w * channels (HWC) or rowBytes < w /
 * planeBytes < rowBytes * h (CHW), alpha outside -1..255 with channels 4; YK_ERR_STATE before yk_decode_begin, or alpha = -1 with no
 * decoded 'ALPM' plane.  ORDERING is the caller's, as for the yk_decode_*_device entry points: devOut is written on THIS handle's stream.
 * Order earlier work on devOut first (yk_stream_wait_for(c, producerStream)) and the consumer after the call (yk_stream_handoff(c,
 * consumerStream) or yk_synchronize).  Timed as YK_STAGE_DEC_DETILE. */
int yk_decode_output_device(yk_ctx* c, uint8_t* devOut, size_t rowBytes, size_t planeBytes, int channels, int alpha);
/* the three planes of tile4x4Mask back to back (planes 1 and 2 are meaningful once a partial-plane pass has split the masks) */
int yk_decode_tile4x4_planes(yk_ctx* c, uint8_t* hostOut, size_t cap);

/* ---- decode windows: only the tiles a rectangle of the image needs ----
 * yk_decode_set_window: with a window W = (x0, y0, ww, wh) set on the handle, the decode calls leave in the handle's planes, for every pixel
 * inside W, exactly what the whole-image decode leaves there; outside W the planes hold whatever they held.  Any stage may ignore the window and
 * write more, none writes less: the all-planes gradient passes (either path) render only the 64x64 blocks W touches and still mark every tile in
 * tile4x4Mask, the shared-mask 1-D chunk counts and scans the whole image (stream offsets are global prefix sums) and decodes only W's tiles; in
 * that flow no byte of the planes outside W rounded out to multiples of 64 (clipped to the image) is written.  '3DTL' and plane-subset chunks, and
 * the 1-D chunk behind a plane-subset chunk, write the whole image as before.
 * Valid after yk_decode_begin and before any chunk of that image is decoded (gradient, plane-subset, mask split, '3DTL', 1-D); otherwise, and on a
 * handle begun with yk_decode_begin_batch, YK_ERR_STATE.  x0, y0, ww, wh: multiples of 8, ww, wh >= 8, the rectangle inside the image; otherwise
 * YK_ERR_BAD_ARG.  ww == wh == 0 clears the window; yk_decode_begin always clears it.
 * While a window is set, the calls that need the whole image return YK_ERR_STATE with a message that names the window: yk_decode_output,
 * yk_decode_output_alpha, yk_decode_output_reference_rgba, yk_decode_output_device and yk_decode_compare_*.  yk_decode_planes[_device] and
 * yk_decode_tile4x4[_planes] stay allowed: the planes are exact inside W (unspecified outside), the marks are whole-image and exact.
 * yk_decode_alpha is not affected: the 'ALPM' plane stays whole.
 * yk_decode_output_window_device: yk_decode_output_device for the window: tile (x0 / 8 + jx, y0 / 8 + jy) of the planes goes to pixel (8 jx, 8 jy)
 * of a ww x wh destination with the layout rules of yk_decode_output_device (HWC or CHW, any pitch, only pixel bytes written; the pitch checks
 * are made against ww x wh).  alpha = -1 reads the decoded 'ALPM' plane at the window's offset.  With no window set it is
 * yk_decode_output_device.  Timed as one YK_STAGE_DEC_DETILE interval. */
int yk_decode_set_window(yk_ctx* c, int x0, int y0, int ww, int wh);
int yk_decode_output_window_device(yk_ctx* c, uint8_t* devOut, size_t rowBytes, size_t planeBytes, int channels, int alpha);

/* ---- many windows of one image: prepare once, render 64x64 blocks on demand ----
 * A viewer fetching tiles, a texture pager or a trainer taking crops asks for many windows of the same image.  yk_decode_prepare_device does the
 * map-sized work of the image once -- the corner lattice (mapRGB), the marks of every tile in tile4x4Mask, the per-tile offsets into the 1-D
 * streams -- and writes no byte of the planes.  yk_decode_render_windows_device then writes K windows of one size: it renders the 64x64 blocks
 * its windows touch that no earlier call rendered (gradient tiles, 1-D tiles, zeros in unmarked cells where the image has no 1-D chunk), each
 * block at most once per prepared image, and de-tiles the K windows.  Every window is, byte for byte, the crop of the whole-image decode.
 * yk_decode_prepare_device: the gradient arguments of yk_decode_gradient_all_device and the 1-D arguments of yk_decode_1d_device, all in device
 * memory; an image without a 1-D chunk passes typeBytes == pixBytes == 0 (devType, devPix and compressionRange are then not looked at).  Valid
 * right after yk_decode_begin: not on a batch, not under a window, before any gradient, plane-subset, mask-split, '3DTL' or 1-D call of the image
 * and not twice; otherwise YK_ERR_STATE.  yk_decode_alpha and yk_decode_mask are free to come before or after.  At most 7 passes, every pass below
 * 2^25 tile slots, colour streams below 4 GB: anything larger is YK_ERR_BAD_ARG (decode such an image window by window, yk_decode_set_window).
 * Every argument is checked before the first launch and a refusal leaves the handle usable.  The handle's buffers are grown before the first
 * launch too: an allocation that fails (YK_ERR_HIP) leaves the image as yk_decode_begin left it.  A HIP error after the first launch leaves the
 * image neither fresh nor prepared: yk_decode_begin again.  A yk_decode_begin that fails for device memory ends the prepared image with the
 * decode buffers it releases: the render calls then return YK_ERR_STATE.  The tile bitmaps and the 1-D streams are copied
 * into buffers of the handle and the colour streams are consumed, so once the call's work has completed on the handle's stream the caller may
 * free or overwrite every input.  Timed as one YK_STAGE_DEC_GRADIENT interval and, with 1-D streams, one YK_STAGE_DEC_1D interval.
 * yk_decode_render_windows_device: nWindows (1..1024) windows of ww x wh with origins xy[2k], xy[2k + 1] (host memory), each under the rule of
 * yk_decode_set_window; window k goes to devOut + k * windowBytes with the layout, pitch, channels and alpha rules of
 * yk_decode_output_window_device (alpha = -1 reads the decoded 'ALPM' plane at each window's offset); windowBytes is checked like frameBytes of
 * yk_decode_output_batch_device.  Before prepare: YK_ERR_STATE.  Bad arguments: YK_ERR_BAD_ARG before anything is queued, with the rendered
 * blocks and the planes untouched.  A call that finds a block to render queues one YK_STAGE_DEC_GRADIENT interval (the render over the sorted
 * list of new blocks; for an image without a 1-D chunk also the zeroing of their unmarked cells), one YK_STAGE_DEC_1D interval when the image
 * has 1-D streams, and one YK_STAGE_DEC_DETILE interval; a call whose blocks are all rendered queues the de-tile alone.
 * yk_decode_prepared_blocks: how many 64x64 blocks are rendered and how many the image has ((w + 63) / 64 x (h + 63) / 64); either pointer may be
 * NULL.  Before prepare: YK_ERR_STATE.
 * While an image is prepared, until the next yk_decode_begin[_batch]: the chunk calls above, yk_decode_set_window, yk_decode_output_window_device
 * and the whole-image calls (yk_decode_output*, yk_decode_compare_*) return YK_ERR_STATE with a message that names
 * yk_decode_render_windows_device.  yk_decode_planes[_device] stay: exact inside rendered blocks, untouched outside them;
 * yk_decode_tile4x4[_planes] stay: whole and exact, no render changes them. */
int yk_decode_prepare_device(yk_ctx* c, int nPasses, const int* tileShiftX, const int* tileShiftY,
                             const uint8_t* const* devBitmap, const size_t* bitmapBytes, const uint8_t* const* devRgb, const size_t* rgbBytes, int remapRange,
                             const uint8_t* devType, size_t typeBytes, const uint8_t* devPix, size_t pixBytes, int compressionRange);
int yk_decode_render_windows_device(yk_ctx* c, int nWindows, const int* xy, int ww, int wh,
                                    uint8_t* devOut, size_t rowBytes, size_t planeBytes, size_t windowBytes, int channels, int alpha);
int yk_decode_prepared_blocks(yk_ctx* c, int* rendered, int* total);

/* ---- outputs at reduced resolution: 1/2, 1/4 and 1/8 size ----
 * level = 0..3, s = 1 << level.  Where the full-size call writes dec[y][x][k] of a w x h image or window, the scaled call writes
 * (w >> level) x (h >> level) pixels
 *     out[Y][X][k] = (sum over dy, dx < s of dec[s Y + dy][s X + dx][k]  +  s s / 2) >> (2 level):
 * the box mean, halves rounded up, computed from the level-0 bytes in integers (not from the rounded means of the level before).  Alpha is
 * averaged like a colour channel, without premultiplication: alpha = -1 averages the decoded plane, a constant stays that constant.  Sides and
 * windows are multiples of 8, so every level divides exactly and the reduced window is the crop of the reduced image.  The reduction runs in the
 * de-tile kernel on the lanes that hold a tile's bytes: the planes are read once and only the reduced pixels are written; the planes are not
 * changed.  level = 0 forwards to the full-size call.  Layout rules are those of the full-size calls (HWC with planeBytes == 0, CHW otherwise, any
 * base and pitch, only pixel bytes written); every pitch, plane, frame and window check is made against the REDUCED width and height.  A level
 * outside 0..3 is YK_ERR_BAD_ARG; the further refusals are those of the full-size calls; every refusal comes before the first launch and writes
 * nothing.  No host synchronisation: ordering is the caller's, as for yk_decode_output_device.  Each call is one YK_STAGE_DEC_DETILE interval.
 * yk_decode_output_scaled_device: the image begun, or the selected frame of a batch; with a window set (yk_decode_set_window) the reduced window,
 * under the state rules of yk_decode_output_window_device.  Unmarked cells are settled first.  On a prepared image: YK_ERR_STATE, with a message
 * that names yk_decode_render_windows_scaled_device.
 * yk_decode_output_scaled_batch_device: every frame of a decode batch in one launch, frame f at devOut + f * frameBytes; alpha = -1 reads the
 * planes of yk_decode_alpha[_mask]_batch_device (YK_ERR_STATE when the batch has none), 0..255 is a constant.
 * yk_decode_render_windows_scaled_device: yk_decode_render_windows_device with reduced crops.  xy, ww and wh are full-resolution pixels under the
 * rule of yk_decode_set_window; the blocks the windows touch are rendered at full size, each at most once per prepared image -- the bitmap of
 * rendered blocks is the one of the full-size call, so the two may be mixed freely -- and the gradient and 1-D intervals are recorded as there;
 * window k goes to devOut + k * windowBytes at (ww >> level) x (wh >> level). */
int yk_decode_output_scaled_device(yk_ctx* c, int level, uint8_t* devOut, size_t rowBytes, size_t planeBytes, int channels, int alpha);
int yk_decode_output_scaled_batch_device(yk_ctx* c, int level, uint8_t* devOut, size_t rowBytes, size_t planeBytes, size_t frameBytes, int channels, int alpha);
int yk_decode_render_windows_scaled_device(yk_ctx* c, int level, int nWindows, const int* xy, int ww, int wh,
                                           uint8_t* devOut, size_t rowBytes, size_t planeBytes, size_t windowBytes, int channels, int alpha);

/* ---- a full mip chain in one call: every level down to the last, the planes read once ----
 * A w x h image has levels 0 .. top, top = floor(log2(min(w, h))) (yk_decode_mip_levels gives top + 1, at most YK_MIP_MAX_LEVELS).  Level k has
 * (w >> k) x (h >> k) pixels, s = 1 << k:
 *     out_k[Y][X][c] = (sum over dy, dx < s of dec[s Y + dy][s X + dx][c]  +  s s / 2) >> (2 k):
 * the box mean of the level-0 bytes in integers, halves rounded up, never the mean of another level's rounded means.  Levels 0..3 are byte for
 * byte what yk_decode_output_device and yk_decode_output_scaled_device write.  From level 4 on w and h need not divide by s: the w - s (w >> k)
 * rightmost columns and h - s (h >> k) bottom rows are in no box and are ignored (the floor convention of texture mip chains).  Levels where a
 * side would become 0 do not exist.  Alpha is averaged like a colour channel; a constant stays that constant.  Sums are exact at every size.
 * levels[i] (a host array, read at call time) is the destination of level firstLevel + i, laid out as in yk_decode_output_device: HWC with
 * planeBytes == 0, CHW otherwise, any base, any pitch that holds the level's row, only pixel bytes written; frameBytes is used by the batch call.
 * Any contiguous run may be asked for: firstLevel = 0 is the whole chain with the full-size pixels, firstLevel = 5, nLevels = 1 one 1/32
 * thumbnail.  All levels of a call share `channels` and the HWC / CHW form (mixing them: YK_ERR_BAD_ARG).  alpha as in the scaled calls: -1 the
 * decoded 'ALPM' plane (batch call: the planes of yk_decode_alpha[_mask]_batch_device, YK_ERR_STATE when there are none), 0..255 a constant.
 * yk_decode_output_mipchain_device: the image begun, or the selected frame of a batch; unmarked cells are settled first.  With a window set, or on
 * a prepared image: YK_ERR_STATE (windows have no chain).  yk_decode_output_mipchain_batch_device: every frame, frame f of a level at
 * devOut + f * frameBytes.  Every check (level range, NULL pointers, pitches, channels, state) is made against the level's own size, every
 * refusal comes before the first launch and writes nothing, and the handle stays usable.  At most two launches however many levels and frames:
 * one kernel reads the planes once and writes levels 0..6 and a sum per 64x64 block, a small second one makes the levels from 7 up of those sums
 * (it runs only when such a level is asked for).  No host synchronisation (the handle's scratch may grow on the first call of a size); one
 * YK_STAGE_DEC_DETILE interval per call.  The planes are not changed.  Level buffers that overlap are the caller's error and are not detected. */
#define YK_MIP_MAX_LEVELS 15
typedef struct { uint8_t* devOut; size_t rowBytes, planeBytes, frameBytes; } yk_mip_level;
int yk_decode_mip_levels(int w, int h);                         /* top + 1, or YK_ERR_BAD_ARG for sides the decoder does not take */
int yk_decode_output_mipchain_device(yk_ctx* c, int firstLevel, int nLevels, const yk_mip_level* levels, int channels, int alpha);
int yk_decode_output_mipchain_batch_device(yk_ctx* c, int firstLevel, int nLevels, const yk_mip_level* levels, int channels, int alpha);

/* ---- decode batches: nFrames images of ONE shape on a handle, every kernel launched once over nFrames x blocks ----
 * A frame of 2048 x 2048 or less is a fraction of the grids the decode kernels were tuned on, and one image costs about a dozen dependent stream
 * operations; a batch costs the same dozen.  yk_decode_begin_batch allocates the 8x8-tiled planes, the mapRGB lattice, its `loaded` flags, the
 * lattice owners and tile4x4Mask nFrames (1..1024) times back to back (frame f at base + f * stride, like the encoder's batches) and clears what a
 * new image needs cleared, for all frames at once.  Buffers are kept while shape and frame count stay the same.  Size rules: yk_decode_begin,
 * which is a batch of one.  An allocation that does not fit returns YK_ERR_HIP with every decode buffer released; the next begin starts afresh.
 *
 * yk_decode_select_frame (default 0) points the single-image entry points at one frame of the batch: yk_decode_gradient[_device],
 * yk_decode_gradient_all_device, yk_decode_1d[_device], yk_decode_planes[_device], yk_decode_tile4x4[_planes], yk_decode_output and
 * yk_decode_output_device then read and write that frame only, so a caller can mix both forms and cross-check them.  (yk_decode_planes and the
 * output calls first zero what no chunk has written yet, in every frame.)  'MIPM', '3DTL', plane-subset chunks and the single-image 'ALPM' call are
 * not batched ('ALPM' has a batch call of its own below): with
 * nFrames > 1, yk_decode_alpha, yk_decode_output_alpha, yk_decode_output_reference_rgba, yk_decode_gradient_planes, yk_decode_split_masks,
 * yk_decode_lut3d and yk_decode_mask return YK_ERR_STATE and touch nothing.
 *
 * yk_decode_gradient_all_batch_device: yk_decode_gradient_all_device for every frame.  The pass list (nPasses <= 7, tile shapes, bitmapBytes[p]) is
 * the same for all frames; devBitmap / devRgb / rgbBytes hold nFrames * nPasses entries, frame-major (entry f * nPasses + p).  A pass without
 * tiles in some frame is an all-zero bitmap with rgbBytes 0 (devRgb may then be NULL).  The per-frame plans (pointers, lengths) are written once
 * per call into a table in HBM.  There is no pass-after-pass fallback: a pass of 2^25 tile slots or more is refused.
 * yk_decode_1d_batch_device: yk_decode_1d_device for every frame; four tables of nFrames entries.  A frame with empty streams (lengths 0, pointers
 * may be NULL) reads nothing; like a frame whose streams end early, the quadrants nothing marked are zero afterwards.  Pixel streams are read in
 * place and must be 16-byte aligned (the encoder's are).
 * yk_decode_output_batch_device: yk_decode_output_device for every frame, frame f at devOut + f * frameBytes; HWC when planeBytes == 0, CHW
 * otherwise; channels 3, or 4 with a constant alpha 0..255 (ignored with 3).  Only pixel bytes are written.
 *
 * Results per frame are bit-identical to decoding that frame alone.  None of the three calls synchronises with the host (the scratch buffer grows
 * on the first call of a shape, as in the single-image calls; a call waits for a table copy only when four earlier batch calls are still queued).
 * ORDERING is the caller's, exactly as for the yk_decode_*_device entry points above: streams are read and devOut is written on THIS handle's
 * stream.  Timed as one YK_STAGE_DEC_GRADIENT / YK_STAGE_DEC_1D / YK_STAGE_DEC_DETILE interval per call.
 * Every refusal writes nothing and leaves the handle usable: YK_ERR_BAD_ARG for nFrames outside 1..1024, a frame index out of range, a NULL table,
 * a NULL bitmap pointer, rgbBytes != 0 (or a 1-D length != 0) with a NULL pointer, a misaligned pixel stream, an unsupported tile shape,
 * nPasses > 7, a pass of >= 2^25 tile slots, a colour stream of 4 GB or more, compressionRange <= 0, the layout errors of yk_decode_output_device,
 * frameBytes < rowBytes * h (HWC) or < planeBytes * channels (CHW) with more than one frame, alpha outside 0..255 with 4 channels; YK_ERR_RANGE
 * for bitmapBytes[p] shorter than the shape needs; YK_ERR_STATE before any begin.  yk_last_error then holds the message of that refusal. */
int yk_decode_begin_batch(yk_ctx* c, int w, int h, int nFrames);
int yk_decode_select_frame(yk_ctx* c, int frame);
int yk_decode_gradient_all_batch_device(yk_ctx* c, int nPasses, const int* tileShiftX, const int* tileShiftY, const uint8_t* const* devBitmap,
                                        const size_t* bitmapBytes, const uint8_t* const* devRgb, const size_t* rgbBytes, int remapRange);
int yk_decode_1d_batch_device(yk_ctx* c, const uint8_t* const* devType, const size_t* typeBytes, const uint8_t* const* devPix,
                              const size_t* pixBytes, int compressionRange);
int yk_decode_output_batch_device(yk_ctx* c, uint8_t* devOut, size_t rowBytes, size_t planeBytes, size_t frameBytes, int channels, int alpha);
/* 'ALPM' in a batch.  yk_decode_alpha_batch_device writes the w x h alpha plane of EVERY frame of the batch begun by yk_decode_begin_batch in one
 * launch, frame f's at a stride of w * h rounded up to 16: modes[f] = 1, 4, 5 or 6 as in yk_decode_alpha (refQuirk = 0), bboxes[4 * f ..] = {x, y, w,
 * h}, devPayload[f] / payBytes[f] = the DECOMPRESSED payload in device memory, read in place; modes[f] = -1 (no chunk: all 255, empty box, no alpha
 * plane) gives a plane of the constant noChunkAlpha (0..255; 255 = opaque) and ignores the frame's other entries.  The records travel through the
 * pinned ring and an HBM table like those of the other batch calls: no host synchronisation, ORDERING is the caller's.  Everything is validated on
 * the host before the first launch; a refusal writes nothing and leaves earlier valid planes valid: YK_ERR_BAD_ARG for a NULL table, a box outside
 * the image or empty, a width not a multiple of 8 (mode 1) or 4 (modes 4, 5), modes 0 and 7, modes 2 and 3 (the mask modes are not batched), a NULL
 * payload with a length, noChunkAlpha outside 0..255; YK_ERR_RANGE for a payload shorter than its box needs; YK_ERR_STATE before any begin.
 * Afterwards yk_decode_alpha_plane returns the SELECTED frame's plane and yk_decode_output_device(alpha = -1) de-tiles the selected frame with it;
 * yk_decode_begin[_batch] invalidates the planes.
 * yk_decode_output_batch_alpha_device: yk_decode_output_batch_device with four channels and every frame's alpha taken from those planes (HWC when
 * planeBytes == 0, CHW otherwise; the same layout rules and refusals), YK_ERR_STATE when the batch has no valid alpha planes.  Timed as
 * YK_STAGE_DEC_DETILE. */
int yk_decode_alpha_batch_device(yk_ctx* c, const int32_t* modes /* nFrames */, const int32_t* bboxes /* nFrames x {x,y,w,h} */,
                                 const uint8_t* const* devPayload, const size_t* payBytes, int noChunkAlpha);
int yk_decode_output_batch_alpha_device(yk_ctx* c, uint8_t* devOut, size_t rowBytes, size_t planeBytes, size_t frameBytes);
/* The mask modes of 'ALPM' in a batch.  yk_decode_alpha_mask_batch_device does everything yk_decode_alpha_batch_device does (same planes, stride,
 * validity and refusals) and adds modes 2 and 3: frame f's plane is byte for byte what yk_decode_mask(bits, w, h) followed by yk_decode_alpha(mode,
 * bbox, payload, mask, maskBytes = w * h * 32, maskBBox = the tile box << 4, refQuirk 0) leaves for that frame.  devMipBits[f] / mipBytes[f] = the
 * 'MIPM' payload as the file holds it (1 bit per 16x16 tile, LSB first) in device memory, read in place: the mask is never expanded, the bit of a
 * mask position follows from the tile bitmap.  mipBoxes[4 * f ..] = the 'MIPM' box {x, y, w, h} in tiles; w == 0: the frame has no 'MIPM'.  At most
 * four launches whatever nFrames is (the unmasked one, then row count, per-frame scan and decode over the masked frames; those three are skipped
 * when no frame is masked), no host synchronisation.  Further refusals, all before the first launch: YK_ERR_BAD_ARG for a NULL mask table, mode 2
 * or 3 on a frame with w == 0 or NULL bits, mode 2 or 3 with a box width that is not a multiple of 4, a tile box (of a frame with a chunk) with w
 * or h < 0 or w * h larger than the image's tile grid ((W + 15) >> 4) * ((H + 15) >> 4); YK_ERR_RANGE for mipBytes[f] < (w * h + 7) / 8.
 * A payload shorter than the mask selects cannot be known without a read-back and is no refusal: the missing bytes read as 0, nothing is read out
 * of bounds, and yk_decode_alpha_batch_status (synchronises, reads one word per masked frame) reports per frame 0, or 1 when (selected * 6 + 7) / 8
 * > payBytes[f]; frames of other modes report 0.  YK_ERR_STATE when the batch has no valid alpha planes. */
int yk_decode_alpha_mask_batch_device(yk_ctx* c, const int32_t* modes /* nFrames */, const int32_t* bboxes /* nFrames x {x,y,w,h} */,
                                      const uint8_t* const* devPayload, const size_t* payBytes, const uint8_t* const* devMipBits,
                                      const size_t* mipBytes, const int32_t* mipBoxes /* nFrames x {x,y,w,h} in 16-px tiles */, int noChunkAlpha);
int yk_decode_alpha_batch_status(yk_ctx* c, int32_t* out /* nFrames */);

/* ---- a window of every frame of a batch: one rectangle size, one origin per frame ----
 * yk_decode_set_batch_windows gives frame f of the batch begun by yk_decode_begin_batch the window (xy[2 f], xy[2 f + 1], ww, wh); xy is host
 * memory, nFrames pairs, read before the call returns.  From here on the batch chunk calls owe frame f's planes only the pixels inside its window,
 * exactly as yk_decode_set_window does for a single image: yk_decode_gradient_all_batch_device does the map-sized work of every frame whole (owner
 * lattice, corner count, scan and emit, the marks of every block in tile4x4Mask) and renders only the 64x64 blocks a frame's window touches,
 * yk_decode_1d_batch_device counts and scans every tile and decodes only the window's; for every pixel inside its window frame f holds what the whole
 * batch decode leaves there, its tile4x4Mask is whole and exact, and no byte of its planes outside its window rounded out to multiples of 64
 * (clipped to the image) is written.  yk_decode_alpha[_mask]_batch_device are not affected: the 'ALPM' planes stay whole.
 * Valid after yk_decode_begin_batch (a batch of one frame included) and before any chunk of that batch is decoded (gradient, plane-subset, mask
 * split, '3DTL', 1-D); otherwise, and on a handle begun with yk_decode_begin, YK_ERR_STATE.  Every rectangle obeys the rule of
 * yk_decode_set_window (x0, y0, ww, wh multiples of 8, ww, wh >= 8, inside the image); anything else, and a NULL xy, is YK_ERR_BAD_ARG.  Every
 * argument is checked before anything is queued; a refused argument leaves the batch with no windows.  ww == wh == 0 clears the windows (xy is not
 * looked at); yk_decode_begin and yk_decode_begin_batch always clear them.  yk_decode_set_window stays refused on a batch.
 * The rectangles travel through the pinned ring into a table in HBM that the handle owns, on the handle's stream: kernels of an earlier batch that
 * are still queued read the earlier rectangles.  No host synchronisation (a ring slot is waited for only when four later table copies are queued).
 * While windows are set, the calls that need whole frames return YK_ERR_STATE with a message that names the windows:
 * yk_decode_output_batch_device, yk_decode_output_batch_alpha_device, yk_decode_output_scaled_batch_device,
 * yk_decode_output_mipchain_batch_device, yk_decode_compare_*, and every single-image output and chunk call on the selected frame.
 * yk_decode_select_frame, yk_decode_planes[_device] and yk_decode_tile4x4[_planes] stay allowed: the selected frame's planes are exact inside its
 * window (unspecified outside), its marks whole and exact.
 * yk_decode_output_batch_windows_device: frame f's window goes to devOut + f * frameBytes as ww x wh pixels, with the layout, pitch and channel
 * rules of yk_decode_output_batch_device (the pitch checks are made against ww x wh).  alpha = 0..255 is a constant; alpha = -1 reads frame f's
 * plane of yk_decode_alpha[_mask]_batch_device at its window's offset (YK_ERR_STATE when the batch has no valid alpha planes).  YK_ERR_STATE with
 * no windows set.  One launch, timed as one YK_STAGE_DEC_DETILE interval. */
int yk_decode_set_batch_windows(yk_ctx* c, const int* xy /* nFrames x {x0, y0}, host memory */, int ww, int wh);
int yk_decode_output_batch_windows_device(yk_ctx* c, uint8_t* devOut, size_t rowBytes, size_t planeBytes, size_t frameBytes, int channels, int alpha);

/* ---- windows at any pixel offset and size, cropped in the de-tile ----
 * The three window calls above for rectangles that obey no alignment: a pixel window is x0, y0 >= 0, ww, wh >= 1, x0 + ww <= w, y0 + wh <= h.
 * Everything upstream of the de-tile works on an 8-aligned COVER of the rectangle (yaik_amd/csrc/yk_window_px.h); the de-tile kernel clips the
 * cover's 8-pixel row segments to the rectangle and writes exactly its ww x wh pixels -- no second buffer, no second pass, no second launch.
 * No existing call changes what it accepts or refuses.  Every refusal below comes before the first launch, writes nothing, leaves the handle as
 * the aligned namesake leaves it and names the call in yk_last_error.
 * yk_decode_set_window_px: the state rules of yk_decode_set_window.  The handle's window becomes the smallest 8-aligned rectangle that contains
 * (x0, y0, ww, wh), so every chunk call behaves exactly as under yk_decode_set_window(cover): yk_decode_planes* are exact inside the cover,
 * yk_decode_tile4x4* whole and exact.  ww == wh == 0 clears the window, yk_decode_begin clears it, yk_decode_set_window replaces it.
 * yk_decode_output_window_device then writes the ww x wh crop: the pitch checks are made against ww x wh and alpha = -1 reads the 'ALPM' plane at
 * (x0, y0).  yk_decode_output_scaled_device (levels 1..3) returns YK_ERR_STATE with a message that names the pixel window: its boxes would not be
 * aligned.  The whole-image outputs, the mip chain and yk_decode_prepare_device refuse as under any window.
 * yk_decode_render_windows_px_device: yk_decode_render_windows_device for pixel windows of a prepared image.  It renders the 64x64 blocks the pixel
 * rectangles touch that no earlier call rendered -- one bitmap for this call, the aligned and the scaled one, so the three may be mixed freely --
 * and queues the same intervals: one YK_STAGE_DEC_DETILE, and the render intervals only when a block was new.
 * yk_decode_set_batch_windows_px: yk_decode_set_batch_windows for pixel windows.  Every frame gets a cover of one size, min(w, 8 ceil((ww + 7) / 8))
 * wide (likewise in y), at x0 & ~7 or pulled back to the image's edge; the batch chunk calls treat it as the frame's window.
 * yk_decode_output_batch_windows_device then writes ww x wh per frame (pitch checks against ww x wh, alpha = -1 at each window's own offset).
 * Rectangles that are all 8-aligned with 8-aligned sizes run the kernels of the aligned calls. */
int yk_decode_set_window_px(yk_ctx* c, int x0, int y0, int ww, int wh);
int yk_decode_render_windows_px_device(yk_ctx* c, int nWindows, const int* xy, int ww, int wh,
                                       uint8_t* devOut, size_t rowBytes, size_t planeBytes, size_t windowBytes, int channels, int alpha);
int yk_decode_set_batch_windows_px(yk_ctx* c, const int* xy /* nFrames x {x0, y0}, host memory */, int ww, int wh);

/* ---- normalised fp16 / bf16 / fp32 outputs with a per-frame horizontal mirror ----
 * "Crop - mirror - normalize" in the de-tile store: what the uint8 device outputs write, converted on the way out.  For a decoded byte v (0..255)
 * of channel k (R, G, B, A = 0..3; alpha is treated like a colour channel, whether it comes from a decoded plane or is the constant)
 *     f   = fp32_add_rn(fp32_mul_rn((float)v, scale[k]), bias[k])          two roundings, never an fma
 *     out = f (YK_ELEM_F32), or f rounded to nearest even (YK_ELEM_F16, YK_ELEM_BF16; IEEE overflow to +-inf, fp16 subnormals kept).
 * scale[k] and bias[k] must be finite and either 0 or of magnitude in [2^-100, 2^100]: then no fp32 intermediate is subnormal or overflows and the
 * result does not depend on a denormal mode.  mirror != 0 flips horizontally: pixel x of the (cropped) frame goes to column ww - 1 - x.
 * yk_decode_output_norm_device writes the image begun (or the selected frame of a batch without windows), or the window set on it by
 * yk_decode_set_window or yk_decode_set_window_px.  yk_decode_output_norm_batch_device writes every frame of a batch, frame f at
 * devOut + f * frameBytes: whole frames, or each frame's window if yk_decode_set_batch_windows[_px] is set; mirror is NULL (no frame is flipped) or
 * nFrames flags in host memory, which travel through the pinned ring like the window tables.
 * Pitches are in BYTES.  channels, alpha (-1 = the decoded plane or planes, 0..255 = a constant byte, which is normalised like any other),
 * planeBytes == 0 (HWC: element (x, y, k) at y * rowBytes + (x * channels + k) * es) and planeBytes > 0 (CHW: k * planeBytes + y * rowBytes + x * es)
 * follow the uint8 namesakes, with the pitch-size rules taken against elements of es = sizeof(dtype) bytes.  devOut and every pitch must be
 * multiples of es.  YK_ERR_BAD_ARG: NULL arguments, a dtype that is none of YK_ELEM_*, parameters outside the rule above, misalignment, pitches too
 * small, channels / alpha out of range.  YK_ERR_STATE: nothing begun, a prepared image, the single call on a batch with windows, the batch call on
 * an image with a window, alpha = -1 without valid decoded planes.  Every refusal comes before the first launch, sets yk_last_error, writes nothing
 * and leaves the handle decoding correctly.  One launch, timed as one YK_STAGE_DEC_DETILE interval; no host synchronisation.  Only pixel elements
 * are written: padding keeps what it held.  No other call changes what it accepts, refuses or launches. */
enum { YK_ELEM_F16 = 1, YK_ELEM_BF16 = 2, YK_ELEM_F32 = 3 };
typedef struct yk_norm { int32_t dtype; float scale[4]; float bias[4]; } yk_norm;
int yk_decode_output_norm_device(yk_ctx* c, const yk_norm* norm, int mirror, void* devOut, size_t rowBytes, size_t planeBytes, int channels, int alpha);
int yk_decode_output_norm_batch_device(yk_ctx* c, const yk_norm* norm, const uint8_t* mirror /* nFrames, host memory, or NULL */, void* devOut,
                                       size_t rowBytes, size_t planeBytes, size_t frameBytes, int channels, int alpha);

/* ---- per-frame rectangles resampled to one output size ----
 * A random resized crop in the decoder: frame f has a source rectangle (x0, y0, sw, sh) of its own size and aspect, and every rectangle is resampled
 * to one ow x oh.  x0, y0 >= 0, sw, sh >= 1, x0 + sw <= w, y0 + sh <= h, no alignment; 1 <= ow, oh <= 16384 and sw, sh <= 16384.  Per axis, in
 * integers (x shown; y the same with sh, oh):
 *     step   = floor(sw * 65536 / ow)                         16.16 source pixels per output pixel
 *     off    = (step >> 1) - 32768                            half-pixel centres: (i + 0.5) * sw / ow - 0.5
 *     pos(i) = clamp(off + i * step, 0, (sw - 1) << 16)       i = 0 .. ow - 1
 *     ix = pos >> 16,  fx = (pos >> 8) & 255,  ix1 = min(ix + 1, sw - 1)
 * so taps never leave the rectangle ("crop, then resize": torch's bilinear with align_corners=False, antialias=False on the crop).  With the bytes
 * a = S(ix, iy), b = S(ix1, iy), c = S(ix, iy1), d = S(ix1, iy1) of a channel, S being the whole decode at (x0 + ., y0 + .):
 *     v = ((a (256 - fx) + b fx) (256 - fy) + (c (256 - fx) + d fx) fy + 32768) >> 16            0 .. 255
 * Alpha is resampled like a colour channel, from the 'ALPM' plane or the constant.  Mirror is horizontal and applied to the OUTPUT: output column i
 * lands at ow - 1 - i.  The element is v itself (norm == NULL: uint8) or the normalised element of the section above computed from v.  sw == ow and
 * sh == oh give the pixel-window outputs byte for byte; sw == 2 ow, sh == 2 oh give (a + b + c + d + 2) >> 2.  There is NO antialiasing filter: a
 * rectangle more than twice the output size aliases.
 * yk_decode_set_batch_rects has the state rules of yk_decode_set_batch_windows (after yk_decode_begin_batch, before any chunk).  Frame f's window for
 * the chunk calls becomes the smallest 8-aligned rectangle that contains its rectangle; inside it the frame holds what the whole batch decode leaves
 * there, tile4x4Mask is whole and exact, and no byte of its planes outside that cover rounded out to 64 is written.  rects == NULL clears the
 * rectangles.  Rectangles and windows replace each other; yk_decode_begin[_batch] clears both.  While rectangles are set every call that refuses
 * under batch windows refuses (YK_ERR_STATE, naming the rectangles), and so do yk_decode_output_batch_windows_device and
 * yk_decode_output_norm_batch_device.
 * yk_decode_output_resampled_batch_device writes frame f at devOut + f * frameBytes: its rectangle, or the whole frame if neither rectangles nor
 * windows are set (YK_ERR_STATE with windows).  yk_decode_output_resampled_device does the same for an image begun with yk_decode_begin or the
 * selected frame of a batch that has neither: rect = {x0, y0, sw, sh} must lie inside the window set on the handle (aligned or pixel), NULL means
 * that window or the whole image; a prepared image is refused.  Layout, pitches, channels, alpha and alignment follow
 * yk_decode_output_norm_batch_device, taken against ow x oh elements of 1 byte (norm == NULL) or of the dtype.  One launch under
 * YK_STAGE_DEC_DETILE, no host synchronisation, only pixel elements are written.  Every refusal comes before anything is queued, names the call in
 * yk_last_error, writes nothing and leaves the handle decoding correctly. */
int yk_decode_set_batch_rects(yk_ctx* c, const int* rects /* nFrames x {x0, y0, sw, sh}, host memory, or NULL */);
int yk_decode_output_resampled_batch_device(yk_ctx* c, const yk_norm* norm /* NULL = uint8 */, const uint8_t* mirror /* NULL or nFrames, host memory */,
                                            void* devOut, int ow, int oh, size_t rowBytes, size_t planeBytes, size_t frameBytes, int channels, int alpha);
int yk_decode_output_resampled_device(yk_ctx* c, const int* rect /* 4 ints, or NULL */, const yk_norm* norm, int mirror, void* devOut, int ow, int oh,
                                      size_t rowBytes, size_t planeBytes, int channels, int alpha);

/* ---- round-trip quality (new): what the decode holds against a source image, both in HBM -----------------------------------------
 * The codec is lossy; these calls say how lossy a round trip was without moving a pixel to the host.  One kernel reads the decoder's 8x8-tiled
 * planes (and, with four channels, the decoded 'ALPM' plane) and the source where it lies, a second one folds the workgroups' records; per frame
 * and channel k (0 = R, 1 = G, 2 = B, 3 = alpha): sse[k] = sum (dec - src)^2, sad[k] = sum |dec - src|, nDiff[k] = samples that differ,
 * maxAbs[k] = max |dec - src|, over nSamples = w * h samples.  Integers only: the figures are exact and do not depend on summation order
 * (PSNR = 10 log10(255^2 nSamples / sse) is the caller's one division).  Unused entries of the arrays are 0.
 *   yk_decode_compare_device        the selected frame (or the single image) against 8-bit pixels;
 *   yk_decode_compare_batch_device  every frame of the batch, frame f's source at devSrc + f * frameBytes; out[nFrames];
 *   yk_decode_compare_planes_device every frame against int32 planes as the encoder binds them (yk_bind_device_planes / yk_bind_device_batch:
 *                                   plane k of frame f at frame0Planes[k] + f * frameStrideElems, row pitch strideElems; the low byte of a
 *                                   sample is taken, as the fused kernel does); out[nFrames].
 * 8-bit sources: planeBytes == 0 is HWC, sample (x, y, k) at devSrc[y * rowBytes + x * srcChannels + k], srcChannels = 3 or 4; otherwise CHW, at
 * devSrc[k * planeBytes + y * rowBytes + x] (srcChannels only has to be 3 or 4 and >= channels).  Any base address and pitch is accepted.
 * channels = 3 compares R, G, B (the 4th byte of an RGBA source is skipped); 4 also compares alpha against the plane yk_decode_alpha left (single
 * image) or the planes of yk_decode_alpha_batch_device.
 * devTileSse (may be NULL): device memory for one uint32 per 8x8 tile, the SSE over the compared channels; row-major (w / 8) x (h / 8), frame f at
 * f * (w / 8) * (h / 8) elements.  8x8 is the decoder's tile and the range quantiser's, so the map shows which tiles an encoder setting hurt.
 * Exactly those elements are written; the map stays in HBM and is complete when the call returns.
 * The calls first zero what no chunk has written yet, as the output calls do: they compare exactly what yk_decode_output[_batch]_device would
 * write.  The statistics come back to the host: ONE blocking read-back per call, whatever nFrames is (two launches; the records buffer belongs
 * to the handle and only grows).  ORDERING is the caller's, as for the yk_decode_*_device entry points: the source is read and the map written on
 * THIS handle's stream, and nothing orders that stream behind the producer's (yk_stream_wait_for(c, producerStream) or a host fence first).
 * Timed as one YK_STAGE_DEC_COMPARE interval per call.
 * A refusal launches nothing, writes nothing to out or the map, leaves the handle usable and sets yk_last_error: YK_ERR_BAD_ARG for a NULL
 * devSrc, out or needed plane pointer, channels other than 3 / 4, srcChannels other than 3 / 4 or < channels, rowBytes < w * srcChannels (HWC) or
 * rowBytes < w / planeBytes < rowBytes * h (CHW), frameBytes < rowBytes * h (HWC) or < planeBytes * channels (CHW) with more than one frame,
 * strideElems < w; YK_ERR_STATE before yk_decode_begin[_batch], and for channels = 4 without valid alpha planes. */
typedef struct yk_quality {
    uint64_t sse[4], sad[4], nDiff[4];
    uint32_t maxAbs[4];
    uint64_t nSamples;          /* w * h */
} yk_quality;
int yk_decode_compare_device(yk_ctx* c, const uint8_t* devSrc, size_t rowBytes, size_t planeBytes,
                             int srcChannels, int channels, yk_quality* out, uint32_t* devTileSse);
int yk_decode_compare_batch_device(yk_ctx* c, const uint8_t* devSrc, size_t rowBytes, size_t planeBytes,
                                   size_t frameBytes, int srcChannels, int channels,
                                   yk_quality* out, uint32_t* devTileSse);
int yk_decode_compare_planes_device(yk_ctx* c, const int32_t* const frame0Planes[4], int strideElems,
                                    size_t frameStrideElems, int channels,
                                    yk_quality* out, uint32_t* devTileSse);

/* ---- timing hooks for bench.py: HIP events on the handle's stream around the alpha stage, the fused kernel (alone) and the compaction.
 * One record separates the alpha kernel from the fused kernel; it sits behind the wait of yk_order_fused_after, so a handle that is held
 * back there counts the wait as alpha time.  yk_encode_frame records one interval around its replay, reported as the fused kernel's.
 * An interval that did not take place (alpha of an RGB image, compaction of a replay) counts as 0.  Returns the averages over the yk_encode_tiles calls since the previous query (a ring of 64 event sets, older ones are
 * dropped), so a caller can queue many frames back to back and read the per-kernel times once, without a sync per frame.
 * Synchronises with the most recent encode. */
int yk_last_kernel_ms(yk_ctx* c, float* fusedEncodeMs, float* alphaMs, float* packMs);
/* Device time of the stages outside the fused encode, from HIP events recorded on the launch stream around the stage's KERNELS
 * (host<->device copies of the decode entry points are outside the intervals).  Returns the sum of the intervals recorded since
 * the last query of that stage and their number, and resets both. */
enum { YK_STAGE_CORNERS = 0,       /* yk_gradient_corners: lattice clear + owner / count / scan / emit kernels of the 7 passes */
       YK_STAGE_RANGE1D = 1,       /* yk_range1d_encode: yk_range1d_kernel (the dominant kernel of the live 1-D path) */
       YK_STAGE_RANGE1D_PACK = 2,  /* yk_range1d_encode: scans + yk_range1d_pack_kernel */
       YK_STAGE_DEC_GRADIENT = 3,  /* yk_decode_gradient: owner / corner / scan / render kernels of one pass per interval */
       YK_STAGE_DEC_1D = 4,        /* yk_decode_1d: count / scans / yk_dec1d_kernel */
       YK_STAGE_DEC_DETILE = 5,    /* yk_decode_output / _alpha / _reference_rgba / yk_decode_output_device: yk_dec_detile_kernel */
       YK_STAGE_LUT3D = 6,         /* yk_lut_search: yk_lut_search_kernel (one interval per tile shape) */
       YK_STAGE_UNPACK = 7,        /* yk_upload_pixels_u8 / yk_load_device_pixels_u8: yk_unpack_u8_kernel (the host copy is outside the interval) */
       YK_STAGE_DEC_COMPARE = 8,   /* yk_decode_compare_*: yk_quality_compare_kernel + yk_quality_fold_kernel (the read-back is outside the interval) */
       YK_STAGE_PALETTE = 9,       /* yk_palette_compress*: the clears and the eight yk_pal_*_kernel launches of a call (the read-back is outside the interval) */
       YK_STAGE_PALETTE_DEC = 10 };/* yk_palette_decompress_streams, yk_decode_gradient_palette: the six yk_pd_*_kernel launches of a call */
int yk_stage_ms(yk_ctx* c, int stage, float* msSum, int* intervals);

/* ---- diagnostics: the MEASURED HBM roof of this device (roofline fractions are quoted against the 8 TB/s specification
 * AND against what the part really streams).  Two hand-written kernels with 16-byte accesses, eight loads per lane in flight, on a
 * scratch pair of `bytes` each (allocated and freed inside the call; >= 1 MiB): *copyGBs = best of `reps` of dst[i] = src[i], read + write
 * bytes counted (the figure MI355X_MICROARCH.md quotes: 6.29 TB/s); *readGBs = best of `reps` of a read-only stream.  Synchronises the
 * handle's stream.  No part of the tile path. */
int yk_measure_roof(yk_ctx* c, size_t bytes, int reps, double* copyGBs, double* readGBs);

#ifdef __cplusplus
}
#endif
#endif /* YAIK_HIP_H */
