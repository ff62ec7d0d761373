// Batch file writer (an extension: the reference converts one image per process): n frames of ONE width x height that lie in DEVICE memory as
// 8-bit interleaved pixels become n .yaik streams in host memory, with a fixed number of kernel launches, read-backs and copies per batch.
//
// Per call: yk_set_image + yk_set_batch + yk_load_device_pixels_u8, yk_encode_batch(3, 0), yk_encode_streams_batch (corner and 1-D streams),
// yk_palette_compress_batch (every frame from a fresh book, like one image of a fresh process), for RGBA yk_alpha_bitmaps_batch and, with
// emitAlpha, yk_alpha_values_batch(1); then ONE yk_device_gather of every frame's pieces in file order into a grow-only HBM buffer and ONE
// yk_device_download into grow-only host staging.  `threads` workers then compress and frame (encode_frame.h): every stream of every frame is a
// job of its own, so a batch of few frames still fills them.
//
// zstdLevel 0: stream f is byte for byte the file EncoderContext::ConvertHotPath writes for frame f alone with the same emitAlpha and alpha6Bit
// off (either palette coder).  zstdLevel 1..22: every ZStd stream, 'ALPM' included, is compressed at that level (no sweep); chunk order, headers
// apart from the compressed sizes, padding and every decompressed payload equal the level-0 stream's.  No byte depends on `threads`.
//
// devPixels: frame f at devPixels + f * frameBytes, rows of `channels` (3 = RGB, 4 = RGBA with four planes) bytes per pixel at a pitch of
// rowBytes (yk_load_device_pixels_u8's layout; frameBytes is ignored for n = 1).  The pixels are read on the encoder's own stream: ORDERING
// against their producer is the caller's, and they may be reused when the call returns.
// Failures: bad arguments (a NULL encoder or pixel pointer, n outside 1..1024, channels not 3 or 4, sides that are not multiples of 8 from 8 to
// 32760, pitches shorter than a row or a frame, emitAlpha not 0 or 1, zstdLevel outside 0..22, threads outside 1..16) fail before anything is
// launched, with *failedIndex = -1; a device call that fails returns false with *failedIndex = -1 and the handle's message; a frame that cannot
// be framed -- every case where ConvertHotPath fails, e.g. "a pass has colours but no tile" -- sets *failedIndex to the lowest such frame.
// failedIndex may be NULL.  The encoder is usable afterwards; the streams of a failed call are not handed out.
#pragma once
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct YAIK_Encoder* YAIK_ENC;
YAIK_ENC    YAIK_EncoderCreate(int device);                                  /* NULL without a usable HIP device: there is no CPU fallback */
void        YAIK_EncoderRelease(YAIK_ENC e);
bool        YAIK_EncodeImagesFromDevice(YAIK_ENC e, const uint8_t* devPixels, size_t rowBytes, size_t frameBytes, int channels,
                                        int width, int height, int n, int emitAlpha, int zstdLevel, int threads, int32_t* failedIndex);
bool        YAIK_EncodedStream(YAIK_ENC e, int frame, const uint8_t** data, uint32_t* length);   /* owned by e until the next call */
const char* YAIK_EncoderLastError(YAIK_ENC e);
void        YAIK_LastEncodeStageMs(YAIK_ENC e, double out[4]);   /* host clocks in ms: device calls, gather + download, entropy + framing, total */

#ifdef __cplusplus
}
#endif
