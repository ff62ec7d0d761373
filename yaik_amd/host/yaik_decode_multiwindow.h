// Many windows of one .yaik stream: the map-sized work of the image once, then every window pays for the 64x64 blocks nobody rendered before it
// and its own de-tile (yk_decode_prepare_device / yk_decode_render_windows_device, include/yaik_hip.h).
//
// After YAIK_DecodeImagePre, set outputImage to DEVICE memory for nWindows windows of ww x wh pixels, window k at outputImage + k * windowBytes,
// and outputImageStride to the row pitch (>= ww * 3, or ww * 4 when the stream has an 'ALPM' chunk: rows are RGB888, or RGBA8888 with the
// decoded alpha read at each window's offset).  xy holds nWindows pairs x0, y0.  What window k receives equals the crop of
// YAIK_DecodeImageToDevice's image, byte for byte.
//
// A stream the batch planner calls batchable (planStream, batch_plan.h) takes the prepared path: ZStd and the host's PaletteDecompressor expand
// it into the slot's staging buffer, one upload, yk_decode_prepare_device, the single-image 'MIPM' / 'ALPM' calls, one
// yk_decode_render_windows_device.  Any other stream ('3DTL', plane-subset chunks, a chunk order of its own) runs the chain of
// YAIK_DecodeImageWindowToDevice once per window, into that window's slice: the same bytes.  YAIK_SetDevicePalette is not looked at on the
// prepared path.
//
// nWindows is 1..1024; x0, y0, ww, wh must be multiples of 8 with ww, wh >= 8 and every rectangle inside the image; anything else gives
// YAIK_DECIMG_INVALIDCTX (the slot is released, nothing is written).  Every other failure is that of YAIK_DecodeImageToDevice; a custom image
// builder is refused likewise.
#pragma once
#include "yaik_decode.h"
#ifdef __cplusplus
extern "C" {
#endif

bool YAIK_DecodeImageWindowsToDevice(void* stream, uint32_t length, YAIK_SDecodedImage* context, int nWindows, const int* xy, int ww, int wh, size_t windowBytes);
int  YAIK_LastWindowsPrepared(void);   /* 1: the last call went through prepare; 0: per-window fallback */

#ifdef __cplusplus
}
#endif
