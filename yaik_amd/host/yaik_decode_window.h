// YAIK_DecodeImageToDevice (yaik_decode.h) for a window of the image: the same stream, the same slot, the same chunk chain, but only the
// pixels of the rectangle (x0, y0, ww, wh) are produced.
//
// After YAIK_DecodeImagePre, set outputImage to DEVICE memory of ww x wh pixels and outputImageStride to its row pitch (>= ww * 3, or ww * 4 when
// the stream has an 'ALPM' chunk: rows are RGB888, or RGBA8888 with the decoded alpha read at the window's offset).  The window is set on the
// slot's handle right after yk_decode_begin (yk_decode_set_window), so the gradient render and the 1-D range decode skip the tiles outside it,
// and the call ends in yk_decode_output_window_device.  What it writes equals the crop of YAIK_DecodeImageToDevice's image, byte for byte.
//
// x0, y0, ww, wh must be multiples of 8 with ww, wh >= 8 and the rectangle inside the image; anything else gives YAIK_DECIMG_INVALIDCTX (the
// slot is released, nothing is written).  Every other failure is that of YAIK_DecodeImageToDevice; a custom image builder is refused likewise.
#pragma once
#include "yaik_decode.h"
#ifdef __cplusplus
extern "C" {
#endif

bool YAIK_DecodeImageWindowToDevice(void* stream, uint32_t length, YAIK_SDecodedImage* context, int x0, int y0, int ww, int wh);

#ifdef __cplusplus
}
#endif
