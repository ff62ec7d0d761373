// YAIK_DecodeImageToDevice (yaik_decode.h) at reduced resolution: the same stream, the same slot, the same chunk chain, but the image is written at
// 1 / (1 << level) of its size, level = 0..3 (1/1, 1/2, 1/4, 1/8).
//
// After YAIK_DecodeImagePre, set outputImage to DEVICE memory of (width >> level) x (height >> level) pixels and outputImageStride to its row pitch
// (>= (width >> level) * 3, or * 4 when the stream has an 'ALPM' chunk: rows are RGB888, or RGBA8888 with the decoded alpha averaged like a colour
// channel).  Every pixel is the mean of its (1 << level) x (1 << level) box of YAIK_DecodeImageToDevice's image, halves rounded up, computed from
// the full-size bytes in integers inside the de-tile kernel (yk_decode_output_scaled_device): no full-size image is written anywhere.  Level 0 is
// YAIK_DecodeImageToDevice.
//
// A level outside 0..3 gives YAIK_DECIMG_INVALIDCTX before any chunk is decoded or any byte written (the slot is released).  Every other failure
// is that of YAIK_DecodeImageToDevice; a custom image builder is refused likewise.
#pragma once
#include "yaik_decode.h"
#ifdef __cplusplus
extern "C" {
#endif

bool YAIK_DecodeImageScaledToDevice(void* stream, uint32_t length, YAIK_SDecodedImage* context, int level);

#ifdef __cplusplus
}
#endif
