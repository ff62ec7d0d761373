// YAIK_DecodeImageToDevice (yaik_decode.h) with a mip chain as its output: the same stream, the same slot, the same chunk chain, but the image is
// written as the levels firstLevel .. firstLevel + nLevels - 1 of its chain in one call (yk_decode_output_mipchain_device).
//
// A width x height image has levels 0 .. top, top = floor(log2(min(width, height))); level k has (width >> k) x (height >> k) pixels and every
// pixel is the mean of its (1 << k) x (1 << k) box of YAIK_DecodeImageToDevice's image, halves rounded up, computed from the full-size bytes in
// integers (never from another level's rounded means).  From level 4 on the columns and rows that fill no whole box are ignored.
//
// After YAIK_DecodeImagePre, levelImages[i] is DEVICE memory for level firstLevel + i and levelStrides[i] its row pitch (>= (width >> k) * 3, or
// * 4 when the stream has an 'ALPM' chunk: rows are RGB888, or RGBA8888 with the decoded alpha averaged like a colour channel).  outputImage and
// outputImageStride of the context are not used.  firstLevel = 0 gives the whole chain, the full-size pixels included.
//
// A level range outside the chain, a NULL table or a NULL level pointer gives YAIK_DECIMG_INVALIDCTX before any chunk is decoded or any byte
// written (the slot is released).  Every other failure is that of YAIK_DecodeImageToDevice; a custom image builder is refused likewise.
#pragma once
#include "yaik_decode.h"
#ifdef __cplusplus
extern "C" {
#endif

bool YAIK_DecodeImageMipchainToDevice(void* stream, uint32_t length, YAIK_SDecodedImage* context, int firstLevel, int nLevels, void* const* levelImages,
                                      const uint32_t* levelStrides);

#ifdef __cplusplus
}
#endif
