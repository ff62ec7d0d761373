// n .yaik streams of one shape, a source rectangle of each resampled to one ow x oh in device memory: a random resized crop in the decoder
// (yk_decode_set_batch_rects, yk_decode_output_resampled_batch_device, include/yaik_hip.h).
//
// The arguments of YAIK_DecodeImagesNormToDevice (yaik_decode_norm.h) with rects and ow, oh in place of xy, ww, wh: rects is NULL (whole frames) or
// n x {x0, y0, sw, sh}, stream f's own rectangle at any offset and of any size 1..16384 inside the image; 1 <= ow, oh <= 16384.  norm may be NULL:
// devOut then holds uint8 pixels; otherwise elements of norm->dtype computed from the resampled byte.  mirror is NULL or one flag per stream (a
// set one flips that stream's OUTPUT horizontally).  rowBytes, planeBytes (0 = interleaved) and frameBytes are in BYTES, taken against ow x oh
// elements.  The resampling is bilinear in 16.16 fixed point with taps clamped to the rectangle and has no antialiasing filter.
//
// It runs on the batch plan of YAIK_DecodeImagesToDevice with the same fallback: a stream the batch calls cannot take goes through the single-image
// chain on the same slot with yk_decode_set_window_px on its rectangle and ends in yk_decode_output_resampled_device into the stream's slot of
// devOut.  A size or rectangle outside the rule, a whole frame above 16384 pixels on a side, and what YAIK_DecodeImagesNormToDevice refuses for norm
// give YAIK_DECIMG_INVALIDCTX before a decode slot is taken: nothing is written.  Every other failure is the namesake's.
#pragma once
#include "yaik_decode.h"
#include "../../include/yaik_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

bool YAIK_DecodeImagesResampledToDevice(YAIK_LIB lib, void* const* streams, const uint32_t* lengths, int n, void* devOut, size_t rowBytes, size_t planeBytes,
                                        size_t frameBytes, int channels, int threads, int32_t* failedIndex, const int* rects, int ow, int oh,
                                        const yk_norm* norm, const uint8_t* mirror);

#ifdef __cplusplus
}
#endif
