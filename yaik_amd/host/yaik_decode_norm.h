// n .yaik streams of one shape into normalised fp16 / bf16 / fp32 elements in device memory, with a horizontal mirror per stream
// (yk_decode_output_norm_batch_device, include/yaik_hip.h).
//
// The arguments of YAIK_DecodeImagesWindowsPxToDevice (yaik_decode_window_px.h) plus the conversion: norm (dtype, and scale and bias per channel;
// out = fp32(v) * scale[k], then + bias[k], two roundings, stored as fp32 or rounded to nearest even) and mirror (NULL, or one flag per stream:
// non-zero flips that stream's output horizontally).  xy == NULL means whole frames (ww, wh are not looked at); otherwise stream f's ww x wh pixel
// window at (xy[2f], xy[2f + 1]), any rectangle inside the image.  devOut holds elements of norm->dtype; rowBytes, planeBytes (0 = interleaved) and
// frameBytes are in BYTES, and they and devOut are multiples of the element size.
//
// It runs on the batch plan of YAIK_DecodeImagesToDevice with the same fallback: a stream the batch calls cannot take goes through the single-image
// chain on the same slot, which ends in yk_decode_output_norm_device into the stream's slot of devOut (YAIK_LastBatchFallbacks,
// YAIK_LastBatchStageMs report as for the namesake).  A NULL norm, a dtype that is none of YK_ELEM_*, a scale or bias outside the device call's rule
// (finite, 0 or of magnitude in [2^-100, 2^100]), a misaligned devOut or pitch and a window outside the image give YAIK_DECIMG_INVALIDCTX before a
// decode slot is taken: nothing is written.  Every other failure is the namesake's.
#pragma once
#include "yaik_decode.h"
#include "../../include/yaik_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

bool YAIK_DecodeImagesNormToDevice(YAIK_LIB lib, void* const* streams, const uint32_t* lengths, int n, void* devOut, size_t rowBytes, size_t planeBytes,
                                   size_t frameBytes, int channels, int threads, int32_t* failedIndex, const int* xy, int ww, int wh,
                                   const yk_norm* norm, const uint8_t* mirror);

#ifdef __cplusplus
}
#endif
