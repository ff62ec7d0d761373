// One window of each of n .yaik streams of one shape: YAIK_DecodeImagesToDevice with a rectangle per stream, all of one size
// (yk_decode_set_batch_windows / yk_decode_output_batch_windows_device, include/yaik_hip.h).
//
// The arguments are those of YAIK_DecodeImagesToDevice (yaik_decode.h); xy holds n pairs x0, y0 (host memory), the window of stream f is
// (xy[2 f], xy[2 f + 1], ww, wh).  devOut is DEVICE memory for n windows of ww x wh pixels, window f at devOut + f * frameBytes, with the layout,
// pitch and channel rules of YAIK_DecodeImagesToDevice taken against ww x wh: RGB888 / RGBA8888 rows (planeBytes == 0) or planes; with four
// channels the alpha of a stream with an 'ALPM' chunk is its decoded alpha read at the window's offset, 255 otherwise.  What window f receives
// equals the crop of YAIK_DecodeImagesToDevice's frame f, byte for byte.
//
// Streams the batch planner calls batchable (planStream, batch_plan.h; 'ALPM' in 8-bit mode and in the 6-bit mask mode included) go through the
// device's batch calls with the windows set: every kernel once over the n frames, the pixel-sized work of a frame only inside its window.  Any
// other stream ('3DTL', plane-subset chunks, a chunk order of its own) runs the chain of YAIK_DecodeImageWindowToDevice into its slice: the same
// bytes.  YAIK_LastBatchFallbacks and YAIK_LastBatchStageMs report on this call as they do on YAIK_DecodeImagesToDevice.
//
// x0, y0, ww, wh must be multiples of 8 with ww, wh >= 8 and every rectangle inside the image; anything else, and a NULL xy, gives
// YAIK_DECIMG_INVALIDCTX before a decode slot is taken: nothing is written.  Every other failure is that of YAIK_DecodeImagesToDevice.
#pragma once
#include "yaik_decode.h"
#ifdef __cplusplus
extern "C" {
#endif

bool YAIK_DecodeImagesWindowsToDevice(YAIK_LIB lib, void* const* streams, const uint32_t* lengths, int n, uint8_t* devOut, size_t rowBytes,
                                      size_t planeBytes, size_t frameBytes, int channels, int threads, int32_t* failedIndex,
                                      const int* xy, int ww, int wh);

#ifdef __cplusplus
}
#endif
