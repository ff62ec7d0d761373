// Windows of .yaik streams at any pixel offset and size: the three window calls (yaik_decode_window.h, yaik_decode_multiwindow.h,
// yaik_decode_batch_windows.h) for rectangles that obey no alignment (yk_decode_set_window_px, yk_decode_render_windows_px_device,
// yk_decode_set_batch_windows_px, include/yaik_hip.h).
//
// Each call takes the arguments of its aligned namesake and writes the same bytes that namesake's whole-image decode holds inside the rectangle:
// ww x wh pixels per window, the pitch rules taken against ww x wh, the alpha of a stream with an 'ALPM' chunk read at the window's own offset.
// The device decodes the rectangle's 8-aligned cover and the de-tile kernel clips it: no second buffer and no second launch.  The paths are those
// of the namesakes -- the prepared image for YAIK_DecodeImageWindowsPxToDevice (YAIK_LastWindowsPrepared reports on it), the batch calls for
// YAIK_DecodeImagesWindowsPxToDevice (YAIK_LastBatchFallbacks, YAIK_LastBatchStageMs) -- and so are the fallbacks to the single-image chain.
//
// A pixel window is x0, y0 >= 0, ww, wh >= 1, x0 + ww <= width, y0 + wh <= height.  Anything else, and a NULL xy, gives YAIK_DECIMG_INVALIDCTX
// before a chunk is decoded (the batch call: before a decode slot is taken): nothing is written.  Every other failure is the namesake's.
#pragma once
#include "yaik_decode.h"
#ifdef __cplusplus
extern "C" {
#endif

bool YAIK_DecodeImageWindowPxToDevice(void* stream, uint32_t length, YAIK_SDecodedImage* info, int x0, int y0, int ww, int wh);
bool YAIK_DecodeImageWindowsPxToDevice(void* stream, uint32_t length, YAIK_SDecodedImage* info, int nWindows, const int* xy, int ww, int wh,
                                       size_t windowBytes);
bool YAIK_DecodeImagesWindowsPxToDevice(YAIK_LIB lib, void* const* streams, const uint32_t* lengths, int n, uint8_t* devOut, size_t rowBytes,
                                        size_t planeBytes, size_t frameBytes, int channels, int threads, int32_t* failedIndex,
                                        const int* xy, int ww, int wh);

#ifdef __cplusplus
}
#endif
