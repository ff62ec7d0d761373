// YAIK_EncodeImagesFromDevice (yaik_encode.h) with ConvertHotPath's alpha6Bit option: the same batch, the same encoder object, the same getters.
//
// alpha6Bit = 0 is YAIK_EncodeImagesFromDevice exactly.  alpha6Bit = 1 takes effect only with emitAlpha on RGBA frames: after
// yk_alpha_bitmaps_batch the 'MIPM' bits of every frame are fetched in ONE download (their slots lie in one buffer, at the addresses
// yk_alpha_bitmap_device hands out), the rule of
// alpha6_rule.h (EncoderContext::alpha6BitDecodable's) is applied per frame, and yk_alpha_values_mask_batch writes the 'ALPM' values of the frames
// that satisfy it in the 6-bit mask mode (IS_6_BIT_USEMIPMAPMASK_INVERSE) and of all others as YAIK_EncodeImagesFromDevice does.  The number of
// launches, read-backs and copies per batch stays fixed.
//
// zstdLevel 0: stream f is byte for byte the file EncoderContext::ConvertHotPath writes for frame f alone with the same emitAlpha and alpha6Bit.
// zstdLevel 1..22, threads, failures and *failedIndex: as YAIK_EncodeImagesFromDevice; alpha6Bit outside 0..1 is a bad argument.
#pragma once
#include "yaik_encode.h"
#ifdef __cplusplus
extern "C" {
#endif

bool YAIK_EncodeImagesFromDeviceAlpha6(YAIK_ENC e, const uint8_t* devPixels, size_t rowBytes, size_t frameBytes, int channels, int width, int height,
                                       int n, int emitAlpha, int alpha6Bit, int zstdLevel, int threads, int32_t* failedIndex);

#ifdef __cplusplus
}
#endif
