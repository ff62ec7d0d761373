// The alpha6Bit fallback rule of the ConvertHotPath* family and of YAIK_EncodeImagesFromDeviceAlpha6 (ours, not the reference's): a frame's analog
// alpha is written in the 6-bit mask mode only when a decoder can select the same pixels from the file, i.e. when its 'MIPM' chunk exists, has
// bits, and every bit of its tile box {x, y, w, h} is set.  Pure: reads its arguments only.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace yaikalpha6 {
inline bool decodable(bool hasChunk, const int32_t tileBox[4], const uint8_t* bits, size_t nBytes) {
    if (!hasChunk || !bits || !nBytes || tileBox[2] <= 0 || tileBox[3] <= 0) return false;
    const size_t nBits = (size_t)tileBox[2] * (size_t)tileBox[3];
    if (nBytes < (nBits + 7) / 8) return false;
    for (size_t i = 0; i < nBits; i++)
        if (!((bits[i >> 3] >> (i & 7)) & 1)) return false;
    return true;
}
}  // namespace yaikalpha6
