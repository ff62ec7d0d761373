// The plan of YAIK_DecodeImagesToDevice: which streams of a batch can go through the device's batch calls, and where their pieces lie.
// Pure host code: it reads the chunk framing only (no ZStd, no HIP), so that a CPU tool can link it (batch_plan_tool).
//
// A stream is BATCHABLE when it is: file header, optional 'MIPM', optional 'ALPM' (mode 1..6 under the single decoder's state rules), then 'GTIL'
// chunks for all three planes (plane == 7) whose tile shapes are a strictly increasing subsequence of the seven shipped passes, then an optional
// '1DTL' (one in front of every 'GTIL' is ignored, as the single decoder ignores it), then the terminator -- and every size check the single decoder's chunk loop makes holds, together with the checks the device calls
// behind it make on the host (alpha box, payload lengths, the 'MIPM' box against the image's tile grid).  Any other stream is a FALLBACK stream:
// '3DTL', a plane-subset 'GTIL', another chunk order, a repeated shape, any structural error.  The single-image chain decodes those, and
// reports their errors with its own codes.
#pragma once
#include <cstddef>
#include <cstdint>

namespace yaikplan {

static const int NUM_PASSES = 7;
extern const int PASS_SHIFT[NUM_PASSES][2];          // the shipped passes in encode order: {4,4} {4,3} {3,4} {3,3} {3,2} {2,3} {2,2}

struct GradChunk {
    bool present = false;
    const uint8_t* zBitmap = nullptr; uint32_t zBitmapBytes = 0, bitmapBytes = 0;       // ZStd frame, expanded size (from the shape)
    const uint8_t* zColor = nullptr;  uint32_t zColorBytes = 0, payloadBytes = 0, rgbBytes = 0;   // ZStd frame, PaletteCompressor payload, colour stream
    uint8_t colorCompression = 0;
};
struct StreamPlan {
    bool batchable = false;
    const char* why = "";                             // the first rule a fallback stream broke
    bool hasMip = false; int32_t mipBox[4] = { 0, 0, 0, 0 }; const uint8_t* mipBits = nullptr; uint32_t mipBytes = 0;   // box in 16-pixel tiles
    bool hasAlpha = false; int alphaMode = -1; int32_t alphaBox[4] = { 0, 0, 0, 0 };
    const uint8_t* zAlpha = nullptr; uint32_t zAlphaBytes = 0, alphaBytes = 0;
    GradChunk grad[NUM_PASSES];
    bool has1d = false; const uint8_t* zType = nullptr; const uint8_t* zPix = nullptr;
    uint32_t zTypeBytes = 0, typeBytes = 0, zPixBytes = 0, pixBytes = 0; uint8_t compressionRange = 0;
    // a fallback stream whose chunks were in order up to a '1DTL' with compressionRange 0: no decoder takes it (the range divides), so the batch
    // call can fail before it writes a byte instead of after the other frames
    bool range0 = false;
};

// the checks of YAIK_DecodeImagePre: 0 = fine (width, height, rgba filled), 1 = no stream at all (YAIK_INVALID_STREAM), 2 = YAIK_INVALID_HEADER
int readHeader(const void* stream, uint32_t length, int* width, int* height, bool* rgba);
// expanded bytes of the tile bitmap of pass `pass` at w x h
uint32_t bitmapBytes(int pass, int w, int h);
// the plan of one stream whose header readHeader accepted; returns out.batchable
bool planStream(const void* stream, uint32_t length, StreamPlan& out);

}  // namespace yaikplan
