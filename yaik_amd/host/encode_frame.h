// The pieces of one encoded frame -> its .yaik stream: the entropy stage and the chunk framing behind YAIK_EncodeImagesFromDevice.
// Pure host code (chunks.cpp + ZStd, no HIP), so that a CPU tool can link it (encode_frame_tool).
//
// The stream is what EncoderContext::ConvertHotPath writes for the frame alone: file header, 'MIPM' (RGBA frames whose box of kept tiles is not the
// whole image), 'ALPM' (when the caller hands in a payload), the 'GTIL' chunks of the seven shipped passes that have an accepted tile and
// colours, '1DTL' (when there are pixel bytes), the terminator.  level 0 compresses like ConvertHotPath (ZStd level 18, 'ALPM' at the smallest of
// levels 5..21); level 1..22 compresses every stream at that level.  Chunk order, headers apart from the compressed sizes, padding and every
// decompressed payload do not depend on the level, and no byte depends on the number of threads.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>
#include "framework.h"

namespace yaikenc {

struct FramePieces {
    int width = 0, height = 0; bool hasAlpha = false;
    bool mipHasChunk = false; int mipBox[4] = { 0, 0, 0, 0 }; const u8* mipBits = nullptr; size_t mipBytes = 0;      // box in 16-pixel tiles
    int alphaMode = -1; int alphaBox[4] = { 0, 0, 0, 0 }; const u8* alpha = nullptr; size_t alphaBytes = 0;          // mode -1: no 'ALPM' chunk
    const u8* bitmap[7] = {}; size_t bitmapBytes[7] = {};                       // swizzled tile bitmaps of the seven passes
    size_t rgbBytes[7] = {};                                                    // corner colour streams: only their lengths go into the file
    const u8* palette[7] = {}; size_t paletteBytes[7] = {};                     // PaletteCompressor payloads, every frame from a fresh book
    const u8* pix = nullptr; size_t pixBytes = 0; const u8* type = nullptr; size_t typeBytes = 0;                     // 1-D streams
};

// what the workers make of a frame: one ZStd frame per stream
struct FrameStreams {
    bool has[7] = {};
    std::vector<u8> zAlpha, zBitmap[7], zRgb[7], zPix, zType;
};
static const int JOBS_PER_FRAME = 17;               // 0 = 'ALPM', 1..7 = tile bitmaps, 8..14 = colour payloads, 15 = 1-D pixels, 16 = 1-D types

// which passes get a chunk; false (and err) where ConvertHotPath fails: a pass with colours but no accepted tile
bool planFrame(const FramePieces& p, FrameStreams& s, std::string& err);
// one stream of the frame through ZStd (nothing to do for a stream the frame does not have); after planFrame
bool compressJob(const FramePieces& p, FrameStreams& s, int job, int level, std::string& err);
// the framed stream; after every job of the frame
bool emitFrame(const FramePieces& p, const FrameStreams& s, int colorCompressionQuad, int colorCompression1D, int rangeCompression1D,
               std::vector<u8>& out, std::string& err);
// fn(i) for i in [0, n) on up to `threads` threads (the caller's included); returns when all have run
void parallelFor(size_t n, int threads, const std::function<void(size_t)>& fn);
// n frames: every stream of every frame is a job of its own, so that a batch of few frames still fills the workers; then the frames are framed in
// parallel.  out[f] = frame f's stream.  Returns false with *failedIndex = the lowest frame that could not be framed and its message in err.
bool encodeFrames(const FramePieces* frames, int n, int level, int threads, std::vector<std::vector<u8>>& out, int* failedIndex, std::string& err);

}  // namespace yaikenc
