// Decoder drop-in for the tile hot path: the C API of the reference's include/YAIK.h (YAIK_Init .. YAIK_GetErrorCode,
// lines 52-143) with the chunk loops executed on an MI355X through include/yaik_hip.h.  Programs keep including the
// reference's own YAIK.h and link this library instead of the reference decoder: the declarations below repeat that header's
// types with identical layout, names and enumerator values so both sides agree on the ABI.
//
// On the path: file header, 'MIPM' (mask decode), 'GTIL' (gradient decode, all planes or a plane subset), '3DTL' (3-D LUT tiles, after
// YAIK_AssignLUT), '1DTL' (range decode), 'ALPM' (alpha values: the plane stays in HBM; RGBA 4 B/pixel rows from the default builder, a linear
// planeA with strideA = w for a custom builder), terminator, the default image builder (RGB888 / RGBA8888 rows at outputImageStride) and the
// custom-builder callback (8x8-tiled planes).
// 'ALPM' keeps the reference's state rules and codes: a mipmap-mask mode at state 0 gives YAIK_ALPHA_FORMAT_IMPOSSIBLE, IS_1_BIT_USEMIPMAPMASK
// YAIK_ALPHA_UNSUPPORTED_YET, parameters 7 YAIK_INVALID_ALPHA_FORMAT, a stream shorter than expectedDecompressionSize YAIK_INVALID_DECOMPRESSION,
// a box outside the image or a payload shorter than the box YAIK_INVALID_STREAM.  A '3DTL' chunk without an assigned LUT gives YAIK_INVALID_LUT.  Images whose sides are not multiples of 8 are refused
// (YAIK_INVALID_HEADER).  Sides of 8 (mod 16) decode with the project's consistent reading of the format, not through the reference's
// mis-strided loops (decoder/YAIK_Gradient.cpp:15).
#pragma once
#include <stddef.h>
#include <stdint.h>

typedef void* YAIK_LIB;
typedef void* YAIK_INSTANCE;

typedef void* (*YAIK_allocFunc)(void* customContext, size_t size);
typedef void  (*YAIK_freeFunc)(void* customContext, void* address);     // must accept NULL
struct YAIK_SMemAlloc {
    YAIK_SMemAlloc() : customAlloc(0), customFree(0), customContext(0) {}
    YAIK_allocFunc customAlloc;
    YAIK_freeFunc  customFree;
    void*          customContext;
};

struct YAIK_SDecodedImage;
struct YAIK_SCustomDataSource {                // 8x8-tiled u8 planes R,G,B (+ linear alpha or NULL) and their strides
    uint8_t *planeR, *planeG, *planeB, *planeA;
    int32_t strideR, strideG, strideB;         // bytes to the next row of tiles
    int32_t strideA;                           // bytes to the next line
};
typedef void (*imageBuilderFunc)(struct YAIK_SDecodedImage* userInfo, struct YAIK_SCustomDataSource* sourceImageInternal);

struct YAIK_SDecodedImage {
    uint16_t         width, height;            // filled by YAIK_DecodeImagePre
    bool             hasAlpha;                 // filled by YAIK_DecodeImagePre
    imageBuilderFunc customImageOutput;        // Pre installs the default builder; the user may replace it before YAIK_DecodeImage
    void*            userContextCustomImage;
    YAIK_SMemAlloc   userMemoryAllocator;      // Pre installs malloc/free; the user may replace it.  HOST memory of a decode only: the planes,
                                                // corner lattice, masks and streams of this implementation live in HBM (hipMalloc, owned by the
                                                // decode slot's device handle) and never come from this allocator
    uint8_t*         outputImage;              // user buffer, required by YAIK_DecodeImage
    int32_t          outputImageStride;
    bool             hasAlpha1Bit;
    YAIK_INSTANCE    internalTag;              // owned by the library between Pre and Decode
};

enum YAIK_ERROR_CODE {
    YAIK_NO_ERROR = 0, YAIK_INVALID_LIBRARYCTX, YAIK_MALLOC_FAIL, YAIK_INVALID_CONTEXT_COUNT, YAIK_INIT_FAIL,
    YAIK_RELEASE_EMPTY_LIBRARY, YAIK_INVALID_STREAM, YAIK_INVALID_HEADER, YAIK_NO_EMPTYDECODE_SLOT, YAIK_DECIMG_INVALIDCTX,
    YAIK_DECIMG_DIFFSTREAM, YAIK_DECIMG_BUFFERNOTSET, YAIK_INVALID_CONTEXT_MEMALLOCATOR, YAIK_INVALID_DECOMPRESSION, YAIK_INVALID_LUT,
    YAIK_DECOMPRESSION_CREATE_FAIL, YAIK_INVALID_MIPMAP_LEVEL, YAIK_ALPHA_FORMAT_IMPOSSIBLE, YAIK_INVALID_ALPHA_FORMAT,
    YAIK_ALPHA_UNSUPPORTED_YET, YAIK_INVALID_TAG_ID, YAIK_INVALID_PLANE_ID,
};

YAIK_LIB        YAIK_Init(uint8_t maxDecodeThreadContext, YAIK_SMemAlloc* libraryMemAllocator);
void            YAIK_AssignLUT(YAIK_LIB lib, uint8_t* lutData, uint32_t lutDataLength);     // the 3-D LUT file ('LUL0'); needed before a stream with a '3DTL' chunk
void            YAIK_Release(YAIK_LIB lib);
bool            YAIK_DecodeImagePre(YAIK_LIB lib, void* sourceStreamAligned, uint32_t streamLength, YAIK_SDecodedImage* getUserInfo);
bool            YAIK_DecodeImage(void* sourceStreamAligned, uint32_t streamLength, YAIK_SDecodedImage* context);
YAIK_ERROR_CODE YAIK_GetErrorCode();

// extension (not in the reference): HIP device used by the decode slots created by the next YAIK_Init (default 0)
void            YAIK_SetDevice(int device);
// extension: YAIK_DecodeImage into DEVICE memory.  context->outputImage is an address in HBM of the device YAIK_SetDevice named when YAIK_Init
// created the slots, outputImageStride its row pitch; the rows are RGB888, or RGBA8888 when the stream has an 'ALPM' chunk (the default
// builder's rule), and row padding is left untouched.  The pixels never cross PCIe: the de-tile kernel writes them in place.  The buffer
// must not be in use by work still queued on other streams.  The call returns once the pixels are in place (it synchronises the slot's
// stream before releasing the slot).  Everything else is YAIK_DecodeImage's contract; a custom customImageOutput (it takes host planes) is
// refused with YAIK_DECIMG_INVALIDCTX, and the slot is released as after any other failure.
bool            YAIK_DecodeImageToDevice(void* sourceStreamAligned, uint32_t streamLength, YAIK_SDecodedImage* context);
// extension: how 'GTIL' chunks for one or two planes (HeaderGradientTile::plane 1..6) mark tile4x4Mask.  0 (default) = exactly what the
// reference's DecompressGradient4x4R/G/B/RG/GB/RB loops do (R/G/B leave the mask alone, GB/RB put the B marks at tile4x4Mask +
// tile4x4MaskSize/2; decoder/YAIK_Gradient.cpp:1420-2732), after which the reference's own Decompress1D reads a different number of
// tiles than the encoder wrote; 1 = every pass marks the planes it filled, which decodes such streams correctly.
void            YAIK_SetPartialPlaneMarks(int consistent);
// extension: where PaletteDecompressor runs for 'GTIL' chunks of all three planes (HeaderGradientTile::plane 7).  0 (default) = on the host
// (palette.cpp), the expanded colour stream is uploaded; 1 = the payload is uploaded as ZStd left it and decompressed on the device
// (yk_decode_gradient_palette).  Same images; a malformed payload gives YAIK_INVALID_STREAM either way.  Plane-subset chunks stay on the host.
void            YAIK_SetDevicePalette(int on);
// extension: n (1..1024) streams of ONE width x height decoded as a batch into DEVICE memory: frame f at devOut + f * frameBytes with the layout rules
// of yk_decode_output_batch_device (HWC rows of rowBytes, or CHW planes planeBytes apart when planeBytes > 0; only pixel bytes are written).
// channels 3 = RGB; 4 = RGBA, alpha from the frame's 'ALPM' chunk or 255 for a frame without one.  Frame f's pixel bytes are those
// YAIK_DecodeImageToDevice writes for stream f (255 added as alpha where that call writes RGB).  Streams made of header, optional 'MIPM', optional
// 'ALPM', the shipped 'GTIL' passes for all planes in order, optional '1DTL' and the terminator go through the device's batch calls: ZStd (and
// PaletteDecompressor, unless YAIK_SetDevicePalette(1) and one colorCompression for the batch) on `threads` (1..16) workers into one staging
// buffer, ONE upload, every kernel once over the n frames (batch_plan.h has the rules).  Any other stream -- '3DTL', plane-subset 'GTIL', another
// order, a structural or ZStd error, a '1DTL' compressionRange other than the batch's first -- is decoded afterwards by the single-image chain
// on the same slot.  The call takes one free decode slot and returns it.  A stream whose header differs from stream 0's size fails with
// YAIK_INVALID_HEADER; a stream YAIK_DecodeImageToDevice rejects makes the call return false with that call's error code; *failedIndex (may be NULL)
// is the lowest failing index, -1 otherwise.  After a failure the pixel bytes of the n frames are unspecified, except that a stream whose chunks
// are in batch order up to a '1DTL' chunk with compressionRange 0 fails the call (YAIK_INVALID_STREAM) before a byte is written.  Bad arguments (n, channels,
// threads, NULL tables) give YAIK_DECIMG_INVALIDCTX, a NULL devOut YAIK_DECIMG_BUFFERNOTSET.
bool            YAIK_DecodeImagesToDevice(YAIK_LIB lib, void* const* streams, const uint32_t* lengths, int n, uint8_t* devOut, size_t rowBytes,
                                          size_t planeBytes, size_t frameBytes, int channels, int threads, int32_t* failedIndex);
// how many streams of the last YAIK_DecodeImagesToDevice took the single-image chain, and its host clocks in ms: {plan + expansion, upload,
// batch calls up to the synchronise}
int             YAIK_LastBatchFallbacks();
void            YAIK_LastBatchStageMs(double out[3]);
