// Drop-in mirror of the hot-path part of the reference's `EncoderContext` (encoder/EncoderContext.h:183-370 in KLab/YAIK):
// same method names, argument meaning and call order for MipPrefilter -> 7x FittingQuadSmooth -> DynamicTileEncode x3
// (-> DynamicTileCompressor x3), executed on an MI355X through the C-ABI of include/yaik_hip.h.
//
// Differences a caller sees:
//   * with `outFile` set the passes append the same chunks as the reference ('MIPM', 'GTIL', 'PLNT', '1DTL'; PaletteCompressor
//     and ZStd run on host cores, see chunks.h); with `outFile == NULL` they write nothing.  Either way the raw streams each
//     pass hands to the entropy stage are exposed through the Last*() accessors (bitmap, corner stream, tile defs, nibbles);
//   * the seven FittingQuadSmooth calls must come in the shipped order (4,4)(4,3)(3,4)(3,3)(3,2)(2,3)(2,2) with the image's
//     planes 0,1,2 (EncoderContext.cpp:9057-9093): the first one launches the fused kernel, the others return its cached results;
//   * errors follow the reference's convention (message on stdout, neutral return value) plus LastError().
// The methods are public here: this class is the surface of the path, not of Convert().
#pragma once
#include <cstdio>
#include <string>
#include <vector>
#include "framework.h"

struct yk_ctx;

struct EncoderContext {
public:
    EncoderContext();
    ~EncoderContext();

    // same tunables as the reference constructor defaults (EncoderContext.h:185-228)
    int colorCompressionQuad, colorCompressionLUT3D, colorCompression1D, rangeCompression1D;
    // mipmap-mask bounding box in pixels + bookkeeping the range quantiser reads (EncoderContext.h:246-253)
    int mipMapTileSize, boundX0, boundY0, boundX1, boundY1, remainingPixels;
    bool dumpImage, evaluateLUT, evaluateLUT2D;
    FILE* outFile;                                      // chunks are appended here when set (the reference requires it; NULL = streams only)
    int fileOutSize;

    bool SetImageToEncode(Image* newImage);             // takes ownership, deletes the previous image (EncoderContext.cpp:1227-1233)
    // EncoderContext::LoadImagePNG (:1235-1242) from the point stbi_load has decoded the file, for a caller that holds 8-bit interleaved
    // pixels: rows of `channels` (3 = RGB, 4 = RGBA) bytes per pixel at a pitch of rowBytes; sides multiples of 8, as Image::LoadPNG
    // requires.  Builds `original` as Image::LoadPNG does (encoder/Image.cpp:200-229): the host int32 planes are filled, because this class
    // hands out Plane* and ConvertHotPathStripes reads them.  The GPU, however, is bound through yk_upload_pixels_u8 instead of
    // yk_upload_planes: one byte per sample crosses PCIe and a kernel widens it.  Everything after it is unchanged, ConvertHotPath* included.
    // The mirror still reads no PNG file itself.
    bool LoadImagePixels(const u8* pixels, int w, int h, int channels, size_t rowBytes);
    Image* ImageToEncode() { return original; }         // the image the passes read (the reference's protected `original`)
    yk_ctx* Handle() const { return ctx; }              // the C-ABI handle behind the passes (e.g. for yk_stage_ms); owned by this object
    void Release();

    void CheckMipmapMask();                             // EncoderContext.cpp:2784
    void PrepareQuadSmooth();                           // empty in the reference too (:2796)
    void MipPrefilter(bool active);                     // :1257
    // :1429-1682, on the GPU (yk_alpha_values) after MipPrefilter: the alpha VALUES.  With outFile set it appends the 'ALPM' chunk (none for
    // an image without alpha, all-255 alpha or alpha below 4 everywhere).  force8Bit = true is what Convert passes (:9027-9028); false writes
    // analog alpha as IS_6_BIT_USEMIPMAPMASK_INVERSE over the pixels of the kept 16x16 tiles, exactly as the reference does.
    void ProcessAlpha(bool force8Bit);
    // opt-in: the ConvertHotPath* family calls ProcessAlpha right after MipPrefilter, like the commented-out call in Convert()
    // (:9027-9028).  Off by default: files stay byte for byte what they were.
    bool emitAlpha;
    // opt-in with emitAlpha (not a reference option; Convert never passes false): ProcessAlpha(false) instead of ProcessAlpha(true), but only
    // when a 'MIPM' chunk was written and every bit of its tile bitmap is set.  The decoder reads the mask of the 6-bit mask modes the way the
    // reference does ("Mask-mode finding"), which gives the right pixels only then; otherwise the chunk is the 8-bit one.
    bool alpha6Bit;
    int  FittingQuadSmooth(int rejectFactor, Plane* a, Plane* b, Plane* c, Image* testOutput, bool useYCoCg,
                           int tileBitSizeX, int tileBitSizeY);                           // :3710, returns TileDone
    int  DynamicTileEncode(bool mode3BitOnly, Plane* plane, Plane* dst, bool isCo, bool isCg, bool isHalfX, bool isHalfY);   // :4365
    u8*  DynamicTileCompressor(u8* stream, Plane* src, Plane* map, Plane* debug);         // :8398, returns the advanced cursor
    // (f)4 3-D LUT tiles, where Convert() runs them (:9117-9218): after the gradient passes, before the 1-D compressor
    void Load3DPattern(const char* fileName);                                             // :7851, one 'Bank3D' .lut file (u8 count, r[], g[], b[])
    bool Save3DLutFile(const char* fileName);                                             // the decoder's 'LUL0' file RegisterAndCreate3DLut writes (:7820-7847)
    void StartCorrelationSearch(bool is3D);                                               // :7316
    void Correlation3DSearch(Image* input, Image* output, int tileShiftX, int tileShiftY);// :6245
    void EndCorrelationSearch(bool is3D, u8 component);                                   // :7366, appends the '3DTL' chunk to outFile
    int  correlationPatternCount3D;
    int  LastCorrelationMatches() const { return lutMatched; }                            // "MATCHED TILE" of the last Correlation3DSearch
    void GenerateDynamicTileChunk(u8* stream, int sizeStream);                            // :8524, '1DTL' chunk of the three planes' streams
    // The chunk sequence of Convert() restricted to this path (:9007-9016, :9057-9093, :9451-9470, :9779-9781): file header,
    // ['MIPM' for RGBA], 7x 'GTIL', '1DTL', terminator — a stream the reference's YAIK_DecodeImage accepts.  Takes no ownership of f.
    bool ConvertHotPath(FILE* f);
    // The same file, byte for byte, with the entropy stage threaded: PaletteCompressor keeps its pass order on one
    // thread (its code book carries over from chunk to chunk), the sixteen ZStd streams (7 bitmaps, 7 colour streams, the 1-D pixel and
    // type streams) are compressed by `threads` workers, the chunks are written in file order.  ConvertHotPathBegin returns as soon as
    // every raw stream is on the host: the GPU and this object are then free for SetImageToEncode + the passes of the NEXT image while
    // the previous files are still being compressed (each stage has its own thread and its own PaletteCompressor code book, started
    // empty like a fresh process; up to kMaxStages images in flight, Begin waits for the oldest beyond that); ConvertHotPathFinish
    // waits for all of them.  `f` belongs to its stage between Begin and Finish.
    bool ConvertHotPathBegin(FILE* f, int threads);
    bool ConvertHotPathFinish();
    // opt-in (off by default): ConvertHotPath and ConvertHotPathBegin take the seven 'GTIL' colour payloads from the GPU (yk_palette_reset +
    // yk_palette_compress: PaletteCompressor on the corner streams where they lie in HBM) instead of running palette.cpp on the host; the
    // entropy stage then only hands them to ZStd.  The file is byte for byte the one written with the option off.  The raw corner streams are
    // still downloaded pass by pass (LastGradientRGBStream keeps working and the chunk header needs their sizes).  Plane-subset passes and the
    // pass-by-pass form (FittingQuadSmooth with outFile set) keep the host coder.
    void SetDevicePalette(bool on) { devicePalette = on; }
    bool ConvertHotPathParallel(FILE* f, int threads) { return ConvertHotPathBegin(f, threads) && ConvertHotPathFinish(); }
    // The tile maps of the image, encoded as row stripes on several GPUs of the node by THIS process (the reference is one
    // process, include/YAIK.h:42-47): stripe i = a band of 64-row blocks + one halo row (the BL / BR corner samples at y + T,
    // EncoderContext.cpp:3853-3856) on devices[i]; the image-wide kept-tile box of MipPrefilter is combined on the host (no collective);
    // the per-stripe maps are concatenated on the first device by ONE grouped RCCL transfer (yk_gather_maps_all) and come back in one copy.
    // Stripes that share a device (a one-GPU box) are simply read back one by one.  The result equals the whole-image encode bit for bit:
    // 7 swizzled bitmaps, and per plane the tile definitions and the nibble stream of DynamicTileEncode.
    struct StripeTileMaps {
        std::vector<u8> bitmap[7];
        std::vector<u16> defs[3];
        std::vector<u8> nibbles[3];
        size_t nNibbles[3] = { 0, 0, 0 };
        int bounds[4] = { 0, 0, 0, 0 };                 // boundX0, boundY0, boundX1, boundY1 of the whole image
        int stripes = 0, gatherRanks = 0;               // ranks of the RCCL communicator the gather used (0 = no transfer between devices)
    };
    bool ConvertHotPathStripes(const int* devices, int nStripes, bool mode3BitOnly, StripeTileMaps* out);

    // raw streams of the last call of each kind (what the reference compresses and writes, before entropy coding)
    const std::vector<u8>&  LastGradientBitmap() const { return gradBitmap; }             // pFillBitMap (:3775)
    const std::vector<u8>&  LastGradientRGBStream() const { return gradRgb; }             // rgbStream (:3783)
    const std::vector<u16>& LastTileDefs() const { return tileDefs; }                     // streamTileDef (:4419)
    const std::vector<u8>&  LastTileIndexStream() const { return tileIdx; }               // streamTileIdx (:4421), closed to a byte
    size_t                  LastTileIndexCount() const { return nNibbles; }
    const std::vector<u8>&  MipmapBitmap() const { return mipBitmap; }                    // 'MIPM' payload (:1317-1327)
    bool                    MipmapHasChunk() const { return mipHasChunk; }
    int                     AlphaMode() const { return alphaMode; }                        // AlphaHeader::parameters of the last ProcessAlpha, -1 = no chunk
    const std::vector<u8>&  AlphaPayload() const { return alphaPayload; }                  // its decompressed payload
    const int*              AlphaBBox() const { return alphaBox; }
    const std::vector<u8>&  TileTypeStream1D() const { return type1d; }                   // streamType (:8217)
    const char*             LastError() const { return err.c_str(); }
    int                     device;                                                        // HIP device ordinal, set before SetImageToEncode

private:
    struct EntropyStage;                                // the streams of one image + the thread that compresses and writes them
    enum { kMaxStages = 8 };
    std::vector<EntropyStage*> stages;
    bool stagesOk = true; std::string stagesErr;
    void retireOldestStage();
    bool ensureEncoded(int rejectFactor, bool mode3, bool wantDst);
    bool adoptImage(Image* newImage, const u8* pixels, size_t rowBytes);   // SetImageToEncode / LoadImagePixels (pixels != NULL)
    bool fail(const char* what);
    bool alpha6BitDecodable() const;
    bool devicePalette = false;
    bool devicePalettePayloads(std::vector<u8> pal[7]);      // yk_palette_reset + yk_palette_compress of the current frame, payloads to the host
    Image* original;
    yk_ctx* ctx;
    bool bound, alphaDone, encoded, enc3, encDst, oneDReady;
    int encReject, nextPass;
    std::vector<u8> gradBitmap, gradRgb, tileIdx, mipBitmap, pix1d, type1d;
    std::vector<u16> tileDefs;
    size_t nNibbles, cursor1d;
    bool mipHasChunk;
    int mipTiles[4] = {0, 0, 0, 0};                    // MipmapHeader.bbox of the last 'MIPM' chunk, in 16-px tiles
    int alphaMode, alphaBox[4];
    std::vector<u8> alphaPayload;
    int lutMatched;
    std::vector<std::vector<u8>> lutPatterns;          // as loaded (count x 3, interleaved): the factor tables of the LUT file come from them
    std::string err;
};
