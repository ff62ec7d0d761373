// yk_streams_batch.hip — yk_encode_streams_batch: the seven corner colour streams and the two 1-D streams of EVERY frame of a handle with one launch
// per kernel, one blocking read-back and one table upload per batch.  Host-side sequence only: the kernels are the single-image ones'
// bodies run with the frame as a grid dimension (yk_corners.hip, yk_range1d.hip).
//
//   count:  lattice clear, owners, corners per block, corner scan (a workgroup per frame) | 1-D offsets, 1-D scan (a workgroup per frame)
//   read back 9 uint32 per frame: the stream lengths -- the layout below needs all of them, and nothing else of the batch is needed on the host
//   layout: every stream at the next multiple of 16 of one buffer that is exactly as long as the streams; a record of bases per frame -> HBM
//   emit:   corner emit kernel, 1-D coder; every workgroup reads its frame's record
#include "yk_common.h"

extern "C" {

int yk_encode_streams_batch(yk_ctx* c, int what) {
    if (!c) return YK_ERR_BAD_ARG;
    if (what < 1 || what > 3) return yk_refuse(c, YK_ERR_BAD_ARG, "what must be YK_STREAMS_CORNERS (1), YK_STREAMS_RANGE1D (2) or both (3)");
    if (c->y0 != 0 || c->h != c->fullH) return yk_refuse(c, YK_ERR_STATE, "yk_encode_streams_batch works on whole images, not on a stripe");
    if (!yk_batch_planes_bound(c)) return yk_refuse(c, YK_ERR_STATE, "bind planes first");
    if (!c->encoded) return yk_refuse(c, YK_ERR_STATE, "yk_encode_batch first (or, for one frame, yk_encode_tiles / yk_encode_frame)");
    if (c->ppActive) return yk_refuse(c, YK_ERR_STATE, "a plane-subset pass ran: its per-plane coverage is not batched");
    YK_HIP(c, hipSetDevice(c->device));
    const int N = c->nFrames;
    const bool corners = (what & YK_STREAMS_CORNERS) != 0, r1 = (what & YK_STREAMS_RANGE1D) != 0;
    YkStreamsBatch& b = c->img.sb;
    b.valid = false; c->pal.valid = false;
    YK_HIP(c, b.counts.reserve(c->stream, (size_t)N * YK_SB_COUNTS));
    YK_HIP(c, b.tab.reserve(c->stream, (size_t)N));
    // ---- count phase ----
    if (r1) {
        { int rc = yk_stage_begin(c, YK_STAGE_RANGE1D_PACK); if (rc) return rc; }
        { int rc = yk_range1d_batch_count(c); if (rc) return rc; }
        { int rc = yk_stage_end(c, YK_STAGE_RANGE1D_PACK); if (rc) return rc; }
    }
    if (corners) {
        // ends behind the emit kernel: the interval spans the read-back.  A failure in between returns with the interval open, which costs nothing:
        // yk_stage_end is what counts an interval, so the slot and its events are taken again by the next yk_stage_begin and no time is accounted.
        { int rc = yk_stage_begin(c, YK_STAGE_CORNERS); if (rc) return rc; }
        { int rc = yk_corners_batch_count(c); if (rc) return rc; }
    }
    // ---- the one read-back: only the stream lengths; a phase that was not requested leaves its counts unwritten and they are not looked at ----
    std::vector<uint32_t> cnt((size_t)N * YK_SB_COUNTS);
    YK_HIP(c, hipMemcpyAsync(cnt.data(), b.counts, cnt.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));
    // ---- layout: every stream on a multiple of 16, nothing reserved for what a frame might have produced ----
    b.table.assign((size_t)N, yk_frame_streams{});
    std::vector<size_t> offs((size_t)N * 9, (size_t)-1);
    size_t total = 0;
    auto place = [&](size_t bytes) { const size_t o = total; total = (total + bytes + 15) & ~(size_t)15; return o; };
    for (int f = 0; f < N; f++) {
        const uint32_t* k = &cnt[(size_t)f * YK_SB_COUNTS];
        yk_frame_streams& t = b.table[(size_t)f];
        const YkFrameView V = yk_frame(c, f);
        for (int p = 0; p < 7; p++) {
            t.bitmap[p] = V.bitmap[p]; t.bitmapBytes[p] = c->bitmapBytes[p];
            t.rgbBytes[p] = corners ? (size_t)k[p] * 3 : 0;
            if (t.rgbBytes[p]) offs[(size_t)f * 9 + p] = place(t.rgbBytes[p]);
        }
        t.pixBytes = r1 ? (size_t)k[8] * 3 : 0; t.typeBytes = r1 ? (size_t)k[7] * 9 : 0;      // three planes; a parameter triple per coded tile and plane
        if (t.pixBytes) offs[(size_t)f * 9 + 7] = place(t.pixBytes);
        if (t.typeBytes) offs[(size_t)f * 9 + 8] = place(t.typeBytes);
    }
    YK_HIP(c, b.out.reserve(c->stream, total + 64));
    int slot; void* host;
    { const int rc = yk_dec_table_host(c, (size_t)N * sizeof(YkStreamRec), &slot, &host); if (rc) return rc; }
    YkStreamRec* rec = static_cast<YkStreamRec*>(host);
    for (int f = 0; f < N; f++) {
        yk_frame_streams& t = b.table[(size_t)f];
        const size_t* o = &offs[(size_t)f * 9];
        for (int p = 0; p < 7; p++) { rec[f].rgb[p] = o[p] == (size_t)-1 ? nullptr : b.out + o[p]; t.rgb[p] = rec[f].rgb[p]; }
        rec[f].pix = o[7] == (size_t)-1 ? nullptr : b.out + o[7]; t.pix = rec[f].pix;
        rec[f].type = o[8] == (size_t)-1 ? nullptr : b.out + o[8]; t.type = rec[f].type;
    }
    { const int rc = yk_dec_table_upload(c, slot, b.tab, (size_t)N * sizeof(YkStreamRec)); if (rc) return rc; }
    // ---- emit phase ----
    if (corners) {
        { int rc = yk_corners_batch_emit(c); if (rc) return rc; }
        { int rc = yk_stage_end(c, YK_STAGE_CORNERS); if (rc) return rc; }
    }
    if (r1) {
        { int rc = yk_stage_begin(c, YK_STAGE_RANGE1D); if (rc) return rc; }
        { int rc = yk_range1d_batch_emit(c); if (rc) return rc; }
        { int rc = yk_stage_end(c, YK_STAGE_RANGE1D); if (rc) return rc; }
    }
    b.valid = true; b.what = what;
    return YK_OK;
}

int yk_batch_streams_table(yk_ctx* c, yk_frame_streams* out) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!out) return yk_refuse(c, YK_ERR_BAD_ARG, "out is NULL");
    if (!c->img.sb.valid || (int)c->img.sb.table.size() != c->nFrames) return yk_refuse(c, YK_ERR_STATE, "yk_encode_streams_batch first (the table does not outlive an encode, a new image or new planes)");
    for (int f = 0; f < c->nFrames; f++) out[f] = c->img.sb.table[(size_t)f];
    return YK_OK;
}

}  // extern "C"
