// yk_palette_dec.hip — PaletteDecompressor (decoder/YAIK_GenericFunctions.cpp:139-241; host form: yaik_amd/host/palette.cpp) on the GPU, byte-exact
// with the reference's decoder as the project's CPU restatement executes it.
//
// The work is a list of STREAMS (payload pointer, payload bytes n, colours N = outBytes / 3); every kernel below is launched once over all streams of
// a call, and a workgroup finds its stream by binary search over first-workgroup numbers, as in yk_palette.hip.  A payload is read as if followed by
// zeros, and its token bytes start at hdr = 1 + 3 * codeBookSize + 3, whatever n is.  Per call, all on the handle's stream, no host synchronisation:
//   walk     token bytes are cut into chunks of PD_CB bytes counted from hdr.  A token's length follows from its first byte alone (1, or 1 + popcount
//            of the mask), so a chunk can be walked from each of the four offsets 0..3 at which its first token may start: four threads per chunk
//            record where the walk leaves the chunk (0..3 into the next), how many colours it wrote, and where its first error was (an extension
//            code, or a token that would start at or beyond n + 385), counted in colours written before it
//   link     a workgroup per stream composes the chunks' four-state maps (a scan of 8-bit maps), which gives every chunk its true entry offset,
//            then a prefix sum of the colours written from that entry gives every chunk the index of its first colour.  An error counts only when
//            fewer than N colours were written in front of it; the header check (1 + 3 * codeBookSize > n) is made here too.  One status word
//            per stream.  The back-references a chunk ends in (any, the last one's d, the largest d) are scanned the same way, so that a run of
//            them, however long, reaches the next writing token without any thread walking more than its chunk
//   mark     a thread per chunk walks it again from the true entry and stores, for every colour 1..N-1, the offset of the token that writes it and
//            the distance to its parent with the largest distance any back-reference in front of it named
//   parent   colour chunks of PD_CC colours, a thread per colour: the back-references in front of its token give its parent (every one of them is
//            checked against colour 0, the last one wins), the token gives per channel {add a | set c}.  These records
//            compose associatively: ten rounds of pointer jumping in LDS resolve every colour either to constants or to "colour h of the 65 in
//            front of the chunk, plus a"
//   carry    one workgroup per stream walks its colour chunks in order and turns the last 65 records of a chunk into the 65 colours in front of the
//            next (65 lanes work; the others help fetching the records of 32 chunks at a time into LDS)
//   apply    a thread per colour: constant, or halo colour + a; PaletteFullRangeRemapping; three byte stores into the stream's slot
// Nothing is read back by the call itself: yk_palette_decode_status synchronises and reads 4 bytes per stream.  No scratch memory, no inline
// assembly, nothing captured into a graph.
//
// Bounds.  Every payload read goes through pd_rd (offset < n, else 0).  Token offsets are only written for colour indices 1..N-1 and lie below
// n + 385.  The colour kernels of a stream do nothing when its status is non-zero after `link`; with status 0 every colour 1..N-1 has a token offset,
// because a walk that ends without N colours ends in the "input exhausted" error.  A back-reference before colour 0 turns its colour into a constant,
// so no parent index leaves the chunk's 65-colour halo.  Output stores are guarded by colour < N and go to slot offset + 3 * colour only.
#include "yk_common.h"

#define PD_CB      64                       // token bytes per chunk
#define PD_WGCH    64                       // chunks per workgroup of the walk / mark kernels
#define PD_LPITCH  68                       // LDS pitch of a chunk: 17 words, so that the walkers of a wave hit different banks
#define PD_CC      1024                     // colours per chunk = threads per workgroup of the parent / apply kernels
#define PD_BACK    65                       // a colour's parent is at most 65 back
#define PD_SLACK   385u                     // a token may start at any offset below n + 385 (the reference's inEnd = input + 1 + inputSize + 384)
#define PD_NOERR   127u
#define PD_MAX_COLOURS (1u << 28)
#define PD_MAX_SEGS    65536
#define PD_MARGIN  64                       // bytes kept free in front of and behind the used range of the output buffer

// status bits (only zero / non-zero is contract): what was found at or before the token that writes the last colour.  After the first error the
// walk goes on over bytes the reference never looks at, so only the lowest-positioned finding is the reference's reason; the bits are the union.
#define PD_ST_HEADER    1u                  // 1 + 3 * codeBookSize > n
#define PD_ST_EXTENSION 2u                  // a token 1001xxxx / 101xxxxx
#define PD_ST_EXHAUSTED 4u                  // a token would start at or beyond n + 385
#define PD_ST_BACKREF   8u                  // a back-reference before colour 0

struct YkPdSeg {
    const uint8_t* src;
    uint32_t n;                             // payload bytes
    uint32_t N;                             // colours to write
    uint32_t aWg0;                          // first workgroup of the token-chunk grid (PD_WGCH chunks each)
    uint32_t nAWg;
    uint32_t cWg0;                          // first workgroup of the colour-chunk grid
    uint32_t colOff;                        // first colour's record
    uint32_t outOff;                        // the slot in the output buffer (a multiple of 16)
    uint32_t pad;
};

struct YkPdBufs {
    const YkPdSeg* segs; uint32_t nSeg;
    uint32_t* rec;                          // [chunks][4]: exit | colours << 2 | colours before the first error << 9 | its kind << 16 | the run of
                                            // back-references the walk ends in: any << 19 | the last one's d << 20 | the largest d << 26
    uint32_t* chunkBack;                    // [chunks]: the back-references pending at the chunk's true entry: any << 1 | last d << 2 | largest d << 8
    uint16_t* backInfo;                     // per colour: distance to its parent (1..65) | the largest distance any back-reference in front of it named << 8
    uint32_t* chunkInfo;                    // [chunks]: min(first colour, N) << 2 | entry offset
    uint32_t* tokOff;                       // per colour: offset of the token that writes it
    uint32_t* sumVal;                       // per colour: r | g << 8 | b << 16 | constant-channel flags << 24
    uint8_t* sumPtr;                        // per colour: which of the 65 colours in front of its chunk the non-constant channels add to
    uint32_t* halo;                         // [colour chunks][65]: the colours in front of a chunk, packed
    uint32_t* status;                       // [2][nSeg]: what the link kernel found, what the parent kernel found (a word of its own: the parent
                                            // kernel's workgroups read the first while others of them already write)
};

template <bool COLOURS> __device__ inline uint32_t pd_find_seg(const YkPdSeg* __restrict__ segs, uint32_t nSeg, uint32_t i) {
    uint32_t lo = 0, hi = nSeg - 1;
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        const uint32_t first = COLOURS ? segs[mid].cWg0 : segs[mid].aWg0;
        if (first <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ inline uint32_t pd_rd(const uint8_t* __restrict__ src, uint32_t n, uint32_t off) { return off < n ? (uint32_t)src[off] : 0u; }
__device__ inline uint32_t pd_hdr(const YkPdSeg& S) { return 4u + 3u * pd_rd(S.src, S.n, 0); }
__device__ inline bool pd_is_explicit(uint32_t b) { return (b & 0xF0u) == 0x80u; }          // kinds 0 and 1; 0x90..0xBF are the extension codes
__device__ inline uint32_t pd_map_apply(uint32_t m, uint32_t e) { return (m >> (2 * e)) & 3u; }
__device__ inline uint32_t pd_map_then(uint32_t f, uint32_t g) {                             // first f, then g
    return pd_map_apply(g, pd_map_apply(f, 0)) | (pd_map_apply(g, pd_map_apply(f, 1)) << 2) | (pd_map_apply(g, pd_map_apply(f, 2)) << 4) | (pd_map_apply(g, pd_map_apply(f, 3)) << 6);
}

// A run of back-reference tokens in front of a writing token, however long, as one word: wrote << 0 | any << 1 | the last one's d << 2 | the largest
// d << 8.  `wrote` marks a summary that contains a writing token, behind which only its trailing run counts.  pd_run_then is associative, so the
// runs of the chunks are scanned like the entry offsets; no thread ever walks a run longer than its chunk.
__device__ inline uint32_t pd_run_push(uint32_t r, uint32_t d) {
    const uint32_t mx = (r & 2u) ? max((r >> 8) & 63u, d) : d;
    return (r & 1u) | 2u | (d << 2) | (mx << 8);
}
__device__ inline uint32_t pd_run_then(uint32_t a, uint32_t b) {            // first a, then b
    if (b & 1u) return b;
    if (!(b & 2u)) return a;
    if (!(a & 2u)) return (a & 1u) | (b & ~1u);
    return (a & 1u) | 2u | (b & 0xFCu) | (max((a >> 8) & 63u, (b >> 8) & 63u) << 8);
}

// the PD_WGCH chunks of workgroup `w` of a stream, staged in LDS at PD_LPITCH bytes per chunk (256 threads)
__device__ inline void pd_stage_chunks(uint8_t* lds, const YkPdSeg& S, uint32_t base, uint32_t t) {
    for (uint32_t q = t; q < PD_WGCH * PD_CB; q += 256) {
        const uint32_t off = base + q;                                      // < 2^32: n + 385 + a workgroup's bytes stays far below
        lds[(q / PD_CB) * PD_LPITCH + (q % PD_CB)] = (uint8_t)pd_rd(S.src, S.n, off);
    }
}

// ---- (a) token starts -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void yk_pd_walk_kernel(YkPdBufs B) {
    __shared__ uint8_t lds[PD_WGCH * PD_LPITCH];
    const uint32_t t = threadIdx.x, wg = blockIdx.x;
    const YkPdSeg S = B.segs[pd_find_seg<false>(B.segs, B.nSeg, wg)];
    const uint32_t base = pd_hdr(S) + (wg - S.aWg0) * (PD_WGCH * PD_CB), limit = S.n + PD_SLACK;
    pd_stage_chunks(lds, S, base, t);
    __syncthreads();
    const uint32_t ch = t >> 2, e = t & 3u;
    const uint8_t* b = lds + ch * PD_LPITCH;
    const uint32_t cbase = base + ch * PD_CB;
    uint32_t p = e, cnt = 0, errW = PD_NOERR, kind = 0, run = 0;            // run: pd_run_* of the back-references since the last writing token
    while (p < PD_CB) {
        if (cbase + p >= limit) { if (errW == PD_NOERR) { errW = cnt; kind = PD_ST_EXHAUSTED; } p = PD_CB; break; }
        const uint32_t c = b[p];
        if (c < 0x80u) { cnt++; run = 0; p += 1; }
        else if (c >= 0xC0u) { run = pd_run_push(run, c & 63u); p += 1; }
        else if (pd_is_explicit(c)) { cnt++; run = 0; p += 1u + __popc(c & 7u); }
        else { if (errW == PD_NOERR) { errW = cnt; kind = PD_ST_EXTENSION; } p += 1; }
    }
    B.rec[((size_t)wg * PD_WGCH + ch) * 4 + e] = (p - PD_CB) | (cnt << 2) | (errW << 9) | (kind << 16) | ((run >> 1) << 19);
}

__global__ __launch_bounds__(256) void yk_pd_link_kernel(YkPdBufs B) {
    __shared__ uint32_t sh[256];
    __shared__ uint32_t flags;
    const uint32_t t = threadIdx.x, sg = blockIdx.x;
    const YkPdSeg S = B.segs[sg];
    if (t == 0) B.status[B.nSeg + sg] = 0;
    if (S.N == 0) { if (t == 0) B.status[sg] = 0; return; }
    if (t == 0) flags = (1u + 3u * pd_rd(S.src, S.n, 0) > S.n) ? PD_ST_HEADER : 0u;
    const uint32_t nCh = S.nAWg * PD_WGCH;
    const size_t ch0 = (size_t)S.aWg0 * PD_WGCH;
    uint32_t carryE = 0, carryCol = 1, carryRun = 0;                        // colour 0 comes from the header
    for (uint32_t c0 = 0; c0 < nCh; c0 += 256) {                            // nCh is a multiple of 64: uniform trip count, guarded lanes
        const uint32_t ch = c0 + t;
        uint4 r = make_uint4(0, 0, 0, 0);
        uint32_t m = 0xE4u;                                                 // the identity map
        if (ch < nCh) {
            r = *reinterpret_cast<const uint4*>(B.rec + (ch0 + ch) * 4);
            m = (r.x & 3u) | ((r.y & 3u) << 2) | ((r.z & 3u) << 4) | ((r.w & 3u) << 6);
        }
        __syncthreads();
        sh[t] = m;
        __syncthreads();
        for (uint32_t off = 1; off < 256; off <<= 1) {
            const uint32_t before = t >= off ? sh[t - off] : 0xE4u, mine = sh[t];
            __syncthreads();
            sh[t] = pd_map_then(before, mine);
            __syncthreads();
        }
        const uint32_t e = t ? pd_map_apply(sh[t - 1], carryE) : carryE;
        const uint32_t nextE = pd_map_apply(sh[255], carryE);
        const uint32_t mineRec = e == 0 ? r.x : e == 1 ? r.y : e == 2 ? r.z : r.w;
        const uint32_t cnt = ch < nCh ? (mineRec >> 2) & 127u : 0u;
        __syncthreads();
        sh[t] = cnt;
        __syncthreads();
        for (uint32_t off = 1; off < 256; off <<= 1) {
            const uint32_t x = t >= off ? sh[t - off] : 0u;
            __syncthreads();
            sh[t] += x;
            __syncthreads();
        }
        const uint32_t col0 = carryCol + sh[t] - cnt, total = sh[255];
        const uint32_t myRun = ch < nCh ? (cnt ? 1u : 0u) | ((mineRec >> 19) << 1) : 0u;      // the identity beyond the stream's chunks
        __syncthreads();
        sh[t] = myRun;
        __syncthreads();
        for (uint32_t off = 1; off < 256; off <<= 1) {
            const uint32_t before = t >= off ? sh[t - off] : 0u, mine = sh[t];
            __syncthreads();
            sh[t] = pd_run_then(before, mine);
            __syncthreads();
        }
        const uint32_t runIn = t ? pd_run_then(carryRun, sh[t - 1]) : carryRun, nextRun = pd_run_then(carryRun, sh[255]);
        if (ch < nCh) {
            const uint32_t errW = (mineRec >> 9) & 127u;
            if (errW != PD_NOERR && col0 + errW < S.N) atomicOr(&flags, (mineRec >> 16) & 7u);
            B.chunkInfo[ch0 + ch] = (min(col0, S.N) << 2) | e;
            B.chunkBack[ch0 + ch] = runIn;
        }
        carryE = nextE; carryCol += total; carryRun = nextRun;
    }
    __syncthreads();
    if (t == 0) B.status[sg] = flags;
}

__global__ __launch_bounds__(256) void yk_pd_mark_kernel(YkPdBufs B) {
    __shared__ uint8_t lds[PD_WGCH * PD_LPITCH];
    const uint32_t t = threadIdx.x, wg = blockIdx.x;
    const YkPdSeg S = B.segs[pd_find_seg<false>(B.segs, B.nSeg, wg)];
    const uint32_t info = t < PD_WGCH ? B.chunkInfo[(size_t)wg * PD_WGCH + t] : 0xFFFFFFFFu;
    if (B.chunkInfo[(size_t)wg * PD_WGCH] >> 2 >= S.N) return;              // uniform: the first colour of the workgroup's first chunk is already beyond
    const uint32_t base = pd_hdr(S) + (wg - S.aWg0) * (PD_WGCH * PD_CB), limit = S.n + PD_SLACK;
    pd_stage_chunks(lds, S, base, t);
    __syncthreads();
    if (t >= PD_WGCH) return;
    const uint8_t* b = lds + t * PD_LPITCH;
    const uint32_t cbase = base + t * PD_CB;
    uint32_t p = info & 3u, col = info >> 2, run = B.chunkBack[(size_t)wg * PD_WGCH + t];
    uint32_t* tok = B.tokOff + S.colOff;
    uint16_t* bk = B.backInfo + S.colOff;
    while (p < PD_CB && col < S.N && cbase + p < limit) {
        const uint32_t c = b[p];
        const bool writes = c < 0x80u || pd_is_explicit(c);
        if (writes) {                                                       // without a back-reference the parent is the colour before
            tok[col] = cbase + p;
            bk[col] = (uint16_t)((run & 2u) ? (((run >> 2) & 63u) + 2u) | ((((run >> 8) & 63u) + 2u) << 8) : 1u | (1u << 8));
            col++; run = 0;
            p += c < 0x80u ? 1u : 1u + __popc(c & 7u);
        } else { if (c >= 0xC0u) run = pd_run_push(run, c & 63u); p += 1; }
    }
}

// ---- (b) parent functions ---------------------------------------------------------------------------------------------------------------------------
// a record: val = byte per channel | flags << 24 (bit ch set: the channel IS val; clear: it is val + the same channel of colour ptr)
__device__ inline uint32_t pd_compose(uint32_t mine, uint32_t par) {        // mine's non-constant channels take their base from par
    uint32_t out = mine & 0xFF000000u;
    for (int ch = 0; ch < 3; ch++) {
        const uint32_t mv = (mine >> (8 * ch)) & 255u, pv = (par >> (8 * ch)) & 255u, bit = 1u << (24 + ch);
        if (mine & bit) out |= mv << (8 * ch);
        else { out |= ((mv + pv) & 255u) << (8 * ch); out |= par & bit; }
    }
    return out;
}
#define PD_ALLCONST 0x07000000u

__global__ __launch_bounds__(PD_CC) void yk_pd_parent_kernel(YkPdBufs B) {
    __shared__ uint32_t val[PD_CC + PD_BACK];
    __shared__ uint32_t ptr[PD_CC + PD_BACK];
    const uint32_t t = threadIdx.x, wg = blockIdx.x;
    const uint32_t sg = pd_find_seg<true>(B.segs, B.nSeg, wg);
    const YkPdSeg S = B.segs[sg];
    if (B.status[sg]) return;                                               // uniform: set by the link kernel, an earlier launch
    const uint32_t base = (wg - S.cWg0) * PD_CC, j = base + t, li = t + PD_BACK;
    const uint32_t hdr = pd_hdr(S);
    const uint32_t* tok = B.tokOff + S.colOff;
    uint32_t v = PD_ALLCONST, pp = 0;                                       // beyond the stream: a constant nobody refers to
    if (j == 0) v = PD_ALLCONST | pd_rd(S.src, S.n, hdr - 3) | (pd_rd(S.src, S.n, hdr - 2) << 8) | (pd_rd(S.src, S.n, hdr - 1) << 16);
    else if (j < S.N) {
        const uint32_t off = tok[j];
        const uint32_t bk = B.backInfo[S.colOff + j], back = bk & 255u, maxBack = bk >> 8;     // of the back-references in front of the token
        const uint32_t c = pd_rd(S.src, S.n, off);
        if (c < 0x80u) {
            const uint32_t row = 1u + 3u * c;                               // the rows are the bytes behind byte 0, whatever codeBookSize says
            v = pd_rd(S.src, S.n, row) | (pd_rd(S.src, S.n, row + 1) << 8) | (pd_rd(S.src, S.n, row + 2) << 16);
        } else {
            uint32_t q = off + 1;
            v = (c & 8u) ? (c & 7u) << 24 : 0u;                             // absolute: the flagged channels are constants
            for (uint32_t ch = 0; ch < 3; ch++) if (c & (1u << ch)) v |= pd_rd(S.src, S.n, q++) << (8 * ch);
        }
        if (maxBack > j) { atomicOr(&B.status[B.nSeg + sg], PD_ST_BACKREF); v = PD_ALLCONST; }
        else pp = li - back;                                                // >= 0: back <= 65, and back <= j in the first chunk
    }
    val[li] = v; ptr[li] = pp;
    if (t < PD_BACK) { val[t] = 0; ptr[t] = t; }                            // the halo: "itself, plus nothing"
    __syncthreads();
    for (int round = 0; round < 10; round++) {                              // 2^10 = PD_CC: the longest chain inside a chunk
        uint32_t nv = v, np = pp;
        if ((v & PD_ALLCONST) != PD_ALLCONST && pp >= PD_BACK) { nv = pd_compose(v, val[pp]); np = ptr[pp]; }
        __syncthreads();
        v = nv; pp = np;
        val[li] = v; ptr[li] = pp;
        __syncthreads();
    }
    if (j < S.N) { B.sumVal[S.colOff + j] = v; B.sumPtr[S.colOff + j] = (uint8_t)(pp < PD_BACK ? pp : 0u); }
}

// the records are fetched PD_CARRY_BATCH chunks at a time by the whole workgroup, so that the walk itself, one dependent step per chunk, runs out of LDS
#define PD_CARRY_BATCH 32
__global__ __launch_bounds__(256) void yk_pd_carry_kernel(YkPdBufs B) {
    __shared__ uint32_t sv[PD_CARRY_BATCH][PD_BACK];
    __shared__ uint8_t sp[PD_CARRY_BATCH][PD_BACK + 3];
    __shared__ uint32_t h[2][PD_BACK];
    const uint32_t t = threadIdx.x, sg = blockIdx.x;
    const YkPdSeg S = B.segs[sg];
    if (S.N == 0 || B.status[sg] || B.status[B.nSeg + sg]) return;
    const uint32_t nCc = (S.N + PD_CC - 1) / PD_CC;
    if (t < PD_BACK) h[0][t] = 0;                                           // chunk 0 resolves to constants: read, never used
    for (uint32_t k0 = 1; k0 < nCc; k0 += PD_CARRY_BATCH) {                 // the colours in front of chunk k are the last 65 of chunk k - 1
        const uint32_t nb = min((uint32_t)PD_CARRY_BATCH, nCc - k0);
        __syncthreads();
        for (uint32_t i = t; i < nb * PD_BACK; i += 256) {
            const uint32_t kk = i / PD_BACK, e = i % PD_BACK;
            const size_t at = (size_t)S.colOff + (size_t)(k0 + kk) * PD_CC - PD_BACK + e;      // < colOff + N: chunk k0 + kk exists
            sv[kk][e] = B.sumVal[at]; sp[kk][e] = B.sumPtr[at];
        }
        __syncthreads();
        for (uint32_t kk = 0; kk < nb; kk++) {                              // uniform trip count
            const uint32_t k = k0 + kk;
            const uint32_t* in = h[(k - 1) & 1]; uint32_t* out = h[k & 1];
            if (t < PD_BACK) { const uint32_t c = pd_compose(sv[kk][t], in[sp[kk][t]] | PD_ALLCONST) & 0xFFFFFFu; out[t] = c; sv[kk][t] = c; }
            __syncthreads();
        }
        for (uint32_t i = t; i < nb * PD_BACK; i += 256) B.halo[((size_t)S.cWg0 + k0 + i / PD_BACK) * PD_BACK + i % PD_BACK] = sv[i / PD_BACK][i % PD_BACK];
    }
}

__global__ __launch_bounds__(PD_CC) void yk_pd_apply_kernel(YkPdBufs B, uint8_t* __restrict__ out, uint32_t factor) {
    const uint32_t t = threadIdx.x, wg = blockIdx.x;
    const uint32_t sg = pd_find_seg<true>(B.segs, B.nSeg, wg);
    const YkPdSeg S = B.segs[sg];
    if (B.status[sg] || B.status[B.nSeg + sg]) return;
    const uint32_t k = wg - S.cWg0, j = k * PD_CC + t;
    if (j >= S.N) return;
    uint32_t v = B.sumVal[S.colOff + j];
    if ((v & PD_ALLCONST) != PD_ALLCONST) v = pd_compose(v, B.halo[(size_t)wg * PD_BACK + B.sumPtr[S.colOff + j]] | PD_ALLCONST);      // k >= 1 here
    uint8_t* dst = out + S.outOff + (size_t)j * 3;
    for (int ch = 0; ch < 3; ch++) {
        const uint32_t b = (v >> (8 * ch)) & 255u;
        dst[ch] = (uint8_t)(factor ? (b * factor) >> 16 : b);              // PaletteFullRangeRemapping, as yk_dec_remap_kernel
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------------------------
static int yk_pd_validate(yk_ctx* c, const uint8_t* const* dev, const size_t* payBytes, const size_t* outBytes, int nStreams, int remapRange) {
    if (!dev || !payBytes || !outBytes) return yk_refuse(c, YK_ERR_BAD_ARG, "devPayloads, payBytes or outBytes is NULL");
    if (nStreams < 1 || nStreams > PD_MAX_SEGS) return yk_refuse(c, YK_ERR_BAD_ARG, "nStreams must be 1..65536");
    if (remapRange < 0 || remapRange > 255) return yk_refuse(c, YK_ERR_BAD_ARG, "remapRange must be 0..255");
    size_t colours = 0, bytes = 0;
    for (int s = 0; s < nStreams; s++) {
        if (outBytes[s] % 3) return yk_refuse(c, YK_ERR_BAD_ARG, "an output length is not a multiple of 3 (plane-subset streams stay on the host coder)");
        if (outBytes[s] && (!payBytes[s] || !dev[s])) return yk_refuse(c, YK_ERR_BAD_ARG, "a stream has an output length and an empty payload or a NULL pointer");
        if (!outBytes[s]) continue;
        if (payBytes[s] > ((size_t)1 << 31)) return yk_refuse(c, YK_ERR_BAD_ARG, "more than 2^31 payload bytes in one call");
        colours += outBytes[s] / 3; bytes += payBytes[s];
        if (colours > PD_MAX_COLOURS) return yk_refuse(c, YK_ERR_BAD_ARG, "more than 2^28 colours in one call");
        if (bytes > ((size_t)1 << 31)) return yk_refuse(c, YK_ERR_BAD_ARG, "more than 2^31 payload bytes in one call");
    }
    return YK_OK;
}

// the caller has validated
static int yk_pd_run(yk_ctx* c, const uint8_t* const* dev, const size_t* payBytes, const size_t* outBytes, int nSeg, int remapRange) {
    YkPaletteDec& P = c->pdec;
    YK_HIP(c, hipSetDevice(c->device));
    // the stream table travels through the decoder's ring of pinned buffers (an event behind every copy): the call returns while the copy may
    // still be queued, and the next call must neither wait for it nor overwrite it
    int slot = 0; void* tabHost = nullptr;
    { int rc = yk_dec_table_host(c, (size_t)nSeg * sizeof(YkPdSeg), &slot, &tabHost); if (rc) return rc; }
    YkPdSeg* segs = static_cast<YkPdSeg*>(tabHost);
    std::vector<size_t> slotOff((size_t)nSeg), slotLen((size_t)nSeg);
    uint32_t nAWg = 0, nCWg = 0, nCol = 0; size_t outUsed = 0;
    for (int s = 0; s < nSeg; s++) {
        const uint32_t N = (uint32_t)(outBytes[s] / 3), n = N ? (uint32_t)payBytes[s] : 0u;
        segs[s] = YkPdSeg{ N ? dev[s] : nullptr, n, N, nAWg, 0u, nCWg, nCol, (uint32_t)(PD_MARGIN + outUsed), 0u };
        slotOff[(size_t)s] = PD_MARGIN + outUsed; slotLen[(size_t)s] = outBytes[s];
        if (!N) continue;
        // tokens start at hdr >= 4 and none starts at or beyond n + 385: chunks up to there, and one position beyond so that a walk that leaves
        // the last real chunk still meets the "exhausted" test
        segs[s].nAWg = (uint32_t)(((size_t)n + PD_SLACK + PD_WGCH * PD_CB - 1) / (PD_WGCH * PD_CB));
        nAWg += segs[s].nAWg; nCWg += (N + PD_CC - 1) / PD_CC; nCol += N;
        outUsed += (outBytes[s] + 15) & ~(size_t)15;
    }
    size_t cur = 0;
    auto place = [&](size_t bytes) { const size_t o = cur; cur = (cur + bytes + 255) & ~(size_t)255; return o; };
    const size_t oSeg = place((size_t)nSeg * sizeof(YkPdSeg)), oRec = place((size_t)nAWg * PD_WGCH * 16), oInfo = place((size_t)nAWg * PD_WGCH * 4);
    const size_t oTok = place((size_t)nCol * 4), oVal = place((size_t)nCol * 4), oPtr = place((size_t)nCol), oHalo = place((size_t)nCWg * PD_BACK * 4);
    const size_t oStat = place((size_t)nSeg * 8), oCb = place((size_t)nAWg * PD_WGCH * 4), oBk = place((size_t)nCol * 2);
    P.valid = false;
    YK_HIP(c, P.scratch.reserve(c->stream, cur));
    YK_HIP(c, P.out.reserve(c->stream, outUsed + 2 * PD_MARGIN));
    YkPdBufs B;
    B.segs = reinterpret_cast<const YkPdSeg*>(P.scratch + oSeg); B.nSeg = (uint32_t)nSeg;
    B.rec = reinterpret_cast<uint32_t*>(P.scratch + oRec); B.chunkInfo = reinterpret_cast<uint32_t*>(P.scratch + oInfo);
    B.tokOff = reinterpret_cast<uint32_t*>(P.scratch + oTok); B.sumVal = reinterpret_cast<uint32_t*>(P.scratch + oVal); B.sumPtr = P.scratch + oPtr;
    B.chunkBack = reinterpret_cast<uint32_t*>(P.scratch + oCb); B.backInfo = reinterpret_cast<uint16_t*>(P.scratch + oBk);
    B.halo = reinterpret_cast<uint32_t*>(P.scratch + oHalo); B.status = reinterpret_cast<uint32_t*>(P.scratch + oStat);
    { int rc = yk_dec_table_upload(c, slot, P.scratch + oSeg, (size_t)nSeg * sizeof(YkPdSeg)); if (rc) return rc; }
    { int rc = yk_stage_begin(c, YK_STAGE_PALETTE_DEC); if (rc) return rc; }
    if (nAWg) hipLaunchKernelGGL(yk_pd_walk_kernel, dim3(nAWg), dim3(256), 0, c->stream, B);
    hipLaunchKernelGGL(yk_pd_link_kernel, dim3((unsigned)nSeg), dim3(256), 0, c->stream, B);
    if (nAWg) {
        hipLaunchKernelGGL(yk_pd_mark_kernel, dim3(nAWg), dim3(256), 0, c->stream, B);
        hipLaunchKernelGGL(yk_pd_parent_kernel, dim3(nCWg), dim3(PD_CC), 0, c->stream, B);
        hipLaunchKernelGGL(yk_pd_carry_kernel, dim3((unsigned)nSeg), dim3(256), 0, c->stream, B);
        hipLaunchKernelGGL(yk_pd_apply_kernel, dim3(nCWg), dim3(PD_CC), 0, c->stream, B, P.out,
                           remapRange > 0 ? (uint32_t)((255u << 16) / (uint32_t)remapRange) : 0u);
    }
    YK_HIP(c, hipGetLastError());
    { int rc = yk_stage_end(c, YK_STAGE_PALETTE_DEC); if (rc) return rc; }
    P.slotOff.swap(slotOff); P.slotLen.swap(slotLen); P.statusOff = oStat; P.nSeg = nSeg; P.valid = true;
    return YK_OK;
}

extern "C" {

int yk_palette_decompress_streams(yk_ctx* c, const uint8_t* const* devPayloads, const size_t* payBytes, const size_t* outBytes, int nStreams, int remapRange) {
    if (!c) return YK_ERR_BAD_ARG;
    { int rc = yk_pd_validate(c, devPayloads, payBytes, outBytes, nStreams, remapRange); if (rc) return rc; }
    return yk_pd_run(c, devPayloads, payBytes, outBytes, nStreams, remapRange);
}

int yk_palette_decoded_device(yk_ctx* c, int index, const uint8_t** dev, size_t* nBytes) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!dev || !nBytes) return yk_refuse(c, YK_ERR_BAD_ARG, "dev or nBytes is NULL");
    if (!c->pdec.valid) return yk_refuse(c, YK_ERR_STATE, "yk_palette_decompress_streams first");
    if (index < 0 || index >= c->pdec.nSeg) return yk_refuse(c, YK_ERR_BAD_ARG, "stream index out of range");
    const size_t n = c->pdec.slotLen[(size_t)index];
    *dev = n ? c->pdec.out + c->pdec.slotOff[(size_t)index] : nullptr; *nBytes = n;
    return YK_OK;
}

int yk_palette_decoded(yk_ctx* c, int index, uint8_t* hostOut, size_t cap, size_t* nBytes) {
    if (!c) return YK_ERR_BAD_ARG;
    const uint8_t* dev = nullptr; size_t n = 0;
    { int rc = yk_palette_decoded_device(c, index, &dev, &n); if (rc) return rc; }
    if (nBytes) *nBytes = n;
    if (!hostOut) return YK_OK;                                         // size query
    if (cap < n) return yk_refuse(c, YK_ERR_RANGE, "output buffer too small");
    if (n) {
        YK_HIP(c, hipSetDevice(c->device));
        YK_HIP(c, hipMemcpyAsync(hostOut, dev, n, hipMemcpyDeviceToHost, c->stream));
        YK_HIP(c, hipStreamSynchronize(c->stream));
    }
    return YK_OK;
}

int yk_palette_decode_status(yk_ctx* c, int32_t* out) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!out) return yk_refuse(c, YK_ERR_BAD_ARG, "out is NULL");
    if (!c->pdec.valid) return yk_refuse(c, YK_ERR_STATE, "yk_palette_decompress_streams first");
    YK_HIP(c, hipSetDevice(c->device));
    YkPaletteDec& P = c->pdec;
    P.statusHost.resize((size_t)P.nSeg * 2);
    YK_HIP(c, hipMemcpyAsync(P.statusHost.data(), P.scratch + P.statusOff, (size_t)P.nSeg * 8, hipMemcpyDeviceToHost, c->stream));
    YK_HIP(c, hipStreamSynchronize(c->stream));
    for (int s = 0; s < P.nSeg; s++) out[s] = (int32_t)(P.statusHost[(size_t)s] | P.statusHost[(size_t)P.nSeg + s]);
    return YK_OK;
}

int yk_decode_gradient_palette(yk_ctx* c, int sx, int sy, const uint8_t* bitmap, size_t bitmapBytes, const uint8_t* payload, size_t payloadBytes,
                               size_t rgbBytes, int colorCompression) {
    if (!c) return YK_ERR_BAD_ARG;
    if (!bitmap || !bitmapBytes) return yk_refuse(c, YK_ERR_BAD_ARG, "NULL or empty tile bitmap");
    if (!yk_dec_begun(c)) return yk_refuse(c, YK_ERR_STATE, "yk_decode_begin first");
    YK_DEC_NO_PREPARED(c, "yk_decode_gradient_palette");                        // before the palette decode, not only in the pass behind it
    YK_DEC_NO_BATCH_WINDOWS(c, "yk_decode_gradient_palette");
    if (colorCompression < 0 || colorCompression > 255) return yk_refuse(c, YK_ERR_BAD_ARG, "colorCompression must be 0..255");
    if (rgbBytes && !payload) return yk_refuse(c, YK_ERR_BAD_ARG, "a stream has an output length and an empty payload or a NULL pointer");
    YkPaletteDec& P = c->pdec;
    YK_HIP(c, hipSetDevice(c->device));
    const size_t oPay = (bitmapBytes + 15) & ~(size_t)15;
    YK_HIP(c, P.stage.reserve(c->stream, oPay + payloadBytes + 16));
    const uint8_t* devPay = P.stage + oPay;
    { int rc = yk_pd_validate(c, &devPay, &payloadBytes, &rgbBytes, 1, colorCompression); if (rc) return rc; }
    YK_HIP(c, hipMemcpyAsync(P.stage, bitmap, bitmapBytes, hipMemcpyHostToDevice, c->stream));
    if (payloadBytes) YK_HIP(c, hipMemcpyAsync(P.stage + oPay, payload, payloadBytes, hipMemcpyHostToDevice, c->stream));
    { int rc = yk_pd_run(c, &devPay, &payloadBytes, &rgbBytes, 1, colorCompression ? colorCompression : 1); if (rc) return rc; }   // range 0 divides like 1 in the reference
    int32_t st = 0;
    { int rc = yk_palette_decode_status(c, &st); if (rc) return rc; }       // synchronises: the host buffers have been read
    if (st) return yk_refuse(c, YK_ERR_BAD_ARG, "malformed 'GTIL' colour payload (PaletteDecompressor rejects it)");
    const uint8_t* devRgb = nullptr; size_t n = 0;
    { int rc = yk_palette_decoded_device(c, 0, &devRgb, &n); if (rc) return rc; }
    { int rc = yk_decode_gradient_device(c, sx, sy, P.stage, bitmapBytes, devRgb, n, 0); if (rc) return rc; }
    YK_HIP(c, hipStreamSynchronize(c->stream));                             // like yk_decode_gradient: the pass is done when the call returns
    return YK_OK;
}

}  // extern "C"
