// va_jpeg_decode.hip -- batched baseline JPEG decoding behind video.ops.jpeg_decode and
// video.io.backend_mjpeg.VideoMJPEG (the reference reads its frames one by one through cv2.VideoCapture.read,
// VideoOpenCV.get_frame, video/io/backend_opencv.py, behind load_any_video, video/io/file.py:37-46).  The decoder is
// pinned in DESIGN.md §9, "Motion-JPEG decoding"; the serial arithmetic is va_jpeg_decode_math.h, the same text the
// host tests compile.
//
// Every restart interval of every frame is an independent entropy segment, and everything behind the entropy decode
// is per block.  One flow serves the four layouts (monochrome; 3 components with luma 1 x 1, 2 x 1 (4:2:2) or 2 x 2
// (4:2:0) and chroma 1 x 1; DESIGN.md §9, "Subsampled Motion-JPEG decoding"): the MCU grid of a frame is worked out
// once (JpegGrid), and a chunk of frames takes these launches on one stream:
//   locate       one workgroup per frame walks the frame's entropy bytes in tiles of 2048, 8 bytes a lane: the
//                markers FF xx (xx not 00, FF) get their rank in the frame from ballots' popcounts scanned over the
//                workgroup; the k-th one ends segment k and, while it is RST(k mod 8), begins segment k + 1.  The
//                first other marker ends the scan.  Fills the chunk's table of nseg (begin, end) byte ranges (-1: a
//                missing segment) and stores the frame's status word, the marker-sequence bit or 0.
//   entropy      one lane per segment, one kernel instantiated per layout: va_jpeg::decode_block over the segment's
//                MCUs with a 64-bit bit buffer and the tables in LDS; the coefficients go to the workspace as int16 in
//                natural order where va_jpeg::mcu_block_at puts the block, [frame][Y: by V x bx H blocks | Cb: by x bx
//                | Cr: by x bx][64] (for 1 x 1 that is [frame][component][block row][block column][64]), a zeroed
//                block (16-byte stores) and then its non-zero entries.  An error zeroes its block and the rest of the
//                segment and is ORed into the frame's status word.
// and then, for a monochrome or 1 x 1 file, one more:
//   reconstruct  one lane per MCU: dequantise, both inverse passes and the colour conversion in registers; the lanes
//                of a wave hold neighbouring MCUs of a block row, so each of the 8 pixel rows goes out as 8 (or 24)
//                contiguous bytes a lane, 512 (1536) bytes a wave, where the row is complete and aligned, and
//                bytewise at the frame's edges (store_row).
// or, for a 4:2:2 or 4:2:0 file, two, because the triangle filter reads chroma samples of neighbouring MCUs:
//   chroma planes  one lane per chroma block: its 64 samples as eight 8-byte rows of [frame][2][by 8][bx 8] bytes
//   pixels         one lane per luma block, the lanes of a wave along a block row: the Y block's samples, the 6 x 6
//                  (4:2:0) or 8 x 6 (4:2:2) chroma samples around its quarter or half of the chroma block, clamped to
//                  the real samples, the upsampling and the colour conversion; the pixel rows go out through the same
//                  store_row
// The only atomic is the OR into the status word, whose result does not depend on the order; every output byte
// depends on its frame alone.  Loops over stream bytes end at the segment's end, loops over blocks at the segment's
// MCU range.  A frame without restart markers is one segment and one lane here; launch_jpeg_decode_split further
// down gives it one lane per subsequence of its bytes ("split segments").
#include <limits.h>

#include "va_common.h"
#include "va_jpeg_decode_math.h"
#include "va_scan.h"

static_assert(sizeof(va_jpeg::HuffDecode) == VA_JPEG_HUFF_DECODE_BYTES, "the table size is part of the ABI");

namespace va {

namespace {

constexpr int kLocBlock = 256;
constexpr int kLocWaves = kLocBlock / kWave;
constexpr int kLocPer = 8;                               // bytes a lane looks at
constexpr int kLocTile = kLocBlock * kLocPer;
constexpr int kEntBlock = kWave;
constexpr int kRecBlock = 256;

__device__ __forceinline__ long long wave_min_ll(long long v)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const long long u = __shfl_xor(v, d, kWave);
        v = u < v ? u : v;
    }
    return v;
}

// table[f][k] = (begin, end) of segment k of frame f as offsets into `bytes`; status[f] = the marker-sequence bit
__global__ void __launch_bounds__(kLocBlock)
jpeg_locate_kernel(const uint8_t *__restrict__ bytes, const int64_t *__restrict__ offsets,
                   const int64_t *__restrict__ scan_begin, int nseg, int64_t *__restrict__ table,
                   int32_t *__restrict__ status)
{
    __shared__ int32_t wave_count[2][kLocWaves];
    __shared__ long long wave_bad[2][kLocWaves];
    __shared__ int32_t terminator;

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t f = blockIdx.x;
    const int64_t fb = offsets[f], fe = offsets[f + 1] > fb ? offsets[f + 1] : fb;
    int64_t sb = scan_begin[f];
    sb = fb + (sb < 0 ? 0 : sb > fe - fb ? fe - fb : sb);
    int64_t *tab = table + 2 * f * nseg;
    for (int k = tid; k < nseg; k += kLocBlock) {
        tab[2 * k] = k == 0 ? sb : -1;
        tab[2 * k + 1] = -1;
    }
    if (tid == 0)
        terminator = -1;
    __syncthreads();

    constexpr long long kNone = LLONG_MAX;
    long long carry = 0, nfound = 0;                     // markers before this tile
    bool stopped = false;
    int par = 0;
    for (int64_t base = sb; base < fe; base += kLocTile, par ^= 1) {
        const int64_t p0 = base + (int64_t)kLocPer * tid;
        uint32_t b[kLocPer + 1];
#pragma unroll
        for (int i = 0; i <= kLocPer; i++)
            b[i] = p0 + i < fe ? bytes[p0 + i] : 0u;
        uint32_t mask = 0;
#pragma unroll
        for (int i = 0; i < kLocPer; i++)
            if (b[i] == 0xFFu && b[i + 1] != 0u && b[i + 1] != 0xFFu)
                mask |= 1u << i;
        const int mine = __popc(mask);
        const int incl = wave_inclusive(mine, lane);
        if (lane == kWave - 1)
            wave_count[par][wave] = incl;
        __syncthreads();
        int before = 0, tile = 0;
#pragma unroll
        for (int k = 0; k < kLocWaves; k++) {
            before += k < wave ? wave_count[par][k] : 0;
            tile += wave_count[par][k];
        }
        if (tile == 0)
            continue;
        const long long first = carry + before + incl - mine;
        long long bad = kNone, k = first;
#pragma unroll
        for (int i = 0; i < kLocPer; i++)
            if (mask >> i & 1u) {
                if (b[i + 1] != 0xD0u + (uint32_t)(k & 7) && bad == kNone)
                    bad = k;
                k++;
            }
        bad = wave_min_ll(bad);
        if (lane == 0)
            wave_bad[par][wave] = bad;
        __syncthreads();
        long long kbad = kNone;
#pragma unroll
        for (int i = 0; i < kLocWaves; i++)
            kbad = wave_bad[par][i] < kbad ? wave_bad[par][i] : kbad;
        k = first;
#pragma unroll
        for (int i = 0; i < kLocPer; i++)
            if (mask >> i & 1u) {
                if (k <= kbad) {
                    if (k < nseg)
                        tab[2 * k + 1] = p0 + i;
                    if (k < kbad && k + 1 < nseg)
                        tab[2 * (k + 1)] = p0 + i + 2;
                    if (k == kbad)
                        terminator = (int32_t)b[i + 1];
                }
                k++;
            }
        if (kbad != kNone) {
            stopped = true;
            nfound = kbad + 1;
            break;
        }
        carry += tile;
    }
    __syncthreads();
    if (tid == 0) {
        if (!stopped) {                                  // the file ends inside the last segment
            nfound = carry + 1;
            if (carry < nseg)
                tab[2 * carry + 1] = fe;
        }
        const bool good = stopped && terminator == 0xD9 && nfound == nseg;
        status[f] = good ? 0 : va_jpeg::kStatusMarker;
    }
}

struct EntropyArgs {
    const uint8_t *bytes;
    const int64_t *table;
    const va_jpeg::HuffDecode *huff;     // [c][2]: the DC and the AC table of each component
    int16_t *coef;
    int32_t *status;
    int64_t nsegs;                       // segments of the chunk
    int nseg, ri, bx, by;
    const int32_t *skip;                 // kSkip: per frame, not 0 where the frame is already decoded
};

// the 2 * C tables into LDS, by the whole workgroup
template <int C>
__device__ __forceinline__ void stage_tables(va_jpeg::HuffDecode *tabs, const va_jpeg::HuffDecode *huff)
{
    static_assert(sizeof(va_jpeg::HuffDecode) % 4 == 0, "the tables are copied as words");
    constexpr int words = 2 * C * (int)sizeof(va_jpeg::HuffDecode) / 4;
    const uint32_t *src = reinterpret_cast<const uint32_t *>(huff);
    uint32_t *dst = reinterpret_cast<uint32_t *>(tabs);
    for (int i = threadIdx.x; i < words; i += kEntBlock)
        dst[i] = src[i];
    __syncthreads();
}

// C components, luma LH x LV, chroma 1 x 1; a.bx, a.by count MCUs of 8 LH x 8 LV pixels, and a monochrome MCU is its
// one block.  An error zeroes its block and every later block of the segment; the MCU's earlier blocks keep their
// coefficients.
template <int C, int LH, int LV, bool kSkip = false>
__global__ void __launch_bounds__(kEntBlock) jpeg_entropy_kernel(EntropyArgs a)
{
    static_assert(C == 3 || (C == 1 && LH == 1 && LV == 1), "one component has no sampling");
    constexpr int kBlocks = C == 1 ? 1 : va_jpeg::mcu_blocks(LH, LV);
    __shared__ va_jpeg::HuffDecode tabs[2 * C];
    stage_tables<C>(tabs, a.huff);
    const int64_t s = (int64_t)blockIdx.x * kEntBlock + threadIdx.x;
    if (s >= a.nsegs)
        return;
    const int64_t f = s / a.nseg;
    if constexpr (kSkip)
        if (a.skip[f])
            return;
    const int j = (int)(s % a.nseg);
    const int64_t begin = a.table[2 * s], end = a.table[2 * s + 1];
    const int64_t mcus = (int64_t)a.bx * a.by;
    const int64_t m0 = (int64_t)j * a.ri, m1 = m0 + a.ri < mcus ? m0 + a.ri : mcus;
    bool dead = begin < 0 || end < begin;
    int32_t st = 0;
    va_jpeg::BitReader r = va_jpeg::open_bits(a.bytes, dead ? 0 : begin, dead ? 0 : end);
    int pred[C];
#pragma unroll
    for (int ch = 0; ch < C; ch++)
        pred[ch] = 0;
    int16_t *frame = a.coef + ((f * kBlocks * mcus) << 6);
    for (int64_t m = m0; m < m1; m++) {
        const int64_t row = m / a.bx, col = m % a.bx;
#pragma unroll
        for (int k = 0; k < kBlocks; k++) {
            int comp = 0;
            int16_t *blk = frame + (va_jpeg::mcu_block_at(k, LH, LV, a.by, a.bx, row, col, comp) << 6);
            // 1 x 1: the same address as [frame][component][by][bx][64] spells it.  From the line above the compiler
            // makes other code for these two instantiations (no division in the monochrome one), which measured 0.1
            // to 0.4 % slower where the entropy launch decides the time
            if constexpr (LH * LV == 1)
                blk = a.coef + ((((f * C + k) * a.by + row) * a.bx + col) << 6);
            uint4 *blk16 = reinterpret_cast<uint4 *>(blk);
#pragma unroll
            for (int i = 0; i < 8; i++)
                blk16[i] = make_uint4(0, 0, 0, 0);
            if (dead)
                continue;
            const int32_t e = va_jpeg::decode_block(r, tabs[2 * comp], tabs[2 * comp + 1], pred[comp],
                                                    [&](int i, int v) { blk[i] = (int16_t)v; });
            if (e) {
                st = e;
                dead = true;
#pragma unroll
                for (int i = 0; i < 8; i++)
                    blk16[i] = make_uint4(0, 0, 0, 0);
            }
        }
    }
    if (st)
        atomicOr(&a.status[f], st);
}

struct ReconArgs {
    const int16_t *coef;
    const uint8_t *qtables;              // [c][64], natural order
    uint8_t *out;
    int64_t nmcus;                       // MCUs of the chunk
    int h, w, bx, by;
};

struct BlockBytes {
    uint32_t w[16];
};

// the 64 samples of one block as bytes in natural order.  Not inlined: a colour MCU calls it three times, and with the
// three transforms scheduled into one another the kernel needs more registers than the vector file holds
__device__ __noinline__ BlockBytes block_samples(const int16_t *__restrict__ coef, const uint8_t *q)
{
    const uint4 *src = reinterpret_cast<const uint4 *>(coef);
    int16_t cf[64];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint4 v = src[i];
        const uint32_t word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            cf[8 * i + 2 * k] = (int16_t)(word[k] & 0xFFFFu);
            cf[8 * i + 2 * k + 1] = (int16_t)(word[k] >> 16);
        }
    }
    uint8_t smp[64];
    va_jpeg::inverse_block(cf, q, smp);
    BlockBytes out;
#pragma unroll
    for (int i = 0; i < 16; i++)
        out.w[i] = (uint32_t)smp[4 * i] | (uint32_t)smp[4 * i + 1] << 8 | (uint32_t)smp[4 * i + 2] << 16
                   | (uint32_t)smp[4 * i + 3] << 24;
    return out;
}

// a row of 8 pixels of C bytes each, as words
template <int C>
struct RowWords {
    uint32_t w[2 * C];
};

// pixel x of a row of RGB pixels that started as zeros
__device__ __forceinline__ void pack_rgb(RowWords<3> &o, int x, int r, int g, int b)
{
    o.w[(3 * x) / 4] |= (uint32_t)r << (8 * ((3 * x) % 4));
    o.w[(3 * x + 1) / 4] |= (uint32_t)g << (8 * ((3 * x + 1) % 4));
    o.w[(3 * x + 2) / 4] |= (uint32_t)b << (8 * ((3 * x + 2) % 4));
}

// the row o to dst, the pixel of column x0 of a row of w pixels: as 8-byte stores where the row holds all 8 pixels and
// dst is 8-byte aligned, bytewise up to the row's end otherwise.  o comes by value: behind a reference the compiler
// keeps an array of jpeg_pixels_kernel<2> in memory (12 KB of LDS a workgroup) that otherwise lives in registers
template <int C>
__device__ __forceinline__ void store_row(uint8_t *dst, const RowWords<C> o, int x0, int w)
{
    if (x0 + 8 <= w && ((uintptr_t)dst & 7) == 0) {
#pragma unroll
        for (int i = 0; i < C; i++)
            reinterpret_cast<uint2 *>(dst)[i] = make_uint2(o.w[2 * i], o.w[2 * i + 1]);
    } else {
#pragma unroll
        for (int i = 0; i < 8 * C; i++)
            if (x0 + i / C < w)
                dst[i] = (uint8_t)(o.w[i / 4] >> (8 * (i % 4)));
    }
}

template <int C>
__global__ void __launch_bounds__(kRecBlock) jpeg_reconstruct_kernel(ReconArgs a)
{
    __shared__ uint8_t qt[C][64];
    for (int i = threadIdx.x; i < C * 64; i += kRecBlock)
        qt[i / 64][i % 64] = a.qtables[i];
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * kRecBlock + threadIdx.x;
    if (idx >= a.nmcus)
        return;
    const int64_t per = (int64_t)a.bx * a.by;
    const int64_t f = idx / per;
    const int row = (int)((idx % per) / a.bx), col = (int)((idx % per) % a.bx);

    uint32_t px[C][16];                  // per component the 64 samples as bytes, natural order
#pragma unroll
    for (int ch = 0; ch < C; ch++) {
        const BlockBytes blk = block_samples(a.coef + ((((f * C + ch) * a.by + row) * a.bx + col) << 6), qt[ch]);
#pragma unroll
        for (int i = 0; i < 16; i++)
            px[ch][i] = blk.w[i];
    }

    const int x0 = col * 8;
#pragma unroll
    for (int y = 0; y < 8; y++) {
        const int gy = row * 8 + y;
        if (gy >= a.h)
            break;
        RowWords<C> o = {};
        if constexpr (C == 1) {
            o.w[0] = px[0][2 * y];
            o.w[1] = px[0][2 * y + 1];
        } else {
#pragma unroll
            for (int x = 0; x < 8; x++) {
                const int sh = 8 * (x & 3), wi = 2 * y + (x >> 2);
                int r, g, b;
                va_jpeg::rgb_of((int)(px[0][wi] >> sh & 255u), (int)(px[1][wi] >> sh & 255u),
                                (int)(px[2][wi] >> sh & 255u), r, g, b);
                pack_rgb(o, x, r, g, b);
            }
        }
        store_row<C>(a.out + ((f * a.h + gy) * a.w + x0) * C, o, x0, a.w);
    }
}

struct PlaneArgs {
    const int16_t *coef;
    const uint8_t *qtables;              // [3][64], natural order
    uint8_t *planes;                     // [frame][2][by * 8][bx * 8]
    int64_t nblocks;                     // chroma blocks of the chunk
    int bx, by, luma;                    // MCUs of the frame, luma blocks of an MCU
};

__global__ void __launch_bounds__(kRecBlock) jpeg_chroma_planes_kernel(PlaneArgs a)
{
    __shared__ uint8_t qt[2][64];
    for (int i = threadIdx.x; i < 2 * 64; i += kRecBlock)
        qt[i / 64][i % 64] = a.qtables[64 + i];
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * kRecBlock + threadIdx.x;
    if (idx >= a.nblocks)
        return;
    const int64_t mcus = (int64_t)a.bx * a.by;
    const int64_t f = idx / (2 * mcus);
    const int comp = (int)((idx % (2 * mcus)) / mcus);
    const int row = (int)((idx % mcus) / a.bx), col = (int)((idx % mcus) % a.bx);
    const BlockBytes blk = block_samples(a.coef + (((f * (a.luma + 2) + a.luma + comp) * mcus + idx % mcus) << 6),
                                         qt[comp]);
    const int64_t stride = (int64_t)a.bx * 8;
    uint8_t *dst = a.planes + ((f * 2 + comp) * a.by * 8 + row * 8) * stride + col * 8;
#pragma unroll
    for (int y = 0; y < 8; y++)
        *reinterpret_cast<uint2 *>(dst + y * stride) = make_uint2(blk.w[2 * y], blk.w[2 * y + 1]);
}

struct PixelArgs {
    const int16_t *coef;
    const uint8_t *qtables;
    const uint8_t *planes;
    uint8_t *out;
    int64_t nblocks;                     // luma blocks of the chunk
    int h, w, bx, by;                    // bx, by: MCUs
};

// luma 2 x LV.  The lane of luma block (R, C) writes the pixels 8R .. 8R + 7 x 8C .. 8C + 7; their chroma samples are
// the columns 4C .. 4C + 3 and the rows 4R .. 4R + 3 (LV == 2) or 8R .. 8R + 7 (LV == 1), and the triangle reads one
// more on each side.  Every one is fetched as the nearest real sample, so the padding of the planes is never used.
template <int LV>
__global__ void __launch_bounds__(kRecBlock) jpeg_pixels_kernel(PixelArgs a)
{
    constexpr int kLuma = 2 * LV, kRows = LV == 2 ? 6 : 8;
    __shared__ uint8_t qt[64];
    for (int i = threadIdx.x; i < 64; i += kRecBlock)
        qt[i] = a.qtables[i];
    __syncthreads();
    const int64_t idx = (int64_t)blockIdx.x * kRecBlock + threadIdx.x;
    if (idx >= a.nblocks)
        return;
    const int lbx = a.bx * 2;
    const int64_t mcus = (int64_t)a.bx * a.by, per = mcus * kLuma;
    const int64_t f = idx / per;
    const int row = (int)((idx % per) / lbx), col = (int)((idx % per) % lbx);
    const BlockBytes luma = block_samples(a.coef + ((f * (kLuma + 2) * mcus + idx % per) << 6), qt);

    const int cw = (a.w + 1) / 2, ch = (a.h + LV - 1) / LV;
    const bool tri = va_jpeg::triangle_used(cw);
    const int64_t stride = (int64_t)a.bx * 8;
    // per component and chroma row the six samples of the columns 4C - 1 .. 4C + 4: four in lo, two in hi
    uint32_t lo[2][kRows], hi[2][kRows];
#pragma unroll
    for (int comp = 0; comp < 2; comp++) {
        const uint8_t *plane = a.planes + (f * 2 + comp) * a.by * 8 * stride;
#pragma unroll
        for (int k = 0; k < kRows; k++) {
            const uint8_t *src = plane + va_jpeg::nearest_sample(LV == 2 ? 4 * row - 1 + k : 8 * row + k, ch) * stride;
            const uint32_t mid = *reinterpret_cast<const uint32_t *>(src + 4 * col);
            uint32_t s[6];
            s[0] = src[va_jpeg::nearest_sample(4 * col - 1, cw)];
#pragma unroll
            for (int i = 1; i < 5; i++) {
                s[i] = mid >> (8 * (i - 1)) & 255u;
                if (4 * col - 1 + i > cw - 1)
                    s[i] = s[i - 1];
            }
            s[5] = src[va_jpeg::nearest_sample(4 * col + 4, cw)];
            lo[comp][k] = s[0] | s[1] << 8 | s[2] << 16 | s[3] << 24;
            hi[comp][k] = s[4] | s[5] << 8;
        }
    }

    const int x0 = col * 8;
#pragma unroll
    for (int y = 0; y < 8; y++) {
        const int gy = row * 8 + y;
        if (gy >= a.h)
            break;
        // the local chroma row of this pixel row and the one it blends with (LV == 2: the rows start at 4R - 1)
        const int own = LV == 2 ? 1 + (y >> 1) : y, other = LV == 2 ? va_jpeg::blend_sample(y + 2, kRows, true) : y;
        int s[2][6];
#pragma unroll
        for (int comp = 0; comp < 2; comp++) {
            const uint32_t blo = tri ? lo[comp][other] : lo[comp][own], bhi = tri ? hi[comp][other] : hi[comp][own];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const int sh = 8 * (i & 3);
                const int v = (int)((i < 4 ? lo[comp][own] : hi[comp][own]) >> sh & 255u);
                s[comp][i] = LV == 2 ? va_jpeg::upsample_rows(v, (int)((i < 4 ? blo : bhi) >> sh & 255u)) : v;
            }
        }
        RowWords<3> o = {};
#pragma unroll
        for (int x = 0; x < 8; x++) {
            const int mine = 1 + (x >> 1), next = va_jpeg::blend_sample(x + 2, 6, true);
            const int cb = va_jpeg::upsample_columns(s[0][mine], tri ? s[0][next] : s[0][mine], x, LV);
            const int cr = va_jpeg::upsample_columns(s[1][mine], tri ? s[1][next] : s[1][mine], x, LV);
            int r, g, b;
            va_jpeg::rgb_of((int)(luma.w[2 * y + (x >> 2)] >> (8 * (x & 3)) & 255u), cb, cr, r, g, b);
            pack_rgb(o, x, r, g, b);
        }
        store_row<3>(a.out + ((f * a.h + gy) * a.w + x0) * 3, o, x0, a.w);
    }
}


// the MCU grid of a frame: by x bx MCUs of 8 lh x 8 lv pixels in nseg restart intervals; an MCU holds `blocks`
// blocks, the first `luma` of them Y (a monochrome MCU is one block)
struct JpegGrid {
    int by, bx;
    int64_t mcus;
    int nseg, blocks, luma;
};

JpegGrid jpeg_grid(int h, int w, int c, int ri, int lh, int lv)
{
    JpegGrid g;
    g.by = (h + 8 * lv - 1) / (8 * lv);
    g.bx = (w + 8 * lh - 1) / (8 * lh);
    g.mcus = (int64_t)g.by * g.bx;
    g.nseg = (int)((g.mcus + ri - 1) / ri);
    g.luma = lh * lv;
    g.blocks = c == 1 ? 1 : va_jpeg::mcu_blocks(lh, lv);
    return g;
}

// [segment table | coefficients | chroma planes (subsampled files only)]
struct DecodeLayout {
    size_t table, coef, planes, total;
};

DecodeLayout decode_layout(int64_t n, const JpegGrid &g)
{
    Carve carve;
    DecodeLayout l;
    l.table = carve.take((size_t)n * g.nseg * 2 * sizeof(int64_t));
    l.coef = carve.take((size_t)n * g.blocks * g.mcus * 64 * sizeof(int16_t));
    l.planes = carve.total;
    if (g.luma > 1)
        l.planes = carve.take((size_t)n * 2 * g.mcus * 64);
    l.total = carve.total;
    return l;
}

// the frames of one chunk: as many as the workspace holds, and no more than one launch's grid takes (the largest
// grid has one lane per 8 x 8 block of the frame)
int64_t jpeg_decode_chunk(int n, const JpegGrid &g, size_t workspace_bytes)
{
    const int64_t grid_cap = (((int64_t)1 << 31) - kRecBlock) / (g.mcus * g.luma);
    const int64_t most = n < grid_cap ? n : grid_cap;
    if (most < 1 || decode_layout(most, g).total <= workspace_bytes)
        return most;
    // k frames need at most k times one frame's regions, and a little less: each region rounds up once
    const size_t one = decode_layout(1, g).total;
    int64_t k = (int64_t)(workspace_bytes / one);
    k = k < most ? k : most;
    while (k < most && decode_layout(k + 1, g).total <= workspace_bytes)
        k++;
    return k;
}

// ------------------------------------------------------------------------------------------------ split segments
// DESIGN.md §9, "Split Motion-JPEG decoding": a frame without restart markers is one segment; its raw bytes are cut
// into subsequences of `sub` bytes and every subsequence gets a lane.  Per chunk, behind locate (nseg = 1):
//   scan         max_rounds launches of one lane per subsequence (va_jpeg::scan_lane): round 1 from the truth (lane
//                0) or a guess, round r + 1 from the predecessor's exit of round r (the exits are double-buffered,
//                so the rounds are Jacobi iterations and their number does not depend on the schedule).  A lane
//                whose entry did not change copies its exit on and returns; a workgroup of such lanes does not even
//                stage the tables.
//   check        one workgroup per frame: converged iff every entry is the predecessor's last exit; the exclusive
//                scans over the frame's lanes of the blocks begun and of the DC sums per component; the frame's
//                rounds; the error word reset.
//   (memset)     the chunk's coefficients to zero: a block that straddles two lanes has two writers
//   write        one lane per subsequence of a converged frame: va_jpeg::write_lane from its entry, its block index
//                and its predictors into the coefficients' usual places; an error goes as atomicMin of (block in
//                decode order, status bit) into the frame's 64-bit error word and ends the lane
//   seal         zeroes every block from the error's block on (16-byte stores, through mcu_block_at) and ORs the
//                error's one status bit into the frame's word
//   fallback     jpeg_entropy_kernel with the per-frame skip flag: one lane for each frame that did not converge or
//                is longer than max_bytes
// and then the reconstruction launches as above.  Besides the OR, the atomics are the minimum of the error word and
// a maximum in LDS; both results do not depend on the order.
struct SplitArgs {
    const uint8_t *bytes;
    const int64_t *table;
    const va_jpeg::HuffDecode *huff;
    va_jpeg::ScanState *entry, *exits;   // [frame][lane]; exits: two of them, of the odd and of the even rounds
    int32_t *begun, *last;               // blocks begun in the lane; the last round in which the lane ran
    uint32_t *dc, *pred;                 // [..][3]: the lane's DC sums; the sums in front of the lane
    int64_t *start;                      // blocks begun in front of the lane
    int32_t *converged;                  // per frame
    unsigned long long *err;             // per frame: va_jpeg::error_word
    int32_t *rounds_out;                 // may be NULL
    int16_t *coef;
    int32_t *status;
    int64_t lanes, per, max_bytes;       // lanes of the chunk, of a frame; a longer frame has none
    int sub, round, max_rounds, bx, by;
};

// the segment of frame f and the number of its lanes (0: not scanned)
__device__ __forceinline__ int64_t split_span(const SplitArgs &a, int64_t f, int64_t &b, int64_t &e)
{
    b = a.table[2 * f];
    e = a.table[2 * f + 1];
    if (b < 0 || e < b)
        b = e = 0;
    return e - b > a.max_bytes ? 0 : va_jpeg::subsequences(e - b, a.sub);
}

template <int C, int LH, int LV>
__global__ void __launch_bounds__(kEntBlock) jpeg_split_scan_kernel(SplitArgs a)
{
    constexpr int kBlocks = C == 1 ? 1 : va_jpeg::mcu_blocks(LH, LV);
    __shared__ va_jpeg::HuffDecode tabs[2 * C];
    const int64_t g = (int64_t)blockIdx.x * kEntBlock + threadIdx.x;
    bool run = false;
    int64_t b = 0, e = 0, stop = 0;
    va_jpeg::ScanState entry = va_jpeg::scan_end();
    va_jpeg::ScanState *now = a.exits + (a.round & 1) * a.lanes, *before = a.exits + ((a.round - 1) & 1) * a.lanes;
    if (g < a.lanes) {
        const int64_t i = g % a.per, count = split_span(a, g / a.per, b, e);
        if (i < count) {
            stop = i + 1 == count ? e : b + (i + 1) * a.sub;
            entry = i == 0         ? va_jpeg::scan_state(b, 0, 0, 0)
                    : a.round == 1 ? va_jpeg::scan_guess(a.bytes, b, b + i * a.sub)
                                   : before[g - 1];
            run = a.round == 1 || !va_jpeg::same_state(entry, a.entry[g]);
            if (!run)
                now[g] = before[g];
        }
    }
    if (!__syncthreads_or(run))
        return;
    stage_tables<C>(tabs, a.huff);
    if (!run)
        return;
    const va_jpeg::ScanLane r = va_jpeg::scan_lane(a.bytes, e, entry, stop, tabs, kBlocks, LH * LV);
    a.entry[g] = entry;
    now[g] = r.exit;
    a.begun[g] = r.begun;
    a.last[g] = a.round;
#pragma unroll
    for (int ch = 0; ch < 3; ch++)
        a.dc[3 * g + ch] = r.dc[ch];
}

__global__ void __launch_bounds__(kRecBlock) jpeg_split_check_kernel(SplitArgs a)
{
    constexpr int kRecWaves = kRecBlock / kWave;
    __shared__ long long part64[kRecWaves];
    __shared__ uint32_t part32[kRecWaves];
    __shared__ int32_t rounds;
    const int64_t f = blockIdx.x;
    int64_t b, e;
    const int64_t count = a.max_rounds > 0 ? split_span(a, f, b, e) : 0;
    if (threadIdx.x == 0)
        rounds = 0;
    __syncthreads();
    const va_jpeg::ScanState *exits = a.exits + (a.max_rounds & 1) * a.lanes;
    long long carry = 0;
    uint32_t carry_dc[3] = {0, 0, 0};
    bool good = true;
    int32_t mine = 0;
    for (int64_t i0 = 0; i0 < count; i0 += kRecBlock) {
        const int64_t i = i0 + threadIdx.x, g = f * a.per + i;
        const bool in = i < count;
        if (in) {
            good = good && (i == 0 || va_jpeg::same_state(a.entry[g], exits[g - 1]));
            mine = a.last[g] > mine ? a.last[g] : mine;
        }
        long long total = 0;
        const long long at = block_exclusive<kRecWaves>(in ? (long long)a.begun[g] : 0, part64, total);
        if (in)
            a.start[g] = carry + at;
        carry += total;
#pragma unroll
        for (int ch = 0; ch < 3; ch++) {
            uint32_t sum = 0;
            const uint32_t front = block_exclusive<kRecWaves>(in ? (uint32_t)a.dc[3 * g + ch] : 0u, part32, sum);
            if (in)
                a.pred[3 * g + ch] = carry_dc[ch] + front;
            carry_dc[ch] += sum;
        }
    }
    atomicMax(&rounds, mine);
    const bool all = __syncthreads_and(good) && count > 0;
    if (threadIdx.x == 0) {
        a.converged[f] = all;
        a.err[f] = va_jpeg::kNoError;
        if (a.rounds_out)
            a.rounds_out[f] = all ? rounds : -1;
    }
}

template <int C, int LH, int LV>
__global__ void __launch_bounds__(kEntBlock) jpeg_split_write_kernel(SplitArgs a)
{
    constexpr int kBlocks = C == 1 ? 1 : va_jpeg::mcu_blocks(LH, LV);
    __shared__ va_jpeg::HuffDecode tabs[2 * C];
    const int64_t g = (int64_t)blockIdx.x * kEntBlock + threadIdx.x;
    const int64_t f = g / a.per, i = g % a.per;
    int64_t b = 0, e = 0, count = 0;
    if (g < a.lanes && a.converged[f])
        count = split_span(a, f, b, e);
    const bool run = i < count;
    if (!__syncthreads_or(run))
        return;
    stage_tables<C>(tabs, a.huff);
    if (!run)
        return;
    const int64_t mcus = (int64_t)a.bx * a.by, total = mcus * kBlocks;
    int16_t *frame = a.coef + ((f * total) << 6), *blk = nullptr;
    int64_t at = -1, block = a.start[g];
    uint32_t pred[3] = {a.pred[3 * g], a.pred[3 * g + 1], a.pred[3 * g + 2]};
    const bool last = i + 1 == count;
    const int32_t st = va_jpeg::write_lane(
        a.bytes, e, a.entry[g], last ? e : b + (i + 1) * a.sub, last, tabs, kBlocks, LH * LV, total, block, pred,
        [&](int64_t cur, int idx, int v) {              // cur < total
            if (cur != at) {
                const int64_t m = cur / kBlocks;
                int comp = 0;
                at = cur;
                blk = frame + (va_jpeg::mcu_block_at((int)(cur % kBlocks), LH, LV, a.by, a.bx, m / a.bx, m % a.bx, comp) << 6);
            }
            blk[idx] = (int16_t)v;
        });
    if (st)
        atomicMin(&a.err[f], (unsigned long long)va_jpeg::error_word(block, st));
}

// one lane per block of the chunk; a workgroup lies in one frame
template <int C, int LH, int LV>
__global__ void __launch_bounds__(kRecBlock) jpeg_split_seal_kernel(SplitArgs a, int64_t groups)
{
    constexpr int kBlocks = C == 1 ? 1 : va_jpeg::mcu_blocks(LH, LV);
    const int64_t f = blockIdx.x / groups;
    const unsigned long long word = a.err[f];
    if (word == va_jpeg::kNoError)
        return;
    const int64_t mcus = (int64_t)a.bx * a.by, total = mcus * kBlocks;
    const int64_t cur = (blockIdx.x % groups) * kRecBlock + threadIdx.x;
    if (cur == 0)
        a.status[f] |= (int32_t)(word & 15u);
    if (cur >= total || cur < (int64_t)(word >> 4))
        return;
    const int64_t m = cur / kBlocks;
    int comp = 0;
    uint4 *blk16 = reinterpret_cast<uint4 *>(
        a.coef + ((f * total + va_jpeg::mcu_block_at((int)(cur % kBlocks), LH, LV, a.by, a.bx, m / a.bx, m % a.bx, comp)) << 6));
#pragma unroll
    for (int k = 0; k < 8; k++)
        blk16[k] = make_uint4(0, 0, 0, 0);
}

// behind decode_layout's regions (nseg = 1): [converged | error words | entries | exits | begun | last | dc | pred |
// start], per frame `per` lanes
struct SplitLayout {
    DecodeLayout d;
    size_t converged, err, entry, exits, begun, last, dc, pred, start, total;
};

SplitLayout split_layout(int64_t n, const JpegGrid &g, int64_t per)
{
    SplitLayout l;
    l.d = decode_layout(n, g);
    Carve carve;
    carve.total = l.d.total;
    const size_t lanes = (size_t)n * (size_t)per;
    l.converged = carve.take((size_t)n * sizeof(int32_t));
    l.err = carve.take((size_t)n * sizeof(unsigned long long));
    l.entry = carve.take(lanes * sizeof(va_jpeg::ScanState));
    l.exits = carve.take(2 * lanes * sizeof(va_jpeg::ScanState));
    l.begun = carve.take(lanes * sizeof(int32_t));
    l.last = carve.take(lanes * sizeof(int32_t));
    l.dc = carve.take(3 * lanes * sizeof(uint32_t));
    l.pred = carve.take(3 * lanes * sizeof(uint32_t));
    l.start = carve.take(lanes * sizeof(int64_t));
    l.total = carve.total;
    return l;
}

int64_t split_lanes(int sub, int64_t max_bytes) { return va_jpeg::subsequences(max_bytes, sub); }

// as jpeg_decode_chunk, and no more frames than the scan's and the seal's grids take
int64_t jpeg_split_chunk(int n, const JpegGrid &g, int64_t per, size_t workspace_bytes)
{
    const int64_t room = ((int64_t)1 << 31) - kRecBlock;
    const int64_t groups = (g.mcus * g.blocks + kRecBlock - 1) / kRecBlock;
    int64_t most = room / (g.mcus * g.luma);
    most = most < room / per ? most : room / per;
    most = most < room / groups ? most : room / groups;
    most = most < n ? most : n;
    if (most < 1 || split_layout(most, g, per).total <= workspace_bytes)
        return most;
    const size_t one = split_layout(1, g, per).total;
    int64_t k = (int64_t)(workspace_bytes / one);
    k = k < most ? k : most;
    while (k < most && split_layout(k + 1, g, per).total <= workspace_bytes)
        k++;
    return k;
}

template <int C, int LH, int LV>
int launch_split_entropy(SplitArgs a, EntropyArgs e, int64_t frames, int64_t mcus, hipStream_t st)
{
    constexpr int kBlocks = C == 1 ? 1 : va_jpeg::mcu_blocks(LH, LV);
    const dim3 lanes((unsigned)((a.lanes + kEntBlock - 1) / kEntBlock));
    for (a.round = 1; a.round <= a.max_rounds; a.round++) {
        hipLaunchKernelGGL((jpeg_split_scan_kernel<C, LH, LV>), lanes, dim3(kEntBlock), 0, st, a);
        VA_LAUNCH_CHECK("jpeg_split_scan_kernel");
    }
    hipLaunchKernelGGL(jpeg_split_check_kernel, dim3((unsigned)frames), dim3(kRecBlock), 0, st, a);
    VA_LAUNCH_CHECK("jpeg_split_check_kernel");
    if (a.max_rounds > 0) {
        VA_HIP(hipMemsetAsync(a.coef, 0, (size_t)frames * kBlocks * mcus * 64 * sizeof(int16_t), st));
        hipLaunchKernelGGL((jpeg_split_write_kernel<C, LH, LV>), lanes, dim3(kEntBlock), 0, st, a);
        VA_LAUNCH_CHECK("jpeg_split_write_kernel");
        const int64_t groups = (mcus * kBlocks + kRecBlock - 1) / kRecBlock;
        hipLaunchKernelGGL((jpeg_split_seal_kernel<C, LH, LV>), dim3((unsigned)(frames * groups)), dim3(kRecBlock), 0, st,
                           a, groups);
        VA_LAUNCH_CHECK("jpeg_split_seal_kernel");
    }
    hipLaunchKernelGGL((jpeg_entropy_kernel<C, LH, LV, true>), dim3((unsigned)((frames + kEntBlock - 1) / kEntBlock)),
                       dim3(kEntBlock), 0, st, e);
    VA_LAUNCH_CHECK("jpeg_entropy_kernel");
    return VA_OK;
}

bool jpeg_sampling_taken(int c, int lh, int lv)
{
    return (lh == 1 && lv == 1) || (c == 3 && lh == 2 && (lv == 1 || lv == 2));
}

constexpr int64_t kJpegSplitMaxScanBytes = (int64_t)1 << 40;
bool jpeg_split_sub_taken(int sub) { return sub >= 16 && sub <= 65536 && sub % 16 == 0; }

// both decode entries: `what` names the one that was called
int jpeg_decode_entry(const char *what, const uint8_t *bytes, const int64_t *offsets, const int64_t *scan_begin, int n,
                      int h, int w, int c, int ri, int lh, int lv, const uint8_t *qtables, const void *huff,
                      int huff_bytes, uint8_t *frames_out, int32_t *status_out, void *workspace, int64_t workspace_bytes,
                      void *stream)
{
    VA_ENTER();
    VA_REQUIRE(n >= 0 && h > 0 && w > 0 && ri > 0 && workspace_bytes >= 0,
               "%s: negative or zero size (n %d, h %d, w %d, ri %d, workspace %lld)", what, n, h, w, ri,
               (long long)workspace_bytes);
    VA_REQUIRE(c == 1 || c == 3, "%s: channels must be 1 or 3, got %d", what, c);
    VA_REQUIRE(jpeg_sampling_taken(c, lh, lv),
               "%s: luma sampling %d x %d with %d channel(s); 1 x 1, and with 3 channels 2 x 1 and 2 x 2, are decoded",
               what, lh, lv, c);
    if (n == 0)
        return VA_OK;
    VA_REQUIRE(bytes && offsets && scan_begin && qtables && huff && frames_out && status_out && workspace,
               "%s: NULL argument", what);
    VA_REQUIRE(aligned(offsets, 8) && aligned(scan_begin, 8) && aligned(huff, 4) && aligned(status_out, 4)
                   && aligned(workspace, 16),
               "%s: offsets and scan_begin must be 8-byte aligned, the tables and the status 4-byte, "
               "the workspace 16-byte", what);
    VA_REQUIRE(h <= 65535 && w <= 65535, "%s: SOF0 holds 16-bit sizes, got %d x %d", what, w, h);
    VA_REQUIRE(huff_bytes == 2 * c * VA_JPEG_HUFF_DECODE_BYTES,
               "%s: the Huffman tables of %d component(s) are %d bytes, got %d", what, c,
               2 * c * VA_JPEG_HUFF_DECODE_BYTES, huff_bytes);
    const JpegGrid g = jpeg_grid(h, w, c, ri, lh, lv);
    const int64_t chunk = jpeg_decode_chunk(n, g, (size_t)workspace_bytes);
    if (chunk < 1) {
        set_error("%s: a workspace of %lld bytes does not hold one frame (%lld bytes)", what,
                  (long long)workspace_bytes, (long long)decode_layout(1, g).total);
        return VA_ERR_RANGE;
    }
    hipStream_t st = as_stream(stream);
    const DecodeLayout l = decode_layout(chunk, g);
    int64_t *table = at<int64_t>(workspace, l.table);
    int16_t *coef = at<int16_t>(workspace, l.coef);
    uint8_t *planes = at<uint8_t>(workspace, l.planes);
    void (*const entropy)(EntropyArgs) = c == 1    ? jpeg_entropy_kernel<1, 1, 1>
                                         : lv == 2 ? jpeg_entropy_kernel<3, 2, 2>
                                         : lh == 2 ? jpeg_entropy_kernel<3, 2, 1>
                                                   : jpeg_entropy_kernel<3, 1, 1>;
    const auto blocks_of = [](int64_t lanes) { return dim3((unsigned)((lanes + kRecBlock - 1) / kRecBlock)); };
    for (int64_t f0 = 0; f0 < n; f0 += chunk) {
        const int64_t k = chunk < n - f0 ? chunk : n - f0;
        uint8_t *frames = frames_out + (size_t)f0 * h * w * c;
        hipLaunchKernelGGL(jpeg_locate_kernel, dim3((unsigned)k), dim3(kLocBlock), 0, st, bytes, offsets + f0,
                           scan_begin + f0, g.nseg, table, status_out + f0);
        VA_LAUNCH_CHECK("jpeg_locate_kernel");
        const EntropyArgs e{bytes, table, static_cast<const va_jpeg::HuffDecode *>(huff), coef, status_out + f0,
                            k * g.nseg, g.nseg, ri, g.bx, g.by, nullptr};
        hipLaunchKernelGGL(entropy, dim3((unsigned)((e.nsegs + kEntBlock - 1) / kEntBlock)), dim3(kEntBlock), 0, st, e);
        VA_LAUNCH_CHECK("jpeg_entropy_kernel");
        if (g.luma == 1) {
            const ReconArgs r{coef, qtables, frames, k * g.mcus, h, w, g.bx, g.by};
            if (c == 1)
                hipLaunchKernelGGL(jpeg_reconstruct_kernel<1>, blocks_of(r.nmcus), dim3(kRecBlock), 0, st, r);
            else
                hipLaunchKernelGGL(jpeg_reconstruct_kernel<3>, blocks_of(r.nmcus), dim3(kRecBlock), 0, st, r);
            VA_LAUNCH_CHECK("jpeg_reconstruct_kernel");
            continue;
        }
        const PlaneArgs cp{coef, qtables, planes, k * 2 * g.mcus, g.bx, g.by, g.luma};
        hipLaunchKernelGGL(jpeg_chroma_planes_kernel, blocks_of(cp.nblocks), dim3(kRecBlock), 0, st, cp);
        VA_LAUNCH_CHECK("jpeg_chroma_planes_kernel");
        const PixelArgs p{coef, qtables, planes, frames, k * g.mcus * g.luma, h, w, g.bx, g.by};
        if (lv == 2)
            hipLaunchKernelGGL(jpeg_pixels_kernel<2>, blocks_of(p.nblocks), dim3(kRecBlock), 0, st, p);
        else
            hipLaunchKernelGGL(jpeg_pixels_kernel<1>, blocks_of(p.nblocks), dim3(kRecBlock), 0, st, p);
        VA_LAUNCH_CHECK("jpeg_pixels_kernel");
    }
    return VA_OK;
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

size_t va_jpeg_decode_workspace_bytes(int n, int h, int w, int c, int ri)
{
    if (n <= 0 || h <= 0 || w <= 0 || h > 65535 || w > 65535 || (c != 1 && c != 3) || ri <= 0)
        return 0;
    return decode_layout(n, jpeg_grid(h, w, c, ri, 1, 1)).total;
}

int va_jpeg_decode_u8(const uint8_t *bytes, const int64_t *offsets, const int64_t *scan_begin, int n, int h, int w, int c,
                      int ri, const uint8_t *qtables, const void *huff, int huff_bytes, uint8_t *frames_out,
                      int32_t *status_out, void *workspace, int64_t workspace_bytes, void *stream)
{
    return jpeg_decode_entry("va_jpeg_decode_u8", bytes, offsets, scan_begin, n, h, w, c, ri, 1, 1, qtables, huff,
                             huff_bytes, frames_out, status_out, workspace, workspace_bytes, stream);
}

size_t va_jpeg_decode_sampled_workspace_bytes(int n, int h, int w, int c, int ri, int luma_h, int luma_v)
{
    if (n <= 0 || h <= 0 || w <= 0 || h > 65535 || w > 65535 || (c != 1 && c != 3) || ri <= 0
        || !jpeg_sampling_taken(c, luma_h, luma_v))
        return 0;
    return decode_layout(n, jpeg_grid(h, w, c, ri, luma_h, luma_v)).total;
}

int va_jpeg_decode_sampled_u8(const uint8_t *bytes, const int64_t *offsets, const int64_t *scan_begin, int n, int h,
                              int w, int c, int ri, int luma_h, int luma_v, const uint8_t *qtables, const void *huff,
                              int huff_bytes, uint8_t *frames_out, int32_t *status_out, void *workspace,
                              int64_t workspace_bytes, void *stream)
{
    return jpeg_decode_entry("va_jpeg_decode_sampled_u8", bytes, offsets, scan_begin, n, h, w, c, ri, luma_h, luma_v,
                             qtables, huff, huff_bytes, frames_out, status_out, workspace, workspace_bytes, stream);
}

size_t va_jpeg_decode_split_workspace_bytes(int n, int h, int w, int c, int luma_h, int luma_v, int sub_bytes,
                                            int64_t max_scan_bytes)
{
    if (n <= 0 || h <= 0 || w <= 0 || h > 65535 || w > 65535 || (c != 1 && c != 3)
        || !jpeg_sampling_taken(c, luma_h, luma_v) || !jpeg_split_sub_taken(sub_bytes) || max_scan_bytes < 0
        || max_scan_bytes > kJpegSplitMaxScanBytes)
        return 0;
    const JpegGrid g = jpeg_grid(h, w, c, INT_MAX, luma_h, luma_v);
    return split_layout(n, g, split_lanes(sub_bytes, max_scan_bytes)).total;
}

int va_jpeg_decode_split_u8(const uint8_t *bytes, const int64_t *offsets, const int64_t *scan_begin, int n, int h, int w,
                            int c, int luma_h, int luma_v, const uint8_t *qtables, const void *huff, int huff_bytes,
                            uint8_t *frames_out, int32_t *status_out, void *workspace, int64_t workspace_bytes,
                            int sub_bytes, int max_rounds, int64_t max_scan_bytes, int32_t *rounds_out, void *stream)
{
    const char *what = "va_jpeg_decode_split_u8";
    VA_ENTER();
    VA_REQUIRE(n >= 0 && h > 0 && w > 0 && workspace_bytes >= 0,
               "%s: negative or zero size (n %d, h %d, w %d, workspace %lld)", what, n, h, w, (long long)workspace_bytes);
    VA_REQUIRE(c == 1 || c == 3, "%s: channels must be 1 or 3, got %d", what, c);
    VA_REQUIRE(jpeg_sampling_taken(c, luma_h, luma_v),
               "%s: luma sampling %d x %d with %d channel(s); 1 x 1, and with 3 channels 2 x 1 and 2 x 2, are decoded",
               what, luma_h, luma_v, c);
    if (n == 0)
        return VA_OK;
    VA_REQUIRE(bytes && offsets && scan_begin && qtables && huff && frames_out && status_out && workspace,
               "%s: NULL argument", what);
    VA_REQUIRE(aligned(offsets, 8) && aligned(scan_begin, 8) && aligned(huff, 4) && aligned(status_out, 4)
                   && aligned(workspace, 16) && aligned(rounds_out, 4),
               "%s: offsets and scan_begin must be 8-byte aligned, the tables, the status and the rounds 4-byte, "
               "the workspace 16-byte", what);
    VA_REQUIRE(h <= 65535 && w <= 65535, "%s: SOF0 holds 16-bit sizes, got %d x %d", what, w, h);
    VA_REQUIRE(huff_bytes == 2 * c * VA_JPEG_HUFF_DECODE_BYTES,
               "%s: the Huffman tables of %d component(s) are %d bytes, got %d", what, c,
               2 * c * VA_JPEG_HUFF_DECODE_BYTES, huff_bytes);
    VA_REQUIRE(jpeg_split_sub_taken(sub_bytes), "%s: sub_bytes must be a multiple of 16 in 16 .. 65536, got %d", what,
               sub_bytes);
    VA_REQUIRE(max_rounds >= 0, "%s: max_rounds must not be negative, got %d", what, max_rounds);
    VA_REQUIRE(max_scan_bytes >= 0 && max_scan_bytes <= kJpegSplitMaxScanBytes,
               "%s: max_scan_bytes must lie in 0 .. 2^40, got %lld", what, (long long)max_scan_bytes);
    const JpegGrid g = jpeg_grid(h, w, c, INT_MAX, luma_h, luma_v);              // one segment a frame
    const int64_t per = split_lanes(sub_bytes, max_scan_bytes);
    const int64_t chunk = jpeg_split_chunk(n, g, per, (size_t)workspace_bytes);
    if (chunk < 1) {
        set_error("%s: a workspace of %lld bytes does not hold one frame (%lld bytes)", what, (long long)workspace_bytes,
                  (long long)split_layout(1, g, per).total);
        return VA_ERR_RANGE;
    }
    hipStream_t st = as_stream(stream);
    const SplitLayout l = split_layout(chunk, g, per);
    int64_t *table = at<int64_t>(workspace, l.d.table);
    int16_t *coef = at<int16_t>(workspace, l.d.coef);
    uint8_t *planes = at<uint8_t>(workspace, l.d.planes);
    const auto blocks_of = [](int64_t lanes) { return dim3((unsigned)((lanes + kRecBlock - 1) / kRecBlock)); };
    for (int64_t f0 = 0; f0 < n; f0 += chunk) {
        const int64_t k = chunk < n - f0 ? chunk : n - f0;
        uint8_t *frames = frames_out + (size_t)f0 * h * w * c;
        hipLaunchKernelGGL(jpeg_locate_kernel, dim3((unsigned)k), dim3(kLocBlock), 0, st, bytes, offsets + f0,
                           scan_begin + f0, 1, table, status_out + f0);
        VA_LAUNCH_CHECK("jpeg_locate_kernel");
        const va_jpeg::HuffDecode *tabs = static_cast<const va_jpeg::HuffDecode *>(huff);
        SplitArgs a{};
        a.bytes = bytes, a.table = table, a.huff = tabs;
        a.entry = at<va_jpeg::ScanState>(workspace, l.entry), a.exits = at<va_jpeg::ScanState>(workspace, l.exits);
        a.begun = at<int32_t>(workspace, l.begun), a.last = at<int32_t>(workspace, l.last);
        a.dc = at<uint32_t>(workspace, l.dc), a.pred = at<uint32_t>(workspace, l.pred);
        a.start = at<int64_t>(workspace, l.start);
        a.converged = at<int32_t>(workspace, l.converged), a.err = at<unsigned long long>(workspace, l.err);
        a.rounds_out = rounds_out ? rounds_out + f0 : nullptr;
        a.coef = coef, a.status = status_out + f0;
        a.lanes = k * per, a.per = per, a.max_bytes = max_scan_bytes;
        a.sub = sub_bytes, a.round = 0, a.max_rounds = max_rounds, a.bx = g.bx, a.by = g.by;
        const EntropyArgs e{bytes, table, tabs, coef, status_out + f0, k, 1,
                            (int)(g.mcus < INT_MAX ? g.mcus : INT_MAX), g.bx, g.by, a.converged};
        const int rc = c == 1        ? launch_split_entropy<1, 1, 1>(a, e, k, g.mcus, st)
                       : luma_v == 2 ? launch_split_entropy<3, 2, 2>(a, e, k, g.mcus, st)
                       : luma_h == 2 ? launch_split_entropy<3, 2, 1>(a, e, k, g.mcus, st)
                                     : launch_split_entropy<3, 1, 1>(a, e, k, g.mcus, st);
        if (rc)
            return rc;
        if (g.luma == 1) {
            const ReconArgs r{coef, qtables, frames, k * g.mcus, h, w, g.bx, g.by};
            if (c == 1)
                hipLaunchKernelGGL(jpeg_reconstruct_kernel<1>, blocks_of(r.nmcus), dim3(kRecBlock), 0, st, r);
            else
                hipLaunchKernelGGL(jpeg_reconstruct_kernel<3>, blocks_of(r.nmcus), dim3(kRecBlock), 0, st, r);
            VA_LAUNCH_CHECK("jpeg_reconstruct_kernel");
            continue;
        }
        const PlaneArgs cp{coef, qtables, planes, k * 2 * g.mcus, g.bx, g.by, g.luma};
        hipLaunchKernelGGL(jpeg_chroma_planes_kernel, blocks_of(cp.nblocks), dim3(kRecBlock), 0, st, cp);
        VA_LAUNCH_CHECK("jpeg_chroma_planes_kernel");
        const PixelArgs p{coef, qtables, planes, frames, k * g.mcus * g.luma, h, w, g.bx, g.by};
        if (luma_v == 2)
            hipLaunchKernelGGL(jpeg_pixels_kernel<2>, blocks_of(p.nblocks), dim3(kRecBlock), 0, st, p);
        else
            hipLaunchKernelGGL(jpeg_pixels_kernel<1>, blocks_of(p.nblocks), dim3(kRecBlock), 0, st, p);
        VA_LAUNCH_CHECK("jpeg_pixels_kernel");
    }
    return VA_OK;
}

}  // extern "C"
