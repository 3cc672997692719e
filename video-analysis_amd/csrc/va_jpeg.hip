// va_jpeg.hip -- batched baseline JPEG encoding behind video.io.backend_mjpeg.VideoWriterMJPEG (the reference writes
// its frames through cv2.VideoWriter, video/io/backend_opencv.py:240-242, behind write_video, video/io/file.py:50-64).
// The stream is pinned in DESIGN.md §9, "Motion-JPEG"; the per-block arithmetic is va_jpeg_math.h, the same text the
// host tests compile.
//
// One MCU row of one frame is an independent entropy segment (DRI = one MCU row), so the call has the library's
// counts-then-scan shape over n * ceil(h / 8) segments, three launches on one stream:
//   count  one workgroup per segment: encodes the segment and keeps only its byte length, stuffing included
//   scan   one workgroup: the int64 exclusive prefix over [header | RSTm] + segment + [EOI] of every segment; the
//          frames' offsets and sizes and the total
//   write  one workgroup per segment: the same encoding again, stored at the segment's final offset.  Nothing is
//          stored when the total exceeds the capacity.
// The segment is encoded twice in place of keeping its coefficients: a frame is read twice (its bytes are a small
// part of what the encoder computes) and the call needs no workspace that grows with the pixels.
//
// A segment is walked in chunks of 32 MCUs, so its length is not bounded by LDS.  Per chunk:
//   A   each wave loads 8 MCUs, 8 (or 24) bytes of a pixel row per lane, converts colour and transforms block after
//       block with one lane per sample: the row and column sums and the zigzag order are lane exchanges.  In a
//       subsampled layout (va_jpeg_encode_sampled_u8; DESIGN.md §9, "Subsampled Motion-JPEG encoding") a segment is
//       8 V pixel rows and a chunk 24 (4:2:2) or 16 (4:2:0) MCUs of 16 pixels' width; a wave loads 8 V rows of 64 / V
//       pixels, 4 / V MCUs, at a time, box-averages Cb and Cr in the lane and, for 4:2:0, with the lane of the
//       neighbouring row, and gathers the samples of every block of the MCU from the lanes that hold them
//   B1  one lane per coefficient: the length of its bit string (va_jpeg::coefficient_bits; with tables made on the
//       device, whose codes have up to 16 bits, its two strings of up to 48 + 27 bits), summed per block
//   --  a scan of the blocks' bit counts gives every block its bit position behind the chunk's carry
//   B2  the same strings again, ORed into the chunk's bit buffer in LDS at block position + lane prefix
//   E   the complete 32-bit words (all bytes, padded with 1-bits, in the last chunk) go out in tiles of 256 words:
//       a workgroup scan of bytes + 0xFF counts places each word's stuffed bytes; the unfinished word is the next
//       chunk's carry
// The LDS atomics of B2 only OR disjoint bits into shared words: the result does not depend on their order, and
// every byte written depends on its segment alone.
//
// va_jpeg_encode_optimized_u8 ("Optimised Huffman tables") writes the same stream with Huffman tables
// made for the call, six steps on one stream with no host synchronisation between them:
//   zero      the call's counts, int64 [class][dc | ac][256]
//   histogram one workgroup per segment: phase A as above, then one lane per coefficient adds the symbols of its string
//             (va_jpeg::coefficient_symbols) to a histogram in LDS, and the workgroup adds the non-zero entries to the
//             call's counts.  Integer atomics only: the counts do not depend on the order
//   tables    one workgroup, a wave per table: the code sizes (va_jpeg::huff_code_sizes over 64 lanes: two arg-min
//             reductions and a parallel update per merge), BITS and HUFFVAL, the encoder's entries, and the header
//             with its DHT segments and its length
//   count, scan, write   as above, with the tables, the header and its length read from device memory.  The count
//             adds the header's length to the length of a frame's first segment, so the scan is the plain one
#include "va_common.h"
#include "va_jpeg_math.h"
#include "va_scan.h"

namespace va {

namespace {

constexpr int kJpegBlock = 256;
constexpr int kJpegWaves = kJpegBlock / kWave;
constexpr int kGroupMcus = 8;                          // MCUs a wave loads at once
constexpr int kChunkMcus = kGroupMcus * kJpegWaves;    // MCUs of a chunk of 1 x 1 sampling
// MCUs of a chunk: at most 128 blocks, two entries a lane of the block-position scan; the subsampled layouts keep the
// 96 blocks of 4:4:4, and with them its LDS
constexpr int chunk_mcus(int hs, int vs) { return hs == 1 ? kChunkMcus : vs == 1 ? 24 : 16; }
constexpr int mcu_blocks(int c, int hs, int vs) { return c == 1 ? 1 : hs * vs + 2; }
// a block has at most 22 + 63 * 26 bits: a DC string of 11 + 11, and an AC coefficient behind a run r adds at most
// 11 (r / 16) + 26 bits over its r + 1 lanes
constexpr int kMaxBlockBits = 22 + 63 * 26;
// with tables made on the device a code has up to 16 bits: a DC string of 16 + 11, and an AC coefficient behind a run r
// adds at most 16 (r / 16) + 26 bits over its r + 1 lanes, an EOB 16 on its one
constexpr int kMaxBlockBitsDevice = 27 + 63 * 26;
// words of a chunk's bit buffer: its blocks, the carry, the padding, and put_bits' reach
constexpr int bit_words(int blocks, int block_bits = kMaxBlockBits) { return (blocks * block_bits + 31 + 7) / 32 + 3; }
constexpr int kScanBlock = 256;
constexpr int kScanPerThread = 4;

struct JpegArgs {
    const uint8_t *frames;
    int n, h, w;
    int nseg, mcus;                  // segments of a frame, MCUs of a segment
    const uint8_t *qtables;          // [2][64], natural order
    const uint8_t *header;
    int header_bytes;
    int32_t *seg_len;                // [n * nseg]
    const int64_t *seg_start;        // [n * nseg + 1]
    const int64_t *totals;
    uint8_t *out;
    int64_t cap;
    // the optimised call: the encoder's entries [4][256] (DC0, AC0, DC1, AC1), the header's length, the call's counts
    const uint32_t *huff;
    const int32_t *header_len;
    unsigned long long *freq;
};

// how a segment kernel gets its Huffman tables, or that it counts symbols for them
enum { kHuffAnnexK = 0, kHuffDevice = 1, kHuffCount = 2 };

// the 8 pixels x0 .. x0 + 7 of row y as bytes; columns beyond the frame repeat the last one
template <int C>
__device__ __forceinline__ void load_pixels(const uint8_t *row, int x0, int w, uint32_t (&px)[2 * C])
{
    const uint8_t *p = row + (int64_t)x0 * C;
    if (x0 + 8 <= w && ((uintptr_t)p & 7) == 0) {
#pragma unroll
        for (int i = 0; i < C; i++) {
            const uint2 v = *reinterpret_cast<const uint2 *>(p + 8 * i);
            px[2 * i] = v.x;
            px[2 * i + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 2 * C; i++)
            px[i] = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int x = x0 + i < w ? x0 + i : w - 1;
#pragma unroll
            for (int ch = 0; ch < C; ch++)
                px[(i * C + ch) / 4] |= (uint32_t)row[(int64_t)x * C + ch] << (8 * ((i * C + ch) % 4));
        }
    }
}

// one block, lane = 8 y + x holding its sample minus 128: the lane's coefficient in zigzag order, quantised by q[]
__device__ __forceinline__ int16_t transform_block(int sample, const int (&t_row)[8], const int (&t_col)[8],
                                                   const uint8_t *q, int zz_from, int lane)
{
    int sum = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
        sum += t_row[i] * __shfl(sample, (lane & ~7) | i, kWave);
    const int rows = va_jpeg::row_round(sum);            // lane = 8 y + k
    sum = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
        sum += t_col[i] * __shfl(rows, 8 * i + (lane & 7), kWave);
    const int v = va_jpeg::quantise(sum, q[lane]);       // lane = 8 v + k
    return (int16_t)__shfl(v, zz_from, kWave);
}

// C components with luma sampling HS x VS: <1, 1, 1> monochrome, <3, 1, 1> 4:4:4, <3, 2, 1> 4:2:2, <3, 2, 2> 4:2:0
template <int C, int HS, int VS, bool WRITE, int HUFF = kHuffAnnexK>
__global__ void __launch_bounds__(kJpegBlock) jpeg_segment_kernel(JpegArgs a)
{
    static_assert(!(WRITE && HUFF == kHuffCount), "the histogram writes no stream");
    static_assert(C == 3 ? (HS == 1 || HS == 2) && (VS == 1 || VS == HS) : C == 1 && HS == 1 && VS == 1, "layout");
    constexpr int HV = HS * VS, BPM = mcu_blocks(C, HS, VS);         // luma blocks and all blocks of an MCU
    constexpr int kMcus = chunk_mcus(HS, VS), kBlocks = kMcus * BPM;
    static_assert(kBlocks <= 2 * kWave, "the block-position scan takes two entries a lane");
    constexpr int kBitWords = bit_words(kBlocks, HUFF == kHuffDevice ? kMaxBlockBitsDevice : kMaxBlockBits);
    constexpr int CG = 8 / VS;           // 8-pixel column groups a wave loads at once: lane = CG * row + group
    __shared__ int16_t coef[kBlocks][64];
    __shared__ uint32_t bitbuf[kBitWords];
    __shared__ uint32_t huff_dc[2][16], huff_ac[2][256];
    __shared__ uint8_t qt[2][64];
    __shared__ int32_t block_bits[kBlocks];
    __shared__ int32_t wave_total[kJpegWaves];
    __shared__ int32_t pred[3];
    __shared__ uint32_t chunk_end;
    __shared__ uint32_t hist[HUFF == kHuffCount ? 4 * 256 : 1];

    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t seg = blockIdx.x;
    const int frame = (int)(seg / a.nseg), j = (int)(seg % a.nseg);
    if (WRITE && a.totals[0] > a.cap)
        return;

    if constexpr (HUFF == kHuffCount) {
        for (int i = tid; i < 4 * 256; i += kJpegBlock)
            hist[i] = 0;
    } else if constexpr (HUFF == kHuffDevice) {
        constexpr int kClasses = C == 1 ? 1 : 2;
        for (int i = tid; i < 16 * kClasses; i += kJpegBlock)
            huff_dc[i / 16][i % 16] = a.huff[(i / 16) * 512 + i % 16];
        for (int i = tid; i < 256 * kClasses; i += kJpegBlock)
            huff_ac[i / 256][i % 256] = a.huff[(i / 256) * 512 + 256 + i % 256];
    } else {
        constexpr va_jpeg::HuffTables huff = va_jpeg::make_huff();
        for (int i = tid; i < 32; i += kJpegBlock)
            huff_dc[i / 16][i % 16] = huff.dc[i / 16][i % 16];
        for (int i = tid; i < 512; i += kJpegBlock)
            huff_ac[i / 256][i % 256] = huff.ac[i / 256][i % 256];
    }
    if (tid < 128)
        qt[tid / 64][tid % 64] = a.qtables[tid];
    for (int i = tid; i < kBitWords; i += kJpegBlock)
        bitbuf[i] = 0;
    if (tid < 3)
        pred[tid] = 0;

    // [header | RSTm] in front of the segment
    int64_t out_at = 0, out_end = 0;
    if (WRITE) {
        out_at = a.seg_start[seg];
        out_end = a.seg_start[seg + 1] - (j == a.nseg - 1 ? 2 : 0);
        if (j == 0) {
            const int header_bytes = HUFF == kHuffDevice ? a.header_len[0] : a.header_bytes;
            for (int i = tid; i < header_bytes; i += kJpegBlock)
                if (out_at + i < out_end)
                    a.out[out_at + i] = a.header[i];
            out_at += header_bytes;
        } else {
            if (tid < 2 && out_at + tid < out_end)
                a.out[out_at + tid] = tid == 0 ? (uint8_t)0xFF : (uint8_t)(0xD0 + (j - 1) % 8);
            out_at += 2;
        }
    }

    // this lane's rows of T for the two passes, and where its zigzag coefficient comes from
    int t_row[8], t_col[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        t_row[i] = va_jpeg::dct_at(lane & 7, i);
        t_col[i] = va_jpeg::dct_at(lane >> 3, i);
    }
    const int zz_from = va_jpeg::zigzag_at(lane);
    const int y_load = min(j * 8 * VS + lane / CG, a.h - 1);
    const uint8_t *row = a.frames + ((int64_t)frame * a.h + y_load) * a.w * C;

    uint32_t carry_bits = 0;             // bits of bitbuf[0] that belong to the previous chunk
    int64_t emitted = 0;                 // bytes of the segment so far
    __syncthreads();

    for (int m0 = 0; m0 < a.mcus; m0 += kMcus) {
        const int cm = min(kMcus, a.mcus - m0), nblk = cm * BPM;
        const bool last = m0 + kMcus >= a.mcus;
        // ---------------------------------------------------------------- A: transform
        if constexpr (HV > 1) {
            constexpr int MW = CG / 2;   // MCUs a wave loads at once
            const int cg = lane % CG;
            // the real chroma rows from this segment's first on, and the real chroma columns
            const int crows = (a.h + VS - 1) / VS - j * 8, ccols = (a.w + HS - 1) / HS;
            for (int g = wave * MW; g < cm; g += kJpegWaves * MW) {
                uint32_t px[6];          // the lane's 8 pixels of MCU g + cg / 2, row lane / CG, left or right half
                const int mcu = min(m0 + g + (cg >> 1), a.mcus - 1);
                load_pixels<3>(row, mcu * 16 + (cg & 1) * 8, a.w, px);
                uint32_t luma[2] = {0, 0};           // the 8 Y samples as bytes
                uint32_t sums[2][2] = {{0, 0}, {0, 0}};      // Cb, Cr: the 4 sums of horizontal pairs, 16 bits each
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int r = (px[(3 * i) / 4] >> (8 * ((3 * i) % 4))) & 255;
                    const int gg = (px[(3 * i + 1) / 4] >> (8 * ((3 * i + 1) % 4))) & 255;
                    const int b = (px[(3 * i + 2) / 4] >> (8 * ((3 * i + 2) % 4))) & 255;
                    int yy, cb, cr;
                    va_jpeg::ycbcr(r, gg, b, yy, cb, cr);
                    luma[i / 4] |= (uint32_t)yy << (8 * (i % 4));
                    sums[0][i / 4] += (uint32_t)cb << (16 * ((i / 2) % 2));
                    sums[1][i / 4] += (uint32_t)cr << (16 * ((i / 2) % 2));
                }
                uint32_t chroma[2];                  // Cb, Cr: the 4 averages as bytes; both rows of a pair hold them
#pragma unroll
                for (int ch = 0; ch < 2; ch++) {
                    chroma[ch] = 0;
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        uint32_t s = sums[ch][i];
                        if constexpr (VS == 2)
                            s += __shfl_xor(s, CG, kWave);           // the row below or above: no field overflows
                        chroma[ch] |= (uint32_t)va_jpeg::box_average((int)(s & 0xFFFFu), HV) << (16 * i);
                        chroma[ch] |= (uint32_t)va_jpeg::box_average((int)(s >> 16), HV) << (16 * i + 8);
                    }
                }
                const int here = min(MW, cm - g);
                const int crow = va_jpeg::edge_index(lane >> 3, crows);
                for (int mi = 0; mi < here; mi++) {
                    const int c0 = (m0 + g + mi) * 8;                // (c0 < ccols: the MCU exists)
                    const int ccol = va_jpeg::edge_index(c0 + (lane & 7), ccols) - c0;
#pragma unroll
                    for (int k = 0; k < BPM; k++) {
                        // lane = 8 y + x of the block
                        int sample;
                        if (k < HV) {
                            const int src = ((k / HS) * 8 + (lane >> 3)) * CG + 2 * mi + k % HS;
                            const uint32_t lo = __shfl(luma[0], src, kWave), hi = __shfl(luma[1], src, kWave);
                            const int x = lane & 7;
                            sample = (int)(((x < 4 ? lo : hi) >> (8 * (x & 3))) & 255u) - 128;
                        } else {
                            const int src = crow * VS * CG + 2 * mi + (ccol >> 2);
                            const uint32_t v = __shfl(chroma[k - HV], src, kWave);
                            sample = (int)((v >> (8 * (ccol & 3))) & 255u) - 128;
                        }
                        coef[(g + mi) * BPM + k][lane] =
                            transform_block(sample, t_row, t_col, qt[k < HV ? 0 : 1], zz_from, lane);
                    }
                }
            }
        } else if (const int g = wave * kGroupMcus; g < cm) {
            uint32_t px[2 * C];          // the lane's 8 pixels of MCU g + (lane & 7), row lane >> 3
            const int mcu = min(m0 + g + (lane & 7), a.mcus - 1);
            load_pixels<C>(row, mcu * 8, a.w, px);
            uint32_t comp[C][2];         // per component the 8 samples as bytes
            if constexpr (C == 1) {
                comp[0][0] = px[0], comp[0][1] = px[1];
            } else {
#pragma unroll
                for (int ch = 0; ch < C; ch++)
                    comp[ch][0] = comp[ch][1] = 0;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int r = (px[(3 * i) / 4] >> (8 * ((3 * i) % 4))) & 255;
                    const int gg = (px[(3 * i + 1) / 4] >> (8 * ((3 * i + 1) % 4))) & 255;
                    const int b = (px[(3 * i + 2) / 4] >> (8 * ((3 * i + 2) % 4))) & 255;
                    int yy, cb, cr;
                    va_jpeg::ycbcr(r, gg, b, yy, cb, cr);
                    comp[0][i / 4] |= (uint32_t)yy << (8 * (i % 4));
                    comp[1][i / 4] |= (uint32_t)cb << (8 * (i % 4));
                    comp[2][i / 4] |= (uint32_t)cr << (8 * (i % 4));
                }
            }
            const int blocks_here = min(kGroupMcus, cm - g);
            for (int jj = 0; jj < blocks_here; jj++) {
#pragma unroll
                for (int ch = 0; ch < C; ch++) {
                    // lane = 8 y + x of the block
                    const int src = (lane & ~7) | jj;
                    const uint32_t lo = __shfl(comp[ch][0], src, kWave), hi = __shfl(comp[ch][1], src, kWave);
                    const int x = lane & 7;
                    const int sample = (int)(((x < 4 ? lo : hi) >> (8 * (x & 3))) & 255u) - 128;
                    coef[(g + jj) * C + ch][lane] = transform_block(sample, t_row, t_col, qt[ch ? 1 : 0], zz_from, lane);
                }
            }
        }
        __syncthreads();
        if constexpr (HUFF == kHuffCount) {
            // ------------------------------------------------------------ the symbols of every block, in place of B1 .. E
            for (int q = wave; q < nblk; q += kJpegWaves) {
                const int k = q % BPM, ch = va_jpeg::block_component(k, HV), tab = ch ? 1 : 0;
                const int back = va_jpeg::predictor_back(k, HV, BPM);
                const int v = coef[q][lane];
                const int p = q >= back ? coef[q - back][0] : pred[ch];
                const uint64_t nonzero = __ballot(v != 0);
                va_jpeg::coefficient_symbols(lane, v, p, nonzero, [&](int ac, int symbol, int times) {
                    atomicAdd(&hist[(2 * tab + ac) * 256 + symbol], (uint32_t)times);
                });
            }
            __syncthreads();
            if (tid < C)
                pred[tid] = coef[(cm - 1) * BPM + HV - 1 + tid][0];
            __syncthreads();
            continue;
        }
        // ---------------------------------------------------------------- B1: bits of every block
        for (int q = wave; q < nblk; q += kJpegWaves) {
            const int k = q % BPM, ch = va_jpeg::block_component(k, HV), tab = ch ? 1 : 0;
            const int back = va_jpeg::predictor_back(k, HV, BPM);
            const int v = coef[q][lane];
            const int p = q >= back ? coef[q - back][0] : pred[ch];
            const uint64_t nonzero = __ballot(v != 0);
            int len;
            if constexpr (HUFF == kHuffDevice) {         // codes of up to 16 bits: two strings (coefficient_bits_wide)
                const va_jpeg::WideBits b = va_jpeg::coefficient_bits_wide(huff_dc[tab], huff_ac[tab], lane, v, p, nonzero);
                len = b.zrl.len + b.rest.len;
            } else {
                len = va_jpeg::coefficient_bits(huff_dc[tab], huff_ac[tab], lane, v, p, nonzero).len;
            }
            const int total = wave_sum(len);
            if (lane == 0)
                block_bits[q] = total;
        }
        __syncthreads();
        // the blocks' bit positions: an exclusive scan behind the carry (one wave, two entries a lane)
        if (wave == 0) {
            const int b0 = lane < nblk ? block_bits[lane] : 0, b1 = lane + 64 < nblk ? block_bits[lane + 64] : 0;
            const int i0 = wave_inclusive(b0, lane), t0 = __shfl(i0, kWave - 1, kWave);
            const int i1 = wave_inclusive(b1, lane), t1 = __shfl(i1, kWave - 1, kWave);
            if (lane < nblk)
                block_bits[lane] = (int)carry_bits + i0 - b0;
            if (lane + 64 < nblk)
                block_bits[lane + 64] = (int)carry_bits + t0 + i1 - b1;
            if (lane == 0)
                chunk_end = carry_bits + (uint32_t)(t0 + t1);
        }
        int next_pred = 0;
        if (tid < C)
            next_pred = coef[(cm - 1) * BPM + HV - 1 + tid][0];      // the chunk's last block of component tid
        __syncthreads();
        // ---------------------------------------------------------------- B2: the strings into the bit buffer
        for (int q = wave; q < nblk; q += kJpegWaves) {
            const int k = q % BPM, ch = va_jpeg::block_component(k, HV), tab = ch ? 1 : 0;
            const int back = va_jpeg::predictor_back(k, HV, BPM);
            const int v = coef[q][lane];
            const int p = q >= back ? coef[q - back][0] : pred[ch];
            const uint64_t nonzero = __ballot(v != 0);
            auto or_in = [&](uint32_t wi, uint32_t val) {
                if (wi < (uint32_t)kBitWords)
                    atomicOr(&bitbuf[wi], val);
            };
            if constexpr (HUFF == kHuffDevice) {
                const va_jpeg::WideBits b = va_jpeg::coefficient_bits_wide(huff_dc[tab], huff_ac[tab], lane, v, p, nonzero);
                const int len = b.zrl.len + b.rest.len;
                const uint32_t pos = (uint32_t)(block_bits[q] + wave_inclusive(len, lane) - len);
                va_jpeg::put_bits(pos, b.zrl, or_in);
                va_jpeg::put_bits(pos + (uint32_t)b.zrl.len, b.rest, or_in);
            } else {
                const va_jpeg::Bits b = va_jpeg::coefficient_bits(huff_dc[tab], huff_ac[tab], lane, v, p, nonzero);
                const uint32_t pos = (uint32_t)(block_bits[q] + wave_inclusive(b.len, lane) - b.len);
                va_jpeg::put_bits(pos, b, or_in);
            }
        }
        __syncthreads();
        if (tid < C)
            pred[tid] = next_pred;
        const uint32_t end = chunk_end;
        if (last && tid == 0) {                                  // pad to a byte with 1-bits
            const int pad = (int)(-end & 7u);
            va_jpeg::put_bits(end, va_jpeg::Bits{(1ull << pad) - 1, pad},
                              [&](uint32_t wi, uint32_t val) { bitbuf[wi] |= val; });
        }
        __syncthreads();
        // ---------------------------------------------------------------- E: whole words out, stuffed
        const int nbytes = last ? (int)((end + 7) >> 3) : (int)(end >> 5) * 4;
        const int nwords = (nbytes + 3) >> 2;
        for (int t0 = 0; t0 < nwords; t0 += kJpegBlock) {
            const int wi = t0 + tid;
            const int nvalid = min(max(nbytes - 4 * wi, 0), 4);
            const uint32_t word = nvalid > 0 ? bitbuf[wi] : 0u;
            const int mine = nvalid + va_jpeg::count_ff(word, nvalid);
            const int incl = wave_inclusive(mine, lane);
            if (lane == kWave - 1)
                wave_total[wave] = incl;
            __syncthreads();
            int before = 0, tile = 0;
#pragma unroll
            for (int k = 0; k < kJpegWaves; k++) {
                before += k < wave ? wave_total[k] : 0;
                tile += wave_total[k];
            }
            if (WRITE) {
                const int64_t at = out_at + emitted + before + incl - mine;
                va_jpeg::put_stuffed(word, nvalid, [&](int i, uint8_t v) {
                    if (at + i < out_end)
                        a.out[at + i] = v;
                });
            }
            emitted += tile;
            __syncthreads();
        }
        // the unfinished word becomes word 0 of the next chunk
        if (!last) {
            const uint32_t wlast = end >> 5;
            const uint32_t keep = bitbuf[wlast];
            __syncthreads();
            for (uint32_t i = tid; i <= wlast + 2 && i < (uint32_t)kBitWords; i += kJpegBlock)
                bitbuf[i] = 0;
            __syncthreads();
            if (tid == 0)
                bitbuf[0] = keep;
            carry_bits = end & 31u;
        }
    }
    if constexpr (HUFF == kHuffCount) {
        // (a segment has fewer than 2^32 symbols: at most 8192 MCUs of 6 blocks of 64 coefficients with 4 symbols)
        for (int i = tid; i < 4 * 256; i += kJpegBlock)
            if (hist[i])
                atomicAdd(&a.freq[i], (unsigned long long)hist[i]);
    } else if (!WRITE) {
        if (tid == 0)
            a.seg_len[seg] = (int32_t)emitted + (HUFF == kHuffDevice && j == 0 ? a.header_len[0] : 0);
    } else if (j == a.nseg - 1 && tid < 2) {
        const int64_t at = out_at + emitted + tid;             // EOI
        if (at < a.seg_start[seg + 1])
            a.out[at] = tid == 0 ? (uint8_t)0xFF : (uint8_t)0xD9;
    }
}

// seg_start[0 .. S] = exclusive prefix of [header | RST] + segment + [EOI]; offsets[f] = the start of frame f,
// offsets[n] = totals[0] = the sum; sizes[f] = the bytes of frame f.  One workgroup, 1024 segments a round.
__global__ void __launch_bounds__(kScanBlock)
jpeg_scan_kernel(const int32_t *__restrict__ seg_len, int64_t nsegs, int nseg, int n, int header_bytes,
                 int64_t *__restrict__ seg_start, int64_t *offsets, int64_t *__restrict__ sizes,
                 int64_t *__restrict__ totals)
{
    __shared__ int64_t part[kScanBlock / kWave];
    const int t = (int)threadIdx.x;
    int64_t carry = 0;
    for (int64_t base = 0; base < nsegs; base += kScanBlock * kScanPerThread) {
        int64_t v[kScanPerThread], mine = 0;
#pragma unroll
        for (int i = 0; i < kScanPerThread; i++) {
            const int64_t s = base + (int64_t)t * kScanPerThread + i;
            v[i] = 0;
            if (s < nsegs) {
                const int j = (int)(s % nseg);
                v[i] = (int64_t)seg_len[s] + (j == 0 ? header_bytes : 2) + (j == nseg - 1 ? 2 : 0);
            }
            mine += v[i];
        }
        int64_t sum;
        int64_t at = carry + block_exclusive<kScanBlock / kWave>(mine, part, sum);
#pragma unroll
        for (int i = 0; i < kScanPerThread; i++) {
            const int64_t s = base + (int64_t)t * kScanPerThread + i;
            if (s < nsegs) {
                seg_start[s] = at;
                if (s % nseg == 0)
                    offsets[s / nseg] = at;
            }
            at += v[i];
        }
        carry += sum;
    }
    if (t == 0) {
        seg_start[nsegs] = carry;
        offsets[n] = carry;
        totals[0] = carry;
    }
    __threadfence_block();
    __syncthreads();
    for (int f = t; f < n; f += kScanBlock)
        sizes[f] = offsets[f + 1] - offsets[f];
}

// ------------------------------------------------------------------------------------------------ optimised tables
constexpr int kTableWaves = 4;                         // tables of a workgroup, a wave each
constexpr int kTableBytes = 16 + 256;                  // BITS, HUFFVAL
constexpr int kDhtMaxBytes[2] = {5 + 16 + 12, 5 + 16 + 162};     // a DHT segment of the encoder's DC and AC symbols

struct TableArgs {
    const int64_t *freq;             // [t][256]
    int t;
    uint8_t *bits_vals;              // [t][kTableBytes]
    // the encoder's call (one workgroup, t = 2 or 4 in the order DC0, AC0, DC1, AC1), else NULL:
    uint32_t *huff;                  // [t][256] length << 16 | code
    const uint8_t *pre, *post;       // the header in front of and behind the DHT segments
    int pre_bytes, post_bytes;
    uint8_t *header;                 // [header_cap] pre | DHT * t | post
    int header_cap;
    int32_t *header_len;
};

__global__ void __launch_bounds__(kTableWaves * kWave) jpeg_tables_kernel(TableArgs a)
{
    __shared__ int codesize[kTableWaves][va_jpeg::kHuffSymbols];
    __shared__ int work[kTableWaves][2][va_jpeg::kHuffSymbols];
    __shared__ uint8_t bv[kTableWaves][kTableBytes];
    __shared__ uint32_t codes[kTableWaves][256];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int t = blockIdx.x * kTableWaves + wave;
    // (a wave without a table builds the last one again and stores nothing: the barriers stay uniform)
    const int64_t *freq = a.freq + (int64_t)min(t, a.t - 1) * 256;
    va_jpeg::huff_code_sizes<kWave>(lane, freq, [](va_jpeg::HuffPick p) {
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            va_jpeg::HuffPick o;
            o.freq = (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)p.freq, d, kWave) |
                     (uint64_t)(uint32_t)__shfl_xor((int)(uint32_t)(p.freq >> 32), d, kWave) << 32;
            o.index = __shfl_xor(p.index, d, kWave);
            p = va_jpeg::huff_better(p, o);
        }
        return p;
    }, codesize[wave]);
    __syncthreads();
    if (lane == 0) {
        va_jpeg::huff_bits_vals(codesize[wave], bv[wave], bv[wave] + 16, work[wave][0], work[wave][1]);
        va_jpeg::huff_encoder_table(bv[wave], bv[wave] + 16, codes[wave]);
    }
    __syncthreads();
    if (t < a.t) {
        for (int i = lane; i < kTableBytes; i += kWave)
            a.bits_vals[(int64_t)t * kTableBytes + i] = bv[wave][i];
        if (a.huff)
            for (int i = lane; i < 256; i += kWave)
                a.huff[t * 256 + i] = codes[wave][i];
    }
    if (!a.header)
        return;
    auto put = [&](int at, uint8_t v) {
        if (at < a.header_cap)
            a.header[at] = v;
    };
    for (int i = tid; i < a.pre_bytes; i += kTableWaves * kWave)
        put(i, a.pre[i]);
    int at = a.pre_bytes;
    for (int u = 0; u < a.t; u++) {
        int nsym = 0;
        for (int i = 0; i < 16; i++)
            nsym += bv[u][i];
        // FF C4, the length, Tc << 4 | Th, BITS, the HUFFVAL in use
        for (int i = tid; i < 5 + 16 + nsym; i += kTableWaves * kWave)
            put(at + i, i == 0 ? 0xFF : i == 1 ? 0xC4 : i == 2 ? (uint8_t)((19 + nsym) >> 8) : i == 3 ? (uint8_t)(19 + nsym)
                        : i == 4 ? (uint8_t)((u & 1) << 4 | u >> 1) : bv[u][i - 5]);
        at += 5 + 16 + nsym;
    }
    for (int i = tid; i < a.post_bytes; i += kTableWaves * kWave)
        put(at + i, a.post[i]);
    if (tid == 0)
        a.header_len[0] = min(at + a.post_bytes, a.header_cap);
}

template <bool WRITE, int HUFF>
void launch_segments(int c, int hs, int vs, int64_t nsegs, hipStream_t st, const JpegArgs &a)
{
    const dim3 grid((unsigned)nsegs), block(kJpegBlock);
    if (c == 1)
        hipLaunchKernelGGL((jpeg_segment_kernel<1, 1, 1, WRITE, HUFF>), grid, block, 0, st, a);
    else if (hs == 1)
        hipLaunchKernelGGL((jpeg_segment_kernel<3, 1, 1, WRITE, HUFF>), grid, block, 0, st, a);
    else if (vs == 1)
        hipLaunchKernelGGL((jpeg_segment_kernel<3, 2, 1, WRITE, HUFF>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((jpeg_segment_kernel<3, 2, 2, WRITE, HUFF>), grid, block, 0, st, a);
}

// what the optimised call adds to the plain one's arguments
struct OptimizedArgs {
    const uint8_t *pre, *post;
    int pre_bytes, post_bytes;
    uint8_t *bits_vals_out;
};

// the three entry points; `sampled`: the luma sampling is an argument and checked; opt: the optimised call, whose header
// is opt's two pieces (header: the first, header_bytes: the sum of their lengths)
int jpeg_encode(const char *what, bool sampled, const uint8_t *frames, int n, int h, int w, int c, int hs, int vs,
                const uint8_t *qtables, const uint8_t *header, int header_bytes, int64_t *sizes_out,
                int64_t *offsets_out, int64_t *totals, uint8_t *bytes_out, int64_t cap_bytes, void *stream,
                const OptimizedArgs *opt = nullptr)
{
    VA_ENTER();
    VA_REQUIRE(n >= 0 && h > 0 && w > 0 && header_bytes > 0 && cap_bytes >= 0 &&
                   (!opt || (opt->pre_bytes > 0 && opt->post_bytes > 0)),
               "%s: negative or zero size (n %d, h %d, w %d, header %d, cap %lld)", what, n, h, w, header_bytes,
               (long long)cap_bytes);
    VA_REQUIRE(c == 1 || c == 3, "%s: channels must be 1 or 3, got %d", what, c);
    if (n == 0)
        return VA_OK;
    VA_REQUIRE(frames && qtables && header && sizes_out && offsets_out && totals && (bytes_out || cap_bytes == 0) &&
                   (!opt || (opt->post && opt->bits_vals_out)),
               "%s: NULL argument", what);
    VA_REQUIRE(aligned(sizes_out, 8) && aligned(offsets_out, 8) && aligned(totals, 8),
               "%s: the int64 buffers must be 8-byte aligned", what);
    VA_REQUIRE(h <= 65535 && w <= 65535, "%s: SOF0 holds 16-bit sizes, got %d x %d", what, w, h);
    VA_REQUIRE((int64_t)n * ((h + 7) / 8) < ((int64_t)1 << 31), "%s: the stack has too many MCU rows for one launch",
               what);
    if (sampled) {
        VA_REQUIRE((hs == 1 && vs == 1) || (hs == 2 && (vs == 1 || vs == 2)),
                   "%s: the luma sampling is 1 x 1, 2 x 1 or 2 x 2, got %d x %d", what, hs, vs);
        VA_REQUIRE(c == 3 || hs * vs == 1, "%s: luma sampling %d x %d needs 3 channels", what, hs, vs);
    }
    hipStream_t st = as_stream(stream);
    const int nseg = (h + 8 * vs - 1) / (8 * vs);
    const int64_t nsegs = (int64_t)n * nseg;
    Carve ws;                                        // [seg_len | seg_start]
    const size_t o_len = ws.take((size_t)nsegs * sizeof(int32_t));
    const size_t o_start = ws.take(((size_t)nsegs + 1) * sizeof(int64_t));
    // the optimised call: [counts | encoder entries | header length | header]
    const int tables = c == 1 ? 2 : 4;
    const int header_cap = header_bytes + (tables / 2) * (kDhtMaxBytes[0] + kDhtMaxBytes[1]);
    const size_t o_freq = opt ? ws.take(4 * 256 * sizeof(int64_t)) : 0;
    const size_t o_huff = opt ? ws.take(4 * 256 * sizeof(uint32_t)) : 0;
    const size_t o_hlen = opt ? ws.take(sizeof(int32_t)) : 0;
    const size_t o_head = opt ? ws.take((size_t)header_cap) : 0;
    ScratchLease scratch;
    int rc = scratch.acquire(ws.total, st);
    if (rc)
        return rc;
    int32_t *seg_len = at<int32_t>(scratch.ptr, o_len);
    int64_t *seg_start = at<int64_t>(scratch.ptr, o_start);
    if (opt) {
        int64_t *freq = at<int64_t>(scratch.ptr, o_freq);
        const JpegArgs a{frames, n, h, w, nseg, (w + 8 * hs - 1) / (8 * hs), qtables, at<uint8_t>(scratch.ptr, o_head), 0,
                         seg_len, seg_start, totals, bytes_out, cap_bytes, at<uint32_t>(scratch.ptr, o_huff),
                         at<int32_t>(scratch.ptr, o_hlen), reinterpret_cast<unsigned long long *>(freq)};
        VA_HIP(hipMemsetAsync(freq, 0, 4 * 256 * sizeof(int64_t), st));
        launch_segments<false, kHuffCount>(c, hs, vs, nsegs, st, a);
        VA_LAUNCH_CHECK("jpeg_segment_kernel (histogram)");
        const TableArgs ta{freq, tables, opt->bits_vals_out, at<uint32_t>(scratch.ptr, o_huff), opt->pre, opt->post,
                           opt->pre_bytes, opt->post_bytes, at<uint8_t>(scratch.ptr, o_head), header_cap,
                           at<int32_t>(scratch.ptr, o_hlen)};
        hipLaunchKernelGGL(jpeg_tables_kernel, dim3(1), dim3(kTableWaves * kWave), 0, st, ta);
        VA_LAUNCH_CHECK("jpeg_tables_kernel");
        launch_segments<false, kHuffDevice>(c, hs, vs, nsegs, st, a);
        VA_LAUNCH_CHECK("jpeg_segment_kernel (count)");
        // (the count has added the header's length to every frame's first segment)
        hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(kScanBlock), 0, st, seg_len, nsegs, nseg, n, 0, seg_start,
                           offsets_out, sizes_out, totals);
        VA_LAUNCH_CHECK("jpeg_scan_kernel");
        launch_segments<true, kHuffDevice>(c, hs, vs, nsegs, st, a);
        VA_LAUNCH_CHECK("jpeg_segment_kernel (write)");
        return VA_OK;
    }
    const JpegArgs a{frames, n, h, w, nseg, (w + 8 * hs - 1) / (8 * hs), qtables, header, header_bytes, seg_len,
                     seg_start, totals, bytes_out, cap_bytes, nullptr, nullptr, nullptr};
    launch_segments<false, kHuffAnnexK>(c, hs, vs, nsegs, st, a);
    VA_LAUNCH_CHECK("jpeg_segment_kernel (count)");
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(kScanBlock), 0, st, seg_len, nsegs, nseg, n, header_bytes,
                       seg_start, offsets_out, sizes_out, totals);
    VA_LAUNCH_CHECK("jpeg_scan_kernel");
    launch_segments<true, kHuffAnnexK>(c, hs, vs, nsegs, st, a);
    VA_LAUNCH_CHECK("jpeg_segment_kernel (write)");
    return VA_OK;
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

int va_jpeg_encode_u8(const uint8_t *frames, int n, int h, int w, int c, const uint8_t *qtables, const uint8_t *header,
                      int header_bytes, int64_t *sizes_out, int64_t *offsets_out, int64_t *totals, uint8_t *bytes_out,
                      int64_t cap_bytes, void *stream)
{
    return jpeg_encode("va_jpeg_encode_u8", false, frames, n, h, w, c, 1, 1, qtables, header, header_bytes, sizes_out,
                       offsets_out, totals, bytes_out, cap_bytes, stream);
}

int va_jpeg_encode_sampled_u8(const uint8_t *frames, int n, int h, int w, int c, int luma_h, int luma_v,
                              const uint8_t *qtables, const uint8_t *header, int header_bytes, int64_t *sizes_out,
                              int64_t *offsets_out, int64_t *totals, uint8_t *bytes_out, int64_t cap_bytes,
                              void *stream)
{
    return jpeg_encode("va_jpeg_encode_sampled_u8", true, frames, n, h, w, c, luma_h, luma_v, qtables, header,
                       header_bytes, sizes_out, offsets_out, totals, bytes_out, cap_bytes, stream);
}

int va_jpeg_encode_optimized_u8(const uint8_t *frames, int n, int h, int w, int c, int luma_h, int luma_v,
                                const uint8_t *qtables, const uint8_t *header_pre, int pre_bytes,
                                const uint8_t *header_post, int post_bytes, uint8_t *bits_vals_out, int64_t *sizes_out,
                                int64_t *offsets_out, int64_t *totals, uint8_t *bytes_out, int64_t cap_bytes,
                                void *stream)
{
    const OptimizedArgs opt{header_pre, header_post, pre_bytes, post_bytes, bits_vals_out};
    // (lengths of 2^30 and more are not a header's, and their sum stays an int)
    const int sum = pre_bytes > 0 && post_bytes > 0 && pre_bytes < (1 << 30) && post_bytes < (1 << 30)
                        ? pre_bytes + post_bytes : 0;
    return jpeg_encode("va_jpeg_encode_optimized_u8", true, frames, n, h, w, c, luma_h, luma_v, qtables, header_pre, sum,
                       sizes_out, offsets_out, totals, bytes_out, cap_bytes, stream, &opt);
}

int va_jpeg_optimal_tables(const int64_t *freq, int t, uint8_t *bits_vals_out, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(t >= 0, "va_jpeg_optimal_tables: a negative number of tables (%d)", t);
    if (t == 0)
        return VA_OK;
    VA_REQUIRE(freq && bits_vals_out, "va_jpeg_optimal_tables: NULL argument");
    VA_REQUIRE(aligned(freq, 8), "va_jpeg_optimal_tables: the counts must be 8-byte aligned");
    const TableArgs ta{freq, t, bits_vals_out, nullptr, nullptr, nullptr, 0, 0, nullptr, 0, nullptr};
    hipLaunchKernelGGL(jpeg_tables_kernel, dim3((unsigned)((t + kTableWaves - 1) / kTableWaves)), dim3(kTableWaves * kWave),
                       0, as_stream(stream), ta);
    VA_LAUNCH_CHECK("jpeg_tables_kernel");
    return VA_OK;
}

}  // extern "C"

