// va_jpeg_math.h -- the per-block arithmetic of the baseline JPEG encoder ("Motion-JPEG") as plain
// inline C++ that compiles for the host and for the device: colour conversion, the integer DCT, the quantiser, the
// Huffman strings of one coefficient, the bit writer and the byte stuffing, and what the subsampled layouts add: the box
// average, the edge rule and the maps from a block's place in its MCU to its component and DC predictor.  va_jpeg.hip
// runs it with one lane per coefficient of a block; tests/jpeg_shim.cpp and tests/jpeg_sampled_shim.cpp compile it with
// the host compiler (under sanitizers) into serial encoders whose bytes are the NumPy restatements'
// (tests/jpeg_checks.py, tests/jpeg_subsampled_checks.py: encode_frame).  The construction of optimised Huffman tables
// from symbol counts is here too (tests/jpeg_optimize_shim.cpp, tests/jpeg_optimize_checks.py).
//
// Integers only.  A block is 64 samples minus 128; T[k][n] = rint(2^13 A[k][n]) with A the orthonormal 8-point
// DCT-II matrix.  The row pass keeps (sum + 1024) >> 11, four times the row coefficient; the column pass's sum is the
// coefficient times 2^15; the quantiser is sign * ((|S| + (Q << 14)) / (Q << 15)).  Every intermediate fits int32:
// |row sum| <= 8 * 4017 * 128 < 2^23, |row value| <= 2009, |column sum| <= 8 * 4017 * 2009 < 2^26, and
// (Q << 15) + (Q << 14) < 2^24.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VA_JPEG_FN __host__ __device__ inline
#else
#define VA_JPEG_FN inline
#endif

namespace va_jpeg {

// natural (row-major) index of the k-th coefficient in zigzag order
VA_JPEG_FN constexpr int zigzag_at(int k)
{
    constexpr int t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                           41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                           30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k];
}

// T[k][n] = rint(2^13 A[k][n])
VA_JPEG_FN constexpr int dct_at(int k, int n)
{
    constexpr int t[8][8] = {{2896, 2896, 2896, 2896, 2896, 2896, 2896, 2896},
                             {4017, 3406, 2276, 799, -799, -2276, -3406, -4017},
                             {3784, 1567, -1567, -3784, -3784, -1567, 1567, 3784},
                             {3406, -799, -4017, -2276, 2276, 4017, 799, -3406},
                             {2896, -2896, -2896, 2896, 2896, -2896, -2896, 2896},
                             {2276, -4017, 799, 3406, -3406, -799, 4017, -2276},
                             {1567, -3784, 3784, -1567, -1567, 3784, -3784, 1567},
                             {799, -2276, 3406, -4017, 4017, -3406, 2276, -799}};
    return t[k][n];
}

// JFIF full range in 16-bit fixed point
VA_JPEG_FN void ycbcr(int r, int g, int b, int &y, int &cb, int &cr)
{
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
    cb = (-11059 * r - 21709 * g + 32768 * b + 8421375) >> 16;
    cr = (32768 * r - 27439 * g - 5329 * b + 8421375) >> 16;
}

// ------------------------------------------------------------------------------------------------ sampling layouts
// ("Subsampled Motion-JPEG encoding").  An MCU holds hv = H V luma blocks, then Cb, then Cr (one block,
// hv = 1, in a monochrome file); k is a block's position in its MCU, bpm the blocks of an MCU.

// a chroma sample of the H x V box: the sum of its hv pixels, rounded half up
VA_JPEG_FN int box_average(int sum, int hv) { return (int)(((uint32_t)sum + (uint32_t)hv / 2) / (uint32_t)hv); }

// index i of a plane padded by repeating the last of its `real` rows or columns
VA_JPEG_FN int edge_index(int i, int real) { return i < real ? i : real - 1; }

// the component of the block at position k: 0 luma, 1 Cb, 2 Cr
VA_JPEG_FN int block_component(int k, int hv) { return k < hv ? 0 : k - hv + 1; }

// how many blocks back in coding order the block lies whose DC predicts the block at position k: the luma block
// before it, for the first luma block of an MCU the last one of the MCU before, for Cb and Cr the same component one
// MCU back
VA_JPEG_FN int predictor_back(int k, int hv, int bpm) { return k == 0 ? bpm - hv + 1 : k < hv ? 1 : bpm; }

VA_JPEG_FN int row_round(int sum) { return (sum + 1024) >> 11; }

VA_JPEG_FN int quantise(int s, int q)
{
    const uint32_t mag = (uint32_t)(s < 0 ? -s : s);
    const int v = (int)((mag + ((uint32_t)q << 14)) / ((uint32_t)q << 15));
    return s < 0 ? -v : v;
}

// the 8 x 8 forward transform of one block, serially (the device spreads the same sums over 64 lanes):
// x: samples minus 128 in natural order, q: the quantisation table in natural order; out: zigzag order
VA_JPEG_FN void forward_block(const int *x, const uint8_t *q, int16_t *out)
{
    int rows[64], nat[64];
    for (int y = 0; y < 8; y++)
        for (int k = 0; k < 8; k++) {
            int sum = 0;
            for (int n = 0; n < 8; n++)
                sum += dct_at(k, n) * x[8 * y + n];
            rows[8 * y + k] = row_round(sum);
        }
    for (int v = 0; v < 8; v++)
        for (int k = 0; k < 8; k++) {
            int sum = 0;
            for (int y = 0; y < 8; y++)
                sum += dct_at(v, y) * rows[8 * y + k];
            nat[8 * v + k] = quantise(sum, q[8 * v + k]);
        }
    for (int k = 0; k < 64; k++)
        out[k] = (int16_t)nat[zigzag_at(k)];
}

// ------------------------------------------------------------------------------------------------ Huffman tables
// ITU T.81 Annex K.3 - K.6 as length << 16 | code per symbol (0: the symbol has no code); table 0 luma, 1 chroma
struct HuffTables {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};

VA_JPEG_FN constexpr void huff_fill(const uint8_t *bits, const uint8_t *vals, uint32_t *out)
{
    uint32_t code = 0;
    int k = 0;
    for (int length = 1; length <= 16; length++) {
        for (int i = 0; i < bits[length - 1]; i++)
            out[vals[k++]] = ((uint32_t)length << 16) | code++;
        code <<= 1;
    }
}

// the encoder's 256 entries of one table from run-time BITS and HUFFVAL
VA_JPEG_FN void huff_encoder_table(const uint8_t *bits, const uint8_t *vals, uint32_t *out)
{
    for (int i = 0; i < 256; i++)
        out[i] = 0;
    huff_fill(bits, vals, out);
}

VA_JPEG_FN constexpr HuffTables make_huff()
{
    constexpr uint8_t dc_bits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0},
                                        {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
    constexpr uint8_t dc_vals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
    constexpr uint8_t ac_bits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
                                        {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
    constexpr uint8_t ac_vals[2][162] = {
        {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71,
         0x14, 0x32, 0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72,
         0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37,
         0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
         0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83,
         0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
         0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
         0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2,
         0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
        {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22,
         0x32, 0x81, 0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1,
         0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36,
         0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
         0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a,
         0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a,
         0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
         0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda,
         0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
    HuffTables h{};
    for (int t = 0; t < 2; t++) {
        huff_fill(dc_bits[t], dc_vals, h.dc[t]);
        huff_fill(ac_bits[t], ac_vals[t], h.ac[t]);
    }
    return h;
}

// ------------------------------------------------------------------------------------------------ optimised tables
// ("Optimised Huffman tables").  One table from its 256 counts as libjpeg's jpeg_gen_optimal_table
// builds it (T.81 K.2 with symbol 256 reserved, so that no code is all 1-bits), without its limits on a count and on a
// size before the lengths are limited to 16.  Two steps: the code sizes, spread over LANES lanes that each hold the
// symbols lane, lane + LANES, ..; then, serially, BITS and HUFFVAL from the sizes.
constexpr int kHuffSymbols = 257;       // 0 .. 255 and the reserved one

struct HuffPick {                       // the smallest non-zero count and where it is; index -1: there is none
    uint64_t freq;
    int index;
};

// of two picks the one with the smaller count, of equal counts the one with the larger index
VA_JPEG_FN HuffPick huff_better(HuffPick a, HuffPick b)
{
    if (a.index < 0)
        return b;
    if (b.index < 0)
        return a;
    return b.freq < a.freq || (b.freq == a.freq && b.index > a.index) ? b : a;
}

// the code size of every symbol before the limit: codesize[0 .. 256], which every lane fills for its own symbols.
// freq: the 256 counts, not negative and with a sum below 2^63 (the merges add them in 64 bits); reduce(pick): huff_better over the picks of all lanes, the same answer in every lane.
// libjpeg's `others` chain from a root lists the symbols of that root's tree, so a merge is: every symbol of either
// tree gets one more bit, and both trees are c1's.
template <int LANES, class Reduce>
VA_JPEG_FN void huff_code_sizes(int lane, const int64_t *freq, Reduce reduce, int *codesize)
{
    constexpr int S = (kHuffSymbols + LANES - 1) / LANES;
    uint64_t f[S];
    int tree[S], size[S];
    for (int k = 0; k < S; k++) {
        const int i = lane + LANES * k;
        f[k] = i < 256 ? (uint64_t)freq[i] : i == 256 ? 1u : 0u;
        tree[k] = i;
        size[k] = 0;
    }
    for (;;) {
        HuffPick mine{0, -1};
        for (int k = 0; k < S; k++)
            if (f[k])
                mine = huff_better(mine, HuffPick{f[k], lane + LANES * k});
        const HuffPick c1 = reduce(mine);
        mine = HuffPick{0, -1};
        for (int k = 0; k < S; k++)
            if (f[k] && lane + LANES * k != c1.index)
                mine = huff_better(mine, HuffPick{f[k], lane + LANES * k});
        const HuffPick c2 = reduce(mine);
        if (c2.index < 0)
            break;
        for (int k = 0; k < S; k++) {
            const int i = lane + LANES * k;
            if (i == c1.index)
                f[k] += c2.freq;
            if (i == c2.index)
                f[k] = 0;
            if (tree[k] == c1.index || tree[k] == c2.index) {
                size[k]++;
                tree[k] = c1.index;
            }
        }
    }
    for (int k = 0; k < S; k++)
        if (lane + LANES * k < kHuffSymbols)
            codesize[lane + LANES * k] = size[k];
}

// BITS (16) and HUFFVAL (256, the unused ones 0) from codesize[0 .. 256]; count, start: kHuffSymbols ints of
// workspace each.  Counts that are all 0 give an empty table.
VA_JPEG_FN void huff_bits_vals(const int *codesize, uint8_t *bits, uint8_t *vals, int *count, int *start)
{
    int top = 0;
    for (int s = 0; s < kHuffSymbols; s++)
        count[s] = 0;
    for (int i = 0; i < kHuffSymbols; i++)
        if (codesize[i] > 0) {
            count[codesize[i]]++;
            top = codesize[i] > top ? codesize[i] : top;
        }
    // HUFFVAL: the symbols 0 .. 255 by size, then by value; the limit below moves the borders between the sizes only
    int at = 0;
    for (int s = 1; s <= top; s++) {
        start[s] = at;
        at += count[s];
    }
    for (int i = 0; i < 256; i++)
        vals[i] = 0;
    for (int i = 0; i < 256; i++)
        if (codesize[i] > 0)             // (the reserved symbol, the last of its size, is not listed)
            vals[start[codesize[i]]++ - (codesize[i] > codesize[256] ? 1 : 0)] = (uint8_t)i;
    // T.81 K.2, figure K.3: no code longer than 16
    for (int i = top; i > 16; i--)
        while (count[i] > 0) {
            int j = i - 2;
            while (count[j] == 0)
                j--;
            count[i] -= 2;
            count[i - 1]++;
            count[j + 1] += 2;
            count[j]--;
        }
    int last = top < 16 ? top : 16;
    while (last > 0 && count[last] == 0)
        last--;
    if (last > 0)
        count[last]--;                   // the reserved symbol leaves
    for (int s = 1; s <= 16; s++)
        bits[s - 1] = (uint8_t)(s <= last ? count[s] : 0);
}

// ------------------------------------------------------------------------------------------------ one coefficient
// a bit string of at most 59 bits (the Annex K tables: 3 ZRLs of 11 bits, a code of 16, 10 magnitude bits), the first bit of the stream in the highest of the `len` low bits
struct Bits {
    uint64_t code;
    int len;
};

VA_JPEG_FN int bit_size(int v)          // the JPEG category: bits of |v|
{
    const uint32_t m = (uint32_t)(v < 0 ? -v : v);
    return m ? 32 - __builtin_clz(m) : 0;
}

VA_JPEG_FN void append(Bits &b, uint32_t entry)
{
    const int len = (int)(entry >> 16);
    b.code = (b.code << len) | (entry & 0xFFFFu);
    b.len += len;
}

VA_JPEG_FN void append_magnitude(Bits &b, int v, int size)
{
    const uint32_t mag = (uint32_t)(v >= 0 ? v : v + (1 << size) - 1);
    b.code = (b.code << size) | mag;
    b.len += size;
}

// zeros between coefficient k (>= 1, non-zero) and the non-zero AC coefficient before it; nonzero: bit i set iff
// coefficient i of the block (zigzag order) is not 0
VA_JPEG_FN int run_before(uint64_t nonzero, int k)
{
    const uint64_t below = nonzero & ((1ull << k) - 1) & ~1ull;
    int prev = 0;
    if (below)
        prev = 63 - __builtin_clzll(below);
    return k - prev - 1;
}

// what coefficient k of a block adds to the stream.  k == 0: the DC difference `v - pred`.  A non-zero AC
// coefficient: one ZRL per 16 zeros before it, the code of (run % 16, size) and the magnitude bits.  Coefficient 63
// when it is 0: the EOB.  Any other zero: nothing.  dc, ac: one table of HuffTables each
VA_JPEG_FN Bits coefficient_bits(const uint32_t *dc, const uint32_t *ac, int k, int v, int pred, uint64_t nonzero)
{
    Bits b{0, 0};
    if (k == 0) {
        const int diff = v - pred, size = bit_size(diff);
        append(b, dc[size & 15]);
        append_magnitude(b, diff, size);
    } else if (v != 0) {
        const int run = run_before(nonzero, k), size = bit_size(v);
        for (int z = run >> 4; z > 0; z--)
            append(b, ac[0xF0]);
        append(b, ac[(((run & 15) << 4) | size) & 255]);
        append_magnitude(b, v, size);
    } else if (k == 63) {
        append(b, ac[0]);
    }
    return b;
}

// coefficient_bits for run-time tables ("Optimised Huffman tables"), whose codes have up to 16 bits: a
// coefficient behind a run of 48 or more adds up to 3 * 16 + 16 + 10 = 74 bits, more than a Bits holds.  Two strings,
// the ZRLs (at most 48 bits) and behind them the rest (at most 16 + 11 = 27 bits, the DC string)
struct WideBits {
    Bits zrl, rest;
};

VA_JPEG_FN WideBits coefficient_bits_wide(const uint32_t *dc, const uint32_t *ac, int k, int v, int pred, uint64_t nonzero)
{
    WideBits b{{0, 0}, {0, 0}};
    if (k == 0) {
        const int diff = v - pred, size = bit_size(diff);
        append(b.rest, dc[size & 15]);
        append_magnitude(b.rest, diff, size);
    } else if (v != 0) {
        const int run = run_before(nonzero, k), size = bit_size(v);
        for (int z = run >> 4; z > 0; z--)
            append(b.zrl, ac[0xF0]);
        append(b.rest, ac[(((run & 15) << 4) | size) & 255]);
        append_magnitude(b.rest, v, size);
    } else if (k == 63) {
        append(b.rest, ac[0]);
    }
    return b;
}

// the Huffman symbols coefficient k adds, wherever coefficient_bits looks up a code, through count(ac, symbol, times):
// ac 0 for the DC table, 1 for the AC table of the block's class
template <class Count>
VA_JPEG_FN void coefficient_symbols(int k, int v, int pred, uint64_t nonzero, Count count)
{
    if (k == 0) {
        count(0, bit_size(v - pred) & 15, 1);
    } else if (v != 0) {
        const int run = run_before(nonzero, k), size = bit_size(v);
        if (run >> 4)
            count(1, 0xF0, run >> 4);
        count(1, (((run & 15) << 4) | size) & 255, 1);
    } else if (k == 63) {
        count(1, 0, 1);
    }
}

// ------------------------------------------------------------------------------------------------ bit writer
// The stream is kept as 32-bit words with the first bit of the stream in bit 31 of word 0.  put_bits ORs a string in
// at bit position `pos`; it touches words pos / 32 .. pos / 32 + 2, which hold 0 where nothing was put yet.  `orop`
// is (word index, value): a plain |= on the host, an LDS atomic on the device, where lanes share words.
template <class Or>
VA_JPEG_FN void put_bits(uint32_t pos, Bits b, Or orop)
{
    if (b.len == 0)
        return;
    const uint64_t val = b.code << (64 - b.len);
    const uint32_t w0 = pos >> 5, off = pos & 31;
    const uint32_t a = (uint32_t)((val >> 32) >> off), m = (uint32_t)(val >> off);
    const uint32_t c = off ? (uint32_t)(val << (32 - off)) : 0u;
    if (a)
        orop(w0, a);
    if (m)
        orop(w0 + 1, m);
    if (c)
        orop(w0 + 2, c);
}

// byte i (0 .. 3) of a stream word
VA_JPEG_FN uint32_t stream_byte(uint32_t word, int i) { return (word >> (24 - 8 * i)) & 255u; }

// the 0xFF bytes among the first nvalid bytes of a stream word: each is followed by a 0x00 in the file
VA_JPEG_FN int count_ff(uint32_t word, int nvalid)
{
    int n = 0;
    for (int i = 0; i < 4; i++)
        n += i < nvalid && stream_byte(word, i) == 255u;
    return n;
}

// the first nvalid bytes of a stream word with the stuffing, through put(offset, byte); returns the bytes put
template <class Put>
VA_JPEG_FN int put_stuffed(uint32_t word, int nvalid, Put put)
{
    int n = 0;
    for (int i = 0; i < 4; i++) {
        if (i >= nvalid)
            break;
        const uint32_t v = stream_byte(word, i);
        put(n++, (uint8_t)v);
        if (v == 255u)
            put(n++, (uint8_t)0);
    }
    return n;
}

}  // namespace va_jpeg
