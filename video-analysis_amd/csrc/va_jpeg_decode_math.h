// va_jpeg_decode_math.h -- the serial pieces of the baseline JPEG decoder ("Motion-JPEG decoding") as
// plain inline C++ that compiles for the host and for the device: the bit reader with the stuffing removed, the
// Huffman step, the decode of one block with its status, the dequantiser, the 8-point inverse pass, the colour
// conversion, the MCU walk of every sampling layout, and for 4:2:0 and 4:2:2 files the chroma upsampling.
// va_jpeg_decode.hip runs the entropy decode with one lane per segment and the reconstruction with one lane per MCU
// or per luma block; tests/jpeg_decode_shim.cpp, the one host shim of all layouts, compiles the same text with the
// host compiler (under sanitizers) into a serial decoder whose pixels and status words are the NumPy restatement's
// (tests/jpeg_decode_checks.py, tests/jpeg_subsampled_checks.py).
//
// Integers only.  F = clamp(coef * Q, -2048, 2047); T = rint(2^13 A) is the encoder's matrix (va_jpeg_math.h).  The
// column pass keeps (sum_v T[v][y] F[v][k] + 2^8) >> 9, sixteen times the half-transformed value; the row pass's
// (sum_k T[k][n] G[y][k] + 2^16) >> 17 is the sample minus 128.  Every intermediate fits int32 for any clamped
// input: the absolute values of a column of T add up to 21641, so |column sum| <= 2048 * 21641 < 2^26,
// |G| <= 86565 < 2^17, and |row sum| + 2^16 <= 21641 * 86565 + 65536 < 1.88e9 < 2^31.
#pragma once
#include <stdint.h>

#include "va_jpeg_math.h"

namespace va_jpeg {

// the bits of a frame's status word
constexpr int32_t kStatusBadCode = 1;       // a code in no table, a DC category > 11, an AC size > 10 (or a run / size
                                            // byte r0 with 0 < r < 15), a DC value outside -2048 .. 2047
constexpr int32_t kStatusOverrun = 2;       // a coefficient index beyond 63
constexpr int32_t kStatusTruncated = 4;     // bits are needed beyond the segment's end
constexpr int32_t kStatusMarker = 8;        // the scan did not end on EOI, or has another number of segments

constexpr int kIdctShift1 = 9, kIdctShift2 = 17;

// ------------------------------------------------------------------------------------------------ bit reader
// The bytes p[pos .. end) of one entropy segment; FF 00 inside it is the byte FF, every other byte is itself.  `acc`
// holds the next `cnt` bits of the stream in its highest bits and zeros below them.
struct BitReader {
    const uint8_t *p;
    int64_t pos, end;
    uint64_t acc;
    int cnt;
};

VA_JPEG_FN BitReader open_bits(const uint8_t *p, int64_t begin, int64_t end) { return BitReader{p, begin, end, 0, 0}; }

// at least 57 bits, or all that the segment still has
VA_JPEG_FN void refill(BitReader &r)
{
    while (r.cnt <= 56 && r.pos < r.end) {
        const uint32_t b = r.p[r.pos++];
        if (b == 0xFFu && r.pos < r.end && r.p[r.pos] == 0)
            r.pos++;
        r.acc |= (uint64_t)b << (56 - r.cnt);
        r.cnt += 8;
    }
}

VA_JPEG_FN void skip_bits(BitReader &r, int n)          // 0 <= n <= min(cnt, 63)
{
    r.acc <<= n;
    r.cnt -= n;
}

// ------------------------------------------------------------------------------------------------ Huffman step
// One table as the host builds it from a DHT segment (video.ops._jpeg_decode_table):
//   look[the next 9 bits]  length << 8 | symbol of a code of at most 9 bits, 0 where the code is longer or none
//   maxcode[l]             the largest code of l bits (l = 1 .. 16), -1 where there is none
//   valoff[l]              the index in vals of the first symbol of l bits, minus the smallest code of l bits
struct HuffDecode {
    uint16_t look[512];
    int32_t maxcode[17];
    int32_t valoff[17];
    uint8_t vals[256];
};

// the code at the head of peek16 (the next 16 bits, zeros behind the stream's end): its length 1 .. 16 and symbol,
// or 0 when no code of the table begins these bits.  Whatever the table holds, nothing outside it is read.
VA_JPEG_FN int huff_step(const HuffDecode &t, uint32_t peek16, int &sym)
{
    const uint32_t e = t.look[(peek16 >> 7) & 511u];
    if (e) {
        sym = (int)(e & 255u);
        const int len = (int)(e >> 8);
        return len <= 9 ? len : 0;
    }
    for (int l = 10; l <= 16; l++) {
        const int32_t code = (int32_t)(peek16 >> (16 - l));
        if (code <= t.maxcode[l]) {
            sym = t.vals[(uint32_t)(t.valoff[l] + code) & 255u];
            return l;
        }
    }
    return 0;
}

// the next symbol without consuming it: 0, or the status bit.  A decoder that reads bit by bit meets the end of the
// segment exactly where this one finds no code in fewer than 16 bits, or a code longer than what is left.
VA_JPEG_FN int32_t next_symbol(BitReader &r, const HuffDecode &t, int &sym, int &len)
{
    refill(r);
    len = huff_step(t, (uint32_t)(r.acc >> 48), sym);
    if (len == 0)
        return r.cnt >= 16 ? kStatusBadCode : kStatusTruncated;
    return len > r.cnt ? kStatusTruncated : 0;
}

// `size` (0 .. 11, at most cnt) magnitude bits as the signed value of T.81 F.2.2.1
VA_JPEG_FN int receive_extend(BitReader &r, int size)
{
    if (size == 0)
        return 0;
    const int v = (int)(r.acc >> (64 - size));
    skip_bits(r, size);
    return (v >> (size - 1)) ? v : v - (1 << size) + 1;
}

// One block: store(natural index, value) for the DC value and every AC coefficient the stream codes (the caller
// zeroes the block first).  Returns 0 or the status bit of the first error; the checks come in this order: the
// Huffman step (truncated / bad code), the symbol (bad code), the index (overrun), the magnitude bits (truncated),
// the DC range (bad code).  At most 64 symbols are read.
template <class Store>
VA_JPEG_FN int32_t decode_block(BitReader &r, const HuffDecode &dc, const HuffDecode &ac, int &pred, Store store)
{
    int sym = 0, len = 0;
    int32_t st = next_symbol(r, dc, sym, len);
    if (st)
        return st;
    if (sym > 11)
        return kStatusBadCode;
    if (len + sym > r.cnt)
        return kStatusTruncated;
    skip_bits(r, len);
    pred += receive_extend(r, sym);
    if (pred < -2048 || pred > 2047)
        return kStatusBadCode;
    store(0, pred);
    int k = 1;
    while (k < 64) {
        st = next_symbol(r, ac, sym, len);
        if (st)
            return st;
        const int run = sym >> 4, size = sym & 15;
        if (size == 0) {
            if (run == 0) {                 // EOB
                skip_bits(r, len);
                break;
            }
            if (run != 15)
                return kStatusBadCode;
            k += 16;                        // ZRL
            if (k > 64)
                return kStatusOverrun;
            skip_bits(r, len);
            continue;
        }
        if (size > 10)
            return kStatusBadCode;
        k += run;
        if (k > 63)
            return kStatusOverrun;
        if (len + size > r.cnt)
            return kStatusTruncated;
        skip_bits(r, len);
        store(zigzag_at(k), receive_extend(r, size));
        k++;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------ reconstruction
VA_JPEG_FN int dequantise(int coef, int q)
{
    const int f = coef * q;
    return f < -2048 ? -2048 : f > 2047 ? 2047 : f;
}

VA_JPEG_FN int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// out[i * so] = (sum_j T[j][i] in[j * si] + (1 << (shift - 1))) >> shift
VA_JPEG_FN void inverse_pass(const int *in, int si, int *out, int so, int shift)
{
#pragma unroll
    for (int i = 0; i < 8; i++) {
        int sum = 1 << (shift - 1);
#pragma unroll
        for (int j = 0; j < 8; j++)
            sum += dct_at(j, i) * in[j * si];
        out[i * so] = sum >> shift;
    }
}

// coef: 64 quantised coefficients in natural order, q: the table in natural order; out: 64 samples 0 .. 255
VA_JPEG_FN void inverse_block(const int16_t *coef, const uint8_t *q, uint8_t *out)
{
    int f[64], g[64];
#pragma unroll
    for (int i = 0; i < 64; i++)
        f[i] = dequantise(coef[i], q[i]);
#pragma unroll
    for (int k = 0; k < 8; k++)
        inverse_pass(f + k, 8, g + k, 8, kIdctShift1);          // columns: v -> y
#pragma unroll
    for (int y = 0; y < 8; y++)
        inverse_pass(g + 8 * y, 1, f + 8 * y, 1, kIdctShift2);  // rows: k -> n
#pragma unroll
    for (int i = 0; i < 64; i++)
        out[i] = (uint8_t)clip8(f[i] + 128);
}

// JFIF full range in 16-bit fixed point, the inverse of va_jpeg::ycbcr
VA_JPEG_FN void rgb_of(int y, int cb, int cr, int &r, int &g, int &b)
{
    cb -= 128;
    cr -= 128;
    r = clip8(y + ((91881 * cr + 32768) >> 16));
    g = clip8(y - ((22554 * cb + 46802 * cr + 32768) >> 16));
    b = clip8(y + ((116130 * cb + 32768) >> 16));
}

// ------------------------------------------------------------------------------------------------ subsampled chroma
// DESIGN.md §9, "Subsampled Motion-JPEG decoding": the luma component has H x V = 2 x 1 (4:2:2) or 2 x 2 (4:2:0)
// blocks in an MCU of 8H x 8V pixels, Cb and Cr one each.

VA_JPEG_FN constexpr int mcu_blocks(int lh, int lv) { return lh * lv + 2; }

// Block k of the MCU (row, col) of a frame of my x mx MCUs, in coding order: Y (V rows of H blocks, row by row), Cb,
// Cr.  Returns the block's index in the frame's coefficients [Y: my V x mx H blocks | Cb: my x mx | Cr: my x mx]
// and sets its component.
VA_JPEG_FN int64_t mcu_block_at(int k, int lh, int lv, int64_t my, int64_t mx, int64_t row, int64_t col, int &comp)
{
    const int luma = lh * lv;
    if (k < luma) {
        comp = 0;
        return (row * lv + k / lh) * (mx * lh) + col * lh + k % lh;
    }
    comp = 1 + k - luma;
    return (int64_t)k * my * mx + row * mx + col;           // the Y planes hold lh * lv * my * mx blocks
}

// libjpeg's triangle filter is used on a chroma plane of more than 2 real columns; a narrower plane (a frame of at
// most 4 columns) is replicated in both directions
VA_JPEG_FN bool triangle_used(int cw) { return cw > 2; }

// the real sample nearest to sample i of 0 .. n - 1
VA_JPEG_FN int nearest_sample(int i, int n) { return i < 0 ? 0 : i > n - 1 ? n - 1 : i; }

// the sample that pixel g of a doubled direction blends its own sample g >> 1 with: the one before for an even g,
// behind for an odd g, clamped to the real samples; its own sample where the plane is replicated
VA_JPEG_FN int blend_sample(int g, int n, bool triangle)
{
    return triangle ? nearest_sample((g >> 1) + ((g & 1) ? 1 : -1), n) : g >> 1;
}

// V = 2, the vertical step: four times the sample of a pixel row from its own chroma row and the blended one
VA_JPEG_FN int upsample_rows(int own, int other) { return 3 * own + other; }

// the horizontal step at pixel column g: `own` and `other` are the values of blend_sample's two columns, 4 times
// the sample after upsample_rows (lv == 2) or the samples themselves (lv == 1)
VA_JPEG_FN int upsample_columns(int own, int other, int g, int lv)
{
    const int sum = 3 * own + other;
    if (lv == 2)
        return (sum + ((g & 1) ? 7 : 8)) >> 4;
    return (sum + ((g & 1) ? 2 : 1)) >> 2;
}

// the upsampled sample of pixel (gy, gx) of a chroma plane with ch x cw real samples, read through c(row, column);
// H = 2
template <class Fetch>
VA_JPEG_FN int upsampled_at(Fetch c, int gy, int gx, int lv, int ch, int cw)
{
    const bool tri = triangle_used(cw);
    const int i = gx >> 1, i2 = blend_sample(gx, cw, tri);
    if (lv == 2) {
        const int j = gy >> 1, j2 = blend_sample(gy, ch, tri);
        return upsample_columns(upsample_rows(c(j, i), c(j2, i)), upsample_rows(c(j, i2), c(j2, i2)), gx, 2);
    }
    return upsample_columns(c(gy, i), c(gy, i2), gx, 1);
}

}  // namespace va_jpeg
