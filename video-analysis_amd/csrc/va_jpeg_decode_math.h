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

// ------------------------------------------------------------------------------------------------ split segments
// DESIGN.md §9, "Split Motion-JPEG decoding": one entropy segment, the raw bytes [b, e), decoded by one lane per
// subsequence of S raw bytes.  A state is where the serial decoder stands in front of a symbol; the scan carries
// states from lane to lane until they are the serial decoder's, the write pass decodes from them.
//
// q: the raw offset of the byte that holds the next unread bit, never a stuffing byte (a 00 behind an FF, as refill
// skips it), or e where the segment is used up; -1 is END.  w = bit | k << 3 | z << 6: the bit 0 .. 7 (0 is the
// byte's highest), the block's index k in the MCU, z = 0 in front of a DC symbol or the zigzag index 1 .. 63 of the
// next AC symbol.
struct ScanState {
    int64_t q;
    int32_t w, unused;
};

VA_JPEG_FN ScanState scan_state(int64_t q, int bit, int k, int z) { return ScanState{q, bit | k << 3 | z << 6, 0}; }
VA_JPEG_FN ScanState scan_end() { return ScanState{-1, 0, 0}; }
VA_JPEG_FN bool same_state(const ScanState &a, const ScanState &b) { return a.q == b.q && a.w == b.w; }
VA_JPEG_FN int state_bit(const ScanState &s) { return s.w & 7; }
VA_JPEG_FN int state_k(const ScanState &s) { return s.w >> 3 & 7; }
VA_JPEG_FN int state_z(const ScanState &s) { return s.w >> 6 & 63; }

// the subsequences of a segment of len raw bytes: at least one, the last one ends with the segment
VA_JPEG_FN int64_t subsequences(int64_t len, int sub) { return len > sub ? (len + sub - 1) / sub : 1; }

// what lane i > 0 enters with before it has heard of its predecessor: the first non-stuffing byte of its subsequence
VA_JPEG_FN ScanState scan_guess(const uint8_t *p, int64_t b, int64_t at)
{
    return scan_state(at > b && p[at] == 0 && p[at - 1] == 0xFFu ? at + 1 : at, 0, 0, 0);
}

// a bit reader that knows where it stands: (q, bit) follow from the bits consumed, not from how far `r` has read ahead
struct SpanReader {
    BitReader r;
    int64_t q;
    int bit;
};

VA_JPEG_FN SpanReader open_span(const uint8_t *p, int64_t e, int64_t q, int bit)
{
    q = q < 0 ? e : q < e ? q : e;
    SpanReader s{open_bits(p, q, e), q, q < e ? bit : 0};
    refill(s.r);
    skip_bits(s.r, s.bit);                  // q < e: the reader holds at least this byte
    return s;
}

// n bits (at most cnt) have left the reader
VA_JPEG_FN void span_moved(SpanReader &s, int n)
{
    s.bit += n;
    while (s.bit >= 8) {
        s.bit -= 8;
        s.q++;
        if (s.q < s.r.end && s.r.p[s.q] == 0 && s.r.p[s.q - 1] == 0xFFu)
            s.q++;
    }
}

// One symbol, the code and its magnitude bits: a DC symbol for z == 0, the AC symbol in front of zigzag index z else.
// The checks are decode_block's in its order (Huffman step, symbol, index, magnitude bits); the DC range is the
// caller's.  A failed symbol consumes nothing.
struct Symbol {
    int32_t status;     // 0 or the status bit
    int next;           // the zigzag index behind the symbol; 64: the block is complete
    int index;          // the zigzag index of `value`, -1 where the symbol carries none (EOB, ZRL)
    int value;          // the DC difference or the coefficient
};

VA_JPEG_FN Symbol read_symbol(SpanReader &s, const HuffDecode &dc, const HuffDecode &ac, int z)
{
    int sym = 0, len = 0;
    const int32_t st = next_symbol(s.r, z ? ac : dc, sym, len);
    if (st)
        return Symbol{st, z, -1, 0};
    int size = sym, next = 1, index = 0;
    if (z) {
        const int run = sym >> 4;
        size = sym & 15;
        if (size == 0) {
            if (run != 0 && run != 15)
                return Symbol{kStatusBadCode, z, -1, 0};
            if (run == 15 && z + 16 > 64)
                return Symbol{kStatusOverrun, z, -1, 0};
            skip_bits(s.r, len);
            span_moved(s, len);
            return Symbol{0, run ? z + 16 : 64, -1, 0};
        }
        if (size > 10)
            return Symbol{kStatusBadCode, z, -1, 0};
        index = z + run;
        if (index > 63)
            return Symbol{kStatusOverrun, z, -1, 0};
        next = index + 1;
    } else if (sym > 11) {
        return Symbol{kStatusBadCode, z, -1, 0};
    }
    if (len + size > s.r.cnt)
        return Symbol{kStatusTruncated, z, -1, 0};
    skip_bits(s.r, len);
    const int value = receive_extend(s.r, size);
    span_moved(s, len + size);
    return Symbol{0, next, index, value};
}

// the component of block k of an MCU of `blocks` blocks, the first `luma` of them Y
VA_JPEG_FN int mcu_component(int k, int blocks, int luma) { return blocks == 1 || k < luma ? 0 : k - luma + 1; }

// What a lane of the scan learns from its subsequence [.., stop): where the decoder stands behind it, how many
// blocks begin in it, and the sum of their DC differences per component (uint32: behind an error the sums mean
// nothing and may wrap).
struct ScanLane {
    ScanState exit;
    int32_t begun;
    uint32_t dc[3];
};

// The scan step, from `entry` while the state lies in front of `stop` (at most e).  A symbol that needs bits beyond
// e ends the scan (END).  Every other failure moves one bit on, to a DC symbol of the same block: the recovery rule,
// without which a lane that was guessed wrong would never meet the right chain.  tabs: [component][DC, AC].
VA_JPEG_FN ScanLane scan_lane(const uint8_t *p, int64_t e, ScanState entry, int64_t stop, const HuffDecode *tabs,
                              int blocks, int luma)
{
    ScanLane out{entry, 0, {0, 0, 0}};
    if (entry.q < 0)
        return out;
    SpanReader s = open_span(p, e, entry.q, state_bit(entry));
    int k = state_k(entry) % blocks, z = state_z(entry);
    while (s.q < stop) {
        const int comp = mcu_component(k, blocks, luma);
        const Symbol sym = read_symbol(s, tabs[2 * comp], tabs[2 * comp + 1], z);
        out.begun += z == 0;
        if (sym.status == kStatusTruncated) {
            out.exit = scan_end();
            return out;
        }
        if (sym.status) {
            skip_bits(s.r, 1);
            span_moved(s, 1);
            z = 0;
            continue;
        }
        if (z == 0)
            out.dc[comp] += (uint32_t)sym.value;
        z = sym.next;
        if (z == 64) {
            z = 0;
            k = k + 1 == blocks ? 0 : k + 1;
        }
    }
    out.exit = scan_state(s.q, s.bit, k, z);
    return out;
}

// The write pass of one lane: the real decode from the lane's entry state while the state lies in front of `stop`
// (the last lane: no stop, it goes on while blocks remain, so that a stream which ends early is reported where the
// serial decoder reports it) and blocks remain.  `block` comes in as the number of blocks begun in front of the
// entry, pred as the sums of the DC differences in front of it; store(block in decode order, natural index,
// value).  Returns 0, or the status bit of the first error with its block in `block`; the checks are decode_block's
// in its order.
template <class Store>
VA_JPEG_FN int32_t write_lane(const uint8_t *p, int64_t e, ScanState entry, int64_t stop, bool last,
                              const HuffDecode *tabs, int blocks, int luma, int64_t total, int64_t &block,
                              uint32_t *pred, Store store)
{
    if (entry.q < 0)
        return 0;
    SpanReader s = open_span(p, e, entry.q, state_bit(entry));
    int z = state_z(entry);
    int64_t cur = z ? block - 1 : block;
    if (cur < 0)
        return 0;
    while (cur < total && (last || s.q < stop)) {
        const int comp = mcu_component((int)(cur % blocks), blocks, luma);
        const Symbol sym = read_symbol(s, tabs[2 * comp], tabs[2 * comp + 1], z);
        if (sym.status) {
            block = cur;
            return sym.status;
        }
        if (z == 0) {
            pred[comp] += (uint32_t)sym.value;
            const int32_t v = (int32_t)pred[comp];
            if (v < -2048 || v > 2047) {
                block = cur;
                return kStatusBadCode;
            }
            store(cur, 0, (int)v);
        } else if (sym.index >= 0) {
            store(cur, zigzag_at(sym.index), sym.value);
        }
        z = sym.next;
        if (z == 64) {
            z = 0;
            cur++;
        }
    }
    return 0;
}

// an error as one word whose minimum over a frame is the serial decoder's error: the block in decode order above
// the status bit
VA_JPEG_FN uint64_t error_word(int64_t block, int32_t status) { return (uint64_t)block << 4 | (uint64_t)status; }
constexpr uint64_t kNoError = ~(uint64_t)0;

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
