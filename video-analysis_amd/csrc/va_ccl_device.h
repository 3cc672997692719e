// va_ccl_device.h -- the device-side definitions that the labelling passes (va_ccl.hip) and the contour
//                    tracers (va_contours.hip) share: the lane <-> (row, word span) map of the sparse passes and
//                    the encoding of a forest word.  Included by those two files only.
#pragma once
#include "va_common.h"

namespace va {

constexpr int kBlock = 256;            // 4 waves

// The sparse passes (init / link / flatten / rank) map a wave onto EIGHT consecutive rows:
// lane = (row = lane & 7, word group = lane >> 3), each lane walks a contiguous span of the
// row's words.  Compared with one row per wave this cuts the number of waves 8x and, more
// importantly, puts the unions of vertically adjacent runs (the same word column on
// consecutive rows -- blob edges) on different lanes, so their dependent load/atomic chains run
// in parallel instead of one after the other.
constexpr int kRowsPerWave = 8;
constexpr int kSparseRowsPerBlock = kRowsPerWave * (kBlock / kWave);   // 32

// a ranked forest word is negative: -(label) at a component's first pixel (its root); the per-frame kernel writes
// -(label | kNonRootBit) at the other run starts
constexpr int kNonRootBit = 1 << 30;

struct SpanCtx {
    bool valid;      // this lane has a row and a non-empty word span
    int lane, f, y;
    size_t row;      // f*h + y
    int w0, w1;      // word span [w0, w1)
};

static __device__ __forceinline__ SpanCtx span_ctx(int h, int w32, size_t total_rows)
{
    SpanCtx c;
    c.lane = threadIdx.x & (kWave - 1);
    c.row = (size_t)blockIdx.x * kSparseRowsPerBlock + (size_t)(threadIdx.x >> 6) * kRowsPerWave +
            (c.lane & (kRowsPerWave - 1));
    const int g = c.lane >> 3, G = (w32 + 7) >> 3;
    c.w0 = g * G;
    c.w1 = min(w32, c.w0 + G);
    const bool has_row = c.row < total_rows;
    c.valid = has_row && c.w0 < c.w1;
    const size_t r = has_row ? c.row : 0;
    c.f = (int)(r / h);
    c.y = (int)(r % h);
    return c;
}

}  // namespace va
