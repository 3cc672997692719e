// va_sliding_median_math.h -- the state layout and the per-pixel step of the sliding-window median (DESIGN.md §9,
// "Sliding median") that the kernels of va_sliding_median.hip and the host test tests/sliding_median_shim.cpp share.
//
// A pixel keeps the histogram of the values in its window (256 counters), and a tracker: `lower`, the value at rank
// (cnt - 1) / 2 of the sorted window, `below`, the count of window values under `lower`, and `upper`, the value at
// rank cnt / 2.  A frame takes the outputs from the tracker, removes the leaving value, adds the entering one, and
// walks `lower` bin by bin to the new rank; `upper` is `lower` when its bin reaches rank cnt / 2 and the next
// non-empty bin otherwise.  The leaving value is removed before the entering one is added, so no counter ever holds
// more than `window`: a uint8 counter is enough up to 255, a uint16 counter up to 65535.
//
// State (the caller's memory, all zeros = the empty window), for px pixels in tiles of kTilePixels:
//   tile i at i * tile_bytes(window):  hist [256][kTilePixels] counters, bin-major, pixel q of the tile in column
//                                      column(q, counter bytes); lower[kTilePixels] u8; upper[kTilePixels] u8;
//                                      below[kTilePixels] u16
//   ring at tiles * tile_bytes:        [window][tiles * kTilePixels] u8, frame k in slot k % window
// The pixels of the last tile beyond px are kept like any other, on frames of zeros.  Every index into the histogram
// is a byte value or a tracker byte, so a state of arbitrary bytes is walked inside its tile, and every walk ends
// after at most 255 steps.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VA_SLIDE_HD __host__ __device__ __forceinline__
#else
#define VA_SLIDE_HD inline
#endif

namespace va_slide {

constexpr int kTilePixels = 128;             // L: the pixels of a workgroup, two waves
constexpr int kBins = 256;
constexpr int kMaxWindow = 65535;            // a uint16 counter holds the whole window
constexpr int kByteWindow = 255;             // ... and a uint8 counter this much

VA_SLIDE_HD size_t counter_bytes(int window) { return window <= kByteWindow ? 1 : 2; }
VA_SLIDE_HD size_t hist_bytes(int window) { return (size_t)kBins * kTilePixels * counter_bytes(window); }
VA_SLIDE_HD size_t tile_bytes(int window) { return hist_bytes(window) + 4 * (size_t)kTilePixels; }
VA_SLIDE_HD size_t tiles(size_t px) { return (px + kTilePixels - 1) / kTilePixels; }
VA_SLIDE_HD size_t ring_offset(size_t px, int window) { return tiles(px) * tile_bytes(window); }
VA_SLIDE_HD size_t ring_stride(size_t px) { return tiles(px) * kTilePixels; }
VA_SLIDE_HD size_t state_bytes(size_t px, int window)
{
    return ring_offset(px, window) + (size_t)window * ring_stride(px);
}
// the tracker planes of a tile, from the tile's first byte
VA_SLIDE_HD size_t lower_offset(int window) { return hist_bytes(window); }
VA_SLIDE_HD size_t upper_offset(int window) { return hist_bytes(window) + kTilePixels; }
VA_SLIDE_HD size_t below_offset(int window) { return hist_bytes(window) + 2 * (size_t)kTilePixels; }

// The column of pixel q (0 .. kTilePixels - 1) in a histogram row.  The 32 lanes that the LDS serves together are
// the pixels 32 g .. 32 g + 31: they get the 32 dwords (banks) of a row, whatever bins they touch -- group g takes
// byte g of every dword (uint8 counters), or half g % 2 of the dwords 32 (g / 2) .. (uint16 counters).
VA_SLIDE_HD uint32_t column(uint32_t q, size_t counter)
{
    return counter == 1 ? ((q & 31u) << 2) | (q >> 5) : ((q & 31u) << 1) | ((q >> 5) & 1u) | (q & 64u);
}

// One frame of one pixel.  h: the pixel's column of the histogram (bin v at h[v * kTilePixels]); cnt: the values in
// the window before this frame (min(k, window)); leaves: cnt == window, and y is the value of frame k - window.
// The outputs are those of frame k; lower / upper / below leave as the tracker of frame k + 1.
template <class T>
VA_SLIDE_HD void step(T *h, uint32_t &lower, uint32_t &upper, uint32_t &below, uint32_t cnt, uint32_t x, bool leaves,
                      uint32_t y, uint32_t &out_lower, uint32_t &out_upper, uint32_t &out_diff)
{
    out_lower = lower;
    out_upper = upper;
    const int32_t d = 2 * (int32_t)x - (int32_t)lower - (int32_t)upper;
    const uint32_t mag = (uint32_t)(d < 0 ? -d : d) >> 1;
    out_diff = mag > 255u ? 255u : mag;
    if (leaves) {
        h[y * kTilePixels] = (T)(h[y * kTilePixels] - 1);
        below -= y < lower;
    } else {
        cnt++;
    }
    h[x * kTilePixels] = (T)(h[x * kTilePixels] + 1);
    below += x < lower;
    const uint32_t rank = (cnt - 1) >> 1;
    while (below > rank && lower > 0) {
        lower--;
        below -= h[lower * kTilePixels];
    }
    uint32_t c = h[lower * kTilePixels];
    while (below + c <= rank && lower < 255) {
        below += c;
        lower++;
        c = h[lower * kTilePixels];
    }
    upper = lower;
    if (below + c <= (cnt >> 1)) {
        while (upper < 255) {
            upper++;
            if (h[upper * kTilePixels])
                break;
        }
    }
}

}  // namespace va_slide
