// A stand-alone host program around video-analysis_amd/csrc/va_sliding_median_math.h for
// tests/test_sliding_median_host.py: the sliding-window median of DESIGN.md §9, "Sliding median", computed serially
// with the header's state layout and per-pixel step, compiled with the host C++ compiler under
// -fsanitize=address,undefined.  A run is a sequence of calls on one state that starts as zeros, as
// va_sliding_median_u8 would get them: the leaving value of frame j of a call is the call's own frame j - window
// where there is one and the ring's otherwise, and the last `window` frames of a call go into the ring.  Every buffer
// has exactly the size of what it holds -- state_bytes(px, window) of state, (frames - 1) * stride + px bytes of
// frames -- so an access outside the state or beyond a plane's last byte is reported.
// Input (stdin, binary), any number of runs: int64 px, stride, window, calls; `calls` int64 frame counts; the frames
// of all calls as one stack.
// Output (stdout, binary) per run: lower, upper, diff (frames, px) uint8 each; the current lower and upper planes
// (px) each; the state bytes.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "va_sliding_median_math.h"

static bool read_all(void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, stdin) == bytes; }

template <class T>
static void one_call(const uint8_t *frames, int64_t n, size_t px, size_t stride, int window, int64_t n_seen,
                     uint8_t *state, uint8_t *lower_out, uint8_t *upper_out, uint8_t *diff_out)
{
    const size_t tiles = va_slide::tiles(px), tile_bytes = va_slide::tile_bytes(window);
    uint8_t *ring = state + va_slide::ring_offset(px, window);
    const size_t ring_stride = va_slide::ring_stride(px);
    for (size_t p = 0; p < tiles * va_slide::kTilePixels; p++) {
        uint8_t *tile = state + (p / va_slide::kTilePixels) * tile_bytes;
        const uint32_t q = (uint32_t)(p % va_slide::kTilePixels);
        T *h = reinterpret_cast<T *>(tile) + va_slide::column(q, sizeof(T));
        uint8_t *lower_at = tile + va_slide::lower_offset(window) + q, *upper_at = tile + va_slide::upper_offset(window) + q;
        uint16_t *below_at = reinterpret_cast<uint16_t *>(tile + va_slide::below_offset(window)) + q;
        uint32_t lower = *lower_at, upper = *upper_at, below = *below_at;
        for (int64_t j = 0; j < n; j++) {
            const int64_t k = n_seen + j;
            const uint32_t x = p < px ? frames[(size_t)j * stride + p] : 0;
            const bool leaves = k >= window;
            uint32_t y = 0;
            if (leaves && j >= window)
                y = p < px ? frames[(size_t)(j - window) * stride + p] : 0;
            else if (leaves)
                y = ring[(size_t)(k % window) * ring_stride + p];
            uint32_t lo, up, df;
            va_slide::step<T>(h, lower, upper, below, (uint32_t)(k < window ? k : window), x, leaves, y, lo, up, df);
            if (p < px) {
                lower_out[(size_t)j * px + p] = (uint8_t)lo;
                upper_out[(size_t)j * px + p] = (uint8_t)up;
                diff_out[(size_t)j * px + p] = (uint8_t)df;
            }
            if (j + window >= n)
                ring[(size_t)(k % window) * ring_stride + p] = (uint8_t)x;
        }
        *lower_at = (uint8_t)lower;
        *upper_at = (uint8_t)upper;
        *below_at = (uint16_t)below;
    }
}

int main()
{
    int64_t head[4];
    while (fread(head, 1, sizeof head, stdin) == sizeof head) {
        const size_t px = (size_t)head[0], stride = (size_t)head[1];
        const int window = (int)head[2];
        const int64_t calls = head[3];
        if (px < 1 || stride < px || head[2] < 1 || head[2] > va_slide::kMaxWindow || calls < 0 || calls > 1 << 20)
            return 2;
        std::vector<int64_t> counts((size_t)calls);
        if (!read_all(counts.data(), counts.size() * sizeof(int64_t)))
            return 2;
        int64_t total = 0;
        for (int64_t n : counts) {
            if (n < 0)
                return 2;
            total += n;
        }
        std::vector<uint8_t> frames(total ? (size_t)(total - 1) * stride + px : 0);
        if (!read_all(frames.data(), frames.size()))
            return 2;
        std::vector<uint8_t> state(va_slide::state_bytes(px, window), 0);
        std::vector<uint8_t> lower((size_t)total * px, 0xA5), upper(lower), diff(lower);
        int64_t seen = 0;
        for (int64_t n : counts) {
            const uint8_t *at = frames.data() + (size_t)seen * stride;
            uint8_t *lo = lower.data() + (size_t)seen * px, *up = upper.data() + (size_t)seen * px;
            uint8_t *df = diff.data() + (size_t)seen * px;
            if (va_slide::counter_bytes(window) == 1)
                one_call<uint8_t>(at, n, px, stride, window, seen, state.data(), lo, up, df);
            else
                one_call<uint16_t>(at, n, px, stride, window, seen, state.data(), lo, up, df);
            seen += n;
        }
        std::vector<uint8_t> now(2 * px);
        for (size_t p = 0; p < px; p++) {
            const uint8_t *tile = state.data() + (p / va_slide::kTilePixels) * va_slide::tile_bytes(window);
            now[p] = tile[va_slide::lower_offset(window) + p % va_slide::kTilePixels];
            now[px + p] = tile[va_slide::upper_offset(window) + p % va_slide::kTilePixels];
        }
        fwrite(lower.data(), 1, lower.size(), stdout);
        fwrite(upper.data(), 1, upper.size(), stdout);
        fwrite(diff.data(), 1, diff.size(), stdout);
        fwrite(now.data(), 1, now.size(), stdout);
        fwrite(state.data(), 1, state.size(), stdout);
    }
    return 0;
}
