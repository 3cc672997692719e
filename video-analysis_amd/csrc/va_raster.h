// va_raster.h -- OpenCV's integer rasterisers (drawing.cpp) as plain inline C++ that compiles for the host and for
// the device: clipLine, the 8-connected Line (LineIterator, left to right) and the integer Circle.  va_polygon.hip
// draws the edges of fillPoly with them, va_compose.hip the polylines and circles of a composed frame, and
// tests/raster_shim.cpp compiles them with the host compiler.  The definitions are pinned in DESIGN.md §9,
// "Polygons" and "Composer".  Every rasteriser hands its pixels to a `plot(x, y)` callable, inside the image only.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VA_RASTER_FN __host__ __device__ inline
#else
#define VA_RASTER_FN inline
#endif

namespace va {

// OpenCV's clipLine (drawing.cpp) on int64 points: the corrections are computed in double and truncated
VA_RASTER_FN bool clip_line(int64_t w, int64_t h, int64_t &x1, int64_t &y1, int64_t &x2, int64_t &y2)
{
    const int64_t right = w - 1, bottom = h - 1;
    if (w <= 0 || h <= 0)
        return false;
    int c1 = (x1 < 0) + (x1 > right) * 2 + (y1 < 0) * 4 + (y1 > bottom) * 8;
    int c2 = (x2 < 0) + (x2 > right) * 2 + (y2 < 0) * 4 + (y2 > bottom) * 8;
    if ((c1 & c2) == 0 && (c1 | c2) != 0) {
        int64_t a;
        if (c1 & 12) {
            a = c1 < 8 ? 0 : bottom;
            x1 += (int64_t)((double)(a - y1) * (double)(x2 - x1) / (double)(y2 - y1));
            y1 = a;
            c1 = (x1 < 0) + (x1 > right) * 2;
        }
        if (c2 & 12) {
            a = c2 < 8 ? 0 : bottom;
            x2 += (int64_t)((double)(a - y2) * (double)(x2 - x1) / (double)(y2 - y1));
            y2 = a;
            c2 = (x2 < 0) + (x2 > right) * 2;
        }
        if ((c1 & c2) == 0 && (c1 | c2) != 0) {
            if (c1) {
                a = c1 == 1 ? 0 : right;
                y1 += (int64_t)((double)(a - x1) * (double)(y2 - y1) / (double)(x2 - x1));
                x1 = a;
                c1 = 0;
            }
            if (c2) {
                a = c2 == 1 ? 0 : right;
                y2 += (int64_t)((double)(a - x2) * (double)(y2 - y1) / (double)(x2 - x1));
                x2 = a;
                c2 = 0;
            }
        }
    }
    return (c1 | c2) == 0;
}

// Line(img, p1, p2, color, 8): LineIterator(img, p1, p2, 8, leftToRight = true); plot(x, y) per pixel
template <typename Plot>
VA_RASTER_FN void line8(int w, int h, int64_t x1, int64_t y1, int64_t x2, int64_t y2, Plot plot)
{
    if (x1 < 0 || x1 >= w || x2 < 0 || x2 >= w || y1 < 0 || y1 >= h || y2 < 0 || y2 >= h)
        if (!clip_line(w, h, x1, y1, x2, y2))
            return;
    int64_t dx = x2 - x1, dy = y2 - y1;
    if (dx < 0) {                          // left to right: start at the other end
        dx = -dx;
        dy = -dy;
        x1 = x2;
        y1 = y2;
    }
    const int64_t sy = dy < 0 ? -1 : 1;
    dy = dy < 0 ? -dy : dy;
    const bool steep = dy > dx;
    const int64_t major = steep ? dy : dx, minor = steep ? dx : dy;
    int64_t err = major - 2 * minor, x = x1, y = y1;
    for (int64_t k = 0; k <= major; k++) {
        if (x >= 0 && x < w && y >= 0 && y < h)          // always true after clipLine; kept as a guard
            plot(x, y);
        const bool step_minor = err < 0;
        err += -2 * minor + (step_minor ? 2 * major : 0);
        if (steep) {
            y += sy;
            x += step_minor;
        } else {
            x += 1;
            y += step_minor ? sy : 0;
        }
    }
}

// the line into a dense (h, w) plane of T, every pixel of it set to `value`
template <typename T>
VA_RASTER_FN void draw_line8(T *img, int w, int h, int64_t x1, int64_t y1, int64_t x2, int64_t y2, T value)
{
    line8(w, h, x1, y1, x2, y2, [=](int64_t x, int64_t y) { img[y * w + x] = value; });
}

// Circle(img, center, radius, color, fill) of OpenCV: the steps of its integer recurrence, from err = 0, dx = r,
// dy = 0, plus = 1, minus = 2r - 1 while dx >= dy.  Step number `first`, first + stride, ... of the recurrence is
// handed out, so that several lanes can share one circle: every caller runs the whole recurrence and draws its own
// steps.  Outline: the eight points (cx +- dx, cy +- dy), (cx +- dy, cy +- dx); filled: the four spans, rows
// cy +- dy over cx - dx .. cx + dx and rows cy +- dx over cx - dy .. cx + dy; all intersected with the image.
// A negative radius draws nothing.
template <typename Plot>
VA_RASTER_FN void circle_steps(int w, int h, int64_t cx, int64_t cy, int64_t r, bool filled, int64_t first,
                               int64_t stride, Plot plot)
{
    if (r < 0 || w <= 0 || h <= 0)
        return;
    int64_t err = 0, dx = r, dy = 0, plus = 1, minus = 2 * r - 1, step = 0, mine = first;
    while (dx >= dy) {
        if (step == mine) {
            mine += stride;
            if (filled) {
                const int64_t rows[4] = {cy - dy, cy + dy, cy - dx, cy + dx};
                const int64_t half[4] = {dx, dx, dy, dy};
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    const int64_t y = rows[s];
                    if (y < 0 || y >= h)
                        continue;
                    int64_t xa = cx - half[s], xb = cx + half[s];
                    xa = xa < 0 ? 0 : xa;
                    xb = xb > w - 1 ? w - 1 : xb;
                    for (int64_t x = xa; x <= xb; x++)
                        plot(x, y);
                }
            } else {
                const int64_t px[8] = {cx - dx, cx + dx, cx - dx, cx + dx, cx - dy, cx + dy, cx - dy, cx + dy};
                const int64_t py[8] = {cy - dy, cy - dy, cy + dy, cy + dy, cy - dx, cy - dx, cy + dx, cy + dx};
#pragma unroll
                for (int s = 0; s < 8; s++)
                    if (px[s] >= 0 && px[s] < w && py[s] >= 0 && py[s] < h)
                        plot(px[s], py[s]);
            }
        }
        step++;
        dy += 1;
        err += plus;
        plus += 2;
        if (err > 0) {
            err -= minus;
            dx -= 1;
            minus -= 2;
        }
    }
}

}  // namespace va
