// va_contours.hip -- outer contours of bit-packed masks (A8): the largest contour of a frame, every outer contour
//                    of a frame stack, and the start point of the longest outer contour.
//
// replaces cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)[1]: the largest contour
//          video/analysis/regions.py:178-197, the whole list :180-182, :229-231, :575-576 and
//          video/io/composer.py:228
//
// The tracers start from the labelling forest of va_ccl.hip: launch_ccl(..., paint = false) leaves -(label) at
// the first raster pixel of every component, which is where OpenCV's border following starts too.
#include "va_ccl_device.h"
#include "va_scan.h"

namespace va {

namespace {

// ---- A8: outer border following (cv2.findContours RETR_EXTERNAL / CHAIN_APPROX_SIMPLE) -----
// OpenCV's icvFetchContour walk, started at a component's first raster pixel (= its forest
// root).  Direction codes: 0 E, 1 NE, 2 N, 3 NW, 4 W, 5 SW, 6 S, 7 SE (y grows downwards).
struct BitImage {
    const uint32_t *bits;
    int h, w, w32;
    __device__ __forceinline__ int at(int x, int y) const
    {
        if (x < 0 || x >= w || y < 0 || y >= h)
            return 0;
        return (bits[(size_t)y * w32 + (x >> 5)] >> (x & 31)) & 1u;
    }
};
__device__ __forceinline__ int code_dx(int s) { return (0x1 | 0x2 | 0x80) >> s & 1 ? 1 : ((0x8 | 0x10 | 0x20) >> s & 1 ? -1 : 0); }
__device__ __forceinline__ int code_dy(int s) { return (0x2 | 0x4 | 0x8) >> s & 1 ? -1 : ((0x20 | 0x40 | 0x80) >> s & 1 ? 1 : 0); }

// the eight neighbours of (x, y) as a mask, bit s = the pixel in direction s: eight independent loads (clamped
// coordinates, the result masked), one memory round trip per step of the walk instead of one per probed neighbour
__device__ __forceinline__ uint32_t neighbours8(const BitImage &im, int x, int y)
{
    uint32_t nb = 0;
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const int xx = x + code_dx(s), yy = y + code_dy(s);
        const bool in = (unsigned)xx < (unsigned)im.w && (unsigned)yy < (unsigned)im.h;
        const int xc = min(max(xx, 0), im.w - 1), yc = min(max(yy, 0), im.h - 1);
        const uint32_t bit = (im.bits[(size_t)yc * im.w32 + (xc >> 5)] >> (xc & 31)) & 1u;
        nb |= (in ? bit : 0u) << s;
    }
    return nb;
}

template <class Emit>
__device__ void trace_outer_border(const BitImage &im, int x0, int y0, Emit &emit)
{
    int s_end = 4, s = 4, x1, y1;
    const uint32_t nb0 = neighbours8(im, x0, y0);
    do {
        s = (s - 1) & 7;
        x1 = x0 + code_dx(s);
        y1 = y0 + code_dy(s);
    } while (!((nb0 >> s) & 1u) && s != s_end);
    if (s == s_end) {   // single pixel
        emit(x0, y0);
        return;
    }
    int x3 = x0, y3 = y0, px = x0, py = y0, prev_s = s ^ 4;
    const long long max_steps = 8ll * im.h * im.w + 16;   // a border visits a pixel at most 8 times
    for (long long step = 0; step < max_steps; step++) {
        int x4 = x3, y4 = y3;
        const uint32_t nb = neighbours8(im, x3, y3);
        while (s < 15) {
            ++s;
            x4 = x3 + code_dx(s & 7);
            y4 = y3 + code_dy(s & 7);
            if ((nb >> (s & 7)) & 1u)
                break;
        }
        s &= 7;
        if (s != prev_s) {   // CHAIN_APPROX_SIMPLE: keep a point only where the direction changes
            emit(px, py);
            prev_s = s;
        }
        px += code_dx(s);
        py += code_dy(s);
        if (x4 == x0 && y4 == y0 && x3 == x1 && y3 == y1)
            break;
        x3 = x4;
        y3 = y4;
        s = (s + 4) & 7;
    }
}

struct AreaEmit {   // shoelace sum over the emitted points (cv2.contourArea before *0.5 and abs)
    long long cross = 0;
    int n = 0, fx = 0, fy = 0, lx = 0, ly = 0;
    __device__ __forceinline__ void operator()(int x, int y)
    {
        if (n == 0) {
            fx = x;
            fy = y;
        } else {
            cross += (long long)lx * y - (long long)ly * x;
        }
        lx = x;
        ly = y;
        n++;
    }
    __device__ __forceinline__ long long twice_area() const
    {
        long long c = cross + ((long long)lx * fy - (long long)ly * fx);   // close the polygon
        return c < 0 ? -c : c;
    }
};

// every component: trace, keep max (contour area, then first-pixel index) per frame.  OpenCV
// returns the contours most-recent-first, so np.argmax's "first maximum" is the component
// whose first pixel comes LAST in raster order: the larger index wins ties.
__global__ void __launch_bounds__(kBlock)
contour_areas_kernel(const uint32_t *__restrict__ bits, const int32_t *__restrict__ forest,
                     unsigned long long *__restrict__ best, int h, int w, int w32,
                     size_t total_rows)
{
    const SpanCtx c = span_ctx(h, w32, total_rows);
    if (!c.valid)
        return;
    const uint32_t *row = bits + c.row * w32;
    const int32_t *L = forest + (size_t)c.f * h * w;
    BitImage im{bits + (size_t)c.f * h * w32, h, w, w32};
    uint32_t prev = c.w0 > 0 ? row[c.w0 - 1] >> 31 : 0u;
    for (int wi = c.w0; wi < c.w1; wi++) {
        const uint32_t m = row[wi];
        uint32_t s = m & ~((m << 1) | prev);
        prev = m >> 31;
        while (s) {
            const int b = __ffs(s) - 1;
            s &= s - 1;
            const int x = (wi << 5) + b, idx = c.y * w + x;
            const int v = L[idx];
            if (v >= 0 || (-v & kNonRootBit))
                continue;   // not a component's first pixel
            AreaEmit e;
            trace_outer_border(im, x, c.y, e);
            const unsigned long long key =
                ((unsigned long long)e.twice_area() << 32) | (unsigned long long)(unsigned)(idx + 1);
            atomicMax(best + c.f, key);
        }
    }
}

struct PointEmit {
    int32_t *pts;
    int cap;
    AreaEmit a;
    __device__ __forceinline__ void operator()(int x, int y)
    {
        if (a.n < cap) {
            pts[2 * a.n] = x;
            pts[2 * a.n + 1] = y;
        }
        a(x, y);
    }
};

__global__ void contour_points_kernel(const uint32_t *__restrict__ bits,
                                      const unsigned long long *__restrict__ best, int h, int w,
                                      int w32, int32_t *__restrict__ points, int max_points,
                                      int32_t *__restrict__ npoints, double *__restrict__ area)
{
    const int f = blockIdx.x;
    if (threadIdx.x != 0)
        return;
    const unsigned long long key = best[f];
    if (key == 0) {
        npoints[f] = 0;
        if (area)
            area[f] = 0.0;
        return;
    }
    const int idx = (int)(key & 0xFFFFFFFFull) - 1;
    BitImage im{bits + (size_t)f * h * w32, h, w, w32};
    PointEmit e{points + (size_t)f * max_points * 2, max_points, AreaEmit()};
    trace_outer_border(im, idx % w, idx / w, e);
    npoints[f] = e.a.n;
    if (area)
        area[f] = 0.5 * (double)e.a.twice_area();
}

// ---- the start point of get_farthest_points (video/analysis/regions.py:574-583) -----------------
// max(contours, key=cv2.arcLength(c, closed=True)) over the RETR_EXTERNAL contours, first point.
// arcLength adds float32 sqrt(dx*dx + dy*dy) of float32 differences into a double.  Every term is 0
// or a float in [1, 2^16) (a multiple of 2^-23) and the sum stays below 2^30, so the double sum is
// exact in any order: the closing segment may be added last instead of first.
struct ArcEmit {
    double len = 0.0;
    int n = 0, fx = 0, fy = 0, lx = 0, ly = 0;
    __device__ static double seg(int x0, int y0, int x1, int y1)
    {
        const float dx = (float)x1 - (float)x0, dy = (float)y1 - (float)y0;
        return (double)__fsqrt_rn(dx * dx + dy * dy);
    }
    __device__ __forceinline__ void operator()(int x, int y)
    {
        if (n == 0) {
            fx = x;
            fy = y;
        } else {
            len += seg(lx, ly, x, y);
        }
        lx = x;
        ly = y;
        n++;
    }
    __device__ __forceinline__ double total() const { return n ? len + seg(lx, ly, fx, fy) : 0.0; }
};

// RETR_EXTERNAL keeps a component only if it lies in no hole of another: the 4-connected background
// component directly left of its first raster pixel (always background) must reach the frame edge.
// The perimeter ranking needs this test explicitly -- unlike the contour area, a longer outline can
// sit inside a ring's hole.  bg_labels: 4-connected labels of the inverted mask; edge_bits: bit l set
// when background label l touches the frame edge.
__device__ __forceinline__ bool is_external(const int32_t *bgl, const uint32_t *edge_bits, int w, int x, int y)
{
    if (x == 0)
        return true;
    const int l = bgl[(size_t)y * w + x - 1];
    return (edge_bits[l >> 5] >> (l & 31)) & 1u;
}

__global__ void __launch_bounds__(kBlock)
invert_bits_kernel(const uint32_t *__restrict__ bits, uint32_t *__restrict__ inv, int w, int w32, size_t total)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= total)
        return;
    const int wi = (int)(i % w32), nvalid = min(32, w - wi * 32);
    inv[i] = ~bits[i] & (nvalid == 32 ? 0xffffffffu : (1u << nvalid) - 1u);
}

__global__ void __launch_bounds__(kBlock)
edge_labels_kernel(const int32_t *__restrict__ bgl, uint32_t *__restrict__ edge_bits, int h, int w,
                   int edge_words)
{
    const int f = blockIdx.y;
    const int per = 2 * (w + h);
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= per)
        return;
    int x, y;
    if (i < w) {
        x = i;
        y = 0;
    } else if (i < 2 * w) {
        x = i - w;
        y = h - 1;
    } else if (i < 2 * w + h) {
        x = 0;
        y = i - 2 * w;
    } else {
        x = w - 1;
        y = i - 2 * w - h;
    }
    const int l = bgl[(size_t)f * h * w + (size_t)y * w + x];
    if (l > 0)
        atomicOr(edge_bits + (size_t)f * edge_words + (l >> 5), 1u << (l & 31));
}

// pass 0: the longest external outline per frame (atomicMax on the bits of a non-negative double);
// pass 1: among the outlines of exactly that length, the largest first-pixel index (OpenCV lists
// contours most-recent-first and Python's max keeps the first maximum)
template <int PASS>
__global__ void __launch_bounds__(kBlock)
contour_perimeters_kernel(const uint32_t *__restrict__ bits, const int32_t *__restrict__ forest,
                          const int32_t *__restrict__ bg_labels, const uint32_t *__restrict__ edge_bits,
                          int edge_words, unsigned long long *__restrict__ best_len,
                          unsigned long long *__restrict__ best_idx, int h, int w, int w32, size_t total_rows)
{
    const SpanCtx c = span_ctx(h, w32, total_rows);
    if (!c.valid)
        return;
    const uint32_t *row = bits + c.row * w32;
    const int32_t *L = forest + (size_t)c.f * h * w;
    const int32_t *B = bg_labels + (size_t)c.f * h * w;
    const uint32_t *E = edge_bits + (size_t)c.f * edge_words;
    BitImage im{bits + (size_t)c.f * h * w32, h, w, w32};
    uint32_t prev = c.w0 > 0 ? row[c.w0 - 1] >> 31 : 0u;
    for (int wi = c.w0; wi < c.w1; wi++) {
        const uint32_t m = row[wi];
        uint32_t s = m & ~((m << 1) | prev);
        prev = m >> 31;
        while (s) {
            const int b = __ffs(s) - 1;
            s &= s - 1;
            const int x = (wi << 5) + b, idx = c.y * w + x;
            const int v = L[idx];
            if (v >= 0 || (-v & kNonRootBit))
                continue;   // not a component's first pixel
            if (!is_external(B, E, w, x, c.y))
                continue;
            ArcEmit e;
            trace_outer_border(im, x, c.y, e);
            const unsigned long long len = (unsigned long long)__double_as_longlong(e.total());
            if (PASS == 0)
                atomicMax(best_len + c.f, len);
            else if (len == best_len[c.f])
                atomicMax(best_idx + c.f, (unsigned long long)(idx + 1));
        }
    }
}

struct FirstEmit {
    int n = 0, x = -1, y = -1;
    __device__ __forceinline__ void operator()(int px, int py)
    {
        if (n++ == 0) {
            x = px;
            y = py;
        }
    }
};

__global__ void longest_contour_start_kernel(const uint32_t *__restrict__ bits,
                                             const unsigned long long *__restrict__ best_idx, int h, int w,
                                             int w32, int32_t *__restrict__ p1)
{
    const int f = blockIdx.x;
    if (threadIdx.x != 0)
        return;
    const unsigned long long key = best_idx[f];
    FirstEmit e;
    if (key != 0) {
        const int idx = (int)key - 1;
        BitImage im{bits + (size_t)f * h * w32, h, w, w32};
        trace_outer_border(im, idx % w, idx / w, e);
    }
    p1[2 * f] = e.x;
    p1[2 * f + 1] = e.y;
}

// ---- every outer contour of every frame (va_find_contours) -----------------------------------------
// replaces  cv2.findContours(mask.astype(np.uint8), cv2.RETR_EXTERNAL, cv2.CHAIN_APPROX_SIMPLE)[1] used as a
//           whole list: video/analysis/regions.py:180-182, :229-231, :575-576, video/io/composer.py:228
// A contour starts at a forest root (its component's first raster pixel) that passes is_external.  OpenCV
// lists the most recently found contour first, so contour k of frame f is the start with the k-th LARGEST pixel
// index, at global slot frame_first[f] + k.  Slots are ranks: counts per cell (a lane's word span of a row, eight
// per row, in raster order), one scan per frame, one scan over the frames -- no atomic decides a position, so two
// runs write identical buffers.  The walks then run over the compacted start list, one lane per slot: a wave
// holds 64 walks instead of the few that a lane-per-span grid finds.
constexpr int kCellsPerRow = 8;   // span_ctx's word groups

// fn(x, idx) for every external start of the lane's span, left to right
template <class F>
__device__ __forceinline__ void for_external_starts(const SpanCtx &c, const uint32_t *bits, const int32_t *forest,
                                                    const int32_t *bg_labels, const uint32_t *edge_bits,
                                                    int edge_words, int h, int w, int w32, F &&fn)
{
    const uint32_t *row = bits + c.row * w32;
    const int32_t *L = forest + (size_t)c.f * h * w;
    const int32_t *B = bg_labels + (size_t)c.f * h * w;
    const uint32_t *E = edge_bits + (size_t)c.f * edge_words;
    uint32_t prev = c.w0 > 0 ? row[c.w0 - 1] >> 31 : 0u;
    for (int wi = c.w0; wi < c.w1; wi++) {
        const uint32_t m = row[wi];
        uint32_t s = m & ~((m << 1) | prev);
        prev = m >> 31;
        while (s) {
            const int b = __ffs(s) - 1;
            s &= s - 1;
            const int x = (wi << 5) + b, idx = c.y * w + x;
            const int v = L[idx];
            if (v >= 0 || (-v & kNonRootBit))
                continue;   // not a component's first pixel
            if (is_external(B, E, w, x, c.y))
                fn(x, idx);
        }
    }
}

__global__ void __launch_bounds__(kBlock)
contour_cell_count_kernel(const uint32_t *__restrict__ bits, const int32_t *__restrict__ forest,
                          const int32_t *__restrict__ bg_labels, const uint32_t *__restrict__ edge_bits,
                          int edge_words, int32_t *__restrict__ cell_cnt, int h, int w, int w32, size_t total_rows)
{
    const SpanCtx c = span_ctx(h, w32, total_rows);
    int cnt = 0;
    if (c.valid)
        for_external_starts(c, bits, forest, bg_labels, edge_bits, edge_words, h, w, w32, [&](int, int) { cnt++; });
    if (c.row < total_rows)   // (a lane whose span is empty still owns its cell)
        cell_cnt[c.row * kCellsPerRow + (c.lane >> 3)] = cnt;
}

// in place, one workgroup per frame: cell counts -> exclusive prefix within the frame (ascending raster order)
__global__ void __launch_bounds__(kBlock)
contour_cell_scan_kernel(int32_t *__restrict__ cells, int32_t *__restrict__ ncontours, long long cells_per_frame)
{
    __shared__ long long part[kBlock / kWave];
    int32_t *c = cells + (size_t)blockIdx.x * cells_per_frame;
    const long long per = (cells_per_frame + kBlock - 1) / kBlock;
    const long long i0 = min(cells_per_frame, threadIdx.x * per), i1 = min(cells_per_frame, i0 + per);
    long long s = 0, sum;
    for (long long i = i0; i < i1; i++)
        s += c[i];
    int run = (int)block_exclusive<kBlock / kWave>(s, part, sum);
    for (long long i = i0; i < i1; i++) {
        const int v = c[i];
        c[i] = run;
        run += v;
    }
    if (threadIdx.x == 0)
        ncontours[blockIdx.x] = (int32_t)sum;
}

// one workgroup: first[0 .. n] = exclusive scan of in[0 .. n), *total = first[n]
template <class T>
__global__ void __launch_bounds__(kBlock)
contour_frame_scan_kernel(const T *__restrict__ in, int n, long long *__restrict__ first,
                          long long *__restrict__ total)
{
    __shared__ long long part[kBlock / kWave];
    const int per = (n + kBlock - 1) / kBlock;
    const int i0 = min(n, (int)threadIdx.x * per), i1 = min(n, i0 + per);
    long long s = 0, sum;
    for (int i = i0; i < i1; i++)
        s += in[i];
    long long run = block_exclusive<kBlock / kWave>(s, part, sum);
    for (int i = i0; i < i1; i++) {
        first[i] = run;
        run += in[i];
    }
    if (threadIdx.x == 0) {
        first[n] = sum;
        *total = sum;
    }
}

// starts[slot] = (frame, first-pixel index), descending within the frame
__global__ void __launch_bounds__(kBlock)
contour_list_kernel(const uint32_t *__restrict__ bits, const int32_t *__restrict__ forest,
                    const int32_t *__restrict__ bg_labels, const uint32_t *__restrict__ edge_bits, int edge_words,
                    const int32_t *__restrict__ cell_off, const int32_t *__restrict__ ncontours,
                    const long long *__restrict__ frame_first, int2 *__restrict__ starts, int h, int w, int w32,
                    size_t total_rows)
{
    const SpanCtx c = span_ctx(h, w32, total_rows);
    if (!c.valid)
        return;
    long long slot = frame_first[c.f] + ncontours[c.f] - 1 - cell_off[c.row * kCellsPerRow + (c.lane >> 3)];
    for_external_starts(c, bits, forest, bg_labels, edge_bits, edge_words, h, w, w32,
                        [&](int, int idx) { starts[slot--] = make_int2(c.f, idx); });
}

struct RecordEmit {   // all that a contour's record holds, from one walk
    AreaEmit a;
    ArcEmit l;
    int xmin = 0x7fffffff, ymin = 0x7fffffff, xmax = -1, ymax = -1;
    __device__ __forceinline__ void operator()(int x, int y)
    {
        a(x, y);
        l(x, y);
        xmin = min(xmin, x);
        ymin = min(ymin, y);
        xmax = max(xmax, x);
        ymax = max(ymax, y);
    }
};

// count pass: one lane per slot of the compacted list (grid-stride: the host does not know the total)
__global__ void __launch_bounds__(kWave)
contour_count_kernel(const uint32_t *__restrict__ bits, const int2 *__restrict__ starts,
                     const long long *__restrict__ totals, int32_t *__restrict__ npts,
                     va_contour_info *__restrict__ info, long long cap_contours, int h, int w, int w32)
{
    const long long total = totals[0], stride = (long long)gridDim.x * kWave;
    for (long long slot = (long long)blockIdx.x * kWave + threadIdx.x; slot < total; slot += stride) {
        const int2 s = starts[slot];
        const int x0 = s.y % w, y0 = s.y / w;
        BitImage im{bits + (size_t)s.x * h * w32, h, w, w32};
        RecordEmit e;
        trace_outer_border(im, x0, y0, e);
        npts[slot] = e.a.n;
        if (slot < cap_contours) {
            va_contour_info *r = info + slot;
            r->frame = s.x;
            r->npoints = e.a.n;
            r->start_x = x0;
            r->start_y = y0;
            r->rect_x = e.xmin;
            r->rect_y = e.ymin;
            r->rect_w = e.xmax - e.xmin + 1;
            r->rect_h = e.ymax - e.ymin + 1;
            r->area = 0.5 * (double)e.a.twice_area();
            r->perimeter = e.l.total();
        }
    }
}

// one workgroup per frame: the number of points of its contours
__global__ void __launch_bounds__(kBlock)
contour_frame_points_kernel(const int32_t *__restrict__ npts, const long long *__restrict__ frame_first,
                            long long *__restrict__ frame_pts)
{
    __shared__ long long part[kBlock / kWave];
    const long long a = frame_first[blockIdx.x], b = frame_first[blockIdx.x + 1];
    long long s = 0, sum;
    for (long long i = a + threadIdx.x; i < b; i += kBlock)
        s += npts[i];
    block_exclusive<kBlock / kWave>(s, part, sum);
    if (threadIdx.x == 0)
        frame_pts[blockIdx.x] = sum;
}

// one workgroup per frame: point_off[slot] for the slots within the capacity, and the end of the last one
__global__ void __launch_bounds__(kBlock)
contour_offsets_kernel(const int32_t *__restrict__ npts, const long long *__restrict__ frame_first,
                       const long long *__restrict__ pt_first, const long long *__restrict__ totals,
                       long long *__restrict__ point_off, long long cap_contours)
{
    __shared__ long long part[kBlock / kWave];
    const long long a = frame_first[blockIdx.x], b = frame_first[blockIdx.x + 1], total = totals[0];
    const long long per = (b - a + kBlock - 1) / kBlock;
    const long long i0 = min(b, a + threadIdx.x * per), i1 = min(b, i0 + per);
    long long s = 0, sum;
    for (long long i = i0; i < i1; i++)
        s += npts[i];
    long long run = pt_first[blockIdx.x] + block_exclusive<kBlock / kWave>(s, part, sum);
    for (long long i = i0; i < i1; i++) {
        if (i <= cap_contours)
            point_off[i] = run;
        run += npts[i];
        if (i == total - 1 && total <= cap_contours)
            point_off[total] = run;
    }
    if (total == 0 && blockIdx.x == 0 && threadIdx.x == 0)
        point_off[0] = 0;
}

struct RaggedPointEmit {
    int2 *pts;
    int n = 0;
    __device__ __forceinline__ void operator()(int x, int y) { pts[n++] = make_int2(x, y); }
};

// emit pass: the same walk again, writing the points of every contour that fits whole
__global__ void __launch_bounds__(kWave)
contour_emit_kernel(const uint32_t *__restrict__ bits, const int2 *__restrict__ starts,
                    const long long *__restrict__ totals, const int32_t *__restrict__ npts,
                    const long long *__restrict__ point_off, long long cap_contours, int2 *__restrict__ points,
                    long long cap_points, int h, int w, int w32)
{
    const long long total = min(totals[0], cap_contours), stride = (long long)gridDim.x * kWave;
    for (long long slot = (long long)blockIdx.x * kWave + threadIdx.x; slot < total; slot += stride) {
        const long long off = point_off[slot];
        if (off + npts[slot] > cap_points)
            continue;
        const int2 s = starts[slot];
        BitImage im{bits + (size_t)s.x * h * w32, h, w, w32};
        RaggedPointEmit e{points + off};
        trace_outer_border(im, s.y % w, s.y / w, e);
    }
}

}  // namespace

// outer contour of the component with the largest contour area (8-connectivity), on a forest
// prepared by launch_ccl(..., paint = false): roots hold -(label) at their first pixel
static int launch_largest_contour(const uint32_t *bits, const int32_t *forest, int n, int h, int w,
                                  unsigned long long *best_keys, int32_t *points, int max_points,
                                  int32_t *npoints, double *area, hipStream_t st)
{
    VA_REQUIRE(bits && forest && best_keys && points && npoints && max_points > 0,
               "largest_contour: bad argument");
    if (n == 0)
        return VA_OK;
    const int w32 = words_per_row(w);
    const size_t total_rows = (size_t)n * h;
    VA_HIP(hipMemsetAsync(best_keys, 0, sizeof(unsigned long long) * n, st));
    const int sgrid = cdiv((long long)total_rows, 32);
    contour_areas_kernel<<<sgrid, 256, 0, st>>>(bits, forest, best_keys, h, w, w32, total_rows);
    VA_LAUNCH_CHECK("contour_areas_kernel");
    contour_points_kernel<<<n, 64, 0, st>>>(bits, best_keys, h, w, w32, points, max_points, npoints,
                                          area);
    VA_LAUNCH_CHECK("contour_points_kernel");
    return VA_OK;
}

int edge_label_words(int h, int w) { return (int)(((size_t)h * w + 2 + 31) / 32); }

static int launch_invert_bits(const uint32_t *bits, uint32_t *inv, int n, int h, int w, hipStream_t st)
{
    const int w32 = words_per_row(w);
    const size_t total = (size_t)n * h * w32;
    if (total == 0)
        return VA_OK;
    invert_bits_kernel<<<cdiv((long long)total, kBlock), kBlock, 0, st>>>(bits, inv, w, w32, total);
    VA_LAUNCH_CHECK("invert_bits_kernel");
    return VA_OK;
}

// the frame index of edge_labels_kernel is gridDim.y, which holds at most 65535: longer batches go out in pieces
// (frames are independent; every piece starts at its own frame's labels and edge words)
static int launch_edge_labels(const int32_t *bg_labels, uint32_t *edge_bits, int n, int h, int w, int ew,
                              hipStream_t st)
{
    const unsigned gx = (unsigned)cdiv(2ll * (w + h), kBlock);
    for (int f0 = 0; f0 < n; f0 += kMaxGridYZ) {
        const int k = n - f0 < kMaxGridYZ ? n - f0 : kMaxGridYZ;
        edge_labels_kernel<<<dim3(gx, (unsigned)k), kBlock, 0, st>>>(bg_labels + (size_t)f0 * h * w,
                                                                     edge_bits + (size_t)f0 * ew, h, w, ew);
        VA_LAUNCH_CHECK("edge_labels_kernel");
    }
    return VA_OK;
}

// forest (8-connected, unpainted) and bg_labels (the painted 4-connected labels of the inverted mask) of n frames,
// as the external-contour passes below read them.  counts: 2 n (components, then background components); inv:
// the inverted mask; rows_ws: launch_ccl's workspace, used by both labellings in turn
int launch_outline_labels(const uint32_t *bits, uint32_t *inv, int32_t *forest, int32_t *bg_labels, int32_t *counts,
                          void *rows_ws, size_t rows_bytes, int n, int h, int w, hipStream_t st)
{
    int rc = launch_ccl(bits, forest, counts, n, h, w, 8, rows_ws, rows_bytes, nullptr, 0, st, nullptr,
                        /*paint=*/false);
    if (!rc)
        rc = launch_invert_bits(bits, inv, n, h, w, st);
    if (!rc)
        rc = launch_ccl(inv, bg_labels, counts + n, n, h, w, 4, rows_ws, rows_bytes, nullptr, 0, st, nullptr,
                        /*paint=*/true);
    return rc;
}

// get_farthest_points' default start: the first point of the longest (cv2.arcLength) RETR_EXTERNAL
// contour, per frame, (-1, -1) without one.  forest and bg_labels from launch_outline_labels; edge_bits:
// edge_label_words words per frame; keys: 2 n
int launch_longest_external_start(const uint32_t *bits, const int32_t *forest, const int32_t *bg_labels,
                                  uint32_t *edge_bits, int n, int h, int w, unsigned long long *keys,
                                  int32_t *p1, hipStream_t st)
{
    VA_REQUIRE(bits && forest && bg_labels && edge_bits && keys && p1, "longest contour: NULL argument");
    if (n == 0)
        return VA_OK;
    const int w32 = words_per_row(w), ew = edge_label_words(h, w);
    const size_t total_rows = (size_t)n * h;
    VA_HIP(hipMemsetAsync(keys, 0, 2 * sizeof(unsigned long long) * n, st));
    VA_HIP(hipMemsetAsync(edge_bits, 0, sizeof(uint32_t) * ew * (size_t)n, st));
    int rc = launch_edge_labels(bg_labels, edge_bits, n, h, w, ew, st);
    if (rc)
        return rc;
    const int sgrid = cdiv((long long)total_rows, 32);
    contour_perimeters_kernel<0><<<sgrid, 256, 0, st>>>(bits, forest, bg_labels, edge_bits, ew, keys, keys + n, h,
                                                         w, w32, total_rows);
    VA_LAUNCH_CHECK("contour_perimeters_kernel");
    contour_perimeters_kernel<1><<<sgrid, 256, 0, st>>>(bits, forest, bg_labels, edge_bits, ew, keys, keys + n, h,
                                                         w, w32, total_rows);
    VA_LAUNCH_CHECK("contour_perimeters_kernel");
    longest_contour_start_kernel<<<n, 64, 0, st>>>(bits, keys + n, h, w, w32, p1);
    VA_LAUNCH_CHECK("longest_contour_start_kernel");
    return VA_OK;
}

// 8-connected components of a frame: every other row and column
static size_t max_contours_per_frame(int h, int w) { return (size_t)((h + 1) / 2) * (size_t)((w + 1) / 2); }

// every RETR_EXTERNAL contour of every frame as one ragged list (va_find_contours states the outputs); forest and
// bg_labels from launch_outline_labels.  Scratch: edge_bits edge_label_words words per frame; cells 8 int32 per
// row; frame_first, pt_first n + 1 and frame_pts n int64; starts (8 bytes) and npts (int32) one per possible
// contour, n * max_contours_per_frame of them
struct FindContoursScratch {
    uint32_t *edge_bits;
    int32_t *cells;
    int64_t *frame_first, *frame_pts, *pt_first;
    void *starts;
    int32_t *npts;
};
static int launch_find_contours(const uint32_t *bits, const int32_t *forest, const int32_t *bg_labels,
                                const FindContoursScratch &s, int n, int h, int w, int32_t *ncontours,
                                int64_t *totals, va_contour_info *info, int64_t *point_off, int64_t cap_contours,
                                int32_t *points, int64_t cap_points, hipStream_t st)
{
    VA_REQUIRE(bits && forest && bg_labels && ncontours && totals && info && point_off && points,
               "find_contours: NULL argument");
    if (n == 0)
        return VA_OK;
    const int w32 = words_per_row(w), ew = edge_label_words(h, w);
    const size_t total_rows = (size_t)n * h;
    long long *tot = (long long *)totals, *frame_first = (long long *)s.frame_first;
    long long *frame_pts = (long long *)s.frame_pts, *pt_first = (long long *)s.pt_first;
    int2 *starts = (int2 *)s.starts;
    VA_HIP(hipMemsetAsync(s.edge_bits, 0, sizeof(uint32_t) * ew * (size_t)n, st));
    int rc = launch_edge_labels(bg_labels, s.edge_bits, n, h, w, ew, st);
    if (rc)
        return rc;
    const int sgrid = cdiv((long long)total_rows, kSparseRowsPerBlock);
    contour_cell_count_kernel<<<sgrid, kBlock, 0, st>>>(bits, forest, bg_labels, s.edge_bits, ew, s.cells, h, w, w32,
                                                        total_rows);
    VA_LAUNCH_CHECK("contour_cell_count_kernel");
    contour_cell_scan_kernel<<<n, kBlock, 0, st>>>(s.cells, ncontours, (long long)h * kCellsPerRow);
    VA_LAUNCH_CHECK("contour_cell_scan_kernel");
    contour_frame_scan_kernel<int32_t><<<1, kBlock, 0, st>>>(ncontours, n, frame_first, tot);
    VA_LAUNCH_CHECK("contour_frame_scan_kernel");
    contour_list_kernel<<<sgrid, kBlock, 0, st>>>(bits, forest, bg_labels, s.edge_bits, ew, s.cells, ncontours,
                                                  frame_first, starts, h, w, w32, total_rows);
    VA_LAUNCH_CHECK("contour_list_kernel");
    // the walks: up to 64 waves per CU's worth of single-wave workgroups, each lane striding over the slots
    const size_t worst = (size_t)n * max_contours_per_frame(h, w);
    const size_t wblocks = (worst + kWave - 1) / kWave;
    const int wgrid = wblocks < 8192 ? (int)wblocks : 8192;
    contour_count_kernel<<<wgrid, kWave, 0, st>>>(bits, starts, tot, s.npts, info, cap_contours, h, w, w32);
    VA_LAUNCH_CHECK("contour_count_kernel");
    contour_frame_points_kernel<<<n, kBlock, 0, st>>>(s.npts, frame_first, frame_pts);
    VA_LAUNCH_CHECK("contour_frame_points_kernel");
    contour_frame_scan_kernel<long long><<<1, kBlock, 0, st>>>(frame_pts, n, pt_first, tot + 1);
    VA_LAUNCH_CHECK("contour_frame_scan_kernel");
    contour_offsets_kernel<<<n, kBlock, 0, st>>>(s.npts, frame_first, pt_first, tot, (long long *)point_off,
                                                 cap_contours);
    VA_LAUNCH_CHECK("contour_offsets_kernel");
    contour_emit_kernel<<<wgrid, kWave, 0, st>>>(bits, starts, tot, s.npts, (const long long *)point_off, cap_contours,
                                                 (int2 *)points, cap_points, h, w, w32);
    VA_LAUNCH_CHECK("contour_emit_kernel");
    return VA_OK;
}

// va_largest_contour's workspace: [bits | labelling rows | forest | keys]
namespace {
struct ContourLayout { size_t bits, rows, rows_bytes, forest, keys, total; };
ContourLayout contour_layout(int n, int h, int w)
{
    Carve c;
    const CclLayout ccl = ccl_layout(n, h, w);
    const size_t label = c.take(ccl.total);
    return {label + ccl.bits, label + ccl.rows, ccl.rows_bytes, c.take((size_t)n * h * w * sizeof(int32_t)),
            c.take((size_t)n * sizeof(unsigned long long)), c.total};
}

// va_find_contours' workspace: [bits | labelling rows | forest | inverted bits | background labels | edge bits |
// counts | cells | frame_first | frame_pts | pt_first | starts | npts]
struct FindContoursLayout {
    size_t bits, rows, rows_bytes, forest, inv, bgl, edge, counts, cells, frame_first, frame_pts, pt_first, starts,
        npts, total;
};
FindContoursLayout find_contours_layout(int n, int h, int w)
{
    FindContoursLayout g;
    Carve c;
    const CclLayout ccl = ccl_layout(n, h, w);
    const size_t label = c.take(ccl.total), px = (size_t)n * h * w, slots = (size_t)n * max_contours_per_frame(h, w);
    g.bits = label + ccl.bits;
    g.rows = label + ccl.rows;
    g.rows_bytes = ccl.rows_bytes;
    g.forest = c.take(px * sizeof(int32_t));
    g.inv = c.take((size_t)n * h * words_per_row(w) * sizeof(uint32_t));
    g.bgl = c.take(px * sizeof(int32_t));
    g.edge = c.take((size_t)n * edge_label_words(h, w) * sizeof(uint32_t));
    g.counts = c.take((size_t)2 * n * sizeof(int32_t));
    g.cells = c.take((size_t)n * h * 8 * sizeof(int32_t));
    g.frame_first = c.take(((size_t)n + 1) * sizeof(int64_t));
    g.frame_pts = c.take((size_t)n * sizeof(int64_t));
    g.pt_first = c.take(((size_t)n + 1) * sizeof(int64_t));
    g.starts = c.take(slots * 8);
    g.npts = c.take(slots * sizeof(int32_t));
    g.total = c.total;
    return g;
}
}  // namespace

}  // namespace va

using namespace va;

extern "C" {

size_t va_contour_workspace_bytes(int n, int h, int w)
{
    if (n <= 0 || h <= 0 || w <= 0)
        return 256;
    return contour_layout(n, h, w).total;
}

int va_largest_contour(const uint8_t *mask, int n, int h, int w, int32_t *points, int max_points,
                       int32_t *npoints, double *area, int32_t *ncomponents, void *workspace,
                       size_t workspace_bytes, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(h <= 0 || w <= 0 || (size_t)h * (size_t)w < kMaxFramePixels,
               "va_largest_contour: frames above 2^29 pixels are not supported");
    VA_REQUIRE(mask && points && npoints && ncomponents && workspace, "va_largest_contour: NULL argument");
    VA_REQUIRE(n >= 0 && h > 0 && w > 0 && max_points > 0, "va_largest_contour: bad shape");
    VA_REQUIRE(workspace_bytes >= va_contour_workspace_bytes(n, h, w),
               "va_largest_contour: workspace of %zu bytes < required %zu", workspace_bytes,
               va_contour_workspace_bytes(n, h, w));
    if (n == 0)
        return VA_OK;
    hipStream_t st = as_stream(stream);
    const ContourLayout L = contour_layout(n, h, w);
    uint32_t *bits = at<uint32_t>(workspace, L.bits);
    int32_t *forest = at<int32_t>(workspace, L.forest);
    unsigned long long *keys = at<unsigned long long>(workspace, L.keys);
    int rc = launch_pack_bits(mask, bits, n, h, w, 0, st);
    if (rc)
        return rc;
    rc = launch_ccl(bits, forest, ncomponents, n, h, w, 8, at(workspace, L.rows), L.rows_bytes, nullptr, 0, st,
                    nullptr, /*paint=*/false);
    if (rc)
        return rc;
    return launch_largest_contour(bits, forest, n, h, w, keys, points, max_points, npoints, area, st);
}

size_t va_find_contours_workspace_bytes(int n, int h, int w)
{
    if (n <= 0 || h <= 0 || w <= 0)
        return 256;
    return find_contours_layout(n, h, w).total;
}

int va_find_contours(const uint8_t *mask, int n, int h, int w, int32_t *ncontours, int64_t *totals,
                     va_contour_info *info, int64_t *point_off, int64_t cap_contours, int32_t *points,
                     int64_t cap_points, void *workspace, size_t workspace_bytes, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(h <= 0 || w <= 0 || (size_t)h * (size_t)w < kMaxFramePixels,
               "va_find_contours: frames above 2^29 pixels are not supported");
    VA_REQUIRE(mask && ncontours && totals && info && point_off && points && workspace,
               "va_find_contours: NULL argument");
    VA_REQUIRE(n >= 0 && h > 0 && w > 0, "va_find_contours: bad shape");
    VA_REQUIRE(cap_contours >= 0 && cap_points >= 0, "va_find_contours: negative capacity (%lld contours, %lld points)",
               (long long)cap_contours, (long long)cap_points);
    VA_REQUIRE(aligned(points, 8) && aligned(info, 8) && aligned(point_off, 8) && aligned(totals, 8),
               "va_find_contours: points, records, offsets and totals must be 8-byte aligned");
    VA_REQUIRE(workspace_bytes >= va_find_contours_workspace_bytes(n, h, w),
               "va_find_contours: workspace of %zu bytes < required %zu", workspace_bytes,
               va_find_contours_workspace_bytes(n, h, w));
    if (n == 0)
        return VA_OK;
    hipStream_t st = as_stream(stream);
    const FindContoursLayout L = find_contours_layout(n, h, w);
    uint32_t *bits = at<uint32_t>(workspace, L.bits);
    int32_t *forest = at<int32_t>(workspace, L.forest), *bgl = at<int32_t>(workspace, L.bgl);
    int rc = launch_pack_bits(mask, bits, n, h, w, 0, st);
    if (!rc)
        rc = launch_outline_labels(bits, at<uint32_t>(workspace, L.inv), forest, bgl, at<int32_t>(workspace, L.counts),
                                   at(workspace, L.rows), L.rows_bytes, n, h, w, st);
    if (rc)
        return rc;
    const FindContoursScratch s = {at<uint32_t>(workspace, L.edge),       at<int32_t>(workspace, L.cells),
                                   at<int64_t>(workspace, L.frame_first), at<int64_t>(workspace, L.frame_pts),
                                   at<int64_t>(workspace, L.pt_first),    at(workspace, L.starts),
                                   at<int32_t>(workspace, L.npts)};
    return launch_find_contours(bits, forest, bgl, s, n, h, w, ncontours, totals, info, point_off, cap_contours, points,
                                cap_points, st);
}

}  // extern "C"
