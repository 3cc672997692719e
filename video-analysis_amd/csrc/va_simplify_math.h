// va_simplify_math.h -- the arithmetic of the two curve simplifiers ("Simplification"), one curve at a
// time, as plain inline C++ that compiles for the host and for the device: the Ramer-Douglas-Peucker distance and
// span step of curves.simplify_curve (video/analysis/curves.py:22) and the triangle area and heap procedures of
// regions.simplify_contour (video/analysis/regions.py:307-325, Visvalingam).  va_simplify.hip runs the first with
// one wave per curve and the second with one lane per curve; tests/simplify_shim.cpp compiles this text with the
// host compiler and compares it with the restatement of tests/simplify_checks.py.
//
// Every product, sum, quotient and root is IEEE float64, rounded on its own (build with -ffp-contract=off, as
// va_curves_math.h is; the pragma below says the same to a compiler that honours it).  Points are float64 (x, y)
// pairs, P[2 i], P[2 i + 1].  Indices inside one curve are int32: a curve has at most VA_SIMPLIFY_MAX_POINTS points.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

#if defined(__HIPCC__)
#define VA_SIMPLIFY_FN __host__ __device__ inline
#else
#define VA_SIMPLIFY_FN inline
#endif

namespace va_simplify {

// ---- Ramer-Douglas-Peucker ---------------------------------------------------------------------------------
// the distance of x0 from the chord x1 -> x2: |x0.x - x1.x| when the chord's ends have equal x (the reference's
// branch, also taken by a chord whose two ends coincide), else |a x b| / |a| with a = x2 - x1, b = x1 - x0
VA_SIMPLIFY_FN double chord_distance(double x0x, double x0y, double x1x, double x1y, double x2x, double x2y)
{
    if (x1x == x2x)
        return fabs(x0x - x1x);
    const double ax = x2x - x1x, ay = x2y - x1y;
    const double bx = x1x - x0x, by = x1y - x0y;
    const double p = ax * by, q = ay * bx;
    const double u = ax * ax, v = ay * ay;
    return fabs(p - q) / sqrt(u + v);
}

constexpr int32_t kNoIndex = 0x7FFFFFFF;

// the farthest point of a span, so far: the largest distance above 0 and the first index that has it.  A distance
// that is 0 or NaN is never taken, so `index` stays kNoIndex on a span that cannot be split.
struct Farthest {
    double d = 0.0;
    int32_t index = kNoIndex;
    // a point measured in ascending index order
    VA_SIMPLIFY_FN void add(double dist, int32_t i)
    {
        if (dist > d) {
            d = dist;
            index = i;
        }
    }
    // another partial result of the same span, in any order: compares (d, -index)
    VA_SIMPLIFY_FN void merge(double od, int32_t oi)
    {
        if (od > d || (od == d && oi < index)) {
            d = od;
            index = oi;
        }
    }
};

// the points i0 + 1 + first, i0 + 1 + first + stride, .. below i1 of the span (i0, i1), measured against its chord
VA_SIMPLIFY_FN Farthest span_farthest(const double *P, int32_t i0, int32_t i1, int32_t first, int32_t stride)
{
    Farthest best;
    const double x1x = P[2 * i0], x1y = P[2 * i0 + 1], x2x = P[2 * i1], x2y = P[2 * i1 + 1];
    for (int32_t i = i0 + 1 + first; i < i1; i += stride)
        best.add(chord_distance(P[2 * i], P[2 * i + 1], x1x, x1y, x2x, x2y), i);
    return best;
}

// whether a span's farthest point splits it: its distance exceeds max(eps, 0)
VA_SIMPLIFY_FN bool splits(const Farthest &best, double eps) { return best.d > (eps > 0.0 ? eps : 0.0); }

// A span (i0, i1) split at k: the caller goes on with the smaller half and stacks the larger one, so the span it
// works on halves with every entry stacked and the stack holds at most log2(n) spans -- kSpanStack is twice that
// for VA_SIMPLIFY_MAX_POINTS = 2^24.  The kept set does not depend on the order.
constexpr int kSpanStack = 48;
struct Span {
    int32_t i0, i1;
};
VA_SIMPLIFY_FN Span split_span(int32_t &i0, int32_t &i1, int32_t k)
{
    Span later;
    if (k - i0 <= i1 - k) {
        later = {k, i1};
        i1 = k;
    } else {
        later = {i0, k};
        i0 = k;
    }
    return later;
}

// the whole simplification of one curve by one thread: keep[0 .. n - 1] = 0 / 1; returns the number kept
VA_SIMPLIFY_FN int32_t rdp_keep(const double *P, int32_t n, double eps, uint8_t *keep)
{
    if (n < 3) {
        for (int32_t i = 0; i < n; i++)
            keep[i] = 1;
        return n;
    }
    for (int32_t i = 0; i < n; i++)
        keep[i] = (i == 0 || i == n - 1) ? 1 : 0;
    Span stack[kSpanStack];
    int sp = 0;
    int32_t i0 = 0, i1 = n - 1, kept = 2;
    for (;;) {
        if (i1 - i0 >= 2) {
            const Farthest best = span_farthest(P, i0, i1, 0, 1);
            if (splits(best, eps)) {
                keep[best.index] = 1;
                kept++;
                stack[sp++] = split_span(i0, i1, best.index);
                continue;
            }
        }
        if (sp == 0)
            break;
        sp--;
        i0 = stack[sp].i0;
        i1 = stack[sp].i1;
    }
    return kept;
}

// ---- Visvalingam -------------------------------------------------------------------------------------------
// the effective area of p1 between its neighbours p2 (before) and p3 (after), summed left to right
VA_SIMPLIFY_FN double triangle_area(double p1x, double p1y, double p2x, double p2y, double p3x, double p3y)
{
    const double a = p1x * (p2y - p3y);
    const double b = p2x * (p3y - p1y);
    const double c = p3x * (p1y - p2y);
    return fabs((a + b) + c) / 2.0;
}

// One curve's points and its three int32 tables: the heap of point indices and the links of the doubly linked
// list.  Every index read back from a table passes through at(): with a well-formed offset table it changes
// nothing; where two curves of a malformed table share workspace slots it keeps each read inside the curve's own
// points.
struct Ring {
    const double *P;
    int32_t n;
    int32_t *heap, *prev, *next;
    VA_SIMPLIFY_FN int32_t at(int32_t i) const { return (uint32_t)i < (uint32_t)n ? i : 0; }
    // measured afresh at every comparison, as the reference's TriangleCalculator does
    VA_SIMPLIFY_FN double area(int32_t i) const
    {
        const int32_t b = at(prev[i]), a = at(next[i]);
        return triangle_area(P[2 * i], P[2 * i + 1], P[2 * b], P[2 * b + 1], P[2 * a], P[2 * a + 1]);
    }
    VA_SIMPLIFY_FN bool less(int32_t i, int32_t j) const { return area(i) < area(j); }
};

// heapq._siftdown: the entry at pos rises while it is smaller than its parent, not beyond startpos
VA_SIMPLIFY_FN void siftdown(const Ring &r, int32_t startpos, int32_t pos)
{
    const int32_t item = r.at(r.heap[pos]);
    while (pos > startpos) {
        const int32_t parentpos = (pos - 1) >> 1;
        const int32_t parent = r.at(r.heap[parentpos]);
        if (!r.less(item, parent))
            break;
        r.heap[pos] = parent;
        pos = parentpos;
    }
    r.heap[pos] = item;
}

// heapq._siftup: the smaller child rises (the right one unless the left is smaller) down to a leaf, the entry is
// put there and sifted back towards pos
VA_SIMPLIFY_FN void siftup(const Ring &r, int32_t pos, int32_t len)
{
    const int32_t startpos = pos;
    const int32_t item = r.at(r.heap[pos]);
    int32_t childpos = 2 * pos + 1;
    while (childpos < len) {
        const int32_t rightpos = childpos + 1;
        if (rightpos < len && !r.less(r.at(r.heap[childpos]), r.at(r.heap[rightpos])))
            childpos = rightpos;
        r.heap[pos] = r.heap[childpos];
        pos = childpos;
        childpos = 2 * pos + 1;
    }
    r.heap[pos] = item;
    siftdown(r, startpos, pos);
}

// The reference's procedure on one ring (closed: heap 0 .. n - 1, cyclic links, stops at 2 entries) or one open
// line (heap 1 .. n - 2, links to the fixed ends, stops at 0).  Returns the number of heap entries left; they are
// heap[0 ..], in heap order.  n >= 3.
VA_SIMPLIFY_FN int32_t visvalingam_heap(const Ring &r, double thr, bool closed)
{
    const int32_t n = r.n;
    for (int32_t i = 0; i < n; i++) {
        r.prev[i] = i > 0 ? i - 1 : (closed ? n - 1 : 0);
        r.next[i] = i + 1 < n ? i + 1 : (closed ? 0 : n - 1);
    }
    const int32_t base = closed ? 0 : 1, floor_len = closed ? 2 : 0;
    int32_t len = closed ? n : n - 2;
    for (int32_t i = 0; i < len; i++)
        r.heap[i] = i + base;
    for (int32_t i = len / 2 - 1; i >= 0; i--)
        siftup(r, i, len);
    while (len > floor_len) {
        const int32_t top = r.at(r.heap[0]);
        if (r.area(top) >= thr)
            break;
        const int32_t b = r.at(r.prev[top]), a = r.at(r.next[top]);
        r.next[b] = a;
        r.prev[a] = b;
        len--;                                   // heappop: the last entry to slot 0, then siftup(0)
        if (len > 0) {
            r.heap[0] = r.heap[len];
            siftup(r, 0, len);
        }
    }
    return len;
}

// keep[0 .. n - 1] = 0 / 1 and the number kept: a ring of fewer than 3 points, or one left with fewer than 3,
// keeps none (the reference's None); a line of fewer than 3 points keeps all of them
VA_SIMPLIFY_FN int32_t visvalingam_keep(const double *P, int32_t n, double thr, bool closed, int32_t *heap,
                                        int32_t *prev, int32_t *next, uint8_t *keep)
{
    if (n < 3) {
        for (int32_t i = 0; i < n; i++)
            keep[i] = closed ? 0 : 1;
        return closed ? 0 : n;
    }
    const Ring r{P, n, heap, prev, next};
    const int32_t len = visvalingam_heap(r, thr, closed);
    for (int32_t i = 0; i < n; i++)
        keep[i] = 0;
    if (closed && len < 3)
        return 0;
    for (int32_t j = 0; j < len; j++)
        keep[r.at(heap[j])] = 1;
    if (!closed)
        keep[0] = keep[n - 1] = 1;
    return closed ? len : len + 2;
}

}  // namespace va_simplify
