// extern "C" doors into video-analysis_amd/csrc/va_simplify_math.h for tests/test_simplify_host.py: the header is
// compiled with the host C++ compiler (no -march flags, -ffp-contract=off) into a temporary shared object and
// driven through ctypes.  Nothing here computes: every function hands its arguments to the header.
#include "va_simplify_math.h"

extern "C" {

// rows of six doubles (x0, x1, x2 as (x, y) pairs): the distance of x0 from the chord x1 -> x2
void ss_chord_distance(const double *rows, double *out, int64_t n)
{
    for (int64_t i = 0; i < n; i++) {
        const double *r = rows + 6 * i;
        out[i] = va_simplify::chord_distance(r[0], r[1], r[2], r[3], r[4], r[5]);
    }
}

// rows of six doubles (p1, p2, p3): the area of p1 between p2 and p3
void ss_triangle_area(const double *rows, double *out, int64_t n)
{
    for (int64_t i = 0; i < n; i++) {
        const double *r = rows + 6 * i;
        out[i] = va_simplify::triangle_area(r[0], r[1], r[2], r[3], r[4], r[5]);
    }
}

// the span step as a wave runs it: `lanes` strided partial results merged from the last lane to the first.
// Returns the index (va_simplify::kNoIndex for none), the distance in *d
int ss_span_farthest(const double *P, int i0, int i1, int lanes, double *d)
{
    va_simplify::Farthest best;
    for (int lane = lanes - 1; lane >= 0; lane--) {
        const va_simplify::Farthest part = va_simplify::span_farthest(P, i0, i1, lane, lanes);
        best.merge(part.d, part.index);
    }
    *d = best.d;
    return best.index;
}

int ss_rdp_keep(const double *P, int n, double eps, uint8_t *keep) { return va_simplify::rdp_keep(P, n, eps, keep); }

// the heap procedure alone (n >= 3): the number of entries left, heap[0 ..] in heap order
int ss_visvalingam_heap(const double *P, int n, double thr, int closed, int32_t *heap, int32_t *prev, int32_t *next)
{
    return va_simplify::visvalingam_heap(va_simplify::Ring{P, n, heap, prev, next}, thr, closed != 0);
}

int ss_visvalingam_keep(const double *P, int n, double thr, int closed, int32_t *heap, int32_t *prev, int32_t *next,
                        uint8_t *keep)
{
    return va_simplify::visvalingam_keep(P, n, thr, closed != 0, heap, prev, next, keep);
}

}  // extern "C"
