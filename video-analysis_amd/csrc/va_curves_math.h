// va_curves_math.h -- the arithmetic of curves.make_curve_equidistant (video/analysis/curves.py:103-148), one curve
// at a time, as plain inline C++ that compiles for the host and for the device ("Equidistant
// curves").  va_curves.hip runs it with one lane per curve; tests/curves_shim.cpp compiles it with the host
// compiler and compares it with the NumPy function and with the scalar restatement.
//
// Every product, sum and quotient is rounded on its own (build with -ffp-contract=off); the fused operations the
// definition needs are written out with fma().  Points are float64 (x, y) pairs, P[2 i], P[2 i + 1].
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VA_CURVES_FN __host__ __device__ inline
#else
#define VA_CURVES_FN inline
#endif

namespace va_curves {

// cv2.arcLength of the float32 casts of an open curve (curves.curve_length): per segment the float32
// dx*dx + dy*dy, two rounded products and one rounded sum, its correctly rounded float32 root (the double root of a
// float rounds to it), and the roots added in double in point order
struct Length32 {
    double sum = 0.0;
    float px = 0.f, py = 0.f;
    bool first = true;
    VA_CURVES_FN void add(double x, double y)
    {
        const float fx = (float)x, fy = (float)y;
        if (!first) {
            const float dx = fx - px, dy = fy - py;
            const float xx = dx * dx, yy = dy * dy;
            const float s = xx + yy;
            sum += (double)(float)sqrt((double)s);
        }
        px = fx;
        py = fy;
        first = false;
    }
};

VA_CURVES_FN double length_f32(const double *P, int64_t n)
{
    Length32 acc;
    for (int64_t i = 0; i < n; i++)
        acc.add(P[2 * i], P[2 * i + 1]);
    return acc.sum;
}

// np.linalg.norm of a 2-vector where NumPy's dot runs on a BLAS with FMA: the x product is rounded, the y product
// is fused into the sum.  The one fma of the walk.
VA_CURVES_FN double norm2(double dx, double dy) { return sqrt(fma(dy, dy, dx * dx)); }

// math.hypot: the correctly rounded sqrt(x*x + y*y) of finite x, y.  The squares are exact as double-double
// (fma gives the low halves), their sum is a double-double, the root of its high part takes one correction from
// the residual, itself exact up to the low parts.  Outside [2^-500, 2^500] the operands are scaled by a power of
// two, which is exact.  (A non-finite operand gives a non-finite result; callers route those curves elsewhere.)
VA_CURVES_FN double hypot_cr(double x, double y)
{
    double a = fabs(x), b = fabs(y);
    if (a < b) {
        const double t = a;
        a = b;
        b = t;
    }
    if (b == 0.0 || !(a <= 1.7976931348623157e308))
        return a;
    int e = 0;
    frexp(a, &e);
    if (e > 500 || e < -500) {
        a = ldexp(a, -e);
        b = ldexp(b, -e);
    } else {
        e = 0;
    }
    const double p = a * a, pe = fma(a, a, -p);
    const double q = b * b, qe = fma(b, b, -q);
    const double s = p + q;              // p >= q: the error of this sum is q - (s - p), exactly
    const double lo = (q - (s - p)) + (pe + qe);
    const double h = sqrt(s);
    const double hh = h * h, he = fma(h, h, -hh);
    const double r = ((s - hh) - he) + lo;
    const double res = h + r / (2.0 * h);
    return e ? ldexp(res, e) : res;
}

// ---- spacing mode ------------------------------------------------------------------------------------------
// the spacing the walk uses: L / rint(L / spacing), rint rounding half to even as np.round
VA_CURVES_FN double walk_step(double L, double spacing) { return L / rint(L / spacing); }

// The reference's walk (curves.py:117-132) over n >= 2 points with step dx.  Emit is called with every point of
// the result in order, the first input point included, and returns false to stop the walk (room exhausted).
// Returns the number of points emitted, or -1 when Emit stopped it.
template <class Emit>
VA_CURVES_FN int64_t walk(const double *P, int64_t n, double dx, Emit &&emit)
{
    int64_t k = 0;
    if (!emit(P[0], P[1]))
        return -1;
    k++;
    double dist = 0.0;
    for (int64_t i = 0; i + 1 < n; i++) {
        double p1x = P[2 * i], p1y = P[2 * i + 1];
        const double p2x = P[2 * i + 2], p2y = P[2 * i + 3];
        double dp = norm2(p2x - p1x, p2y - p1y);
        while (dist + dp > dx) {
            const double f = (dx - dist) / dp;
            const double mx = f * (p2x - p1x), my = f * (p2y - p1y);
            p1x = p1x + mx;
            p1y = p1y + my;
            if (!emit(p1x, p1y))
                return -1;
            k++;
            dp = norm2(p2x - p1x, p2y - p1y);
            dist = 0.0;
        }
        dist += dp;
    }
    if (dist > 1e-8) {
        if (!emit(P[2 * n - 2], P[2 * n - 1]))
            return -1;
        k++;
    }
    return k;
}

// the number of points of the walk's result, or -1 when it has more than `limit`
VA_CURVES_FN int64_t walk_count(const double *P, int64_t n, double dx, int64_t limit)
{
    int64_t room = limit;
    return walk(P, n, dx, [&](double, double) { return room-- > 0; });
}

// the walk's result into out (room for `cap` points); with `shift` every coordinate is translated by (tx, ty), one
// rounded add each (without it nothing is added: x + 0.0 would turn a -0.0 into +0.0); *out_length receives the
// float32-rule length of what was written.  Returns the number of points, -1 beyond cap.
VA_CURVES_FN int64_t walk_store(const double *P, int64_t n, double dx, bool shift, double tx, double ty, double *out,
                                int64_t cap, double *out_length)
{
    Length32 len;
    int64_t at = 0;
    const int64_t k = walk(P, n, dx, [&](double x, double y) {
        if (at >= cap)
            return false;
        const double ox = shift ? x + tx : x, oy = shift ? y + ty : y;
        out[2 * at] = ox;
        out[2 * at + 1] = oy;
        len.add(ox, oy);
        at++;
        return true;
    });
    *out_length = len.sum;
    return k;
}

// ---- count mode --------------------------------------------------------------------------------------------
// s[n - 1] of s[0] = 0, s[i + 1] = s[i] + hypot(segment i): the serial double sum in point order
VA_CURVES_FN double arc_total(const double *P, int64_t n)
{
    double s = 0.0;
    for (int64_t i = 0; i + 1 < n; i++)
        s = s + hypot_cr(P[2 * i] - P[2 * i + 2], P[2 * i + 1] - P[2 * i + 3]);
    return s;
}

// np.linspace(0, total, count)[k]
VA_CURVES_FN double linspace_at(double total, int64_t count, int64_t k)
{
    if (count > 1 && k == count - 1)
        return total;
    const double step = count > 1 ? total / (double)(count - 1) : 0.0;
    return (double)k * step + 0.0;
}

// np.interp(x, s, fp) at s[j] <= x < s[j + 1]: fp[j] when x == s[j], else slope * (x - s[j]) + fp[j]
VA_CURVES_FN double interp_at(double x, double sj, double sj1, double fj, double fj1)
{
    if (x == sj)
        return fj;
    const double slope = (fj1 - fj) / (sj1 - sj);
    return slope * (x - sj) + fj;
}

// `count` >= 1 points at equal arc length on n >= 2 points (curves.py:134-146): np.interp of each coordinate at
// np.linspace(0, s[-1], count), with j the last index with s[j] <= x and x >= s[-1] giving the last point.  The
// sample positions ascend, so s is walked once alongside them and never stored.  total: arc_total(P, n).
// Writes count points, translated as in walk_store, and the float32-rule length of what was written.
VA_CURVES_FN void interp_store(const double *P, int64_t n, double total, int64_t count, bool shift, double tx,
                               double ty, double *out, double *out_length)
{
    Length32 len;
    int64_t j = 0;
    double sj = 0.0;
    double sj1 = sj + hypot_cr(P[0] - P[2], P[1] - P[3]);
    for (int64_t k = 0; k < count; k++) {
        const double x = linspace_at(total, count, k);
        double rx, ry;
        if (x >= total) {
            rx = P[2 * n - 2];
            ry = P[2 * n - 1];
        } else {
            while (j + 2 < n && sj1 <= x) {        // x < total = s[n - 1]: j stops at n - 2 at the latest
                j++;
                sj = sj1;
                sj1 = sj + hypot_cr(P[2 * j] - P[2 * j + 2], P[2 * j + 1] - P[2 * j + 3]);
            }
            rx = interp_at(x, sj, sj1, P[2 * j], P[2 * j + 2]);
            ry = interp_at(x, sj, sj1, P[2 * j + 1], P[2 * j + 3]);
        }
        const double ox = shift ? rx + tx : rx, oy = shift ? ry + ty : ry;
        out[2 * k] = ox;
        out[2 * k + 1] = oy;
        len.add(ox, oy);
    }
    *out_length = len.sum;
}

}  // namespace va_curves
