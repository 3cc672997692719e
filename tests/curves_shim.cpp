// extern "C" doors into video-analysis_amd/csrc/va_curves_math.h for tests/test_curves_host.py: the header is
// compiled with the host C++ compiler (no -march flags, -ffp-contract=off) into a temporary shared object and
// driven through ctypes.  Nothing here computes: every function hands its arguments to the header.
#include "va_curves_math.h"

extern "C" {

void cs_hypot(const double *x, const double *y, double *out, int64_t n)
{
    for (int64_t i = 0; i < n; i++)
        out[i] = va_curves::hypot_cr(x[i], y[i]);
}

void cs_norm2(const double *x, const double *y, double *out, int64_t n)
{
    for (int64_t i = 0; i < n; i++)
        out[i] = va_curves::norm2(x[i], y[i]);
}

double cs_length_f32(const double *P, int64_t n) { return va_curves::length_f32(P, n); }

// spacing mode as the kernels run it: the count pass (returns the number of points, -1 beyond `limit`) ...
int64_t cs_spacing_count(const double *P, int64_t n, double spacing, int64_t limit)
{
    const double L = va_curves::length_f32(P, n);
    if (L < spacing)
        return n;
    return va_curves::walk_count(P, n, va_curves::walk_step(L, spacing), limit);
}

// ... and the fill pass: the points into out (room for cap), the output's float32-rule length into *out_length
int64_t cs_spacing_store(const double *P, int64_t n, double spacing, int shift, double tx, double ty, double *out,
                         int64_t cap, double *out_length)
{
    const double L = va_curves::length_f32(P, n);
    if (L < spacing) {
        va_curves::Length32 acc;
        for (int64_t i = 0; i < n && i < cap; i++) {
            out[2 * i] = shift ? P[2 * i] + tx : P[2 * i];
            out[2 * i + 1] = shift ? P[2 * i + 1] + ty : P[2 * i + 1];
            acc.add(out[2 * i], out[2 * i + 1]);
        }
        *out_length = acc.sum;
        return n <= cap ? n : -1;
    }
    return va_curves::walk_store(P, n, va_curves::walk_step(L, spacing), shift != 0, tx, ty, out, cap, out_length);
}

double cs_arc_total(const double *P, int64_t n) { return va_curves::arc_total(P, n); }

void cs_count_store(const double *P, int64_t n, int64_t count, int shift, double tx, double ty, double *out,
                    double *out_length)
{
    va_curves::interp_store(P, n, va_curves::arc_total(P, n), count, shift != 0, tx, ty, out, out_length);
}

}  // extern "C"
