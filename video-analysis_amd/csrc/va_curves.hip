// va_curves.hip -- curves.make_curve_equidistant (video/analysis/curves.py:103-148) for m curves of a packed
// buffer in one call ("Equidistant curves"): a curve with spacing > 0 is walked and a point dropped
// every L / rint(L / spacing); a curve with spacing == 0 gets `count` points at equal arc length.  The per-curve
// arithmetic is va_curves_math.h, the same text the host tests compile.
//
// The call has the library's counts-then-scan shape, three launches on one stream:
//   count  one lane per curve: its input length (spacing mode: the float32-rule length L; count mode: the arc
//          total s[-1]) and the number of points of its result.  The walk's result size is not a formula of L --
//          L comes from float32 casts, the walk runs in double -- so the walk itself runs here, storing nothing.
//   scan   one workgroup: the exclusive prefix of the counts (int64) and the total
//   fill   one lane per curve: the same walk again, storing; nothing is written when the total exceeds the capacity
// Both modes are serial recurrences in floating point over one curve (the walk's dist and moved p1, the running
// arc length), so a curve is one lane's work and m curves are m lanes; count mode walks its arc length alongside
// its ascending sample positions and keeps no table.  Every value written depends on its curve alone: two runs
// write the same bytes.
//
// A curve the kernels do not take has the status VA_ERR_RANGE, no points and length 0; the others run.  The walk is
// bounded: a curve whose rint(L / spacing) exceeds VA_CURVES_MAX_STEPS, or whose walk drops more than twice that many
// points plus its own, is refused instead of being run to an end that a lane may never reach.
#include "va_common.h"
#include "va_curves_math.h"
#include "va_scan.h"

namespace va {

namespace {

constexpr int kCurvesBlock = 64;     // one wave: m serial curves spread over as many CUs as there are waves
constexpr int kScanBlock = 256;

// the walk's step and the most points its result may have: false for a curve the walk is not run on
__device__ __forceinline__ bool walk_plan(double L, double spacing, int64_t n, double &dx, int64_t &limit)
{
    const double steps = rint(L / spacing);
    if (!(steps <= (double)VA_CURVES_MAX_STEPS))          // (a NaN fails)
        return false;
    dx = L / steps;
    limit = 2 * (int64_t)steps + n + 2;
    return true;
}

__global__ void __launch_bounds__(kCurvesBlock)
curves_count_kernel(const double *__restrict__ points, const int64_t *__restrict__ point_off, int64_t npoints, int m,
                    const double *__restrict__ spacing, const int32_t *__restrict__ count,
                    int32_t *__restrict__ out_count, double *__restrict__ in_length, int32_t *__restrict__ status)
{
    const int64_t k = (int64_t)blockIdx.x * kCurvesBlock + threadIdx.x;
    if (k >= m)
        return;
    int64_t start = 0, n = 0, found = 0;
    double L = 0.0;
    int st = VA_ERR_RANGE;
    const double sp = spacing[k];
    if (curve_range(point_off, k, npoints, start, n) && n >= 2 && n <= VA_CURVES_MAX_POINTS) {
        const double *P = points + 2 * start;
        if (sp > 0.0) {
            L = va_curves::length_f32(P, n);
            if (L < sp) {
                found = n;
                st = VA_OK;
            } else {
                double dx;
                int64_t limit;
                if (walk_plan(L, sp, n, dx, limit)) {
                    found = va_curves::walk_count(P, n, dx, limit);
                    st = found >= 0 ? VA_OK : VA_ERR_RANGE;
                }
            }
        } else if (sp == 0.0 && count != nullptr && count[k] >= 1) {
            L = va_curves::arc_total(P, n);
            found = count[k];
            st = VA_OK;
        }
    }
    out_count[k] = st == VA_OK ? (int32_t)found : 0;
    in_length[k] = st == VA_OK ? L : 0.0;
    status[k] = st;
}

// out_off[0 .. m] = exclusive prefix of the counts, totals[0] = the sum: one workgroup, chunk after chunk
__global__ void __launch_bounds__(kScanBlock)
curves_scan_kernel(const int32_t *__restrict__ out_count, int m, int64_t *__restrict__ out_off,
                   int64_t *__restrict__ totals)
{
    __shared__ int64_t part[kScanBlock / kWave];
    const int t = (int)threadIdx.x;
    int64_t carry = 0;
    for (int64_t base = 0; base < m; base += kScanBlock) {
        const int64_t k = base + t;
        int64_t sum;
        const int64_t excl = block_exclusive<kScanBlock / kWave>(k < m ? (int64_t)out_count[k] : 0, part, sum);
        if (k < m)
            out_off[k] = carry + excl;
        carry += sum;
    }
    if (t == 0) {
        out_off[m] = carry;
        totals[0] = carry;
    }
}

__global__ void __launch_bounds__(kCurvesBlock)
curves_fill_kernel(const double *__restrict__ points, const int64_t *__restrict__ point_off, int64_t npoints, int m,
                   const double *__restrict__ spacing, const double *__restrict__ translate,
                   const int32_t *__restrict__ out_count, const int64_t *__restrict__ out_off,
                   const double *__restrict__ in_length, const int32_t *__restrict__ status,
                   const int64_t *__restrict__ totals, double *__restrict__ out_points, int64_t cap_points,
                   double *__restrict__ out_length)
{
    const int64_t k = (int64_t)blockIdx.x * kCurvesBlock + threadIdx.x;
    if (k >= m)
        return;
    double len = 0.0;
    const int64_t at = out_off[k], room = out_count[k];
    // (totals[0] <= cap_points: every slot at .. at + room - 1 lies inside the capacity)
    if (totals[0] <= cap_points && status[k] == VA_OK && room > 0 && at >= 0 && at + room <= cap_points) {
        const int64_t start = point_off[k], n = point_off[k + 1] - start;     // (checked by the count pass)
        const double *P = points + 2 * start;
        double *out = out_points + 2 * at;
        const bool shift = translate != nullptr;
        const double tx = shift ? translate[2 * k] : 0.0, ty = shift ? translate[2 * k + 1] : 0.0;
        const double sp = spacing[k], L = in_length[k];
        if (sp > 0.0 && L < sp) {
            va_curves::Length32 acc;
            for (int64_t i = 0; i < n && i < room; i++) {
                const double ox = shift ? P[2 * i] + tx : P[2 * i], oy = shift ? P[2 * i + 1] + ty : P[2 * i + 1];
                out[2 * i] = ox;
                out[2 * i + 1] = oy;
                acc.add(ox, oy);
            }
            len = acc.sum;
        } else if (sp > 0.0) {
            va_curves::walk_store(P, n, L / rint(L / sp), shift, tx, ty, out, room, &len);
        } else {
            va_curves::interp_store(P, n, L, room, shift, tx, ty, out, &len);
        }
    }
    out_length[k] = len;
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

int va_curves_equidistant(const double *points, const int64_t *point_off, int64_t npoints, int m, const double *spacing,
                          const int32_t *count, const double *translate, int32_t *out_count, int64_t *out_off,
                          double *in_length, int32_t *status, int64_t *totals, double *out_points, int64_t cap_points,
                          double *out_length, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(npoints >= 0 && m >= 0 && cap_points >= 0,
               "va_curves_equidistant: negative count (npoints %lld, m %d, cap_points %lld)", (long long)npoints, m,
               (long long)cap_points);
    if (m == 0)
        return VA_OK;
    // (count may be NULL: a curve in count mode then reads none and is refused by the kernel's own test below)
    VA_REQUIRE(points && point_off && spacing && out_count && out_off && in_length && status && totals && out_points &&
                   out_length,
               "va_curves_equidistant: NULL argument");
    VA_REQUIRE(aligned(points, 8) && aligned(point_off, 8) && aligned(spacing, 8) && aligned(count, 4) &&
                   aligned(translate, 8) && aligned(out_count, 4) && aligned(out_off, 8) && aligned(in_length, 8) &&
                   aligned(status, 4) && aligned(totals, 8) && aligned(out_points, 8) && aligned(out_length, 8),
               "va_curves_equidistant: float64 and int64 buffers must be 8-byte aligned, int32 buffers 4-byte aligned");
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)cdiv(m, kCurvesBlock)), block(kCurvesBlock);
    hipLaunchKernelGGL(curves_count_kernel, grid, block, 0, st, points, point_off, npoints, m, spacing, count,
                       out_count, in_length, status);
    VA_LAUNCH_CHECK("curves_count_kernel");
    hipLaunchKernelGGL(curves_scan_kernel, dim3(1), dim3(kScanBlock), 0, st, out_count, m, out_off, totals);
    VA_LAUNCH_CHECK("curves_scan_kernel");
    hipLaunchKernelGGL(curves_fill_kernel, grid, block, 0, st, points, point_off, npoints, m, spacing, translate,
                       out_count, out_off, in_length, status, totals, out_points, cap_points, out_length);
    VA_LAUNCH_CHECK("curves_fill_kernel");
    return VA_OK;
}

}  // extern "C"
