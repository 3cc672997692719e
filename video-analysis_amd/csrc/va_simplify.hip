// va_simplify.hip -- the two curve simplifiers for m curves of a packed buffer in one call each (DESIGN.md §9,
// "Simplification"): Ramer-Douglas-Peucker (curves.simplify_curve, video/analysis/curves.py:22) and Visvalingam
// (regions.simplify_contour, video/analysis/regions.py:307-325).  Both write one uint8 flag per input point, 1 for
// a point that is kept, and the number kept per curve.  The per-curve arithmetic is va_simplify_math.h, the same
// text the host tests compile.
//
//   rdp          one wave per curve.  A span is measured 64 points at a time, every lane keeps the first largest
//                distance of its points, and the lanes' results are merged by (d, -index), so the wave agrees on the
//                first point of largest distance whatever the order.  A split goes on with the smaller half and
//                stacks the larger one in LDS (at most log2(n) spans).  A curve of up to kRdpStagePoints points is
//                copied to LDS first, where every span re-reads it; a longer one is read where it lies.
//   visvalingam  one lane per curve: the heap with its changing keys is a serial procedure.  Heap and links are int32
//                tables in the caller's workspace, [heap | prev | next], each npoints long, a curve's entries at its
//                own point offsets.  The lanes of a wave finish with the longest curve of the wave.
//
// A curve that is not run has the status VA_ERR_RANGE and the count 0, and its flags are 0 where its offsets name
// slots inside the buffer.  Every value written depends on its curve alone and nothing is read before it is
// written: two runs write the same bytes, whatever the workspace held.  Nothing is written outside a curve's own
// flags, count, status and workspace slots.
#include "va_common.h"
#include "va_simplify_math.h"

namespace va {

namespace {

constexpr int kRdpStagePoints = 2048;        // 32 KiB of LDS a workgroup: five curves in flight on a CU
constexpr int kRdpMaxGrid = 65535;           // curves of one launch; a larger batch runs in pieces
static_assert((1 << (va_simplify::kSpanStack / 2)) >= VA_SIMPLIFY_MAX_POINTS, "the span stack holds 2 log2(n) spans");

// the spans of one curve of n >= 3 points, by the whole wave; returns the number of points kept (the same in every
// lane).  Every lane holds the same span and stack pointer and stores the same stack entry, so each reads back what
// it wrote itself and no barrier is needed.
__device__ __forceinline__ int32_t rdp_wave(const double *P, int32_t n, double eps, uint8_t *__restrict__ keep,
                                            va_simplify::Span *stack, int lane)
{
    int sp = 0;
    int32_t i0 = 0, i1 = n - 1, kept = 2;
    for (;;) {
        if (i1 - i0 >= 2) {
            va_simplify::Farthest best = va_simplify::span_farthest(P, i0, i1, lane, kWave);
            for (int off = kWave / 2; off > 0; off >>= 1)
                best.merge(__shfl_xor(best.d, off, kWave), __shfl_xor(best.index, off, kWave));
            if (va_simplify::splits(best, eps)) {
                if (lane == 0)
                    keep[best.index] = 1;
                kept++;
                stack[sp++] = va_simplify::split_span(i0, i1, best.index);
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

__global__ void __launch_bounds__(kWave)
simplify_rdp_kernel(const double *__restrict__ points, const int64_t *__restrict__ point_off, int64_t npoints,
                    int64_t first_curve, const double *__restrict__ eps, uint8_t *__restrict__ keep,
                    int32_t *__restrict__ out_count, int32_t *__restrict__ status)
{
    __shared__ double staged[2 * kRdpStagePoints];
    __shared__ va_simplify::Span stack[va_simplify::kSpanStack];
    const int64_t k = first_curve + blockIdx.x;
    const int lane = (int)threadIdx.x;
    int64_t start = 0, n = 0;
    const bool in_range = curve_range(point_off, k, npoints, start, n);
    const double e = eps[k];
    uint8_t *flags = keep + start;
    int32_t kept = 0;
    int st = VA_ERR_RANGE;
    if (in_range && (n > VA_SIMPLIFY_MAX_POINTS || e != e)) {
        for (int64_t i = lane; i < n; i += kWave)
            flags[i] = 0;
    } else if (in_range && n < 3) {
        if (lane < n)
            flags[lane] = 1;
        kept = (int32_t)n;
        st = VA_OK;
    } else if (in_range) {
        const int32_t np = (int32_t)n;
        const double *P = points + 2 * start;
        for (int32_t i = lane; i < np; i += kWave)
            flags[i] = (i == 0 || i == np - 1) ? 1 : 0;
        __syncthreads();                      // lane 0 sets flags that other lanes have just cleared

        if (np <= kRdpStagePoints) {
            for (int32_t i = lane; i < 2 * np; i += kWave)
                staged[i] = P[i];
            __syncthreads();
            kept = rdp_wave(staged, np, e, flags, stack, lane);
        } else {
            kept = rdp_wave(P, np, e, flags, stack, lane);
        }
        st = VA_OK;
    }
    if (lane == 0) {
        out_count[k] = kept;
        status[k] = st;
    }
}

__global__ void __launch_bounds__(kWave)
simplify_visvalingam_kernel(const double *__restrict__ points, const int64_t *__restrict__ point_off, int64_t npoints,
                            int m, const double *__restrict__ thr, int closed, uint8_t *__restrict__ keep,
                            int32_t *__restrict__ out_count, int32_t *__restrict__ status, int32_t *__restrict__ heap,
                            int32_t *__restrict__ prev, int32_t *__restrict__ next)
{
    const int64_t k = (int64_t)blockIdx.x * kWave + threadIdx.x;
    if (k >= m)
        return;
    int64_t start = 0, n = 0;
    int32_t kept = 0;
    int st = VA_ERR_RANGE;
    if (curve_range(point_off, k, npoints, start, n)) {
        const double t = thr[k];
        if (n > VA_SIMPLIFY_MAX_POINTS || t != t) {
            for (int64_t i = 0; i < n; i++)
                keep[start + i] = 0;
        } else {
            kept = va_simplify::visvalingam_keep(points + 2 * start, (int32_t)n, t, closed != 0, heap + start,
                                                 prev + start, next + start, keep + start);
            st = VA_OK;
        }
    }
    out_count[k] = kept;
    status[k] = st;
}

// Visvalingam's workspace: the heap and the two link tables
struct SimplifyLayout { size_t heap, prev, next, total; };
SimplifyLayout simplify_layout(int64_t npoints)
{
    Carve c;
    const size_t table = (size_t)npoints * sizeof(int32_t);
    return {c.take(table), c.take(table), c.take(table), c.total};
}

// the arguments the two simplifiers share; m == 0 is the caller's
int simplify_check(const char *name, const double *points, const int64_t *point_off, int64_t npoints, int m,
                   const double *tol, const uint8_t *keep, const int32_t *out_count, const int32_t *status)
{
    VA_REQUIRE(npoints >= 0 && m >= 0, "%s: negative count (npoints %lld, m %d)", name, (long long)npoints, m);
    if (m == 0)
        return VA_OK;
    VA_REQUIRE(points && point_off && tol && keep && out_count && status, "%s: NULL argument", name);
    VA_REQUIRE(aligned(points, 8) && aligned(point_off, 8) && aligned(tol, 8) && aligned(out_count, 4) &&
                   aligned(status, 4),
               "%s: float64 and int64 buffers must be 8-byte aligned, int32 buffers 4-byte aligned", name);
    return VA_OK;
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

int va_simplify_rdp(const double *points, const int64_t *point_off, int64_t npoints, int m, const double *eps,
                    uint8_t *keep, int32_t *out_count, int32_t *status, void *stream)
{
    VA_ENTER();
    const int rc = simplify_check("va_simplify_rdp", points, point_off, npoints, m, eps, keep, out_count, status);
    if (rc || m == 0)
        return rc;
    for (int64_t first = 0; first < m; first += kRdpMaxGrid) {
        const unsigned blocks = (unsigned)(m - first < kRdpMaxGrid ? m - first : kRdpMaxGrid);
        hipLaunchKernelGGL(simplify_rdp_kernel, dim3(blocks), dim3(kWave), 0, as_stream(stream), points, point_off,
                           npoints, first, eps, keep, out_count, status);
        VA_LAUNCH_CHECK("simplify_rdp_kernel");
    }
    return VA_OK;
}

size_t va_simplify_visvalingam_workspace_bytes(int64_t npoints)
{
    return npoints < 0 ? 256 : simplify_layout(npoints).total;
}

int va_simplify_visvalingam(const double *points, const int64_t *point_off, int64_t npoints, int m, const double *thr,
                            int closed, uint8_t *keep, int32_t *out_count, int32_t *status, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(closed == 0 || closed == 1, "va_simplify_visvalingam: closed is 0 (lines) or 1 (rings), got %d", closed);
    const int rc = simplify_check("va_simplify_visvalingam", points, point_off, npoints, m, thr, keep, out_count,
                                  status);
    if (rc || m == 0)
        return rc;
    VA_REQUIRE(workspace, "va_simplify_visvalingam: NULL argument");
    VA_REQUIRE(aligned(workspace, 8), "va_simplify_visvalingam: the workspace must be 8-byte aligned");
    VA_REQUIRE(workspace_bytes >= va_simplify_visvalingam_workspace_bytes(npoints),
               "va_simplify_visvalingam: workspace of %zu bytes < required %zu", workspace_bytes,
               va_simplify_visvalingam_workspace_bytes(npoints));
    const SimplifyLayout lay = simplify_layout(npoints);
    hipLaunchKernelGGL(simplify_visvalingam_kernel, dim3((unsigned)cdiv(m, kWave)), dim3(kWave), 0, as_stream(stream),
                       points, point_off, npoints, m, thr, closed, keep, out_count, status,
                       at<int32_t>(workspace, lay.heap), at<int32_t>(workspace, lay.prev),
                       at<int32_t>(workspace, lay.next));
    VA_LAUNCH_CHECK("simplify_visvalingam_kernel");
    return VA_OK;
}

}  // extern "C"
