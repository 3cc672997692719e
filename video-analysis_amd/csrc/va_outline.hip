// va_outline.hip -- the outline queries of DESIGN.md §9, "Outline queries": where a ray first hits an outline
// (get_ray_hitpoint, video/analysis/regions.py:353-391, and the angle loops of get_ray_intersections :395-405 and
// get_farthest_ray_intersection :409-426) and whether a point lies inside a ring (Polygon.contains,
// video/analysis/shapes.py:552-554), for many queries over many outlines in one launch.
//
// Both kernels have one shape: a query (a ray, or a point) reduces over the edges of one outline.  A group of L
// lanes takes one query, lane j looks at edges j, j + L, j + 2 L, ..., and the group is folded with __shfl_xor.
// Edge i reads points i and (i + 1) mod n straight from the packed point buffer.  L is 8 or 64: a whole wave on a
// triangle idles 61 lanes, eight lanes on a ring of thousands of points take eight times as many rounds; the
// caller chooses per launch.  What is reduced does not depend on the order of the reduction -- the smallest pair
// (t, edge) and a count for a ray, a parity and an "any" for a point -- so both widths write the same bytes.
//
// All arithmetic is float64 with every product, sum and quotient rounded on its own (the Makefile's
// -ffp-contract=off), the quotients true IEEE divisions: the expressions are those of the NumPy restatement in
// tests/golden/make_golden_outline.py, operation by operation.  The hit test is written as positive comparisons,
// so a NaN fails it.  The only short cut: t is divided out only for an edge whose den and u have passed, which
// changes no value that is looked at.
//
// A query whose outline index, or whose outline's offsets, are not in range is refused: it reads nothing but its
// index and the two offsets and writes the refused markers; the other queries run.
#include "va_common.h"

namespace va {

namespace {

constexpr int kOutlineBlock = 256;
constexpr int64_t kOutlineMaxPoints = ((int64_t)1 << 31) - 2;

__device__ __forceinline__ double quiet_nan() { return __longlong_as_double(0x7FF8000000000000ll); }

// the points of query k's outline: false when the query is refused
__device__ __forceinline__ bool outline_range(const int64_t *__restrict__ point_off, const int32_t *__restrict__ index,
                                              int64_t k, int64_t npoints, int m, int &o, int64_t &start, int &n)
{
    o = index[k];
    if (o < 0 || o >= m)
        return false;
    const int64_t s = point_off[o], e = point_off[o + 1];
    if (!(s >= 0 && s <= e && e <= npoints && e - s <= kOutlineMaxPoints))
        return false;
    start = s;
    n = (int)(e - s);
    return true;
}

// the query of this lane's group and the lane's place in the group; a whole wave's query is wave-uniform
template <int L>
__device__ __forceinline__ int64_t group_query(int &lane)
{
    constexpr int kGroups = kOutlineBlock / L;
    lane = (int)threadIdx.x & (L - 1);
    int g = (int)threadIdx.x / L;
    if (L == kWave)
        g = __builtin_amdgcn_readfirstlane(g);
    return (int64_t)blockIdx.x * kGroups + g;
}

template <int L>
__global__ void __launch_bounds__(kOutlineBlock)
ray_hits_kernel(const double *__restrict__ points, const int64_t *__restrict__ point_off,
                const uint8_t *__restrict__ closed, int64_t npoints, int m, const double *__restrict__ anchors,
                const double *__restrict__ fars, const int32_t *__restrict__ index, int64_t q,
                double *__restrict__ t_out, double *__restrict__ hits_out, int32_t *__restrict__ edge_out,
                int32_t *__restrict__ count_out)
{
    int lane;
    const int64_t k = group_query<L>(lane);
    const bool live = k < q;                 // (no lane leaves before the shuffles: a group folds as a whole)
    int o = 0, n = 0;
    int64_t start = 0;
    const bool ok = live && outline_range(point_off, index, k, npoints, m, o, start, n);
    double ax = 0, ay = 0, dx = 0, dy = 0;
    int edges = 0;
    if (ok) {
        ax = anchors[2 * k];
        ay = anchors[2 * k + 1];
        dx = fars[2 * k] - ax;
        dy = fars[2 * k + 1] - ay;
        edges = n == 0 ? 0 : (closed[o] != 0 ? n : n - 1);
    }
    const double *P = points + 2 * start;
    double best_t = 0;
    int best_e = -1, count = 0;
    for (int i = lane; i < edges; i += L) {
        const int j = i + 1 == n ? 0 : i + 1;
        const double px = P[2 * (int64_t)i], py = P[2 * (int64_t)i + 1];
        const double qx = P[2 * (int64_t)j], qy = P[2 * (int64_t)j + 1];
        const double ex = qx - px, ey = qy - py;
        const double wx = px - ax, wy = py - ay;
        const double den = dx * ey - dy * ex;
        const double tn = wx * ey - wy * ex;
        const double un = wx * dy - wy * dx;
        const double u = un / den;
        if (den != 0 && u >= 0 && u <= 1) {
            const double t = tn / den;
            if (t >= 0 && t <= 1) {
                count++;
                if (best_e < 0 || t < best_t) {      // (i ascends in a lane: an equal t keeps the lower edge)
                    best_t = t;
                    best_e = i;
                }
            }
        }
    }
#pragma unroll
    for (int s = L / 2; s >= 1; s >>= 1) {
        const double ot = __shfl_xor(best_t, s, L);
        const int oe = __shfl_xor(best_e, s, L);
        count += __shfl_xor(count, s, L);
        if (oe >= 0 && (best_e < 0 || ot < best_t || (ot == best_t && oe < best_e))) {
            best_t = ot;
            best_e = oe;
        }
    }
    if (!live || lane != 0)
        return;
    const bool hit = ok && best_e >= 0;
    t_out[k] = hit ? best_t : quiet_nan();
    hits_out[2 * k] = hit ? ax + best_t * dx : quiet_nan();
    hits_out[2 * k + 1] = hit ? ay + best_t * dy : quiet_nan();
    edge_out[k] = hit ? best_e : -1;
    count_out[k] = ok ? count : -1;
}

template <int L>
__global__ void __launch_bounds__(kOutlineBlock)
points_in_outlines_kernel(const double *__restrict__ points, const int64_t *__restrict__ point_off, int64_t npoints,
                          int m, const double *__restrict__ query, const int32_t *__restrict__ index, int64_t q,
                          uint8_t *__restrict__ inside_out)
{
    int lane;
    const int64_t k = group_query<L>(lane);
    const bool live = k < q;
    int o = 0, n = 0;
    int64_t start = 0;
    const bool ok = live && outline_range(point_off, index, k, npoints, m, o, start, n);
    double x = 0, y = 0;
    int edges = 0;
    if (ok && n >= 3) {
        x = query[2 * k];
        y = query[2 * k + 1];
        if (isfinite(x) && isfinite(y))
            edges = n;
    }
    const double *P = points + 2 * start;
    int parity = 0, any = 0;
    for (int i = lane; i < edges; i += L) {
        const int j = i + 1 == n ? 0 : i + 1;
        const double px = P[2 * (int64_t)i], py = P[2 * (int64_t)i + 1];
        const double qx = P[2 * (int64_t)j], qy = P[2 * (int64_t)j + 1];
        const double c = (qx - px) * (y - py) - (qy - py) * (x - px);
        const bool in_x = (px <= x && x <= qx) || (qx <= x && x <= px);
        const bool in_y = (py <= y && y <= qy) || (qy <= y && y <= py);
        const bool boundary = c == 0 && in_x && in_y;
        const bool toggle = !boundary && ((py > y) != (qy > y)) && (qy > py ? c > 0 : c < 0);
        parity ^= (int)toggle;
        any |= (int)boundary;
    }
#pragma unroll
    for (int s = L / 2; s >= 1; s >>= 1) {
        parity ^= __shfl_xor(parity, s, L);
        any |= __shfl_xor(any, s, L);
    }
    if (live && lane == 0)
        inside_out[k] = ok ? (uint8_t)(!any && parity) : (uint8_t)2;
}

template <int L>
unsigned query_blocks(int64_t q) { return (unsigned)((q + kOutlineBlock / L - 1) / (kOutlineBlock / L)); }

// the arguments the two outline calls share; `lanes` comes back as 8 or 64.  q == 0 and m == 0 are the caller's
int outline_check(const char *name, int64_t npoints, int m, int64_t q, int &lanes)
{
    VA_REQUIRE(npoints >= 0 && m >= 0 && q >= 0, "%s: negative count (npoints %lld, m %d, q %lld)", name,
               (long long)npoints, m, (long long)q);
    VA_REQUIRE(lanes == 0 || lanes == 8 || lanes == 64, "%s: lanes is 0 (the library's choice), 8 or 64, got %d", name,
               lanes);
    if (lanes == 0)
        lanes = m > 0 && npoints / m >= VA_OUTLINE_WIDE_MIN_POINTS ? 64 : 8;
    VA_REQUIRE(q <= (int64_t)0x7FFFFFFF * (256 / lanes), "%s: %lld queries are more than one launch of %d lanes takes",
               name, (long long)q, lanes);
    return VA_OK;
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

int va_ray_hits(const double *points, const int64_t *point_off, const uint8_t *closed, int64_t npoints, int m,
                const double *anchors, const double *fars, const int32_t *index, int64_t q, int lanes, double *t_out,
                double *hits_out, int32_t *edge_out, int32_t *count_out, void *stream)
{
    VA_ENTER();
    int rc = outline_check("va_ray_hits", npoints, m, q, lanes);
    if (rc || q == 0 || m == 0)
        return rc;
    VA_REQUIRE(points && point_off && closed && anchors && fars && index && t_out && hits_out && edge_out && count_out,
               "va_ray_hits: NULL argument");
    hipStream_t st = as_stream(stream);
    const dim3 block(kOutlineBlock);
    if (lanes == 8)
        hipLaunchKernelGGL(ray_hits_kernel<8>, dim3(query_blocks<8>(q)), block, 0, st, points, point_off, closed,
                           npoints, m, anchors, fars, index, q, t_out, hits_out, edge_out, count_out);
    else
        hipLaunchKernelGGL(ray_hits_kernel<64>, dim3(query_blocks<64>(q)), block, 0, st, points, point_off, closed,
                           npoints, m, anchors, fars, index, q, t_out, hits_out, edge_out, count_out);
    VA_LAUNCH_CHECK("ray_hits_kernel");
    return VA_OK;
}

int va_points_in_outlines(const double *points, const int64_t *point_off, int64_t npoints, int m, const double *query,
                          const int32_t *index, int64_t q, int lanes, uint8_t *inside_out, void *stream)
{
    VA_ENTER();
    int rc = outline_check("va_points_in_outlines", npoints, m, q, lanes);
    if (rc || q == 0 || m == 0)
        return rc;
    VA_REQUIRE(points && point_off && query && index && inside_out, "va_points_in_outlines: NULL argument");
    hipStream_t st = as_stream(stream);
    const dim3 block(kOutlineBlock);
    if (lanes == 8)
        hipLaunchKernelGGL(points_in_outlines_kernel<8>, dim3(query_blocks<8>(q)), block, 0, st, points, point_off,
                           npoints, m, query, index, q, inside_out);
    else
        hipLaunchKernelGGL(points_in_outlines_kernel<64>, dim3(query_blocks<64>(q)), block, 0, st, points, point_off,
                           npoints, m, query, index, q, inside_out);
    VA_LAUNCH_CHECK("points_in_outlines_kernel");
    return VA_OK;
}

}  // extern "C"
