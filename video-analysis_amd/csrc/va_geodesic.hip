// va_geodesic.hip -- geodesic distance maps in masks, the shortest-path walk back through such a map,
//                    and the farthest-point iteration over them.
//
// replaces make_distance_map              video/analysis/regions.py:455-509
//          shortest_path_in_distance_map  video/analysis/regions.py:513-565
//          get_farthest_points            video/analysis/regions.py:568-611
//
// The reference runs a Dijkstra over Python sets on the 8-neighbour grid (straight steps 1,
// diagonal steps sqrt2, diagonals may pass between two walls) and writes int(2 + d) at a pixel's
// first fill.  Every geodesic distance is d = a + b*sqrt2 with a straight and b diagonal steps; as
// sqrt2 is irrational the shortest d of a pixel has exactly one pair (a, b), so each relaxation
// order that reaches the fixpoint gives the same map, 2 + a + floor(b*sqrt2).  This file keeps the
// pair per pixel and relaxes to that fixpoint in parallel:
//   * one workgroup per frame; all synchronisation stays inside it
//   * a sweep walks the rows of the working box in order (top-down, then bottom-up); a row is
//     spread over the workgroup, K contiguous columns per thread.  Per row: relax from the three
//     neighbours in the row before (+1 straight, +sqrt2 diagonal), then propagate along the row in
//     both directions with a segmented min-scan whose segments are broken by walls
//   * down-up pairs repeat until one of them changes nothing
//   * every thread owns the same columns in every row and every sweep, so the pairs a thread
//     reads in global memory are ones it wrote itself; the row before lives in registers, and only
//     its two edge values cross threads, through LDS
// Work grows with the number of turns a geodesic takes (a spiral needs a pair per turn).
#include "va_common.h"

namespace va {

namespace {

constexpr int kGeoThreads = 256;                  // 4 waves
constexpr int kGeoWaves = kGeoThreads / kWave;
constexpr int kInfA = 0x3fffffff;                 // unreached: (kInfA, 0); sums with a row width stay in int32
constexpr int kWallA = -1;                        // not fillable: (kWallA, 0)
constexpr double kSqrt2 = 1.4142135623730951;
constexpr double kInvSqrt2 = 1.0 / 1.4142135623730951;   // the reference's 1 / np.sqrt(2)
constexpr int kMaxK = 32;                         // columns per thread: boxes up to 8192 wide

struct Pr {
    int a, b;
};
__device__ __forceinline__ Pr mkp(int a, int b) { return Pr{a, b}; }
__device__ __forceinline__ bool same(Pr x, Pr y) { return x.a == y.a && x.b == y.b; }

// a1 + b1*sqrt2 < a2 + b2*sqrt2, exactly: the double difference decides whenever it is clear of
// its rounding (|p|, |q| < 2^31: error below 1e-6), integers settle the rest
__device__ __forceinline__ bool pless(Pr x, Pr y)
{
    const long long p = (long long)x.a - y.a, q = (long long)x.b - y.b;
    const double d = (double)p + (double)q * kSqrt2;
    if (d < -1e-3)
        return true;
    if (d > 1e-3)
        return false;
    if (p <= 0 && q <= 0)
        return p < 0 || q < 0;
    if (p >= 0 && q >= 0)
        return false;
    if (p < 0)
        return 2 * q * q < p * p;   // q > 0: q*sqrt2 < -p
    return p * p < 2 * q * q;       // p > 0, q < 0: p < -q*sqrt2
}
__device__ __forceinline__ Pr pmin(Pr x, Pr y) { return pless(y, x) ? y : x; }

// floor(b * sqrt2) = isqrt(2 b^2)
__device__ __forceinline__ long long floor_b_sqrt2(int b)
{
    const long long bb = 2ll * b * b;
    long long r = (long long)((double)b * kSqrt2);
    while (r > 0 && r * r > bb)
        r--;
    while ((r + 1) * (r + 1) <= bb)
        r++;
    return r;
}
__device__ __forceinline__ int map_value(Pr p)   // 0 wall, 1 unreached, 2 + floor(d) filled
{
    if (p.a == kWallA)
        return 0;
    if (p.a >= kInfA)
        return 1;
    return (int)(2 + p.a + floor_b_sqrt2(p.b));
}

__device__ __forceinline__ unsigned long long pack(Pr p)
{
    return (unsigned long long)(unsigned)p.a | ((unsigned long long)(unsigned)p.b << 32);
}
__device__ __forceinline__ Pr unpack(unsigned long long v) { return Pr{(int)(unsigned)v, (int)(unsigned)(v >> 32)}; }
// pairs written by other waves of this workgroup (after a barrier): the labelling kernels' idiom
__device__ __forceinline__ Pr ld_shared_pair(const unsigned long long *p)
{
    return unpack(__hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
}

// The row scan composes functions f(in) = min(in + n straight steps, loc); n < 0: a wall in the
// span, f(in) = loc.  Applied to "unreached" a function gives loc (loc is never above it).
struct Fn {
    int n;
    Pr loc;
};
__device__ __forceinline__ Fn fn_id() { return Fn{0, mkp(kInfA, 0)}; }
// first f, then g
__device__ __forceinline__ Fn compose(Fn f, Fn g)
{
    if (g.n < 0)
        return g;
    Fn r;
    r.n = f.n < 0 ? -1 : f.n + g.n;
    r.loc = pmin(mkp(f.loc.a + g.n, f.loc.b), g.loc);
    return r;
}
__device__ __forceinline__ Fn shfl_fn(Fn f, int src)
{
    return Fn{__shfl(f.n, src), mkp(__shfl(f.loc.a, src), __shfl(f.loc.b, src))};
}

struct GeoShared {
    Fn fwd[kGeoWaves], bwd[kGeoWaves];
    Pr first[kGeoThreads], last[kGeoThreads];   // edges of the row before, per thread
    unsigned long long red[kGeoWaves];
    int ired[kGeoWaves][4];
    Pr endp;
    int endi;
};

__host__ __device__ __forceinline__ int row_words(int w) { return (w + 31) / 32; }

struct Box {
    int x0, y0, x1, y1;   // [x0, x1) x [y0, y1); empty when x1 <= x0
};

// one sweep over the rows of the box; returns whether this thread lowered any pair
template <int K>
__device__ __forceinline__ bool sweep(unsigned long long *P, int w, const Box bx, bool down, GeoShared &sh)
{
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wv = tid >> 6;
    const int c0 = bx.x0 + tid * K;
    const int H = bx.y1 - bx.y0;
    bool changed = false;
    Pr up[K];
#pragma unroll
    for (int i = 0; i < K; i++)
        up[i] = mkp(kInfA, 0);
    Pr upl = mkp(kInfA, 0), upr = mkp(kInfA, 0);
    // a row's own pairs do not depend on the row before: the next row's loads are issued one row
    // ahead, so only the LDS exchange stands between two rows
    unsigned long long nxt[K];
    auto load_row = [&](int s) {
        const unsigned long long *row = P + (size_t)(down ? bx.y0 + s : bx.y1 - 1 - s) * w;
#pragma unroll
        for (int i = 0; i < K; i++)
            nxt[i] = c0 + i < bx.x1 ? row[c0 + i] : pack(mkp(kWallA, 0));
    };
    load_row(0);
    for (int s = 0; s < H; s++) {
        const int y = down ? bx.y0 + s : bx.y1 - 1 - s;
        unsigned long long *row = P + (size_t)y * w;
        Pr old[K], r[K];
#pragma unroll
        for (int i = 0; i < K; i++)
            old[i] = unpack(nxt[i]);
        if (s + 1 < H)
            load_row(s + 1);
        // from the row before: straight +1, diagonal +sqrt2
#pragma unroll
        for (int i = 0; i < K; i++) {
            if (old[i].a == kWallA) {
                r[i] = old[i];
                continue;
            }
            const Pr l = i > 0 ? up[i - 1] : upl, rr = i + 1 < K ? up[i + 1] : upr;
            Pr v = pmin(old[i], mkp(up[i].a + 1, up[i].b));
            v = pmin(v, mkp(l.a, l.b + 1));
            v = pmin(v, mkp(rr.a, rr.b + 1));
            r[i] = v;
        }
        // this thread's forward / backward functions
        Fn ff{K, mkp(kInfA, 0)}, fb{K, mkp(kInfA, 0)};
#pragma unroll
        for (int i = 0; i < K; i++) {
            if (r[i].a == kWallA) {
                ff.n = -1;
                ff.loc = mkp(kInfA, 0);
            } else {
                ff.loc = pmin(mkp(ff.loc.a + 1, ff.loc.b), r[i]);
            }
            const int j = K - 1 - i;
            if (r[j].a == kWallA) {
                fb.n = -1;
                fb.loc = mkp(kInfA, 0);
            } else {
                fb.loc = pmin(mkp(fb.loc.a + 1, fb.loc.b), r[j]);
            }
        }
        // wave scans: forward over increasing lanes, backward over decreasing lanes
        Fn sf = ff, sb = fb;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const Fn gf = shfl_fn(sf, lane - off), gb = shfl_fn(sb, lane + off);
            if (lane >= off)
                sf = compose(gf, sf);
            if (lane + off < kWave)
                sb = compose(gb, sb);
        }
        if (lane == kWave - 1)
            sh.fwd[wv] = sf;
        if (lane == 0)
            sh.bwd[wv] = sb;
        Fn ef = shfl_fn(sf, lane - 1), eb = shfl_fn(sb, lane + 1);   // exclusive within the wave
        if (lane == 0)
            ef = fn_id();
        if (lane == kWave - 1)
            eb = fn_id();
        __syncthreads();
        Fn pf = fn_id(), pb = fn_id();
        for (int k = 0; k < wv; k++)
            pf = compose(pf, sh.fwd[k]);
        for (int k = kGeoWaves - 1; k > wv; k--)
            pb = compose(pb, sh.bwd[k]);
        Pr runf = compose(pf, ef).loc, runb = compose(pb, eb).loc;
        Pr fwdv[K];
#pragma unroll
        for (int i = 0; i < K; i++) {
            if (r[i].a == kWallA) {
                runf = mkp(kInfA, 0);
                fwdv[i] = r[i];
            } else {
                runf = pmin(mkp(runf.a + 1, runf.b), r[i]);
                fwdv[i] = runf;
            }
        }
#pragma unroll
        for (int j = K - 1; j >= 0; j--) {
            Pr fin;
            if (r[j].a == kWallA) {
                runb = mkp(kInfA, 0);
                fin = mkp(kInfA, 0);    // the row after sees walls as unreached
            } else {
                runb = pmin(mkp(runb.a + 1, runb.b), r[j]);
                fin = pmin(fwdv[j], runb);
                if (!same(fin, old[j])) {
                    changed = true;
                    row[c0 + j] = pack(fin);
                }
            }
            up[j] = fin;
        }
        sh.first[tid] = up[0];
        sh.last[tid] = up[K - 1];
        __syncthreads();
        upl = tid > 0 ? sh.last[tid - 1] : mkp(kInfA, 0);
        upr = tid + 1 < kGeoThreads ? sh.first[tid + 1] : mkp(kInfA, 0);
    }
    return changed;
}

// init the box from `fill` (a pixel of the frame is fillable iff fill(x, y)), seed the starts,
// relax to the fixpoint; returns the number of sweeps
template <int K, class Fill, class Starts>
__device__ __forceinline__ int build_map(unsigned long long *P, int w, const Box bx, Fill fill, Starts starts,
                         GeoShared &sh)
{
    const int tid = threadIdx.x;
    const int c0 = bx.x0 + tid * K;
    for (int y = bx.y0; y < bx.y1; y++)
        for (int i = 0; i < K; i++) {
            const int x = c0 + i;
            if (x < bx.x1)
                P[(size_t)y * w + x] = pack(fill(x, y) ? mkp(kInfA, 0) : mkp(kWallA, 0));
        }
    starts([&](int x, int y) {   // the owner of column x seeds it
        if (x >= c0 && x < c0 + K && x < bx.x1 && y >= bx.y0 && y < bx.y1 && fill(x, y))
            P[(size_t)y * w + x] = pack(mkp(0, 0));
    });
    int sweeps = 0;
    for (;;) {
        bool ch = sweep<K>(P, w, bx, true, sh);
        ch = sweep<K>(P, w, bx, false, sh) || ch;
        sweeps += 2;
        if (!__syncthreads_or(ch))
            break;
    }
    return sweeps;
}

__device__ __forceinline__ unsigned long long block_max_u64(unsigned long long v, GeoShared &sh)
{
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0)
        sh.red[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long m = sh.red[0];
    for (int k = 1; k < kGeoWaves; k++)
        m = sh.red[k] > m ? sh.red[k] : m;
    __syncthreads();
    return m;
}

// (min x, min y, max x, max y) of the pixels with sel(x, y) over the whole frame
template <class Sel>
__device__ __forceinline__ Box block_bbox(int h, int w, Sel sel, GeoShared &sh)
{
    int v[4] = {w, h, -1, -1};
    for (size_t i = threadIdx.x; i < (size_t)h * w; i += kGeoThreads) {
        const int y = (int)(i / w), x = (int)(i % w);
        if (sel(x, y)) {
            v[0] = min(v[0], x);
            v[1] = min(v[1], y);
            v[2] = max(v[2], x);
            v[3] = max(v[3], y);
        }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        v[0] = min(v[0], __shfl_xor(v[0], off));
        v[1] = min(v[1], __shfl_xor(v[1], off));
        v[2] = max(v[2], __shfl_xor(v[2], off));
        v[3] = max(v[3], __shfl_xor(v[3], off));
    }
    __syncthreads();
    if ((threadIdx.x & (kWave - 1)) == 0)
        for (int k = 0; k < 4; k++)
            sh.ired[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
    Box b{w, h, -1, -1};
    for (int k = 0; k < kGeoWaves; k++) {
        b.x0 = min(b.x0, sh.ired[k][0]);
        b.y0 = min(b.y0, sh.ired[k][1]);
        b.x1 = max(b.x1, sh.ired[k][2]);
        b.y1 = max(b.y1, sh.ired[k][3]);
    }
    __syncthreads();
    b.x1 += 1;   // inclusive -> exclusive (empty: x1 = 0 <= x0)
    b.y1 += 1;
    return b;
}

__device__ __forceinline__ bool box_has(const Box b, int x, int y)
{
    return x >= b.x0 && x < b.x1 && y >= b.y0 && y < b.y1;
}

// ---- the reference's walk down a distance map (one lane) ------------------------------------
// D(x, y) as the reference's padded int64 copy holds it: values <= 1 and the pad read INT64_MAX.
// `visited` (h * ceil(w/32) words, zero) is the `in points` test.  Returns the full path length;
// stores the first `cap` points.
template <class Val>
__device__ __forceinline__ int walk_path(Val val, int h, int w, int ex, int ey, uint32_t *visited, int32_t *out, int cap)
{
    const long long kMax = 0x7fffffffffffffffll;
    const int w32 = row_words(w);
    auto D = [&](int x, int y) -> long long {
        if (x < 0 || y < 0 || x >= w || y >= h)
            return kMax;
        const long long v = val(x, y);
        return v <= 1 ? kMax : v;
    };
    auto mark = [&](int x, int y) {
        uint32_t *p = visited + (size_t)y * w32 + (x >> 5);
        *p |= 1u << (x & 31);
    };
    auto seen = [&](int x, int y) { return (visited[(size_t)y * w32 + (x >> 5)] >> (x & 31)) & 1u; };
    int x = ex, y = ey, n = 0;
    long long d = D(x, y);
    if (d == kMax)
        return 0;
    auto push = [&](int px, int py) {
        if (n < cap) {
            out[2 * n] = px;
            out[2 * n + 1] = py;
        }
        n++;
        mark(px, py);
    };
    push(x, y);
    for (long long guard = (long long)h * w + 1; guard > 0; guard--) {
        double best = 0.0;
        int bi = -1;
        for (int k = 0; k < 9; k++) {   // row-major, first minimum
            const int dy = k / 3, dx = k % 3;
            const double wgt = (dy == 1 || dx == 1) ? 1.0 : kInvSqrt2;
            const double sc = (double)(D(x + dx - 1, y + dy - 1) - d) * wgt;
            if (bi < 0 || sc < best) {
                best = sc;
                bi = k;
            }
        }
        x += bi % 3 - 1;
        y += bi / 3 - 1;
        const long long v = D(x, y);
        if (v < d)
            d = v;
        else if (v == d) {
            if (seen(x, y))
                break;
        } else
            break;
        push(x, y);
    }
    return n;
}

__device__ void zero_words(uint32_t *p, size_t count)
{
    for (size_t i = threadIdx.x; i < count; i += kGeoThreads)
        p[i] = 0;
    __syncthreads();
}

// ---- make_distance_map -------------------------------------------------------------------------
template <int K>
__global__ void __launch_bounds__(kGeoThreads)
distance_map_kernel(const uint8_t *__restrict__ fillable, int h, int w, const int32_t *__restrict__ starts,
                    const int32_t *__restrict__ nstarts, int max_starts, const int32_t *__restrict__ ends,
                    const int32_t *__restrict__ nends, int max_ends, int32_t *__restrict__ out,
                    unsigned long long *__restrict__ pairs, int32_t *__restrict__ sweeps_out)
{
    __shared__ GeoShared sh;
    const int f = blockIdx.x, tid = threadIdx.x;
    const size_t px = (size_t)h * w;
    const uint8_t *F = fillable + f * px;
    unsigned long long *P = pairs + f * px;
    int32_t *O = out + f * px;
    auto fill = [&](int x, int y) { return F[(size_t)y * w + x] != 0; };
    const Box bx = block_bbox(h, w, fill, sh);
    int sweeps = 0;
    if (bx.x1 > bx.x0) {
        const int ns = min(nstarts[f], max_starts);
        const int32_t *S = starts + (size_t)f * max_starts * 2;
        sweeps = build_map<K>(P, w, bx, fill, [&](auto seed) {
            for (int i = 0; i < ns; i++) {
                const int x = S[2 * i], y = S[2 * i + 1];
                if (x >= 0 && x < w && y >= 0 && y < h)
                    seed(x, y);
            }
        }, sh);
    }
    __syncthreads();
    if (tid == 0) {   // the nearest reachable end point (the first listed on ties)
        sh.endi = -1;
        sh.endp = mkp(kInfA, 0);
        const int ne = ends ? min(nends[f], max_ends) : 0;
        const int32_t *E = ends ? ends + (size_t)f * max_ends * 2 : nullptr;
        for (int i = 0; i < ne; i++) {
            const int x = E[2 * i], y = E[2 * i + 1];
            if (x < 0 || x >= w || y < 0 || y >= h || !box_has(bx, x, y))
                continue;
            const Pr p = ld_shared_pair(P + (size_t)y * w + x);
            if (p.a == kWallA || p.a >= kInfA)
                continue;
            if (pless(p, sh.endp)) {
                sh.endp = p;
                sh.endi = y * w + x;
            }
        }
    }
    __syncthreads();
    const int endi = sh.endi;
    const Pr endp = sh.endp;
    for (size_t i = tid; i < px; i += kGeoThreads) {
        const int y = (int)(i / w), x = (int)(i % w);
        int v = 0;
        if (box_has(bx, x, y)) {
            const Pr p = ld_shared_pair(P + i);
            v = map_value(p);
            if (v >= 2 && endi >= 0 && (int)i != endi && !pless(p, endp))
                v = 1;   // at or beyond the end point's distance: left unfilled
        }
        O[i] = v;
    }
    if (tid == 0 && sweeps_out)
        sweeps_out[f] = sweeps;
}

// ---- shortest_path_in_distance_map -------------------------------------------------------------
__global__ void __launch_bounds__(kGeoThreads)
distance_path_kernel(const int32_t *__restrict__ map, int h, int w, const int32_t *__restrict__ end_points,
                     int32_t *__restrict__ path, int max_points, int32_t *__restrict__ npath,
                     uint32_t *__restrict__ visited)
{
    const int f = blockIdx.x;
    const size_t px = (size_t)h * w;
    uint32_t *V = visited + (size_t)f * h * row_words(w);
    zero_words(V, (size_t)h * row_words(w));
    if (threadIdx.x != 0)
        return;
    const int32_t *M = map + f * px;
    const int ex = end_points[2 * f], ey = end_points[2 * f + 1];
    int n = 0;
    if (ex >= 0 && ex < w && ey >= 0 && ey < h)
        n = walk_path([&](int x, int y) { return (long long)M[(size_t)y * w + x]; }, h, w, ex, ey, V,
                      path + (size_t)f * max_points * 2, max_points);
    npath[f] = n;
}

// ---- get_farthest_points -----------------------------------------------------------------------
// p1 (n, 2): the start of each frame.  default_start: p1 came from launch_longest_external_start,
// whose (-1, -1) marks a frame with no component (nothing is computed for it); a caller's own start
// is never read that way -- one outside the frame is ignored by the map, as in the reference.
// dist_out (n): the map value at p2; rounds_out (n, 2): maps built, sweeps over all of them.
template <int K>
__global__ void __launch_bounds__(kGeoThreads)
farthest_points_kernel(const uint8_t *__restrict__ mask, int h, int w, const int32_t *__restrict__ p1_in,
                       int32_t *__restrict__ p1_out, int32_t *__restrict__ p2_out, int32_t *__restrict__ dist_out,
                       int32_t *__restrict__ rounds_out,
                       int32_t *__restrict__ path, int max_points, int32_t *__restrict__ npath,
                       unsigned long long *__restrict__ pairs, uint32_t *__restrict__ visited, int default_start)
{
    __shared__ GeoShared sh;
    const int f = blockIdx.x, tid = threadIdx.x;
    const size_t px = (size_t)h * w;
    const uint8_t *F = mask + f * px;
    unsigned long long *P = pairs + f * px;
    int p1x = p1_in[2 * f], p1y = p1_in[2 * f + 1];
    if (default_start && p1x == -1 && p1y == -1) {
        if (tid == 0) {
            p1_out[2 * f] = p1_out[2 * f + 1] = -1;
            p2_out[2 * f] = p2_out[2 * f + 1] = -1;
            dist_out[f] = rounds_out[2 * f] = rounds_out[2 * f + 1] = 0;
            if (npath)
                npath[f] = 0;
        }
        return;
    }
    auto fill = [&](int x, int y) { return F[(size_t)y * w + x] != 0; };
    Box bx = block_bbox(h, w, fill, sh);
    // the map value anywhere in the frame: pairs inside the box, 1 / 0 outside it
    auto value = [&](const Box b, int x, int y) -> int {
        if (!fill(x, y))
            return 0;
        if (!box_has(b, x, y))
            return 1;
        return map_value(ld_shared_pair(P + (size_t)y * w + x));
    };
    int dist_prev = 0, dist = 0, rounds = 0, sweeps = 0, p2x = 0, p2y = 0;
    for (;;) {
        if (bx.x1 > bx.x0)
            sweeps += build_map<K>(P, w, bx, fill, [&](auto seed) {
                if (p1x >= 0 && p1x < w && p1y >= 0 && p1y < h)
                    seed(p1x, p1y);
            }, sh);
        rounds++;
        __syncthreads();
        // first maximum in raster order, and the box of the reached pixels
        unsigned long long key = 0;
        for (size_t i = tid; i < px; i += kGeoThreads) {
            const int v = value(bx, (int)(i % w), (int)(i / w));
            const unsigned long long k = ((unsigned long long)(unsigned)v << 32) | (0xffffffffu - (unsigned)i);
            key = k > key ? k : key;
        }
        key = block_max_u64(key, sh);
        dist = (int)(key >> 32);
        const int idx = (int)(0xffffffffu - (unsigned)(key & 0xffffffffu));
        p2x = idx % w;
        p2y = idx / w;
        if (dist <= dist_prev)
            break;
        if (dist >= 2) {   // later maps start inside this component: its box is enough
            const Box cur = bx;
            bx = block_bbox(h, w, [&, cur](int x, int y) { return box_has(cur, x, y) && value(cur, x, y) >= 2; }, sh);
        }
        dist_prev = dist;
        p1x = p2x;
        p1y = p2y;
    }
    if (path) {
        uint32_t *V = visited + (size_t)f * h * row_words(w);
        zero_words(V, (size_t)h * row_words(w));
        if (tid == 0)
            npath[f] = walk_path([&](int x, int y) { return (long long)value(bx, x, y); }, h, w, p2x, p2y, V,
                                 path + (size_t)f * max_points * 2, max_points);
    }
    if (tid == 0) {
        p1_out[2 * f] = p1x;
        p1_out[2 * f + 1] = p1y;
        p2_out[2 * f] = p2x;
        p2_out[2 * f + 1] = p2y;
        dist_out[f] = dist;
        rounds_out[2 * f] = rounds;
        rounds_out[2 * f + 1] = sweeps;
    }
}

int cols_per_thread(int w)
{
    int k = 1;
    while (k * kGeoThreads < w)
        k <<= 1;
    return k;
}

}  // namespace

// The workspace: [pairs | visited | inverted bits | labelling rows | edge bits | keys | counts | p1]; while the
// default start is chosen the pairs hold the 8-connected forest and the background labels, the visited
// bitmap the bit mask (the distance maps come after, in stream order)
struct GeoLayout {
    size_t pairs, visited, inv, rows, rows_bytes, edge, keys, counts, p1, total;
};
static GeoLayout geo_layout(int n, int h, int w)
{
    GeoLayout g;
    Carve c;
    const size_t visited_bytes = (size_t)n * h * row_words(w) * sizeof(uint32_t);
    g.pairs = c.take((size_t)n * h * w * sizeof(unsigned long long));
    g.visited = c.take(visited_bytes);
    g.inv = c.take(visited_bytes);
    g.rows_bytes = ccl_rows_workspace_bytes(n, h);
    g.rows = c.take(g.rows_bytes);
    g.edge = c.take((size_t)n * edge_label_words(h, w) * sizeof(uint32_t));
    g.keys = c.take((size_t)2 * n * sizeof(unsigned long long));
    g.counts = c.take((size_t)2 * n * sizeof(int32_t));
    g.p1 = c.take((size_t)2 * n * sizeof(int32_t));
    g.total = c.total;
    return g;
}

#define VA_GEO_DISPATCH(KERNEL, ...)                                                  \
    switch (cols_per_thread(w)) {                                                     \
    case 1: KERNEL<1><<<n, kGeoThreads, 0, st>>>(__VA_ARGS__); break;                 \
    case 2: KERNEL<2><<<n, kGeoThreads, 0, st>>>(__VA_ARGS__); break;                 \
    case 4: KERNEL<4><<<n, kGeoThreads, 0, st>>>(__VA_ARGS__); break;                 \
    case 8: KERNEL<8><<<n, kGeoThreads, 0, st>>>(__VA_ARGS__); break;                 \
    case 16: KERNEL<16><<<n, kGeoThreads, 0, st>>>(__VA_ARGS__); break;               \
    case 32: KERNEL<32><<<n, kGeoThreads, 0, st>>>(__VA_ARGS__); break;               \
    default: set_error("geodesic: frames wider than %d columns are not supported", kMaxK * kGeoThreads); \
        return VA_ERR_INVALID;                                                        \
    }

#define VA_GEO_REQUIRE_SHAPE(name)                                                                        \
    VA_REQUIRE_FRAME_SHAPE(name);                                                                         \
    VA_REQUIRE(cols_per_thread(w) <= kMaxK, name ": frames wider than 8192 columns are not supported");   \
    VA_REQUIRE(ws && ws_bytes >= va_geodesic_workspace_bytes(n, h, w),                                    \
               name ": workspace of %zu bytes < required %zu", ws_bytes, va_geodesic_workspace_bytes(n, h, w))

}  // namespace va

using namespace va;

extern "C" {

size_t va_geodesic_workspace_bytes(int n, int h, int w)
{
    if (n <= 0 || h <= 0 || w <= 0)
        return 256;
    return geo_layout(n, h, w).total;
}

int va_distance_map_i32(const uint8_t *fillable, int n, int h, int w, const int32_t *starts, const int32_t *nstarts,
                        int max_starts, const int32_t *ends, const int32_t *nends, int max_ends, int32_t *map_out,
                        void *ws, size_t ws_bytes, void *stream)
{
    VA_ENTER();
    VA_GEO_REQUIRE_SHAPE("va_distance_map_i32");
    VA_REQUIRE(fillable && map_out && starts && nstarts && max_starts > 0, "va_distance_map_i32: NULL argument");
    VA_REQUIRE(!ends || (nends && max_ends > 0), "va_distance_map_i32: end points without counts");
    if (n == 0)
        return VA_OK;
    hipStream_t st = as_stream(stream);
    VA_GEO_DISPATCH(distance_map_kernel, fillable, h, w, starts, nstarts, max_starts, ends, nends, ends ? max_ends : 0,
                    map_out, at<unsigned long long>(ws, geo_layout(n, h, w).pairs), nullptr);
    VA_LAUNCH_CHECK("distance_map_kernel");
    return VA_OK;
}

int va_distance_map_path(const int32_t *map, int n, int h, int w, const int32_t *end_points, int32_t *path_out,
                         int max_points, int32_t *npath_out, void *ws, size_t ws_bytes, void *stream)
{
    VA_ENTER();
    VA_GEO_REQUIRE_SHAPE("va_distance_map_path");
    VA_REQUIRE(map && end_points && path_out && npath_out && max_points > 0, "va_distance_map_path: NULL argument");
    if (n == 0)
        return VA_OK;
    distance_path_kernel<<<n, kGeoThreads, 0, as_stream(stream)>>>(map, h, w, end_points, path_out, max_points,
                                                                  npath_out,
                                                                  at<uint32_t>(ws, geo_layout(n, h, w).visited));
    VA_LAUNCH_CHECK("distance_path_kernel");
    return VA_OK;
}

int va_farthest_points(const uint8_t *mask, int n, int h, int w, const int32_t *p1, int32_t *p1_out, int32_t *p2_out,
                       int32_t *dist_out, int32_t *rounds_out, int32_t *path_out, int max_points, int32_t *npath_out,
                       void *ws, size_t ws_bytes, void *stream)
{
    VA_ENTER();
    VA_GEO_REQUIRE_SHAPE("va_farthest_points");
    VA_REQUIRE(mask && p1_out && p2_out && dist_out && rounds_out, "va_farthest_points: NULL argument");
    VA_REQUIRE(!path_out || (npath_out && max_points > 0), "va_farthest_points: path without npath / max_points");
    if (n == 0)
        return VA_OK;
    hipStream_t st = as_stream(stream);
    const GeoLayout g = geo_layout(n, h, w);
    unsigned long long *pairs = at<unsigned long long>(ws, g.pairs);
    uint32_t *visited = at<uint32_t>(ws, g.visited);
    const bool default_start = p1 == nullptr;
    if (default_start) {
        uint32_t *bits = visited;
        int32_t *forest = (int32_t *)pairs, *bg_labels = forest + (size_t)n * h * w;
        int32_t *start = at<int32_t>(ws, g.p1);
        int rc = launch_pack_bits(mask, bits, n, h, w, 0, st);
        if (!rc)
            rc = launch_outline_labels(bits, at<uint32_t>(ws, g.inv), forest, bg_labels, at<int32_t>(ws, g.counts),
                                       at(ws, g.rows), g.rows_bytes, n, h, w, st);
        if (!rc)
            rc = launch_longest_external_start(bits, forest, bg_labels, at<uint32_t>(ws, g.edge), n, h, w,
                                               at<unsigned long long>(ws, g.keys), start, st);
        if (rc)
            return rc;
        p1 = start;
    }
    VA_GEO_DISPATCH(farthest_points_kernel, mask, h, w, p1, p1_out, p2_out, dist_out, rounds_out, path_out, max_points,
                    npath_out, pairs, visited, default_start ? 1 : 0);
    VA_LAUNCH_CHECK("farthest_points_kernel");
    return VA_OK;
}

}  // extern "C"
