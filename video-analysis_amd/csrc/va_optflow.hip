// va_optflow.hip -- dense optical flow (Farneback) between consecutive frames
//
// replaces  cv2.calcOpticalFlowFarneback(prev, next, None, pyr_scale, levels, winsize, iterations, poly_n,
//           poly_sigma, 0) and cv2.cartToPolar's magnitude, FilterOpticalFlow._compare_frames,
//           video/filters.py:572-589
//
// OpenCV's scalar algorithm (modules/video/src/optflowgf.cpp, flags = 0), restated operation for operation with
// no contraction (-ffp-contract=off): DESIGN.md "Optical flow" pins every rounding step, and
// tests/golden/make_golden_optflow.py restates it in NumPy.  One call takes n frames and computes the n - 1
// pairs level-major: at each pyramid level every frame is blurred, resized and expanded (PolyExp) once, and
// serves the two pairs it belongs to.  Per level and pair: UpdateMatrices, then per iteration the vertical
// running sums (one lane per pair, column and channel), the horizontal running sums with the 2x2 solve
// (one lane per pair and row; on the last iteration of level 0 it writes the magnitude too), and, before the
// next iteration, UpdateMatrices again from the new flow.  The running sums are sequential recurrences, as in
// OpenCV, which is what keeps them bit-exact.  No kernel uses scratch memory.
#include <math.h>

#include <vector>

#include "va_common.h"

namespace va {
namespace {

constexpr int kBlock = 256;
constexpr int kMinSize = 32;       // calcOpticalFlowFarneback's min_size
constexpr int kMaxPolyN = 7;

struct PolyConsts {
    float g[kMaxPolyN + 1], xg[kMaxPolyN + 1], xxg[kMaxPolyN + 1];   // offsets 0..n
    double ig11, ig03, ig33, ig55;
};

// GaussianBlur row pass (SymmRowSmallFilter for ksize <= 5, RowFilter above), converting to float on the fly
template <class T>
__global__ void __launch_bounds__(kBlock)
of_blur_rows_kernel(const T *__restrict__ src, float *__restrict__ dst, int h, int w, TapsF32 taps)
{
    const int x = blockIdx.x * kBlock + threadIdx.x;
    if (x >= w)
        return;
    const size_t row = ((size_t)blockIdx.z * h + blockIdx.y) * w;
    const T *S = src + row;
    const int k = taps.ksize, r = k / 2;
    float s;
    if (k <= 5) {
        s = (float)S[x] * taps.t[r] + ((float)S[reflect101(x - 1, w)] + (float)S[reflect101(x + 1, w)]) * taps.t[r + 1];
        if (k == 5)
            s = s + ((float)S[reflect101(x - 2, w)] + (float)S[reflect101(x + 2, w)]) * taps.t[r + 2];
    } else {
        s = taps.t[0] * (float)S[reflect101(x - r, w)];
        for (int i = 1; i < k; i++)
            s = s + taps.t[i] * (float)S[reflect101(x + i - r, w)];
    }
    dst[row + x] = s;
}

// GaussianBlur column pass (SymmColumnFilter)
__global__ void __launch_bounds__(kBlock)
of_blur_cols_kernel(const float *__restrict__ src, float *__restrict__ dst, int h, int w, TapsF32 taps)
{
    const int x = blockIdx.x * kBlock + threadIdx.x;
    if (x >= w)
        return;
    const int y = blockIdx.y;
    const float *S = src + (size_t)blockIdx.z * h * w + x;
    const int r = taps.ksize / 2;
    float s = taps.t[r] * S[(size_t)y * w];
    for (int j = 1; j <= r; j++)
        s = s + taps.t[r + j] * (S[(size_t)reflect101(y + j, h) * w] + S[(size_t)reflect101(y - j, h) * w]);
    dst[((size_t)blockIdx.z * h + y) * w + x] = s;
}

// FarnebackPolyExp: one workgroup per 256 outputs of a row; the vertical triples of the row segment (plus n
// columns on each side, replicated at the frame's edges) go through LDS.  R is planar: (frame, 5, h, w).
__global__ void __launch_bounds__(kBlock)
of_poly_exp_kernel(const float *__restrict__ img, float *__restrict__ R, int h, int w, int np, PolyConsts pc)
{
    __shared__ float t0s[kBlock + 2 * kMaxPolyN], t1s[kBlock + 2 * kMaxPolyN], t2s[kBlock + 2 * kMaxPolyN];
    const int x0 = blockIdx.x * kBlock, y = blockIdx.y;
    const size_t plane = (size_t)h * w;
    const float *F = img + (size_t)blockIdx.z * plane;
    for (int i = threadIdx.x; i < kBlock + 2 * np; i += kBlock) {
        const int xs = clampi(x0 - np + i, 0, w - 1);
        float t0 = F[(size_t)y * w + xs] * pc.g[0], t1 = 0.f, t2 = 0.f;
        for (int k = 1; k <= np; k++) {
            const float sm = F[(size_t)max(y - k, 0) * w + xs], sp = F[(size_t)min(y + k, h - 1) * w + xs];
            const float p = sm + sp;
            t0 = t0 + pc.g[k] * p;
            t1 = t1 + pc.xg[k] * (sp - sm);
            t2 = t2 + pc.xxg[k] * p;
        }
        t0s[i] = t0;
        t1s[i] = t1;
        t2s[i] = t2;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w)
        return;
    const int i = threadIdx.x + np;
    double b1 = (double)(t0s[i] * pc.g[0]), b2 = 0, b3 = (double)(t1s[i] * pc.g[0]), b4 = 0,
           b5 = (double)(t2s[i] * pc.g[0]), b6 = 0;
    for (int k = 1; k <= np; k++) {
        const float p0 = t0s[i + k], m0 = t0s[i - k], p1 = t1s[i + k], m1 = t1s[i - k], p2 = t2s[i + k],
                    m2 = t2s[i - k];
        const double tg = (double)(p0 + m0);
        b1 += tg * (double)pc.g[k];
        b4 += tg * (double)pc.xxg[k];
        b2 += (double)((p0 - m0) * pc.xg[k]);
        b3 += (double)((p1 + m1) * pc.g[k]);
        b6 += (double)((p1 - m1) * pc.xg[k]);
        b5 += (double)((p2 + m2) * pc.g[k]);
    }
    float *o = R + (size_t)blockIdx.z * 5 * plane + (size_t)y * w + x;
    o[0] = (float)(b3 * pc.ig11);
    o[plane] = (float)(b2 * pc.ig11);
    o[2 * plane] = (float)(b1 * pc.ig03 + b5 * pc.ig33);
    o[3 * plane] = (float)(b1 * pc.ig03 + b4 * pc.ig33);
    o[4 * plane] = (float)(b6 * pc.ig55);
}

__device__ __forceinline__ float border_weight(int i)
{
    return i < 2 ? 0.14f : 0.4472f;
}

// FarnebackUpdateMatrices at one pixel: R0, R1 are the pair's planar expansions, (dx, dy) the flow there
__device__ __forceinline__ void of_matrices(const float *__restrict__ R0, const float *__restrict__ R1, size_t plane,
                                            int x, int y, int h, int w, float dx, float dy, float M[5])
{
    float fx = (float)x + dx, fy = (float)y + dy;
    const float x1 = floorf(fx), y1 = floorf(fy);
    fx = fx - x1;
    fy = fy - y1;
    const size_t at = (size_t)y * w + x;
    float r2, r3, r4, r5, r6;
    if (x1 >= 0.f && x1 < (float)(w - 1) && y1 >= 0.f && y1 < (float)(h - 1)) {
        const float a00 = (1.f - fx) * (1.f - fy), a01 = fx * (1.f - fy), a10 = (1.f - fx) * fy, a11 = fx * fy;
        const float *p = R1 + (size_t)(int)y1 * w + (int)x1;
        float r[5];
#pragma unroll
        for (int c = 0; c < 5; c++) {
            const float *q = p + c * plane;
            r[c] = a00 * q[0] + a01 * q[1] + a10 * q[w] + a11 * q[w + 1];
        }
        r2 = r[0];
        r3 = r[1];
        r4 = (R0[at + 2 * plane] + r[2]) * 0.5f;
        r5 = (R0[at + 3 * plane] + r[3]) * 0.5f;
        r6 = (R0[at + 4 * plane] + r[4]) * 0.25f;
    } else {
        r2 = r3 = 0.f;
        r4 = R0[at + 2 * plane];
        r5 = R0[at + 3 * plane];
        r6 = R0[at + 4 * plane] * 0.5f;
    }
    r2 = (R0[at] - r2) * 0.5f;
    r3 = (R0[at + plane] - r3) * 0.5f;
    r2 = r2 + (r4 * dy + r6 * dx);
    r3 = r3 + (r6 * dy + r5 * dx);
    if ((unsigned)(x - 5) >= (unsigned)(w - 10) || (unsigned)(y - 5) >= (unsigned)(h - 10)) {
        const float s = (x < 5 ? border_weight(x) : 1.f) * (x >= w - 5 ? border_weight(w - 1 - x) : 1.f) *
                        (y < 5 ? border_weight(y) : 1.f) * (y >= h - 5 ? border_weight(h - 1 - y) : 1.f);
        r2 *= s;
        r3 *= s;
        r4 *= s;
        r5 *= s;
        r6 *= s;
    }
    M[0] = r4 * r4 + r6 * r6;
    M[1] = (r4 + r5) * r6;
    M[2] = r5 * r5 + r6 * r6;
    M[3] = r4 * r2 + r6 * r3;
    M[4] = r6 * r2 + r5 * r3;
}

// FarnebackUpdateMatrices over a level: before its first iteration from the flow it starts from (flow (pair, h, w,
// 2) times fscale, or zero: flow == NULL), and after every iteration but the last from the new flow (fscale 1, exact)
__global__ void __launch_bounds__(kBlock)
of_update_matrices_kernel(const float *__restrict__ R, const float *__restrict__ flow, float fscale,
                          float *__restrict__ M, int h, int w)
{
    const int x = blockIdx.x * kBlock + threadIdx.x;
    if (x >= w)
        return;
    const int y = blockIdx.y;
    const size_t p = blockIdx.z, plane = (size_t)h * w, at = (size_t)y * w + x;
    float dx = 0.f, dy = 0.f;
    if (flow) {
        dx = flow[(p * plane + at) * 2] * fscale;
        dy = flow[(p * plane + at) * 2 + 1] * fscale;
    }
    float m[5];
    of_matrices(R + p * 5 * plane, R + (p + 1) * 5 * plane, plane, x, y, h, w, dx, dy, m);
    float *o = M + p * 5 * plane + at;
#pragma unroll
    for (int c = 0; c < 5; c++)
        o[c * plane] = m[c];
}

// FarnebackUpdateFlow_Blur, vertical: one lane per (pair, channel, column) runs down the column.  V is
// (pair, 5, w, h) doubles, so that the lanes of the horizontal kernel (consecutive rows) read consecutive words;
// a lane's kVsumRows new values go through LDS, so that the wave writes whole 128-byte runs of a column instead
// of one word in each of 64 columns (this kernel took 17 of 32 ms per 32 1080p pairs with direct stores).
constexpr int kVsumRows = 16;
__global__ void __launch_bounds__(kWave)
of_vsum_kernel(const float *__restrict__ M, double *__restrict__ V, int h, int w, int m)
{
    __shared__ double tile[kWave][kVsumRows + 1];
    const int lane = threadIdx.x, e0 = blockIdx.x * kWave, e = e0 + lane, ne = 5 * w;
    const bool live = e < ne;
    const int c = live ? e / w : 0, x = live ? e - c * w : 0;
    const size_t p = blockIdx.y, plane = (size_t)h * w;
    const float *Mc = M + (p * 5 + c) * plane + x;
    double *Vp = V + p * (size_t)ne * h;            // V[p][c * w + x][y]
    double v = 0;
    if (live) {
        v = (double)(Mc[0] * (float)(m + 2));
        for (int y = 1; y < m; y++)
            v += (double)Mc[(size_t)min(y, h - 1) * w];
    }
    for (int y0 = 0; y0 < h; y0 += kVsumRows) {
        if (live) {
#pragma unroll
            for (int r = 0; r < kVsumRows; r++) {
                const int y = y0 + r;
                if (y < h)
                    v += (double)(Mc[(size_t)min(y + m, h - 1) * w] - Mc[(size_t)max(y - m - 1, 0) * w]);
                tile[lane][r] = v;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kVsumRows; j++) {
            const int f = j * kWave + lane, el = f / kVsumRows, r = f % kVsumRows;
            if (e0 + el < ne && y0 + r < h)
                Vp[(size_t)(e0 + el) * h + y0 + r] = tile[el][r];
        }
        __syncthreads();
    }
}

// FarnebackUpdateFlow_Blur, horizontal + solve: one lane per (pair, row) runs along the row; mag != NULL: write
// the flow's magnitude too.  The V words of the next kSolveAhead columns are loaded while the current ones are
// summed: they do not depend on the recurrence, and with one lane per row there are too few waves to hide the
// memory latency otherwise.  (The next iteration's matrices are rebuilt by of_update_matrices_kernel, not here:
// in this loop the gathers from R1, whose addresses depend on the flow just solved, put a memory round trip on
// every step of the sequential chain -- 69 ms of 92 per 32 1080p pairs, DESIGN.md "Optical flow".)
constexpr int kSolveBlock = 64;
constexpr int kSolveAhead = 4;
__global__ void __launch_bounds__(kSolveBlock)
of_solve_kernel(const double *__restrict__ V, float *__restrict__ flow, float *__restrict__ mag, int h, int w, int m,
                double scale)
{
    const int y = blockIdx.x * kSolveBlock + threadIdx.x;
    if (y >= h)
        return;
    const size_t p = blockIdx.y, plane = (size_t)h * w;
    const double *Vp = V + p * 5 * plane + y;
    const size_t cs = (size_t)w * h;            // channel stride of V
    auto at = [&](int c, int x) { return Vp[c * cs + (size_t)clampi(x, 0, w - 1) * h]; };
    double G[5];
#pragma unroll
    for (int c = 0; c < 5; c++) {
        G[c] = at(c, 0) * (double)(m + 2);
        for (int x = 1; x < m; x++)
            G[c] += at(c, x);
    }
    float *frow = flow + (p * plane + (size_t)y * w) * 2;
    float *mrow = mag ? mag + p * plane + (size_t)y * w : nullptr;
    double add[kSolveAhead][5], sub[kSolveAhead][5];
#pragma unroll
    for (int d = 0; d < kSolveAhead; d++)
#pragma unroll
        for (int c = 0; c < 5; c++)
            add[d][c] = at(c, d + m), sub[d][c] = at(c, d - m - 1);
    for (int x0 = 0; x0 < w; x0 += kSolveAhead) {
        double nadd[kSolveAhead][5], nsub[kSolveAhead][5];
#pragma unroll
        for (int d = 0; d < kSolveAhead; d++)
#pragma unroll
            for (int c = 0; c < 5; c++)
                nadd[d][c] = at(c, x0 + kSolveAhead + d + m), nsub[d][c] = at(c, x0 + kSolveAhead + d - m - 1);
#pragma unroll
        for (int d = 0; d < kSolveAhead; d++) {
            const int x = x0 + d;
            if (x >= w)
                break;
#pragma unroll
            for (int c = 0; c < 5; c++)
                G[c] += add[d][c] - sub[d][c];
            const double g11 = G[0] * scale, g12 = G[1] * scale, g22 = G[2] * scale, h1 = G[3] * scale,
                         h2 = G[4] * scale;
            const double idet = 1. / (g11 * g22 - g12 * g12 + 1e-3);
            const float fx = (float)((g11 * h2 - g12 * h1) * idet), fy = (float)((g22 * h1 - g12 * h2) * idet);
            frow[2 * x] = fx;
            frow[2 * x + 1] = fy;
            // (sqrtf: correctly rounded under HIP's default -fhip-fp32-correctly-rounded-divide-sqrt; this
            //  toolchain's __fsqrt_rn is the native approximation unless OCML_BASIC_ROUNDED_OPERATIONS is set)
            if (mrow)
                mrow[x] = sqrtf(fx * fx + fy * fy);
        }
#pragma unroll
        for (int d = 0; d < kSolveAhead; d++)
#pragma unroll
            for (int c = 0; c < 5; c++)
                add[d][c] = nadd[d][c], sub[d][c] = nsub[d][c];
    }
}

int cv_round(double v) { return (int)lrint(v); }   // round half to even, like cvRound

struct OfLevel {
    int k, ksize, h, w;
    double scale, sigma;
};

// the levels from the coarsest down to 0 (calcOpticalFlowFarneback's loop and its 32-pixel rule)
std::vector<OfLevel> of_levels(int h, int w, double pyr_scale, int levels)
{
    double scale = 1;
    int k = 0;
    for (; k < levels; k++) {
        scale *= pyr_scale;
        if (w * scale < kMinSize || h * scale < kMinSize)
            break;
    }
    std::vector<OfLevel> out;
    for (; k >= 0; k--) {
        OfLevel l;
        l.k = k;
        l.scale = 1;
        for (int i = 0; i < k; i++)
            l.scale *= pyr_scale;
        l.sigma = (1. / l.scale - 1) * 0.5;
        l.ksize = cv_round(l.sigma * 5) | 1;
        l.ksize = l.ksize > 3 ? l.ksize : 3;
        l.w = cv_round(w * l.scale);
        l.h = cv_round(h * l.scale);
        out.push_back(l);
    }
    return out;
}

struct OfLayout {
    size_t rows, blur, img, R, flow_prev, flow, M, V, tables, total;
    std::vector<size_t> tab_img, tab_flow;     // per level: offsets of its resize tables (SIZE_MAX: none)
};

OfLayout of_layout(int n, int h, int w, const std::vector<OfLevel> &lv)
{
    OfLayout L;
    const size_t px = (size_t)h * w, P = (size_t)n - 1;
    size_t img_px = 0;
    for (const OfLevel &l : lv)
        if (l.h != h || l.w != w)
            img_px = img_px > (size_t)l.h * l.w ? img_px : (size_t)l.h * l.w;
    Carve c;
    L.rows = c.take((size_t)n * px * 4);
    L.blur = c.take((size_t)n * px * 4);
    L.img = c.take((size_t)n * img_px * 4);
    L.R = c.take((size_t)n * 5 * px * 4);
    L.flow_prev = c.take(P * px * 8);
    L.flow = c.take(P * px * 8);
    L.M = c.take(P * 5 * px * 4);
    L.V = c.take(P * 5 * px * 8);
    L.tables = c.total;
    for (size_t i = 0; i < lv.size(); i++) {
        const OfLevel &l = lv[i];
        L.tab_img.push_back(l.h != h || l.w != w ? c.take(resize_scratch_bytes(h, w, l.h, l.w)) : SIZE_MAX);
        const bool grow = i > 0 && (lv[i - 1].h != l.h || lv[i - 1].w != l.w);
        L.tab_flow.push_back(grow ? c.take(resize_scratch_bytes(lv[i - 1].h, lv[i - 1].w, l.h, l.w)) : SIZE_MAX);
    }
    L.total = c.total + 256;
    return L;
}

// g, xg, xxg: 2 poly_n + 1 floats (offsets -poly_n..poly_n), ig: ig11, ig03, ig33, ig55
int farneback_poly_consts(int n, double sigma, float *g, float *xg, float *xxg, double ig[4])
{
    VA_REQUIRE(n == 5 || n == 7, "optical flow: poly_n must be 5 or 7 (got %d)", n);
    VA_REQUIRE(sigma == sigma, "optical flow: poly_sigma is NaN");
    if (sigma < 1.1920928955078125e-07)         // FLT_EPSILON
        sigma = n * 0.3;
    double s = 0.;
    float gg[2 * kMaxPolyN + 1], *gc = gg + n;
    for (int x = -n; x <= n; x++) {
        gc[x] = (float)exp(-x * x / (2 * sigma * sigma));
        s += gc[x];
    }
    s = 1. / s;
    for (int x = -n; x <= n; x++) {
        gc[x] = (float)(gc[x] * s);
        g[x + n] = gc[x];
        xg[x + n] = (float)(x * gc[x]);
        xxg[x + n] = (float)(x * x * gc[x]);
    }
    double G[6][6] = {};
    for (int y = -n; y <= n; y++)
        for (int x = -n; x <= n; x++) {
            G[0][0] += gc[y] * gc[x];
            G[1][1] += gc[y] * gc[x] * x * x;
            G[3][3] += gc[y] * gc[x] * x * x * x * x;
            G[5][5] += gc[y] * gc[x] * x * x * y * y;
        }
    G[2][2] = G[0][3] = G[0][4] = G[3][0] = G[4][0] = G[1][1];
    G[4][4] = G[3][3];
    G[3][4] = G[4][3] = G[5][5];
    // Mat::inv(DECOMP_CHOLESKY): CholImpl, L with reciprocal square roots on its diagonal, against the identity
    double L[6][6], b[6][6];
    memcpy(L, G, sizeof(L));
    for (int i = 0; i < 6; i++) {
        int j;
        for (j = 0; j < i; j++) {
            double t = G[i][j];
            for (int k = 0; k < j; k++)
                t -= L[i][k] * L[j][k];
            L[i][j] = t * L[j][j];
        }
        double t = G[i][i];
        for (int k = 0; k < j; k++)
            t -= L[i][k] * L[i][k];
        if (t < 2.220446049250313e-16) {
            set_error("optical flow: the polynomial basis of poly_sigma=%g is singular", sigma);
            return VA_ERR_INVALID;
        }
        L[i][i] = 1. / sqrt(t);
    }
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++)
            b[i][j] = i == j;
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            double t = b[i][j];
            for (int k = 0; k < i; k++)
                t -= L[i][k] * b[k][j];
            b[i][j] = t * L[i][i];
        }
    for (int i = 5; i >= 0; i--)
        for (int j = 0; j < 6; j++) {
            double t = b[i][j];
            for (int k = 5; k > i; k--)
                t -= L[k][i] * b[k][j];
            b[i][j] = t * L[i][i];
        }
    ig[0] = b[1][1];
    ig[1] = b[0][3];
    ig[2] = b[3][3];
    ig[3] = b[5][5];
    return VA_OK;
}

int farneback_check(int n, int h, int w, double pyr_scale, int levels, int winsize, int iterations, int poly_n,
                    int flags)
{
    VA_REQUIRE(n >= 2, "optical flow: needs at least 2 frames (got %d)", n);
    VA_REQUIRE(h > 0 && w > 0, "optical flow: bad frame shape %d x %d", h, w);
    VA_REQUIRE((size_t)h * w < kMaxFramePixels, "optical flow: frames above 2^29 pixels are not supported");
    VA_REQUIRE(h <= 65535, "optical flow: frames of more than 65535 rows are not supported");
    VA_REQUIRE(pyr_scale > 0 && pyr_scale < 1, "optical flow: pyr_scale must lie in (0, 1) (got %g)", pyr_scale);
    VA_REQUIRE(levels >= 0, "optical flow: levels must be >= 0 (got %d)", levels);
    VA_REQUIRE(winsize >= 1, "optical flow: winsize must be >= 1 (got %d)", winsize);
    VA_REQUIRE(iterations >= 1, "optical flow: iterations must be >= 1 (got %d)", iterations);
    VA_REQUIRE(poly_n == 5 || poly_n == 7, "optical flow: poly_n must be 5 or 7 (got %d)", poly_n);
    VA_REQUIRE(flags == 0, "optical flow: flags must be 0 (OPTFLOW_USE_INITIAL_FLOW and "
               "OPTFLOW_FARNEBACK_GAUSSIAN are not supported; got %d)", flags);
    VA_REQUIRE(n <= 65535, "optical flow: more than 65535 frames in one call are not supported");
    return VA_OK;
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

int va_farneback_poly_consts(int poly_n, double poly_sigma, float *g, float *xg, float *xxg, double *ig)
{
    VA_REQUIRE(g && xg && xxg && ig, "va_farneback_poly_consts: NULL argument");
    return farneback_poly_consts(poly_n, poly_sigma, g, xg, xxg, ig);
}

size_t va_farneback_workspace_bytes(int n, int h, int w, double pyr_scale, int levels, int winsize, int iterations,
                                    int poly_n)
{
    if (farneback_check(n, h, w, pyr_scale, levels, winsize, iterations, poly_n, 0))
        return 0;
    return of_layout(n, h, w, of_levels(h, w, pyr_scale, levels)).total;
}

int va_optical_flow_farneback(const void *frames, int dtype, int n, int h, int w, double pyr_scale, int levels,
                              int winsize, int iterations, int poly_n, double poly_sigma, int flags, float *flow_out,
                              float *mag_out, void *ws, size_t ws_bytes, void *stream)
{
    VA_ENTER();
    int rc = farneback_check(n, h, w, pyr_scale, levels, winsize, iterations, poly_n, flags);
    if (rc)
        return rc;
    VA_REQUIRE(dtype == VA_U8 || dtype == VA_F32, "optical flow: frames must be VA_U8 or VA_F32 (got dtype %d)", dtype);
    VA_REQUIRE(frames, "optical flow: NULL frames");
    VA_REQUIRE(flow_out || mag_out, "optical flow: flow_out and mag_out are both NULL");
    hipStream_t st = as_stream(stream);
    const std::vector<OfLevel> lv = of_levels(h, w, pyr_scale, levels);
    const OfLayout L = of_layout(n, h, w, lv);
    if (!ws || ws_bytes < L.total) {
        set_error("optical flow: workspace of %zu bytes < required %zu", ws_bytes, L.total);
        return VA_ERR_RANGE;
    }
    PolyConsts pc;
    {
        float g[2 * kMaxPolyN + 1], xg[2 * kMaxPolyN + 1], xxg[2 * kMaxPolyN + 1];
        double ig[4];
        rc = farneback_poly_consts(poly_n, poly_sigma, g, xg, xxg, ig);
        if (rc)
            return rc;
        for (int k = 0; k <= poly_n; k++) {
            pc.g[k] = g[poly_n + k];
            pc.xg[k] = xg[poly_n + k];
            pc.xxg[k] = xxg[poly_n + k];
        }
        pc.ig11 = ig[0], pc.ig03 = ig[1], pc.ig33 = ig[2], pc.ig55 = ig[3];
    }
    std::vector<TapsF32> taps(lv.size());
    for (size_t i = 0; i < lv.size(); i++) {
        const OfLevel &l = lv[i];
        if (l.ksize > kMaxTaps) {
            set_error("optical flow: level %d needs a %d-tap blur, more than the supported %d", l.k, l.ksize, kMaxTaps);
            return VA_ERR_RANGE;
        }
        taps[i].ksize = l.ksize;
        if (l.sigma <= 0 && l.ksize == 3) {         // getGaussianKernel's fixed table (level 0: sigma = 0, 3 taps)
            taps[i].t[0] = 0.25f, taps[i].t[1] = 0.5f, taps[i].t[2] = 0.25f;
        } else {
            double k64[kMaxTaps + 1];
            gauss_taps_f64(l.sigma, l.ksize, k64);
            for (int j = 0; j < l.ksize; j++)
                taps[i].t[j] = (float)k64[j];
        }
    }
    char *base = (char *)ws;
    float *rows = (float *)(base + L.rows), *blur = (float *)(base + L.blur), *img = (float *)(base + L.img);
    float *R = (float *)(base + L.R), *flow_prev = (float *)(base + L.flow_prev), *flow_ws = (float *)(base + L.flow);
    float *M = (float *)(base + L.M);
    double *V = (double *)(base + L.V);
    const int P = n - 1;
    // Every resize table of the call goes up first, each geometry into its own part of the workspace, after the
    // stream has drained: the blocking copies are not ordered with a non-blocking stream, so neither an earlier
    // call's kernels nor this call's may still read a table region while it is written.
    VA_HIP(hipStreamSynchronize(st));
    for (size_t i = 0; i < lv.size(); i++) {
        const OfLevel &l = lv[i];
        if (L.tab_img[i] != SIZE_MAX &&
            (rc = launch_resize_f32(blur, img, n, h, w, 1, l.h, l.w, 1, base + L.tab_img[i], st, ResizeStage::Upload)))
            return rc;
        if (L.tab_flow[i] != SIZE_MAX &&
            (rc = launch_resize_f32(flow_ws, flow_prev, P, lv[i - 1].h, lv[i - 1].w, 2, l.h, l.w, 1,
                                    base + L.tab_flow[i], st, ResizeStage::Upload)))
            return rc;
    }
    const float fscale = (float)(1. / pyr_scale);
    for (size_t i = 0; i < lv.size(); i++) {
        const OfLevel &l = lv[i];
        const int lh = l.h, lw = l.w;
        const bool last_level = i + 1 == lv.size();
        // pyramid images of all n frames: blur the full-resolution frames, then resize
        const dim3 gfull((unsigned)cdiv(w, kBlock), (unsigned)h, (unsigned)n);
        if (dtype == VA_U8)
            of_blur_rows_kernel<uint8_t><<<gfull, kBlock, 0, st>>>((const uint8_t *)frames, rows, h, w, taps[i]);
        else
            of_blur_rows_kernel<float><<<gfull, kBlock, 0, st>>>((const float *)frames, rows, h, w, taps[i]);
        VA_LAUNCH_CHECK("of_blur_rows_kernel");
        of_blur_cols_kernel<<<gfull, kBlock, 0, st>>>(rows, blur, h, w, taps[i]);
        VA_LAUNCH_CHECK("of_blur_cols_kernel");
        const float *level_img = blur;
        if (L.tab_img[i] != SIZE_MAX) {
            if ((rc = launch_resize_f32(blur, img, n, h, w, 1, lh, lw, 1, base + L.tab_img[i], st, ResizeStage::Launch)))
                return rc;
            level_img = img;
        }
        const dim3 glev((unsigned)cdiv(lw, kBlock), (unsigned)lh, (unsigned)n);
        of_poly_exp_kernel<<<glev, kBlock, 0, st>>>(level_img, R, lh, lw, poly_n, pc);
        VA_LAUNCH_CHECK("of_poly_exp_kernel");
        // the flow this level writes (the next level resizes it from flow_ws), and the flow it starts from: zero,
        // or the previous level's, resized (scaled in of_update_matrices_kernel)
        float *flow = last_level && flow_out ? flow_out : flow_ws;
        const float *start = nullptr;
        if (i > 0) {
            if (L.tab_flow[i] != SIZE_MAX) {
                if ((rc = launch_resize_f32(flow_ws, flow_prev, P, lv[i - 1].h, lv[i - 1].w, 2, lh, lw, 1,
                                            base + L.tab_flow[i], st, ResizeStage::Launch)))
                    return rc;
                start = flow_prev;
            } else {
                start = flow_ws;
            }
        }
        const dim3 gpair((unsigned)cdiv(lw, kBlock), (unsigned)lh, (unsigned)P);
        of_update_matrices_kernel<<<gpair, kBlock, 0, st>>>(R, start, fscale, M, lh, lw);
        VA_LAUNCH_CHECK("of_update_matrices_kernel");
        const int m = winsize / 2;
        const double scale = 1. / (winsize * winsize);
        for (int it = 0; it < iterations; it++) {
            const bool last_it = it + 1 == iterations;
            of_vsum_kernel<<<dim3((unsigned)cdiv(5ll * lw, kWave), (unsigned)P), kWave, 0, st>>>(M, V, lh, lw, m);
            VA_LAUNCH_CHECK("of_vsum_kernel");
            of_solve_kernel<<<dim3((unsigned)cdiv(lh, kSolveBlock), (unsigned)P), kSolveBlock, 0, st>>>(
                V, flow, last_it && last_level ? mag_out : nullptr, lh, lw, m, scale);
            VA_LAUNCH_CHECK("of_solve_kernel");
            if (!last_it) {                             // the matrices of the next iteration, from the new flow
                of_update_matrices_kernel<<<gpair, kBlock, 0, st>>>(R, flow, 1.f, M, lh, lw);
                VA_LAUNCH_CHECK("of_update_matrices_kernel");
            }
        }
    }
    return VA_OK;
}

}  // extern "C"
