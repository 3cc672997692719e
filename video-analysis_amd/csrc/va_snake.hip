// va_snake.hip -- the dense and the iterative half of ActiveContour (video/analysis/active_contour.py)
//
// sobel5 : cv2.Sobel(p, CV_64F, 1, 0, ksize=5) and cv2.Sobel(p, CV_64F, 0, 1, ksize=5) in one pass
//          (set_potential, :109-110).  A 128 x 32 output tile stages its (32 + 4) x (128 + 4) source
//          pixels in LDS as float (exact for uint8 and float32).  A lane owns two adjacent columns of its
//          wave's eight rows: it runs both row filters on each staged row and keeps the last five in a
//          register window, from which both column filters give a row of output, written as one 16-byte
//          store per plane.  Arithmetic as
//          OpenCV's FilterEngine with a CV_64F kernel ("Active contours"):
//            row    s = k0*S[x-2]; s += k_i*S[x-2+i], i = 1..4 (the zero tap included)
//            column symmetric      s = 6*S[y] + 0.0; s += 4*(S[y+1] + S[y-1]); s += S[y+2] + S[y-2]
//                   antisymmetric  s = 0.0; s += 2*(S[y+1] - S[y-1]); s += S[y+2] - S[y-2]
//          fx = column-smooth(row-derivative), fy = column-derivative(row-smooth); BORDER_REFLECT_101.
// snake  : every iteration of every contour of a call in one launch (find_contour, :113-196); one
//          workgroup owns one contour, on its frame of an (n, h, w) stack or on its item of a ragged buffer
//          (va_active_contour_ragged: base, row stride and clip bounds are the item's).  Per iteration: bilinear gather of fx, fy (image.subpixels),
//          rhs = p + gamma*f, ps = Pinv @ rhs with acc = P[i,0]*rhs[0], acc += P[i,j]*rhs[j] in
//          ascending j, anchors, residual, clip, and a workgroup-uniform stop.  The matrices arrive
//          transposed (element (j, i) = Pinv[i, j]) so that the lanes of a wave read consecutive
//          words; up to kSnakeLdsMaxN points they are staged in LDS once per contour, above that they are
//          read from global memory (L2) in every iteration.  Residual and total variation sum the
//          2N terms |d| (x of every point, then y of every point) in a fixed order: thread t adds the
//          terms t, t + 256, ... in that order starting from 0.0, then the 256 partials are folded
//          in halves (s[t] += s[t + 128], s[t] += s[t + 64], ..., s[0] += s[1]).
#include "va_common.h"

namespace va {

namespace {

// ------------------------------------------------------------------------------------------- Sobel
constexpr int kSobTW = 128, kSobTH = 32;          // output tile
constexpr int kSobBlock = 256;                    // 64 lanes x 4 waves; a lane: 2 columns of its wave's rows
constexpr int kSobRows = kSobTH / 4;              // output rows per wave
constexpr int kSobSW = kSobTW + 4, kSobSH = kSobTH + 4;

template <typename T>
__global__ void __launch_bounds__(kSobBlock)
sobel5_f64_kernel(const T *__restrict__ src, double *__restrict__ fx, double *__restrict__ fy, int h, int w,
                  int vec2)
{
    __shared__ float s_src[kSobSH][kSobSW];
    const int x0 = blockIdx.x * kSobTW, y0 = blockIdx.y * kSobTH;
    const size_t fbase = (size_t)blockIdx.z * h * w;
    const T *frame = src + fbase;
    const int tid = threadIdx.x;

    for (int i = tid; i < kSobSH * kSobSW; i += kSobBlock) {
        const int r = i / kSobSW, c = i - r * kSobSW;
        const int y = reflect101(y0 + r - 2, h), x = reflect101(x0 + c - 2, w);
        s_src[r][c] = (float)frame[(size_t)y * w + x];
    }
    __syncthreads();

    const int lane = tid & 63, wave = tid >> 6;
    const int c = 2 * lane, x = x0 + c;
    if (x >= w)
        return;
    const int r0 = wave * kSobRows;                // first output row of this wave (staged row r0 + 2)
    // the row filters of the last five staged rows, two columns each: a window that rolls down the tile
    double wd[5][2], ws[5][2];
#pragma unroll
    for (int k = 0; k < kSobRows + 4; k++) {
        const float *S = &s_src[r0 + k][c];
        const double v0 = S[0], v1 = S[1], v2 = S[2], v3 = S[3], v4 = S[4], v5 = S[5];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            wd[q][0] = wd[q + 1][0], wd[q][1] = wd[q + 1][1];
            ws[q][0] = ws[q + 1][0], ws[q][1] = ws[q + 1][1];
        }
        const double a[2] = {v0, v1}, b[2] = {v1, v2}, m[2] = {v2, v3}, d[2] = {v3, v4}, e[2] = {v4, v5};
#pragma unroll
        for (int q = 0; q < 2; q++) {
            double sd = -1.0 * a[q];
            sd += -2.0 * b[q];
            sd += 0.0 * m[q];
            sd += 2.0 * d[q];
            sd += 1.0 * e[q];
            double ss = 1.0 * a[q];
            ss += 4.0 * b[q];
            ss += 6.0 * m[q];
            ss += 4.0 * d[q];
            ss += 1.0 * e[q];
            wd[4][q] = sd;
            ws[4][q] = ss;
        }
        if (k < 4)
            continue;
        const int y = y0 + r0 + k - 4;             // window rows y-2 .. y+2 = wd[0] .. wd[4]
        if (y >= h)
            break;
        double gx[2], gy[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {
            double sx = 6.0 * wd[2][q] + 0.0;
            sx += 4.0 * (wd[3][q] + wd[1][q]);
            sx += 1.0 * (wd[4][q] + wd[0][q]);
            double sy = 0.0;
            sy += 2.0 * (ws[3][q] - ws[1][q]);
            sy += 1.0 * (ws[4][q] - ws[0][q]);
            gx[q] = sx;
            gy[q] = sy;
        }
        const size_t o = fbase + (size_t)y * w + x;
        if (vec2 && x + 1 < w) {          // w even and the planes 16-byte aligned: one store per pair
            if (fx)
                *reinterpret_cast<double2 *>(fx + o) = make_double2(gx[0], gx[1]);
            if (fy)
                *reinterpret_cast<double2 *>(fy + o) = make_double2(gy[0], gy[1]);
        } else {
            if (fx)
                fx[o] = gx[0];
            if (fy)
                fy[o] = gy[0];
            if (x + 1 < w) {
                if (fx)
                    fx[o + 1] = gx[1];
                if (fy)
                    fy[o + 1] = gy[1];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------- snake
constexpr int kSnakeBlock = 256;
// contours of up to kSnakeLdsMaxN points keep their matrix in LDS, longer ones read it from global memory;
// kSnakeMaxN is the longest contour a call takes
constexpr int kSnakeLdsMaxN = 128;
constexpr int kSnakeMaxN = 1024;

struct SnakeArgs {
    const double *fx, *fy;
    // ragged planes (va_active_contour_ragged): item f is (shapes[2f], shapes[2f + 1]) at element offset offsets[f]
    // of `total`; both null for an (n, h, w) stack
    const int32_t *shapes;
    const int64_t *offsets;
    int64_t total;
    int n, h, w, m, max_points;
    const int32_t *npts, *frame;
    const double *mats;
    const int64_t *mat_off;
    int64_t mats_count;
    const uint8_t *anchor_flags;   // (m, max_points): bit 0 = x fixed, bit 1 = y fixed (nullable)
    const double *anchor_vals;     // (m, max_points, 2)
    double gamma, tol_gamma;
    int max_iterations;
    double *pts;                   // (m, max_points, 2) in: the equidistant curve, out: the contour
    int32_t *iterations;
    double *total_variation;
};

__device__ __forceinline__ double clip(double v, double lo, double hi)
{
    return v < lo ? lo : (v > hi ? hi : v);   // np.clip: NaN passes through
}

// image.subpixels: ((tl + tr) + bl) + br, products rounded one by one
__device__ __forceinline__ double subpixel(const double *img, int w, int xi, int yi, double dx, double dy)
{
    const double *p = img + (size_t)yi * w + xi;
    const double wtl = (1.0 - dx) * (1.0 - dy), wtr = dx * (1.0 - dy), wbl = (1.0 - dx) * dy, wbr = dx * dy;
    return ((wtl * p[0] + wtr * p[1]) + wbl * p[w]) + wbr * p[w + 1];
}

// the fixed-order sum of the per-thread partials (see the file comment); every thread gets the total
__device__ __forceinline__ double block_sum(double part, double *s_red)
{
    const int tid = threadIdx.x;
    s_red[tid] = part;
    __syncthreads();
#pragma unroll
    for (int s = kSnakeBlock / 2; s > 0; s >>= 1) {
        if (tid < s)
            s_red[tid] += s_red[tid + s];
        __syncthreads();
    }
    return s_red[0];
}

// NMAX: largest N of the instantiation; LDS: Pinv staged in LDS (else read from global memory)
template <int NMAX, bool LDS>
__global__ void __launch_bounds__(kSnakeBlock)
snake_kernel(SnakeArgs a)
{
    constexpr int TPT = (2 * NMAX + kSnakeBlock - 1) / kSnakeBlock;   // matvec rows (x and y) per thread
    __shared__ double s_p[2][NMAX];        // current (clipped) points, x then y
    __shared__ double s_r[2][NMAX];        // rhs = p + gamma*f
    __shared__ double s_red[kSnakeBlock];
    __shared__ double s_P[LDS ? NMAX * NMAX : 1];
    const int tid = threadIdx.x, c = blockIdx.x;
    const int N = a.npts[c], f = a.frame[c];
    const int64_t off = a.mat_off[c];
    // the contour's plane, once per workgroup: (base, h, w) of its frame of the stack or of its ragged item
    int h = a.h, w = a.w;
    int64_t base = 0;
    bool plane_ok = f >= 0 && f < a.n;
    if (plane_ok) {
        if (a.shapes) {
            h = a.shapes[2 * f];
            w = a.shapes[2 * f + 1];
            base = a.offsets[f];
            plane_ok = h >= 2 && w >= 2 && base >= 0 && base <= a.total - (int64_t)h * w;
        } else {
            base = (int64_t)f * h * w;
        }
    }
    if (N <= 2 || N > a.max_points || N > NMAX || !plane_ok || off < 0 ||
        off > a.mats_count - (int64_t)N * N) {
        if (tid == 0) {                    // nothing to iterate (N <= 2) or an entry the host should not send
            a.iterations[c] = N <= 2 && N >= 0 && N <= a.max_points ? 0 : -1;
            a.total_variation[c] = 0.0;
        }
        return;
    }
    const double xmax = w - 2, ymax = h - 2;
    const double *gx = a.fx + base, *gy = a.fy + base;
    const double *PT = a.mats + off;
    double *pts = a.pts + (size_t)c * a.max_points * 2;
    const uint8_t *af = a.anchor_flags ? a.anchor_flags + (size_t)c * a.max_points : nullptr;
    const double *av = a.anchor_vals + (size_t)c * a.max_points * 2;

    for (int i = tid; i < N; i += kSnakeBlock) {
        s_p[0][i] = clip(pts[2 * i], 0.0, xmax);
        s_p[1][i] = clip(pts[2 * i + 1], 0.0, ymax);
    }
    if (LDS)
        for (int i = tid; i < N * N; i += kSnakeBlock)
            s_P[i] = PT[i];
    const double *P = LDS ? s_P : PT;
    // anchors of this thread's rows, once: bit k = row tid + k*256 is fixed
    uint32_t fixed = 0;
    if (af) {
#pragma unroll
        for (int k = 0; k < TPT; k++) {
            const int t = tid + k * kSnakeBlock;
            if (t < 2 * N) {
                const int d = t >= N, i = t - d * N;
                fixed |= (uint32_t)((af[i] >> d) & 1) << k;
            }
        }
    }
    __syncthreads();

    int it = 0;
    while (it < a.max_iterations) {
        it++;
        // external force at the current points and the right-hand side
        for (int i = tid; i < N; i += kSnakeBlock) {
            const double x = s_p[0][i], y = s_p[1][i];
            // trunc, as astype(int); the clamp only guards the reads (x, y are within the clip range)
            const int xi = (int)fmin(fmax(x, 0.0), xmax), yi = (int)fmin(fmax(y, 0.0), ymax);
            const double dx = x - xi, dy = y - yi;
            const double fex = subpixel(gx, w, xi, yi, dx, dy), fey = subpixel(gy, w, xi, yi, dx, dy);
            s_r[0][i] = x + a.gamma * fex;
            s_r[1][i] = y + a.gamma * fey;
        }
        __syncthreads();
        // ps = Pinv @ rhs for both coordinates, anchors, |ps - p|
        double q[TPT];
        double part = 0.0;
#pragma unroll
        for (int k = 0; k < TPT; k++) {
            const int t = tid + k * kSnakeBlock;
            q[k] = 0.0;
            if (t < 2 * N) {
                const int d = t >= N, i = t - d * N;
                const double *r = s_r[d];
                const double *col = P + i;
                double acc = col[0] * r[0];
#pragma unroll 8
                for (int j = 1; j < N; j++)
                    acc += col[(size_t)j * N] * r[j];
                if ((fixed >> k) & 1)
                    acc = av[2 * i + d];
                q[k] = acc;
                part += fabs(acc - s_p[d][i]);
            }
        }
        const double residual = block_sum(part, s_red);   // its barriers also end every read of s_p
#pragma unroll
        for (int k = 0; k < TPT; k++) {
            const int t = tid + k * kSnakeBlock;
            if (t < 2 * N) {
                const int d = t >= N, i = t - d * N;
                s_p[d][i] = clip(q[k], 0.0, d ? ymax : xmax);
            }
        }
        __syncthreads();
        if (residual < a.tol_gamma)
            break;
    }

    // total variation against the clipped start, same order; the contour goes back in place
    double part = 0.0;
#pragma unroll
    for (int k = 0; k < TPT; k++) {
        const int t = tid + k * kSnakeBlock;
        if (t < 2 * N) {
            const int d = t >= N, i = t - d * N;
            part += fabs(clip(pts[2 * i + d], 0.0, d ? ymax : xmax) - s_p[d][i]);
        }
    }
    const double tv = block_sum(part, s_red);
    for (int i = tid; i < N; i += kSnakeBlock) {
        pts[2 * i] = s_p[0][i];
        pts[2 * i + 1] = s_p[1][i];
    }
    if (tid == 0) {
        a.iterations[c] = it;
        a.total_variation[c] = tv;
    }
}

// shapes, offsets, total: the planes are the items of a ragged buffer (n of them; h, w unused), null for a stack
int launch_active_contour(const double *fx, const double *fy, const int32_t *shapes, const int64_t *offsets,
                          int64_t total, int n, int h, int w, int m, int max_points, const int32_t *npts,
                          const int32_t *frame, const double *mats, const int64_t *mat_off, int64_t mats_count,
                          const uint8_t *anchor_flags, const double *anchor_vals, double gamma, double tol_gamma,
                          int max_iterations, double *pts, int32_t *iterations, double *total_variation,
                          hipStream_t st)
{
    if (m == 0)
        return VA_OK;
    SnakeArgs a{fx, fy, shapes, offsets, total, n, h, w, m, max_points, npts, frame, mats, mat_off, mats_count,
                anchor_flags, anchor_vals, gamma, tol_gamma, max_iterations, pts, iterations, total_variation};
    // the widest contour of the call picks the instantiation; all of them compute the same numbers
    if (max_points <= 64)
        hipLaunchKernelGGL((snake_kernel<64, true>), dim3(m), dim3(kSnakeBlock), 0, st, a);
    else if (max_points <= kSnakeLdsMaxN)
        hipLaunchKernelGGL((snake_kernel<kSnakeLdsMaxN, true>), dim3(m), dim3(kSnakeBlock), 0, st, a);
    else
        hipLaunchKernelGGL((snake_kernel<kSnakeMaxN, false>), dim3(m), dim3(kSnakeBlock), 0, st, a);
    VA_LAUNCH_CHECK("snake_kernel");
    return VA_OK;
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

int va_sobel5_f64(const void *src, int dtype, double *fx_out, double *fy_out, int n, int h, int w, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(dtype == VA_U8 || dtype == VA_F32, "va_sobel5_f64: frames must be VA_U8 or VA_F32 (got dtype %d)",
               dtype);
    VA_REQUIRE(src && (fx_out || fy_out), "va_sobel5_f64: NULL frames, or fx_out and fy_out both NULL");
    VA_REQUIRE(n >= 0 && h > 0 && w > 0 && (size_t)h * w < kMaxFramePixels, "va_sobel5_f64: bad shape (%d, %d, %d)",
               n, h, w);
    if (n == 0)
        return VA_OK;
    hipStream_t st = as_stream(stream);
    const int vec2 = (w % 2 == 0) && ((uintptr_t)fx_out % 16 == 0) && ((uintptr_t)fy_out % 16 == 0);
    for (int f0 = 0; f0 < n; f0 += 65535) {
        const int k = n - f0 < 65535 ? n - f0 : 65535;
        const size_t o = (size_t)f0 * h * w;
        dim3 grid(cdiv(w, kSobTW), cdiv(h, kSobTH), k);
        double *ox = fx_out ? fx_out + o : nullptr, *oy = fy_out ? fy_out + o : nullptr;
        if (dtype == VA_U8)
            hipLaunchKernelGGL(sobel5_f64_kernel<uint8_t>, grid, dim3(kSobBlock), 0, st,
                               static_cast<const uint8_t *>(src) + o, ox, oy, h, w, vec2);
        else
            hipLaunchKernelGGL(sobel5_f64_kernel<float>, grid, dim3(kSobBlock), 0, st,
                               static_cast<const float *>(src) + o, ox, oy, h, w, vec2);
        VA_LAUNCH_CHECK("sobel5_f64_kernel");
    }
    return VA_OK;
}

int va_active_contour(const double *fx, const double *fy, int n, int h, int w, int m, int max_points,
                      const int32_t *npts, const int32_t *frame, const double *mats, const int64_t *mat_offset,
                      int64_t mats_count, const uint8_t *anchor_flags, const double *anchor_vals, double gamma,
                      double tol_gamma, int max_iterations, double *pts_inout, int32_t *iterations_out,
                      double *total_variation_out, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(n > 0 && h >= 2 && w >= 2 && (size_t)h * w < kMaxFramePixels,
               "va_active_contour: bad gradient shape (%d, %d, %d): frames need h, w >= 2", n, h, w);
    VA_REQUIRE(m >= 0 && max_points >= 1 && max_points <= kSnakeMaxN,
               "va_active_contour: bad contour table (%d contours of up to %d points; at most %d points)", m,
               max_points, kSnakeMaxN);
    VA_REQUIRE(max_iterations >= 1, "va_active_contour: max_iterations must be >= 1 (got %d)", max_iterations);
    VA_REQUIRE(mats_count >= 0, "va_active_contour: negative matrix table size");
    if (m == 0)
        return VA_OK;
    VA_REQUIRE(fx && fy && npts && frame && mats && mat_offset && pts_inout && iterations_out && total_variation_out,
               "va_active_contour: NULL argument");
    VA_REQUIRE(!anchor_flags || anchor_vals, "va_active_contour: anchor flags without anchor values");
    return launch_active_contour(fx, fy, nullptr, nullptr, 0, n, h, w, m, max_points, npts, frame, mats, mat_offset,
                                 mats_count, anchor_flags, anchor_vals, gamma, tol_gamma, max_iterations, pts_inout,
                                 iterations_out, total_variation_out, as_stream(stream));
}

int va_active_contour_ragged(const double *fx, const double *fy, const int32_t *shapes, const int64_t *offsets,
                             int64_t total, int n_items, int m, int max_points, const int32_t *npts,
                             const int32_t *item, const double *mats, const int64_t *mat_offset, int64_t mats_count,
                             const uint8_t *anchor_flags, const double *anchor_vals, double gamma, double tol_gamma,
                             int max_iterations, double *pts_inout, int32_t *iterations_out,
                             double *total_variation_out, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(n_items >= 0 && total >= 0, "va_active_contour_ragged: negative count (n_items %d, total %lld)",
               n_items, (long long)total);
    VA_REQUIRE(m >= 0 && max_points >= 1 && max_points <= kSnakeMaxN,
               "va_active_contour_ragged: bad contour table (%d contours of up to %d points; at most %d points)", m,
               max_points, kSnakeMaxN);
    VA_REQUIRE(max_iterations >= 1, "va_active_contour_ragged: max_iterations must be >= 1 (got %d)", max_iterations);
    VA_REQUIRE(mats_count >= 0, "va_active_contour_ragged: negative matrix table size");
    if (m == 0)
        return VA_OK;
    VA_REQUIRE(fx && fy && shapes && offsets && npts && item && mats && mat_offset && pts_inout && iterations_out &&
                   total_variation_out,
               "va_active_contour_ragged: NULL argument");
    VA_REQUIRE(!anchor_flags || anchor_vals, "va_active_contour_ragged: anchor flags without anchor values");
    return launch_active_contour(fx, fy, shapes, offsets, total, n_items, 0, 0, m, max_points, npts, item, mats,
                                 mat_offset, mats_count, anchor_flags, anchor_vals, gamma, tol_gamma, max_iterations,
                                 pts_inout, iterations_out, total_variation_out, as_stream(stream));
}

}  // extern "C"
