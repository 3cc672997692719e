// va_gradients.hip -- ActiveContour.set_potential's dense part for the items of a ragged buffer: the float32
// Gaussian blur and both 5-tap float64 Sobel planes, each item an image with its own borders
// (Polygon.get_centerline_optimized, video/analysis/shapes.py:735-743, for many polygons at once).
//
// One 256-thread workgroup owns one item and keeps it in LDS: plane A holds the source as float (exact for
// uint8 and float32) and later the blurred image, plane B the row pass -- 8 bytes of dynamic LDS per pixel,
// sized by the largest item of the launch.  With the whole item resident there is no halo: reflect101 indexes
// the plane, and an item narrower than the radius reflects more than once.
//   row pass     B[y][x] = acc, acc = 0, acc = fmaf(A[y][reflect(x - r + i)], t[i], acc) for ascending i
//   column pass  A[y][x] = acc, acc = fmaf(B[y][x], t[r], 0),
//                acc = fmaf(B[reflect(y + k)][x] + B[reflect(y - k)][x], t[r + k], acc) for k = 1..r
//   Sobel        of A at the in-image coordinates reflect(y - 2 .. y + 2), reflect(x - 2 .. x + 2), in the
//                order of sobel5_f64_kernel (va_snake.hip); -0.0 and +0.0 as they come out
// The Sobel reflects the BLURRED image: it reads A[reflect(y)][reflect(x)].  Blurring a reflect-extended source
// at the out-of-image coordinate gives the same terms to the row pass in reversed tap order, which rounds
// differently.
// A thread takes pixels in the item's linear order, so loads from LDS and stores to HBM are consecutive per
// lane.  Results leave as 16-byte pairs whenever the planes' bases are 16-byte aligned: the pairs start at the
// first even element offset of the item (offsets are odd after an item with an odd pixel count), and a pair may
// span two rows.
#include "va_common.h"

namespace va {

namespace {

constexpr int kGradBlock = 256;
constexpr int kGradResidentMaxPixels = VA_GRAD_RESIDENT_MAX_PIXELS;

// both Sobel values of pixel (y, x) of the h x w plane A
__device__ __forceinline__ void sobel_at(const float *A, int h, int w, int y, int x, double *gx, double *gy)
{
    int xs[5], ys[5];
    if (x >= 2 && x + 2 < w) {
#pragma unroll
        for (int i = 0; i < 5; i++)
            xs[i] = x - 2 + i;
    } else {
#pragma unroll
        for (int i = 0; i < 5; i++)
            xs[i] = reflect101(x - 2 + i, w);
    }
    if (y >= 2 && y + 2 < h) {
#pragma unroll
        for (int j = 0; j < 5; j++)
            ys[j] = (y - 2 + j) * w;
    } else {
#pragma unroll
        for (int j = 0; j < 5; j++)
            ys[j] = reflect101(y - 2 + j, h) * w;
    }
    double wd[5], ws[5];
#pragma unroll
    for (int j = 0; j < 5; j++) {
        const float *S = A + ys[j];
        const double a = S[xs[0]], b = S[xs[1]], m = S[xs[2]], d = S[xs[3]], e = S[xs[4]];
        double sd = -1.0 * a;
        sd += -2.0 * b;
        sd += 0.0 * m;
        sd += 2.0 * d;
        sd += 1.0 * e;
        double ss = 1.0 * a;
        ss += 4.0 * b;
        ss += 6.0 * m;
        ss += 4.0 * d;
        ss += 1.0 * e;
        wd[j] = sd;
        ws[j] = ss;
    }
    double sx = 6.0 * wd[2] + 0.0;
    sx += 4.0 * (wd[3] + wd[1]);
    sx += 1.0 * (wd[4] + wd[0]);
    double sy = 0.0;
    sy += 2.0 * (ws[3] - ws[1]);
    sy += 1.0 * (ws[4] - ws[0]);
    *gx = sx;
    *gy = sy;
}

template <typename T>
__global__ void __launch_bounds__(kGradBlock)
grad_ragged_kernel(const T *__restrict__ src, const int32_t *__restrict__ shapes, const int64_t *__restrict__ offsets,
                   int64_t total, int max_pixels, const TapsF32 taps, double *__restrict__ fx,
                   double *__restrict__ fy, int vec2, int32_t *__restrict__ status)
{
    extern __shared__ float s_grad[];                // plane A, then plane B: 2 * max_pixels floats
    const int p = blockIdx.x, tid = threadIdx.x;
    const int h = shapes[2 * p], w = shapes[2 * p + 1];
    const int64_t o = offsets[p];
    const int64_t px64 = (int64_t)h * w;
    if (!(h >= 0 && w >= 0 && px64 <= max_pixels && px64 <= VA_GRAD_RESIDENT_MAX_PIXELS && o >= 0 &&
          o + px64 <= total)) {                      // workgroup-uniform: nothing of the item is read or written
        if (tid == 0)
            status[p] = VA_ERR_RANGE;
        return;
    }
    if (tid == 0)
        status[p] = VA_OK;
    const int px = (int)px64;
    if (px == 0)
        return;
    float *A = s_grad, *B = s_grad + max_pixels;
    const T *item = src + o;
    for (int i = tid; i < px; i += kGradBlock)
        A[i] = (float)item[i];
    __syncthreads();

    const int ks = taps.ksize, r = ks / 2;
    if (ks > 0) {
        for (int i = tid; i < px; i += kGradBlock) {
            const int y = i / w, x = i - y * w;
            const float *S = A + y * w;
            float acc = 0.0f;
            if (x - r >= 0 && x + r < w) {
                const float *Sx = S + (x - r);
                for (int k = 0; k < ks; k++)
                    acc = fmaf(Sx[k], taps.t[k], acc);
            } else {
                for (int k = 0; k < ks; k++)
                    acc = fmaf(S[reflect101(x - r + k, w)], taps.t[k], acc);
            }
            B[i] = acc;
        }
        __syncthreads();
        for (int i = tid; i < px; i += kGradBlock) {
            const int y = i / w;
            float acc = fmaf(B[i], taps.t[r], 0.0f);
            if (y - r >= 0 && y + r < h) {
                for (int k = 1; k <= r; k++)
                    acc = fmaf(B[i + k * w] + B[i - k * w], taps.t[r + k], acc);
            } else {
                const int x = i - y * w;
                for (int k = 1; k <= r; k++)
                    acc = fmaf(B[reflect101(y + k, h) * w + x] + B[reflect101(y - k, h) * w + x], taps.t[r + k], acc);
            }
            A[i] = acc;
        }
        __syncthreads();
    }

    double *ox = fx + o, *oy = fy + o;
    if (vec2) {
        // pair q holds the item's pixels 2q - lead and 2q - lead + 1: element offset o + 2q - lead is even
        const int lead = (int)(o & 1);
        const int pairs = (px + lead + 1) / 2;
        for (int q = tid; q < pairs; q += kGradBlock) {
            const int i0 = 2 * q - lead, i1 = i0 + 1;
            double gx0 = 0.0, gy0 = 0.0, gx1 = 0.0, gy1 = 0.0;
            if (i0 >= 0) {
                const int y = i0 / w;
                sobel_at(A, h, w, y, i0 - y * w, &gx0, &gy0);
            }
            if (i1 < px) {
                const int y = i1 / w;
                sobel_at(A, h, w, y, i1 - y * w, &gx1, &gy1);
            }
            if (i0 >= 0 && i1 < px) {
                *reinterpret_cast<double2 *>(ox + i0) = make_double2(gx0, gx1);
                *reinterpret_cast<double2 *>(oy + i0) = make_double2(gy0, gy1);
            } else if (i0 >= 0) {
                ox[i0] = gx0;
                oy[i0] = gy0;
            } else {
                ox[i1] = gx1;
                oy[i1] = gy1;
            }
        }
    } else {
        for (int i = tid; i < px; i += kGradBlock) {
            const int y = i / w;
            double gx, gy;
            sobel_at(A, h, w, y, i - y * w, &gx, &gy);
            ox[i] = gx;
            oy[i] = gy;
        }
    }
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

int va_potential_gradients_ragged(const void *src, int dtype, const int32_t *shapes, const int64_t *offsets,
                                  int64_t total, int m, int max_pixels, double sigma, double *fx_out, double *fy_out,
                                  int32_t *status, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(dtype == VA_U8 || dtype == VA_F32,
               "va_potential_gradients_ragged: items must be VA_U8 or VA_F32 (got dtype %d)", dtype);
    VA_REQUIRE(sigma >= 0 && sigma == sigma, "va_potential_gradients_ragged: sigma must be >= 0 (got %g)", sigma);
    VA_REQUIRE(dtype == VA_F32 || sigma == 0,
               "va_potential_gradients_ragged: VA_U8 items take sigma == 0 only (the 8-bit blur is fixed-point)");
    VA_REQUIRE(m >= 0 && total >= 0, "va_potential_gradients_ragged: negative count (m %d, total %lld)", m,
               (long long)total);
    VA_REQUIRE(max_pixels >= 0 && max_pixels <= kGradResidentMaxPixels,
               "va_potential_gradients_ragged: max_pixels %d outside 0 .. %d", max_pixels, kGradResidentMaxPixels);
    TapsF32 taps;                                    // ksize == 0: no blur
    taps.ksize = 0;
    if (sigma > 0) {
        int rc = gauss_taps_f32(sigma, &taps.ksize, taps.t, kMaxTaps);
        if (rc)
            return rc;
    }
    if (m == 0)
        return VA_OK;
    VA_REQUIRE(shapes && offsets && status && ((src && fx_out && fy_out) || total == 0),
               "va_potential_gradients_ragged: NULL argument");
    hipStream_t st = as_stream(stream);
    const int vec2 = ((uintptr_t)fx_out % 16 == 0) && ((uintptr_t)fy_out % 16 == 0);
    const size_t lds = (size_t)(max_pixels > 0 ? max_pixels : 1) * 2 * sizeof(float);
    const dim3 grid(m), block(kGradBlock);
    if (dtype == VA_U8)
        hipLaunchKernelGGL(grad_ragged_kernel<uint8_t>, grid, block, lds, st, static_cast<const uint8_t *>(src), shapes,
                           offsets, total, max_pixels, taps, fx_out, fy_out, vec2, status);
    else
        hipLaunchKernelGGL(grad_ragged_kernel<float>, grid, block, lds, st, static_cast<const float *>(src), shapes,
                           offsets, total, max_pixels, taps, fx_out, fy_out, vec2, status);
    VA_LAUNCH_CHECK("grad_ragged_kernel");
    return VA_OK;
}

}  // extern "C"
