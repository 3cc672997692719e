// va_warp.hip -- cv2.warpAffine of single-channel uint8 images with INTER_LINEAR and BORDER_CONSTANT 0, batched and
// ragged: line_scan (video/analysis/image.py:89-106) and get_subimage (:61-85).  The definition is pinned in
// DESIGN.md §9, "Affine warps and line scans": the classical fixed-point path of OpenCV 2.4 .. 4.10.
//
// Per item a forward 2x3 float64 matrix is inverted in cv::warpAffine's operation order (float64; the Makefile's
// -ffp-contract=off keeps every product and sum separately rounded, as the NumPy restatement rounds them), and
// destination pixel (x, y) reads the source at
//   X = (R((M1 y + M2) 1024) + 16 + R(M0 x 1024)) >> 5,   Y = (R((M4 y + M5) 1024) + 16 + R(M3 x 1024)) >> 5
// (R: to the nearest integer, halves to even; 1/32 px), sx = X >> 5, fx = X & 31, likewise y:
//   out = ((32-fx)(32-fy) v00 + fx (32-fy) v01 + (32-fx) fy v10 + fx fy v11 + 512) >> 10,  taps outside the image 0.
//
// line scan : work items are (scan, 64-column chunk), one wave each, found by a binary search in the prefix of
//             chunk counts: scans of 10 and of 500 columns share a launch without idle workgroups.  A lane owns a
//             column of the strip, walks its rows and stores the int32 column sum; the strip never exists in HBM.
// warp      : work items are (item, 64 x 16-pixel tile), one workgroup each, found the same way; a thread owns a
//             column of the tile and four of its rows.
// An item beyond the limits (a side above VA_WARP_MAX_SIDE, a coordinate that could reach VA_WARP_COORD_LIMIT, an
// offset outside the output, a frame index outside the stack) gets status VA_ERR_RANGE and nothing of it is
// written; the items after it run.
#include <math.h>

#include "va_common.h"

namespace va {

namespace {

constexpr int kWarpBlock = 256;
constexpr int kWarpWaves = kWarpBlock / kWave;
constexpr int kTileW = VA_WARP_TILE_W, kTileH = VA_WARP_TILE_H;
constexpr int kTileRowsPerThread = kTileH / kWarpWaves;
constexpr double kCoordLimit = (double)VA_WARP_COORD_LIMIT;

struct WarpMap {
    double m0, m1, m2, m3, m4, m5;       // destination -> source
};

__device__ __forceinline__ WarpMap load_map(const double *m, bool inverse)
{
    double M0 = m[0], M1 = m[1], M2 = m[2], M3 = m[3], M4 = m[4], M5 = m[5];
    if (!inverse) {                      // cv::warpAffine's inversion, operation by operation
        double D = M0 * M4 - M1 * M3;
        D = D != 0 ? 1.0 / D : 0.0;
        const double A11 = M4 * D, A22 = M0 * D;
        M0 = A11;
        M1 *= -D;
        M3 *= -D;
        M4 = A22;
        const double b1 = -M0 * M2 - M1 * M5;
        const double b2 = -M3 * M2 - M4 * M5;
        M2 = b1;
        M5 = b2;
    }
    return WarpMap{M0, M1, M2, M3, M4, M5};
}

// every fixed-point coordinate of a dw x dh destination stays below 2^30 in magnitude (the sum of the magnitudes of
// its terms does; a NaN or an infinity fails the comparison), so that the int32 sums below cannot overflow
__device__ __forceinline__ bool map_ok(const WarpMap &M, int dw, int dh)
{
    const double xs = dw > 0 ? dw - 1 : 0, ys = dh > 0 ? dh - 1 : 0;
    const double bx = (fabs(M.m0) * xs + fabs(M.m1) * ys + fabs(M.m2)) * 1024.0;
    const double by = (fabs(M.m3) * xs + fabs(M.m4) * ys + fabs(M.m5)) * 1024.0;
    return bx < kCoordLimit && by < kCoordLimit;
}

__device__ __forceinline__ int round_fixed(double v) { return (int)rint(v); }

// the largest s in 0 .. m - 1 with prefix[s] <= c (prefix[0] == 0 by contract; any table gives an s inside the range)
__device__ __forceinline__ int find_item(const int32_t *prefix, int m, int c)
{
    int lo = 0, hi = m - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (prefix[mid] <= c)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ int warp_pixel(const uint8_t *__restrict__ f, int h, int w, int X, int Y)
{
    const int sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31;
    const bool x0 = (unsigned)sx < (unsigned)w, x1 = (unsigned)(sx + 1) < (unsigned)w;
    const bool y0 = (unsigned)sy < (unsigned)h, y1 = (unsigned)(sy + 1) < (unsigned)h;
    const int64_t i = (int64_t)sy * w + sx;
    const int v00 = x0 && y0 ? f[i] : 0, v01 = x1 && y0 ? f[i + 1] : 0;
    const int v10 = x0 && y1 ? f[i + w] : 0, v11 = x1 && y1 ? f[i + w + 1] : 0;
    return ((32 - fx) * (32 - fy) * v00 + fx * (32 - fy) * v01 + (32 - fx) * fy * v10 + fx * fy * v11 + 512) >> 10;
}

__global__ void __launch_bounds__(kWarpBlock)
line_scan_kernel(const uint8_t *__restrict__ frames, int n, int h, int w, int m, const int32_t *__restrict__ frame_idx,
                 const double *__restrict__ mats, const int32_t *__restrict__ shapes,
                 const int64_t *__restrict__ out_off, const int32_t *__restrict__ prefix, int total_chunks,
                 int64_t total_out, int32_t *__restrict__ sums, int32_t *__restrict__ status)
{
    const int lane = threadIdx.x & (kWave - 1);
    // the wave's work item; wave-uniform, so the tables below are read with scalar loads
    const int c = __builtin_amdgcn_readfirstlane((int)blockIdx.x * kWarpWaves + (int)(threadIdx.x / kWave));
    if (c >= total_chunks)
        return;
    const int s = find_item(prefix, m, c);
    const int chunk = c - prefix[s];
    if (chunk < 0 || chunk > VA_WARP_MAX_SIDE / kWave)       // a malformed prefix table: nothing to do
        return;
    const int rows = shapes[2 * s], cols = shapes[2 * s + 1], f = frame_idx[s];
    const int64_t o = out_off[s];
    const WarpMap M = load_map(mats + 6 * (int64_t)s, false);
    const bool ok = f >= 0 && f < n && rows >= 0 && rows <= VA_WARP_MAX_SIDE && cols >= 0 &&
                    cols <= VA_WARP_MAX_SIDE && o >= 0 && o + cols <= total_out && map_ok(M, cols, rows);
    if (chunk == 0 && lane == 0)
        status[s] = ok ? VA_OK : VA_ERR_RANGE;
    const int x = chunk * kWave + lane;
    if (!ok || x >= cols)
        return;
    const uint8_t *src = frames + (int64_t)f * h * w;
    const int adelta = round_fixed(M.m0 * x * 1024.0), bdelta = round_fixed(M.m3 * x * 1024.0);
    int acc = 0;
#pragma unroll 4
    for (int y = 0; y < rows; y++) {
        const int X0 = round_fixed((M.m1 * y + M.m2) * 1024.0) + 16;
        const int Y0 = round_fixed((M.m4 * y + M.m5) * 1024.0) + 16;
        acc += warp_pixel(src, h, w, (X0 + adelta) >> 5, (Y0 + bdelta) >> 5);
    }
    sums[o + x] = acc;
}

__global__ void __launch_bounds__(kWarpBlock)
warp_affine_kernel(const uint8_t *__restrict__ frames, int n, int h, int w, int m,
                   const int32_t *__restrict__ frame_idx, const double *__restrict__ mats,
                   const int32_t *__restrict__ shapes, const int32_t *__restrict__ flags,
                   const int64_t *__restrict__ out_off, const int32_t *__restrict__ prefix, int64_t total_out,
                   uint8_t *__restrict__ out, int32_t *__restrict__ status)
{
    const int t = blockIdx.x, tid = threadIdx.x;
    const int s = find_item(prefix, m, t);
    const int tile = t - prefix[s];
    const int dh = shapes[2 * s], dw = shapes[2 * s + 1], f = frame_idx[s];
    const int64_t o = out_off[s];
    const WarpMap M = load_map(mats + 6 * (int64_t)s, (flags[s] & VA_WARP_INVERSE_MAP) != 0);
    const bool ok = f >= 0 && f < n && dh >= 0 && dh <= VA_WARP_MAX_SIDE && dw >= 0 && dw <= VA_WARP_MAX_SIDE &&
                    o >= 0 && o + (int64_t)dh * dw <= total_out && map_ok(M, dw, dh);
    if (tile == 0 && tid == 0)
        status[s] = ok ? VA_OK : VA_ERR_RANGE;
    if (!ok || tile < 0)
        return;
    const int tiles_x = (dw + kTileW - 1) / kTileW;
    if (tiles_x == 0)
        return;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int x = tx * kTileW + (tid & (kTileW - 1));
    if (x >= dw)
        return;
    const uint8_t *src = frames + (int64_t)f * h * w;
    const int adelta = round_fixed(M.m0 * x * 1024.0), bdelta = round_fixed(M.m3 * x * 1024.0);
#pragma unroll
    for (int r = 0; r < kTileRowsPerThread; r++) {
        const int y = ty * kTileH + tid / kTileW + r * kWarpWaves;
        if (y < dh) {                                // a malformed prefix table gives rows beyond dh: not written
            const int X0 = round_fixed((M.m1 * y + M.m2) * 1024.0) + 16;
            const int Y0 = round_fixed((M.m4 * y + M.m5) * 1024.0) + 16;
            out[o + (int64_t)y * dw + x] = (uint8_t)warp_pixel(src, h, w, (X0 + adelta) >> 5, (Y0 + bdelta) >> 5);
        }
    }
}

// the arguments the two warp calls share; m == 0 is checked by the caller after this
int warp_check(const char *name, int n, int h, int w, int m, int total_items, int64_t total_out)
{
    VA_REQUIRE(n >= 0 && h > 0 && w > 0, "%s: bad shape (%d, %d, %d)", name, n, h, w);
    VA_REQUIRE((size_t)h * (size_t)w < kMaxFramePixels, "%s: frames above 2^29 pixels are not supported", name);
    VA_REQUIRE(m >= 0 && total_out >= 0, "%s: negative count (m %d, total_out %lld)", name, m, (long long)total_out);
    VA_REQUIRE(total_items >= m, "%s: %d work items for %d items (every item has at least one)", name, total_items,
               m);
    return VA_OK;
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

int va_line_scan_u8(const uint8_t *frames, int n, int h, int w, int m, const int32_t *frame_idx, const double *mats,
                    const int32_t *shapes, const int64_t *out_off, const int32_t *prefix, int total_chunks,
                    int64_t total_out, int32_t *sums, int32_t *status, void *stream)
{
    VA_ENTER();
    int rc = warp_check("va_line_scan_u8", n, h, w, m, total_chunks, total_out);
    if (rc || m == 0)
        return rc;
    VA_REQUIRE(frames && frame_idx && mats && shapes && out_off && prefix && sums && status,
               "va_line_scan_u8: NULL argument");
    const dim3 grid((unsigned)cdiv(total_chunks, kWarpWaves)), block(kWarpBlock);
    hipLaunchKernelGGL(line_scan_kernel, grid, block, 0, as_stream(stream), frames, n, h, w, m, frame_idx, mats, shapes,
                       out_off, prefix, total_chunks, total_out, sums, status);
    VA_LAUNCH_CHECK("line_scan_kernel");
    return VA_OK;
}

int va_warp_affine_u8(const uint8_t *frames, int n, int h, int w, int m, const int32_t *frame_idx, const double *mats,
                      const int32_t *shapes, const int32_t *flags, const int64_t *out_off, const int32_t *prefix,
                      int total_tiles, int64_t total_out, uint8_t *out, int32_t *status, void *stream)
{
    VA_ENTER();
    int rc = warp_check("va_warp_affine_u8", n, h, w, m, total_tiles, total_out);
    if (rc || m == 0)
        return rc;
    VA_REQUIRE(frames && frame_idx && mats && shapes && flags && out_off && prefix && out && status,
               "va_warp_affine_u8: NULL argument");
    const dim3 grid((unsigned)total_tiles), block(kWarpBlock);
    hipLaunchKernelGGL(warp_affine_kernel, grid, block, 0, as_stream(stream), frames, n, h, w, m, frame_idx, mats,
                       shapes, flags, out_off, prefix, total_out, out, status);
    VA_LAUNCH_CHECK("warp_affine_kernel");
    return VA_OK;
}

}  // extern "C"
