// va_polygon.hip -- the two dense steps behind Polygon.get_mask and get_centerline_optimized
// (video/analysis/shapes.py:577-597, 741-742); the definitions are pinned in DESIGN.md §9, "Polygons".
//
// fill_poly : cv2.fillPoly(mask, [contour], color=1, offset) with lineType LINE_8 and shift 0, for m
//             polygons of a call, each into its own (h, w) box of a ragged packed buffer.  One workgroup per
//             polygon.  Its edges (16.16 fixed point, dx = ((x1 - x0) << 16) / (y1 - y0) truncated, active on
//             y0 <= y < y1, horizontal ones skipped) are staged in LDS.  Each wave owns a row at a time: it
//             collects the row's crossings x0 + (y - y0)*dx in LDS and writes every pixel of the row, 1 where
//             OpenCV's sorted-and-paired spans [(xl + 0xFFFF) >> 16, xr >> 16] cover it.  A pixel X is covered
//             iff the number of crossings below X << 16 is odd or a crossing equals X << 16, so
//             the crossings need no sort.  Then one lane per edge draws the edge with OpenCV's 8-connected
//             Line (left to right, clipLine first): every one of those writes stores 1.
// dt_l2_5   : cv2.distanceTransform(mask, DIST_L2, 5) into float32, one workgroup per mask.  Both passes of
//             OpenCV's distanceTransform_5x5 run row by row: the previous-row (next-row) terms of a row are
//             read in parallel from an LDS ring of three rows with the 2-pixel INIT_DIST0 border, and the
//             tmp[j - 1] + HV (tmp[j + 1] + HV) chain is an exact int64 min-plus scan over the row.
#include "va_common.h"
#include "va_raster.h"

namespace va {

namespace {

constexpr int kFillMaxVerts = VA_FILL_MAX_VERTS;
constexpr int kPolyMaxSide = VA_FILL_MAX_SIDE;
constexpr int kDtMaxWidth = VA_DT_MAX_WIDTH;
constexpr int kDtMaxHeight = VA_DT_MAX_HEIGHT;
constexpr int kPolyBlock = 256;
constexpr int kPolyWaves = kPolyBlock / kWave;
constexpr int kDtBlock = 256;
constexpr int kDtMaxChunk = kDtMaxWidth / kDtBlock;       // columns per thread
constexpr uint32_t kHV = 65536, kDiag = 91750, kLong = 143976;   // cvRound({1, 1.4f, 2.1969f} * 65536)
constexpr uint32_t kInitDist0 = 0x7fffffffu, kDistMax = 0x7fffffffu >> 2;

struct FillArgs {
    const int32_t *verts;
    const int64_t *vert_off;
    int64_t nverts;
    const int32_t *boxes;
    const int64_t *out_off;
    int64_t out_elems;
    int32_t *status;
};

template <typename T>
__global__ void __launch_bounds__(kPolyBlock) fill_poly_kernel(FillArgs a, T *out)
{
    __shared__ int32_t s_y0[kFillMaxVerts], s_y1[kFillMaxVerts];
    __shared__ int64_t s_x0[kFillMaxVerts], s_dx[kFillMaxVerts];
    __shared__ int64_t s_cross[kPolyWaves][kFillMaxVerts];
    __shared__ int s_count[kPolyWaves];

    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t v0 = a.vert_off[p], v1 = a.vert_off[p + 1];
    const int bx = a.boxes[4 * p], by = a.boxes[4 * p + 1], w = a.boxes[4 * p + 2], h = a.boxes[4 * p + 3];
    const int64_t o = a.out_off[p];
    const int64_t n = v1 - v0;
    bool ok = v0 >= 0 && v1 <= a.nverts && n >= 1 && n <= kFillMaxVerts && w >= 0 && h >= 0 &&
              w <= kPolyMaxSide && h <= kPolyMaxSide && o >= 0 && o + (int64_t)w * h <= a.out_elems;
    if (!ok) {                             // workgroup-uniform: nothing is read beyond the tables or written
        if (tid == 0)
            a.status[p] = VA_ERR_RANGE;
        return;
    }
    const int32_t *v = a.verts + 2 * v0;
    // edges of CollectPolyEdges: edge i runs from vertex i - 1 (n - 1 for i = 0) to vertex i, offset applied
    int bad = 0;
    for (int i = tid; i < n; i += kPolyBlock) {
        const int j = i == 0 ? (int)n - 1 : i - 1;
        const int64_t X0 = (int64_t)v[2 * j] - bx, Y0 = (int64_t)v[2 * j + 1] - by;
        const int64_t X1 = (int64_t)v[2 * i] - bx, Y1 = (int64_t)v[2 * i + 1] - by;
        bad |= X1 < -kPolyMaxCoord || X1 > kPolyMaxCoord || Y1 < -kPolyMaxCoord || Y1 > kPolyMaxCoord;
        int32_t e0 = 0, e1 = 0;            // a horizontal edge stays inactive on every row
        int64_t ex = 0, edx = 0;
        if (Y0 != Y1) {
            edx = ((X1 - X0) * 65536) / (Y1 - Y0);
            if (Y0 < Y1)
                e0 = (int32_t)Y0, e1 = (int32_t)Y1, ex = X0 * 65536;
            else
                e0 = (int32_t)Y1, e1 = (int32_t)Y0, ex = X1 * 65536;
        }
        s_y0[i] = e0, s_y1[i] = e1, s_x0[i] = ex, s_dx[i] = edx;
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0)
            a.status[p] = VA_ERR_RANGE;
        return;
    }
    // FillEdgeCollection draws nothing with fewer than two (non-horizontal) edges
    __shared__ int s_total;
    int nonhoriz = 0;
    for (int i = tid; i < n; i += kPolyBlock)
        nonhoriz += s_y0[i] != s_y1[i];
    if (tid == 0)
        s_total = 0;
    __syncthreads();
    if (nonhoriz)
        atomicAdd(&s_total, nonhoriz);
    __syncthreads();
    const int total = s_total;
    T *img = out + o;
    for (int yb = 0; yb < h; yb += kPolyWaves) {
        const int y = yb + wave;
        if (lane == 0)
            s_count[wave] = 0;
        __syncthreads();
        if (y < h && total >= 2)
            for (int i = lane; i < n; i += kWave)
                if (s_y0[i] <= y && y < s_y1[i]) {
                    const int k = atomicAdd(&s_count[wave], 1);
                    s_cross[wave][k] = s_x0[i] + (int64_t)(y - s_y0[i]) * s_dx[i];
                }
        __syncthreads();
        if (y < h) {
            const int cnt = total >= 2 ? s_count[wave] : 0;
            for (int x = lane; x < w; x += kWave) {
                const int64_t P = (int64_t)x * 65536;
                int below = 0, at = 0;
                for (int k = 0; k < cnt; k++) {
                    const int64_t c = s_cross[wave][k];
                    below += c < P;
                    at += c == P;
                }
                img[(int64_t)y * w + x] = (T)(((below & 1) || at) ? 1 : 0);
            }
        }
    }
    // the edges' lines overwrite the rows' zeros: complete the row stores before any line store is issued
    __threadfence();
    __syncthreads();
    for (int i = tid; i < n; i += kPolyBlock) {
        const int j = i == 0 ? (int)n - 1 : i - 1;
        draw_line8(img, w, h, (int64_t)v[2 * j] - bx, (int64_t)v[2 * j + 1] - by, (int64_t)v[2 * i] - bx,
                   (int64_t)v[2 * i + 1] - by, (T)1);
    }
    if (tid == 0)
        a.status[p] = VA_OK;
}

// ------------------------------------------------------------------------------ distance transform
// block-wide inclusive min-scan of one value per thread (Hillis-Steele in LDS)
__device__ int64_t block_scan_min(int64_t v, int64_t *s, bool reverse)
{
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
    for (int d = 1; d < kDtBlock; d <<= 1) {
        const int src = reverse ? tid + d : tid - d;
        const int64_t o = (src >= 0 && src < kDtBlock) ? s[src] : INT64_MAX;
        __syncthreads();
        if (o < v)
            v = o;
        s[tid] = v;
        __syncthreads();
    }
    return v;
}

__global__ void __launch_bounds__(kDtBlock)
dt_l2_5_kernel(const uint8_t *__restrict__ masks, const int32_t *__restrict__ shapes,
               const int64_t *__restrict__ offsets, int64_t total, int ring_w, float *__restrict__ out,
               int32_t *__restrict__ status)
{
    extern __shared__ uint32_t s_ring[];             // 3 rows of ring_w + 4 words: columns -2 .. w + 1
    __shared__ int64_t s_scan[kDtBlock];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int h = shapes[2 * p], w = shapes[2 * p + 1];
    const int64_t o = offsets[p];
    if (!(h >= 0 && w >= 0 && h <= kDtMaxHeight && w <= ring_w && w <= kDtMaxWidth && o >= 0 &&
          o + (int64_t)h * w <= total)) {
        if (tid == 0)
            status[p] = VA_ERR_RANGE;
        return;
    }
    if (h == 0 || w == 0) {
        if (tid == 0)
            status[p] = VA_OK;
        return;
    }
    const int stride = w + 4;
    const uint8_t *src = masks + o;
    uint32_t *tmp = reinterpret_cast<uint32_t *>(out + o);      // the forward pass's rows, until overwritten
    float *dst = out + o;
    const int chunk = (w + kDtBlock - 1) / kDtBlock, c0 = tid * chunk;
    // the top (bottom) border rows and the side borders: INIT_DIST0 (initTopBottom and the per-row border)
    for (int i = tid; i < 3 * stride; i += kDtBlock)
        s_ring[i] = kInitDist0;
    __syncthreads();

    // forward pass: t0 = min over the 8 causal neighbours, then tmp[j] = min(t0, tmp[j - 1] + HV); background 0
    for (int i = 0; i < h; i++) {
        const uint32_t *r1 = s_ring + ((i + 2) % 3) * stride + 2;      // row i - 1 (INIT_DIST0 above row 0)
        const uint32_t *r2 = s_ring + ((i + 1) % 3) * stride + 2;      // row i - 2
        int64_t val[kDtMaxChunk];
        int64_t run = INT64_MAX;
#pragma unroll
        for (int k = 0; k < kDtMaxChunk; k++) {
            const int j = c0 + k;
            if (k < chunk && j < w) {
                uint32_t t0 = 0;
                if (src[(int64_t)i * w + j]) {
                    t0 = r2[j - 1] + kLong;
                    uint32_t t = r2[j + 1] + kLong;
                    t0 = t < t0 ? t : t0;
                    t = r1[j - 2] + kLong, t0 = t < t0 ? t : t0;
                    t = r1[j - 1] + kDiag, t0 = t < t0 ? t : t0;
                    t = r1[j] + kHV, t0 = t < t0 ? t : t0;
                    t = r1[j + 1] + kDiag, t0 = t < t0 ? t : t0;
                    t = r1[j + 2] + kLong, t0 = t < t0 ? t : t0;
                }
                // tmp[j] = j*HV + min(INIT_DIST0 + HV, min_{k <= j} (t0[k] - k*HV))
                const int64_t v = (int64_t)t0 - (int64_t)j * kHV;
                run = v < run ? v : run;
                val[k] = run;
            }
        }
        block_scan_min(run, s_scan, false);
        const int64_t before = tid > 0 ? s_scan[tid - 1] : INT64_MAX;
        int64_t carry = (int64_t)kInitDist0 + kHV;
        carry = before < carry ? before : carry;
        uint32_t *r0 = s_ring + (i % 3) * stride + 2;                  // overwrites row i - 3, read by nobody now
#pragma unroll
        for (int k = 0; k < kDtMaxChunk; k++) {
            const int j = c0 + k;
            if (k < chunk && j < w) {
                const int64_t m = val[k] < carry ? val[k] : carry;
                const uint32_t t = (uint32_t)(m + (int64_t)j * kHV);
                r0[j] = t;
                tmp[(int64_t)i * w + j] = t;
            }
        }
        __syncthreads();
    }

    // backward pass: rows h and h + 1 are INIT_DIST0; a pixel with tmp <= HV keeps its value, the others take
    // min(tmp, the 7 anticausal terms of rows i + 1, i + 2, tmp[j + 1] + HV)
    for (int i = tid; i < 3 * stride; i += kDtBlock)
        s_ring[i] = kInitDist0;
    __syncthreads();
    for (int i = h - 1; i >= 0; i--) {
        const int ri = (i % 3 + 3) % 3;
        const uint32_t *r1 = s_ring + ((ri + 1) % 3) * stride + 2;     // row i + 1
        const uint32_t *r2 = s_ring + ((ri + 2) % 3) * stride + 2;     // row i + 2
        int64_t val[kDtMaxChunk];
        uint32_t own[kDtMaxChunk];
        int64_t run = INT64_MAX;
#pragma unroll
        for (int k = kDtMaxChunk - 1; k >= 0; k--) {
            const int j = c0 + k;
            if (k < chunk && j < w) {
                uint32_t t0 = tmp[(int64_t)i * w + j];
                own[k] = t0;
                if (t0 > kHV) {
                    uint32_t t = r2[j + 1] + kLong;
                    t0 = t < t0 ? t : t0;
                    t = r2[j - 1] + kLong, t0 = t < t0 ? t : t0;
                    t = r1[j + 2] + kLong, t0 = t < t0 ? t : t0;
                    t = r1[j + 1] + kDiag, t0 = t < t0 ? t : t0;
                    t = r1[j] + kHV, t0 = t < t0 ? t : t0;
                    t = r1[j - 1] + kDiag, t0 = t < t0 ? t : t0;
                    t = r1[j - 2] + kLong, t0 = t < t0 ? t : t0;
                }
                // tmp'[j] = min(INIT_DIST0 + (w - j)*HV, min_{k >= j} (t0[k] + (k - j)*HV)).  Through a held
                // pixel (tmp <= HV) the chain carries tmp itself: every other term is >= HV >= tmp.
                const int64_t v = (int64_t)t0 + (int64_t)j * kHV;
                run = v < run ? v : run;
                val[k] = run;
            }
        }
        block_scan_min(run, s_scan, true);
        const int64_t after = tid + 1 < kDtBlock ? s_scan[tid + 1] : INT64_MAX;
        int64_t carry = (int64_t)kInitDist0 + (int64_t)w * kHV;
        carry = after < carry ? after : carry;
        uint32_t *r0 = s_ring + ri * stride + 2;
#pragma unroll
        for (int k = 0; k < kDtMaxChunk; k++) {
            const int j = c0 + k;
            if (k < chunk && j < w) {
                const int64_t m = val[k] < carry ? val[k] : carry;
                uint32_t t = own[k] > kHV ? (uint32_t)(m - (int64_t)j * kHV) : own[k];
                r0[j] = t;
                t = t > kDistMax ? kDistMax : t;
                dst[(int64_t)i * w + j] = (float)t * (1.f / 65536);
            }
        }
        __syncthreads();
    }
    if (tid == 0)
        status[p] = VA_OK;
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

int va_fill_poly(const int32_t *verts, const int64_t *vert_off, int64_t nverts, const int32_t *boxes,
                 const int64_t *out_off, int64_t out_elems, int m, int elem_size, void *out, int32_t *status,
                 void *stream)
{
    VA_ENTER();
    VA_REQUIRE(m >= 0 && nverts >= 0 && out_elems >= 0, "va_fill_poly: negative count (m %d, nverts %lld, out %lld)",
               m, (long long)nverts, (long long)out_elems);
    VA_REQUIRE(elem_size == 1 || elem_size == 4, "va_fill_poly: elem_size must be 1 (uint8) or 4 (int32), got %d",
               elem_size);
    if (m == 0)
        return VA_OK;
    VA_REQUIRE(vert_off && boxes && out_off && status && (verts || nverts == 0) && (out || out_elems == 0),
               "va_fill_poly: NULL argument");
    FillArgs a{verts, vert_off, nverts, boxes, out_off, out_elems, status};
    if (elem_size == 1)
        hipLaunchKernelGGL(fill_poly_kernel<uint8_t>, dim3(m), dim3(kPolyBlock), 0, as_stream(stream), a,
                           static_cast<uint8_t *>(out));
    else
        hipLaunchKernelGGL(fill_poly_kernel<int32_t>, dim3(m), dim3(kPolyBlock), 0, as_stream(stream), a,
                           static_cast<int32_t *>(out));
    VA_LAUNCH_CHECK("fill_poly_kernel");
    return VA_OK;
}

int va_distance_transform_l2_5(const uint8_t *masks, const int32_t *shapes, const int64_t *offsets, int64_t total,
                               int m, int max_w, float *out, int32_t *status, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(m >= 0 && total >= 0, "va_distance_transform_l2_5: negative count (m %d, total %lld)", m,
               (long long)total);
    VA_REQUIRE(max_w >= 0 && max_w <= kDtMaxWidth, "va_distance_transform_l2_5: max_w %d outside 0 .. %d", max_w,
               kDtMaxWidth);
    if (m == 0)
        return VA_OK;
    VA_REQUIRE(shapes && offsets && status && ((masks && out) || total == 0),
               "va_distance_transform_l2_5: NULL argument");
    const size_t lds = (size_t)3 * (max_w + 4) * sizeof(uint32_t);
    hipLaunchKernelGGL(dt_l2_5_kernel, dim3(m), dim3(kDtBlock), lds, as_stream(stream), masks, shapes, offsets, total,
                       max_w, out, status);
    VA_LAUNCH_CHECK("dt_l2_5_kernel");
    return VA_OK;
}

}  // extern "C"
