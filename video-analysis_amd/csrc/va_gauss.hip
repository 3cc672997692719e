// va_gauss.hip -- Gaussian blur (A1)
//
// replaces cv2.GaussianBlur(frame.astype(np.uint8), (0, 0), sigma)
//          FilterBlur._process_frame, video/filters.py:388-392           (8-bit fixed point)
//      and cv2.GaussianBlur(float image, (0,0), sigma), video/analysis/active_contour.py:108
//
// Here: the taps, the generic kernels (any radius <= 127, any channel count; row pass -> scratch
// in HBM -> column pass; fallback and cross-check) and the Gaussian plan, which picks one of the
// kernel families (va_common.h, GaussFamily) for every stand-alone call and pipeline.
#include <math.h>

#include "va_common.h"

namespace va {

// ---------------------------------------------------------------------------- host: taps
static int cv_round(double v) { return (int)lrint(v); }  // round-half-even like cvRound

int gauss_ksize(double sigma, bool is_u8)
{
    return cv_round(sigma * (is_u8 ? 3 : 4) * 2 + 1) | 1;
}

static int taps_f64(double sigma, int n, double *out)
{
    // OpenCV getGaussianKernelBitExact: x runs over half-integer steps, hence -0.125
    const int n2 = (n - 1) / 2;
    const double scale2x = -0.125 / (sigma * sigma);
    double sum = 0.0;
    for (int i = 0, x = 1 - n; i < n2; i++, x += 2) {
        out[i] = exp((double)(x * x) * scale2x);
        sum += out[i];
    }
    sum *= 2.0;
    sum += 1.0;
    const double mul1 = 1.0 / sum;
    for (int i = 0; i < n2; i++) {
        double t = out[i] * mul1;
        out[i] = t;
        out[n - 1 - i] = t;
    }
    out[n2] = 1.0 * mul1;
    return 0;
}

void gauss_taps_f64(double sigma, int n, double *out) { taps_f64(sigma, n, out); }

int gauss_taps_q8(double sigma, int *ksize, uint16_t *taps, int cap, int rule)
{
    VA_REQUIRE(sigma > 0 && sigma == sigma, "gaussian: sigma must be > 0 (got %g)", sigma);
    VA_REQUIRE(rule == VA_TAPS_CV4 || rule == VA_TAPS_CV3, "gaussian: unknown tap rule %d", rule);
    const int n = gauss_ksize(sigma, true);
    if (n > cap) {
        set_error("gaussian: sigma=%g needs %d taps, more than the supported %d", sigma, n, cap);
        return VA_ERR_RANGE;
    }
    *ksize = n;
    if (rule == VA_TAPS_CV3) {
        // OpenCV 2.4 / 3.x (the reference's era, video/analysis/regions.py:180-182): float32
        // getGaussianKernel -- exp values rounded to float, summed in double, scaled, rounded to float --
        // then every tap cvRound(k * 256) on its own; the sum is not forced to 256
        float cf[kMaxTaps + 1];
        const double scale2x = -0.5 / (sigma * sigma);
        double sum = 0.0;
        for (int i = 0; i < n; i++) {
            const double x = i - (n - 1) * 0.5;
            cf[i] = (float)exp(scale2x * x * x);
            sum += cf[i];
        }
        sum = 1.0 / sum;
        for (int i = 0; i < n; i++) {
            const float k = (float)(cf[i] * sum);
            taps[i] = (uint16_t)cv_round((double)(k * 256.0f));
        }
        return VA_OK;
    }
    double k[kMaxTaps + 1];
    taps_f64(sigma, n, k);
    // getGaussianKernelFixedPoint_ED: error diffusion from the tails, centre takes the rest
    const int n2 = n / 2;
    double err = 0.0;
    long long sum = 0;
    for (int i = 0; i < n2; i++) {
        double adj = k[i] * 256.0 + err;
        long long v0 = cv_round(adj);
        err = adj - (double)v0;
        taps[i] = (uint16_t)v0;
        taps[n - 1 - i] = (uint16_t)v0;
        sum += v0;
    }
    taps[n2] = (uint16_t)(256 - 2 * sum);
    return VA_OK;
}

int gauss_taps_f32(double sigma, int *ksize, float *taps, int cap)
{
    VA_REQUIRE(sigma > 0 && sigma == sigma, "gaussian: sigma must be > 0 (got %g)", sigma);
    const int n = gauss_ksize(sigma, false);
    if (n > cap) {
        set_error("gaussian: sigma=%g needs %d taps, more than the supported %d", sigma, n, cap);
        return VA_ERR_RANGE;
    }
    double k[kMaxTaps + 1];
    taps_f64(sigma, n, k);
    for (int i = 0; i < n; i++)
        taps[i] = (float)k[i];
    *ksize = n;
    return VA_OK;
}

// ------------------------------------------------------------------------ device: generic
namespace {

constexpr int kBlock = 256;

// T = uint16_t while the row sums fit (tap sum <= 257: every OpenCV >= 4 tap set), uint32_t otherwise
template <class T>
__global__ void __launch_bounds__(kBlock)
gauss_row_u8_generic(const uint8_t *__restrict__ src, T *__restrict__ tmp, int w, int c,
                     TapsQ8 taps, size_t total)
{
    size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total)
        return;
    int ch = (int)(e % c);
    size_t pix = e / c;
    int x = (int)(pix % w);
    size_t rowi = pix / w;
    const uint8_t *row = src + rowi * (size_t)w * c;
    const int r = taps.ksize >> 1;
    uint32_t acc = 0;
    for (int i = 0; i < taps.ksize; i++)
        acc += (uint32_t)taps.t[i] * row[(size_t)reflect101(x + i - r, w) * c + ch];
    tmp[e] = (T)acc;
}

template <class T>
__global__ void __launch_bounds__(kBlock)
gauss_col_u8_generic(const T *__restrict__ tmp, uint8_t *__restrict__ dst, int h, int w,
                     int c, TapsQ8 taps, size_t total)
{
    size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total)
        return;
    size_t wc = (size_t)w * c;
    size_t col = e % wc;
    size_t rowi = e / wc;
    int y = (int)(rowi % h);
    const T *frame = tmp + (rowi - y) * wc;
    const int r = taps.ksize >> 1;
    uint32_t acc = 0;
    for (int j = 0; j < taps.ksize; j++)
        acc += (uint32_t)taps.t[j] * frame[(size_t)reflect101(y + j - r, h) * wc + col];
    uint32_t v = (acc + 32768u) >> 16;
    dst[e] = (uint8_t)(v > 255u ? 255u : v);
}

__global__ void __launch_bounds__(kBlock)
gauss_row_f32_generic(const float *__restrict__ src, float *__restrict__ tmp, int w, int c,
                      TapsF32 taps, size_t total)
{
    size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total)
        return;
    int ch = (int)(e % c);
    size_t pix = e / c;
    int x = (int)(pix % w);
    size_t rowi = pix / w;
    const float *row = src + rowi * (size_t)w * c;
    const int r = taps.ksize >> 1;
    float acc = 0.0f;
    for (int i = 0; i < taps.ksize; i++)  // in-order fmaf chain (OpenCV RowVec_32f)
        acc = fmaf(row[(size_t)reflect101(x + i - r, w) * c + ch], taps.t[i], acc);
    tmp[e] = acc;
}

__global__ void __launch_bounds__(kBlock)
gauss_col_f32_generic(const float *__restrict__ tmp, float *__restrict__ dst, int h, int w, int c,
                      TapsF32 taps, size_t total)
{
    size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (e >= total)
        return;
    size_t wc = (size_t)w * c;
    size_t col = e % wc;
    size_t rowi = e / wc;
    int y = (int)(rowi % h);
    const float *frame = tmp + (rowi - y) * wc;
    const int r = taps.ksize >> 1;
    // centre tap, then symmetric pairs folded (OpenCV SymmColumnVec_32f)
    float acc = fmaf(frame[(size_t)y * wc + col], taps.t[r], 0.0f);
    for (int k = 1; k <= r; k++) {
        float a = frame[(size_t)reflect101(y + k, h) * wc + col];
        float b = frame[(size_t)reflect101(y - k, h) * wc + col];
        acc = fmaf(a + b, taps.t[r + k], acc);
    }
    dst[e] = acc;
}

}  // namespace

static int taps_sum(const TapsQ8 &taps)
{
    int sum = 0;
    for (int i = 0; i < taps.ksize; i++)
        sum += taps.t[i];
    return sum;
}

// generic (any radius / channel count) two-pass Gaussian through a u16 / f32 scratch in HBM
// (16-bit row sums while the tap sum allows)
static int launch_gauss_generic_u8(const uint8_t *src, uint8_t *dst, void *scratch, int n, int h,
                                   int w, int c, const TapsQ8 &taps, hipStream_t st)
{
    size_t total = (size_t)n * h * w * c;
    if (total == 0)
        return VA_OK;
    int grid = cdiv((long long)total, kBlock);
    if (taps_sum(taps) <= 257) {
        gauss_row_u8_generic<uint16_t><<<grid, kBlock, 0, st>>>(src, (uint16_t *)scratch, w, c, taps, total);
        VA_LAUNCH_CHECK("gauss_row_u8_generic");
        gauss_col_u8_generic<uint16_t><<<grid, kBlock, 0, st>>>((const uint16_t *)scratch, dst, h, w, c, taps, total);
    } else {
        gauss_row_u8_generic<uint32_t><<<grid, kBlock, 0, st>>>(src, (uint32_t *)scratch, w, c, taps, total);
        VA_LAUNCH_CHECK("gauss_row_u8_generic");
        gauss_col_u8_generic<uint32_t><<<grid, kBlock, 0, st>>>((const uint32_t *)scratch, dst, h, w, c, taps, total);
    }
    VA_LAUNCH_CHECK("gauss_col_u8_generic");
    return VA_OK;
}

static int launch_gauss_generic_f32(const float *src, float *dst, float *scratch, int n, int h, int w,
                                    int c, const TapsF32 &taps, hipStream_t st)
{
    size_t total = (size_t)n * h * w * c;
    if (total == 0)
        return VA_OK;
    int grid = cdiv((long long)total, kBlock);
    gauss_row_f32_generic<<<grid, kBlock, 0, st>>>(src, scratch, w, c, taps, total);
    VA_LAUNCH_CHECK("gauss_row_f32_generic");
    gauss_col_f32_generic<<<grid, kBlock, 0, st>>>(scratch, dst, h, w, c, taps, total);
    VA_LAUNCH_CHECK("gauss_col_f32_generic");
    return VA_OK;
}

// ---------------------------------------------------------------------------- host: plan
// Frames the matrix-core Gaussian can take after a re-layout: colour frames (the channels are filtered
// independently, as OpenCV does) and widths that are not a multiple of 16 go through planes (frame, channel,
// h, wp).  A plane wider than the frame carries the reflected continuation of every row over at least the
// radius, so its blur is the frame's on the first w columns.  Returns the plane width, or 0 (not applicable).
static int planes_width(int h, int w, int c, const TapsQ8 &t)
{
    const int wp = (w % 16 == 0) ? w : ((w + 16 + 15) / 16) * 16;
    if (c >= 1 && c <= 4 && wp - w < w && gauss_mfma_supported(wp, h, t))
        return wp;
    return 0;
}
// U8Planes scratch: [planes in | planes out]
struct PlanesLayout { size_t in, out, total; };
static PlanesLayout planes_layout(size_t n, int h, int wp, int c)
{
    Carve cv;
    return {cv.take(n * c * h * wp), cv.take(n * c * h * wp), cv.total};
}
static int blur_u8_planes(const uint8_t *src, uint8_t *dst, int n, int h, int w, int wp, int c,
                          const TapsQ8 &t, void *scratch, hipStream_t st)
{
    const PlanesLayout L = planes_layout(n, h, wp, c);
    uint8_t *pin = at<uint8_t>(scratch, L.in), *pout = at<uint8_t>(scratch, L.out);
    int rc = launch_channel_planes(src, pin, n, h, w, wp, c, true, st);
    if (rc)
        return rc;
    rc = launch_gauss_mfma_u8(pin, pout, nullptr, -1, n * c, h, wp, t, st);
    if (rc)
        return rc;
    return launch_channel_planes(pout, dst, n, h, w, wp, c, false, st);
}

int plan_gaussian(GaussPlan *g, int dtype, int h, int w, int c, double sigma, int tap_rule, bool aligned,
                  bool valu_hook, GaussFamily force)
{
    *g = GaussPlan{GaussFamily::None, dtype, h, w, c};
    const int rc = dtype == VA_U8 ? gauss_taps_q8(sigma, &g->tq.ksize, g->tq.t, kMaxTaps, tap_rule)
                                  : gauss_taps_f32(sigma, &g->tf.ksize, g->tf.t, kMaxTaps);
    if (rc)
        return rc;
    if (dtype != VA_U8)
        g->family = aligned && gauss_f32_fused_supported(h, w, c, g->tf) ? GaussFamily::F32Fused
                    : gauss_f32_fast_supported(w, c, g->tf)              ? GaussFamily::F32Fast
                                                                         : GaussFamily::F32Generic;
    else if (force != GaussFamily::None)
        g->family = force;
    else if (c == 1 && aligned && !valu_hook && gauss_mfma_supported(w, h, g->tq))
        g->family = GaussFamily::U8Mfma;
    else if (c == 1 && aligned && gauss_fused_supported(w, h, g->tq))
        g->family = GaussFamily::U8Dot;
    else if ((g->wp = planes_width(h, w, c, g->tq)))
        g->family = GaussFamily::U8Planes;
    else
        g->family = GaussFamily::U8Generic;
    return VA_OK;
}

size_t gauss_scratch_bytes(const GaussPlan &g, size_t n)
{
    const size_t count = n * g.h * g.w * g.c;
    if (g.family == GaussFamily::U8Planes)
        return planes_layout(n, g.h, g.wp, g.c).total;
    if (g.family == GaussFamily::U8Generic)
        return count * (taps_sum(g.tq) <= 257 ? sizeof(uint16_t) : sizeof(uint32_t));     // row sums <= 255 * sum
    return g.dtype == VA_F32 && g.family != GaussFamily::None ? count * sizeof(float) : 0;   // (single pass: none)
}

const char *gauss_plan_name(const GaussPlan &g)
{
    static const char *const names[] = {"none", "mfma-i8", "fused-lds", "mfma-i8-planes", "generic",
                                        "f32-ema-row+col-march", "f32-packed", "generic"};    // GaussFamily order
    return names[(int)g.family];
}

int launch_gaussian(const GaussPlan &g, const void *src, void *dst, uint32_t *bits, int thresh, int mask8_maxval,
                    void *scratch, int n, hipStream_t st, StageProfiler *prof, const float *bg, float *bg_out,
                    int64_t n_seen, double rate)
{
    VA_REQUIRE((!bits || g.single_pass()) && (mask8_maxval <= 0 || g.byte_mask()) && (!bg || g.folds_ema()),
               "gaussian: the planned kernel cannot write the requested output");
    const uint8_t *s8 = (const uint8_t *)src;
    const float *sf = (const float *)src;
    uint8_t *d8 = (uint8_t *)dst;
    float *df = (float *)dst, *scratch_f = (float *)scratch;
    auto marked = [&](int rc, const char *stage) {
        if (rc == VA_OK)
            mark(prof, stage, st);
        return rc;
    };
    switch (g.family) {
    case GaussFamily::U8Mfma:
        return marked(launch_gauss_mfma_u8(s8, d8, bits, thresh, n, g.h, g.w, g.tq, st, mask8_maxval),
                      mask8_maxval > 0 ? "gauss_mfma_mask8" : "gauss_mfma");
    case GaussFamily::U8Dot:
        return marked(launch_gauss_fused_u8(s8, d8, bits, thresh, n, g.h, g.w, g.tq, st), "gauss_fused");
    case GaussFamily::U8Planes:
        return marked(blur_u8_planes(s8, d8, n, g.h, g.w, g.wp, g.c, g.tq, scratch, st), "gauss_planes");
    case GaussFamily::U8Generic:
        return marked(launch_gauss_generic_u8(s8, d8, scratch, n, g.h, g.w, g.c, g.tq, st), "gauss_generic");
    case GaussFamily::F32Fused:     // (marks ema_row_f32 or row_f32, then col_f32)
        return launch_gauss_f32_fused(sf, df, scratch_f, bg, bg_out, n_seen, rate, n, g.h, g.w, g.c, g.tf, st, prof);
    case GaussFamily::F32Fast:
        return marked(launch_gauss_f32_fast(sf, df, scratch_f, n, g.h, g.w, g.c, g.tf, st), "gauss_f32");
    case GaussFamily::F32Generic:
        return marked(launch_gauss_generic_f32(sf, df, scratch_f, n, g.h, g.w, g.c, g.tf, st), "gauss_generic");
    default:
        VA_REQUIRE(false, "gaussian: no kernel planned");
    }
}

// The stand-alone Gaussian calls: argument checks, a plan, a scratch lease and a launch.  The test hooks
// (force != None) keep their terse messages; the dot4/dot2 hook takes one channel only.
static int gaussian_call(const char *who, int dtype, const void *src, void *dst, int n, int h, int w, int c,
                         double sigma, int tap_rule, GaussFamily force, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(h <= 0 || w <= 0 || (size_t)h * (size_t)w < kMaxFramePixels,
               "%s: frames above 2^29 pixels are not supported", who);
    const bool hook = force != GaussFamily::None;
    VA_REQUIRE(src && dst && src != dst, hook ? "%s: bad pointers" : "%s: src/dst must be distinct non-NULL", who);
    VA_REQUIRE(!hook || (n >= 0 && h > 0 && w > 0 && c > 0 && (c == 1 || force != GaussFamily::U8Dot)),
               "%s: bad shape", who);
    VA_REQUIRE(n >= 0 && h > 0 && w > 0 && c > 0, "%s: bad shape (%d,%d,%d,%d)", who, n, h, w, c);
    const bool aligned = (uintptr_t)src % 16 == 0 && (dtype == VA_F32 || (uintptr_t)dst % 4 == 0);
    GaussPlan g;
    int rc = plan_gaussian(&g, dtype, h, w, c, sigma, tap_rule, aligned, false, force);
    if (rc)
        return rc;
    ScratchLease scratch;
    if (!g.single_pass() && (rc = scratch.acquire(gauss_scratch_bytes(g, n), as_stream(stream))))
        return rc;
    return launch_gaussian(g, src, dst, nullptr, -1, 0, scratch.ptr, n, as_stream(stream), nullptr);
}

int g_gauss_u8_valu = 0;

}  // namespace va

using namespace va;

extern "C" {

int va_gauss_taps_q8(double sigma, int *ksize_out, uint16_t *taps_out, int capacity)
{
    return va_gauss_taps_q8_rule(sigma, VA_TAPS_CV4, ksize_out, taps_out, capacity);
}
int va_gauss_taps_q8_rule(double sigma, int tap_rule, int *ksize_out, uint16_t *taps_out, int capacity)
{
    VA_REQUIRE(ksize_out && taps_out, "va_gauss_taps_q8: NULL argument");
    TapsQ8 t;
    int rc = gauss_taps_q8(sigma, &t.ksize, t.t, kMaxTaps, tap_rule);
    if (rc)
        return rc;
    if (t.ksize > capacity) {
        set_error("va_gauss_taps_q8: %d taps > capacity %d", t.ksize, capacity);
        return VA_ERR_RANGE;
    }
    memcpy(taps_out, t.t, sizeof(uint16_t) * t.ksize);
    *ksize_out = t.ksize;
    return VA_OK;
}
int va_gauss_taps_f32(double sigma, int *ksize_out, float *taps_out, int capacity)
{
    VA_REQUIRE(ksize_out && taps_out, "va_gauss_taps_f32: NULL argument");
    TapsF32 t;
    int rc = gauss_taps_f32(sigma, &t.ksize, t.t, kMaxTaps);
    if (rc)
        return rc;
    if (t.ksize > capacity) {
        set_error("va_gauss_taps_f32: %d taps > capacity %d", t.ksize, capacity);
        return VA_ERR_RANGE;
    }
    memcpy(taps_out, t.t, sizeof(float) * t.ksize);
    *ksize_out = t.ksize;
    return VA_OK;
}

int va_gaussian_u8(const uint8_t *src, uint8_t *dst, int n, int h, int w, int c, double sigma,
                   void *stream)
{
    return va_gaussian_u8_rule(src, dst, n, h, w, c, sigma, VA_TAPS_CV4, stream);
}

int va_gaussian_u8_rule(const uint8_t *src, uint8_t *dst, int n, int h, int w, int c, double sigma,
                        int tap_rule, void *stream)
{
    return gaussian_call("va_gaussian_u8", VA_U8, src, dst, n, h, w, c, sigma, tap_rule, GaussFamily::None,
                         stream);
}

// test hook: force the generic two-pass implementation
int va_gaussian_u8_generic(const uint8_t *src, uint8_t *dst, int n, int h, int w, int c,
                           double sigma, void *stream)
{
    return gaussian_call("va_gaussian_u8_generic", VA_U8, src, dst, n, h, w, c, sigma, VA_TAPS_CV4,
                         GaussFamily::U8Generic, stream);
}

// test hook: force the LDS/VALU (dot4/dot2) fused implementation
int va_gaussian_u8_valu(const uint8_t *src, uint8_t *dst, int n, int h, int w, int c, double sigma,
                        void *stream)
{
    return gaussian_call("va_gaussian_u8_valu", VA_U8, src, dst, n, h, w, c, sigma, VA_TAPS_CV4,
                         GaussFamily::U8Dot, stream);
}

int va_gaussian_f32(const float *src, float *dst, int n, int h, int w, int c, double sigma,
                    void *stream)
{
    return gaussian_call("va_gaussian_f32", VA_F32, src, dst, n, h, w, c, sigma, VA_TAPS_CV4, GaussFamily::None,
                         stream);
}

// test / measurement hook: pipelines created while this is set run their 8-bit Gaussian on the VALU
// (dot4/dot2 LDS kernel) instead of the matrix cores -- the north star's "no MFMA" form of the chain
int va_test_hook_gaussian_u8(int force_valu)
{
    g_gauss_u8_valu = force_valu != 0;
    return VA_OK;
}

int va_test_hook_gaussian_f32(int generic_columns)
{
    gauss_f32_test_hook(generic_columns);
    return VA_OK;
}

}  // extern "C"
