// va_common.h -- shared helpers for the HIP sources of libvideoanalysis_hip.so (gfx950 only)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/videoanalysis_hip.h"

namespace va {

// thread-local last-error message (va_last_error)
void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
const char *get_error();

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// the prologue of every entry point that allocates or launches: selects va_init's device for the calling thread
int enter_device();
#define VA_ENTER()                    \
    do {                              \
        int _rc = va::enter_device(); \
        if (_rc)                      \
            return _rc;               \
    } while (0)

#define VA_HIP(call)                                                                        \
    do {                                                                                    \
        hipError_t _e = (call);                                                             \
        if (_e != hipSuccess) {                                                             \
            va::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(_e), __FILE__,  \
                          __LINE__);                                                        \
            return _e == hipErrorOutOfMemory ? VA_ERR_NOMEM : VA_ERR_HIP;                   \
        }                                                                                   \
    } while (0)

#define VA_LAUNCH_CHECK(name)                                                               \
    do {                                                                                    \
        hipError_t _e = hipGetLastError();                                                  \
        if (_e != hipSuccess) {                                                             \
            va::set_error("launch of %s failed: %s", name, hipGetErrorString(_e));          \
            return VA_ERR_HIP;                                                              \
        }                                                                                   \
    } while (0)

#define VA_REQUIRE(cond, ...)                                                               \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            va::set_error(__VA_ARGS__);                                                     \
            return VA_ERR_INVALID;                                                          \
        }                                                                                   \
    } while (0)

constexpr int kWave = 64;  // CDNA wavefront width
// largest frame the kernels take: per-frame byte offsets (4-byte labels) travel in the 32-bit
// fields of raw buffer descriptors / uint32 arithmetic, so h*w*4 must stay below 2^31
constexpr size_t kMaxFramePixels = (size_t)1 << 29;
// the frame-shape guard of an entry that takes (n, h, w) frames and has nothing to check between the two
#define VA_REQUIRE_FRAME_SHAPE(entry)                                                       \
    VA_REQUIRE(h <= 0 || w <= 0 || (size_t)h * (size_t)w < va::kMaxFramePixels,             \
               "%s: frames above 2^29 pixels are not supported", entry);                    \
    VA_REQUIRE(n >= 0 && h > 0 && w > 0, "%s: bad shape (%d,%d,%d)", entry, n, h, w)
// largest gridDim.y / gridDim.z the library launches: a batch or a frame that would need more goes out in pieces,
// takes a kernel with a one-dimensional grid, or is refused before anything is enqueued
constexpr int kMaxGridYZ = 65535;

// Optional per-stage timing with HIP events on the pipeline's own stream (bench.py's roofline
// numbers come from here).  Events are only recorded, never waited for, inside a run.
struct StageProfiler {
    static constexpr int kMaxMarks = 4096;
    bool enabled = false;
    int every = 1, runs = 0;     // events go into every `every`-th run (an event per stage costs the stream ~2 %)
    int n = 0, dropped = 0;
    hipEvent_t ev[kMaxMarks];
    const char *name[kMaxMarks];  // nullptr = start of a run
    bool created[kMaxMarks] = {};
    void mark(const char *nm, hipStream_t st)
    {
        if (!enabled)
            return;
        if (n >= kMaxMarks) {
            dropped++;
            return;
        }
        if (!created[n]) {
            if (hipEventCreate(&ev[n]) != hipSuccess)
                return;
            created[n] = true;
        }
        if (hipEventRecord(ev[n], st) != hipSuccess)
            return;
        name[n++] = nm;
    }
};
// (prof == nullptr: nobody is timing)
inline void mark(StageProfiler *prof, const char *nm, hipStream_t st) { if (prof) prof->mark(nm, st); }

inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
inline int words_per_row(int w) { return (w + 31) / 32; }
inline bool aligned(const void *p, size_t a) { return (reinterpret_cast<uintptr_t>(p) % a) == 0; }

// Carves a workspace into regions that start on 256-byte boundaries.  Each workspace has one function that builds
// a struct of offsets and `total` with this -- often as a braced list {c.take(..), .., c.total}, which is evaluated
// left to right -- and both its size function and its launcher ask that struct.
struct Carve {
    static size_t up(size_t v) { return (v + 255) & ~(size_t)255; }
    size_t total = 0;
    size_t take(size_t bytes)
    {
        const size_t at = total;
        total = up(total + bytes);
        return at;
    }
};
template <class T = void>
inline T *at(void *base, size_t offset) { return reinterpret_cast<T *>(static_cast<char *>(base) + offset); }

// Device scratch of the stand-alone entry points, cached per stream (va_scratch.hip states the contract)
struct ScratchLease {
    void *ptr = nullptr;
    size_t bytes = 0;
    hipStream_t st = nullptr;
    int acquire(size_t need, hipStream_t stream);
    ~ScratchLease();
};
void scratch_release_cached(size_t keep_bytes);   // frees the cache when it holds more than keep_bytes (va_trim)
void scratch_purge_stream(hipStream_t st);        // frees the blocks cached for st (va_stream_destroy)
// va_test_hook_fill: -1 (off), or the byte that every scratch lease and every plane a pipeline allocates is filled
// with before use.  Initial value: $VA_TEST_FILL.
extern int g_test_fill;

#if defined(__HIPCC__)
// BORDER_REFLECT_101 with repeated reflection (kernel wider than the image)
__device__ __forceinline__ int reflect101(int p, int len)
{
    if (len == 1)
        return 0;
    while (p < 0 || p >= len)
        p = p < 0 ? -p : 2 * (len - 1) - p;
    return p;
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the points of curve k of a packed buffer: false when its offsets are not in order inside 0 .. npoints
__device__ __forceinline__ bool curve_range(const int64_t *__restrict__ point_off, int64_t k, int64_t npoints,
                                            int64_t &start, int64_t &n)
{
    const int64_t s = point_off[k], e = point_off[k + 1];
    if (!(s >= 0 && s <= e && e <= npoints))
        return false;
    start = s;
    n = e - s;
    return true;
}
// packed fp32: both halves of a register pair are independent values (v_pk_fma_f32)
typedef float f2 __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }
#endif

// ---- host-side kernels shared between translation units --------------------------------
// Gaussian taps (host): OpenCV's 8-bit fixed-point / float definitions. Return 0 or VA_ERR_*.
int gauss_ksize(double sigma, bool is_u8);
int gauss_taps_q8(double sigma, int *ksize, uint16_t *taps, int cap, int rule = VA_TAPS_CV4);
int gauss_taps_f32(double sigma, int *ksize, float *taps, int cap);
// the n double taps of getGaussianKernelBitExact(n, sigma > 0), before any rounding to float
void gauss_taps_f64(double sigma, int n, double *out);

// ---- launchers (each enqueues on `stream`, returns VA_OK or an error) -------------------
// Only what has callers in more than one file is declared here: the launchers the pipeline sequences, and what
// one op's file borrows from another's.  The launchers, workspace layouts and limits of an op are private to the
// file of its kernels, which also holds its extern "C" entry points.
constexpr int kMaxTaps = 255;  // by-value tap tables in the kernel arguments
struct TapsQ8 {
    int ksize;
    uint16_t t[kMaxTaps + 1];
};
struct TapsF32 {
    int ksize;
    float t[kMaxTaps + 1];
};

// fast float32 path: LDS-staged row pass + register-window column pass (1 or 3 channels)
bool gauss_f32_fast_supported(int w, int c, const TapsF32 &taps);
int launch_gauss_f32_fast(const float *src, float *dst, float *scratch, int n, int h, int w, int c,
                          const TapsF32 &taps, hipStream_t st);
// float32 path in two kernels (va_gauss_f32_fused.hip): [EMA background + |difference| + row pass]
// with the background state in registers, then a marching column pass.  bg == nullptr: plain blur.
#if defined(__HIPCC__)
// Workgroup barrier that orders LDS traffic only.  __syncthreads() also waits for every outstanding
// GLOBAL access of the wave (s_waitcnt vmcnt(0)): with prefetch loads in flight for a later step, or
// streaming stores behind every step, that wait exposes a memory round trip per barrier.
__device__ __forceinline__ void lds_barrier()
{
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
#endif
void gauss_f32_test_hook(int generic_columns);
bool gauss_f32_fused_supported(int h, int w, int c, const TapsF32 &taps);
int launch_gauss_f32_fused(const float *src, float *dst, float *scratch, const float *bg, float *bg_out,
                           int64_t n_seen, double rate, int n, int h, int w, int c, const TapsF32 &taps,
                           hipStream_t st, StageProfiler *prof = nullptr);
// fused single-channel u8 Gaussian (LDS-staged, dot4/dot2), radius <= 31; output either the
// blurred u8 frames (dst), and/or the thresholded bit mask (bits, blurred > thresh)
bool gauss_fused_supported(int w, int h, const TapsQ8 &taps);
int launch_gauss_fused_u8(const uint8_t *src, uint8_t *dst, uint32_t *bits, int thresh, int n,
                          int h, int w, const TapsQ8 &taps, hipStream_t st);
// the same contract on the matrix cores (Toeplitz products with v_mfma_i32_32x32x32_i8):
// taps <= 127, radius <= 16; preferred whenever it applies
bool gauss_mfma_supported(int w, int h, const TapsQ8 &taps);
// mask8_maxval > 0: dst receives the thresholded mask as bytes (maxval / 0) instead of the blur
int launch_gauss_mfma_u8(const uint8_t *src, uint8_t *dst, uint32_t *bits, int thresh, int n,
                         int h, int w, const TapsQ8 &taps, hipStream_t st, int mask8_maxval = 0);

// ---- the Gaussian plan (va_gauss.hip): the one place that chooses the kernel family, for the stand-alone
// calls and the pipeline alike.  Order of preference -- u8: the single pass on the matrix cores, the dot4/dot2
// single pass (both: one channel, `aligned`), the matrix-core kernel on reflected-padded planes, the generic
// two passes; f32: [EMA + row pass] + marching column pass (`aligned`), the fast passes, the generic passes.
enum class GaussFamily { None, U8Mfma, U8Dot, U8Planes, U8Generic, F32Fused, F32Fast, F32Generic };
struct GaussPlan {
    GaussFamily family;   // None: no blur (a pipeline with sigma <= 0)
    int dtype, h, w, c;
    int wp;               // U8Planes: the plane width
    TapsQ8 tq;            // u8 families
    TapsF32 tf;           // f32 families
    int ksize() const { return family == GaussFamily::None ? 0 : dtype == VA_U8 ? tq.ksize : tf.ksize; }
    // one kernel and no scratch; it can threshold and pack the bit mask in its epilogue
    bool single_pass() const { return family == GaussFamily::U8Mfma || family == GaussFamily::U8Dot; }
    bool byte_mask() const { return family == GaussFamily::U8Mfma; }     // ... or write it as 0 / maxval bytes
    bool folds_ema() const { return family == GaussFamily::F32Fused; }   // the f32 EMA update in the row pass
};
// aligned: the pointers suit the single-pass kernels (u8: src % 16, dst % 4; f32: src % 16); pipelines pass
// true and va_pipeline_run checks the caller's pointers at its top, every run (the launchers check again).  valu_hook (va_test_hook_gaussian_u8): the dot4/dot2 single pass in
// place of the matrix-core one (what it cannot take still goes to the planes).  force: U8Dot / U8Generic pin
// that family (the stand-alone test hooks; the launcher checks the shape).
int plan_gaussian(GaussPlan *g, int dtype, int h, int w, int c, double sigma, int tap_rule, bool aligned,
                  bool valu_hook = false, GaussFamily force = GaussFamily::None);
extern int g_gauss_u8_valu;    // what va_test_hook_gaussian_u8 set: the valu_hook of pipelines created from now on
size_t gauss_scratch_bytes(const GaussPlan &g, size_t n);    // device scratch of n frames (0: none)
const char *gauss_plan_name(const GaussPlan &g);             // the pipeline description's name of the family
// Enqueues the planned kernels and marks their stage on prof (F32Fused marks its row and column passes itself).
// bits: single pass only; mask8_maxval > 0: byte_mask only; bg: F32Fused's EMA, as in launch_gauss_f32_fused.
int launch_gaussian(const GaussPlan &g, const void *src, void *dst, uint32_t *bits, int thresh, int mask8_maxval,
                    void *scratch, int n, hipStream_t st, StageProfiler *prof, const float *bg = nullptr,
                    float *bg_out = nullptr, int64_t n_seen = 0, double rate = 0.0);

// recip_scratch: bg_scratch_bytes(n) bytes of device memory for the per-frame reciprocals of the
// division-free running mean of batches above 256 frames (nullptr: the plain-division kernel is used, as it
// is for n_seen + n > 2^53, where the division-free kernels' float64 frame counter stops being exact);
// mean_in_u8_range: the caller vouches that the running-mean state lies in [0, 255] (saturation-free kernel)
size_t bg_scratch_bytes(int n);
int launch_bg(int mode, int dtype, const void *frames, void *diff, void *state, int64_t n_seen,
              double rate, int n, size_t px, hipStream_t st, double *recip_scratch = nullptr,
              bool mean_in_u8_range = false);
// (va_synth.hip) four samples per thread, table-driven normalisation; false: shape not supported, nothing launched
bool launch_pointwise_u8_x4(const uint8_t *src, uint8_t *dst, size_t out_samples, int src_c, int mono, int normalize,
                            double fmin, double fmax, double alpha, double tmin, hipStream_t st);
// (n, h, w, c) interleaved u8 <-> (n, c, h, wp) planes padded to wp columns by reflection
int launch_channel_planes(const uint8_t *src, uint8_t *dst, int n, int h, int w, int wp, int c,
                          bool split, hipStream_t st);

// u8 (src > thresh) or (src != 0 when thresh < 0 ... see .hip) -> bit mask, and back
int launch_pack_bits(const uint8_t *src, uint32_t *bits, int n, int h, int w, int thresh,
                     hipStream_t st);
int launch_unpack_bits(const uint32_t *bits, uint8_t *dst, int n, int h, int w, int maxval,
                       hipStream_t st);

// structuring element as per-row horizontal spans (RECT/CROSS/ELLIPSE are all row-convex)
struct RowSpans {
    int ksize;
    int anchor;
    int8_t lo[64];  // first / last+1 column (relative to the window's left edge); lo>=hi: empty
    int8_t hi[64];
};
int make_row_spans(int shape, int ksize, RowSpans *out);
// scratch (n*h*w bytes, nullable): lets rectangular elements run as a row pass + a column pass
int launch_morph_u8(const uint8_t *src, uint8_t *dst, int n, int h, int w, int op,
                    const RowSpans &se, hipStream_t st, uint8_t *scratch = nullptr);
int launch_morph_bits(const uint32_t *src, uint32_t *dst, int n, int h, int w, int op,
                      const RowSpans &se, hipStream_t st);
// the whole op sequence in one kernel (register-streaming for one or two small rectangles,
// LDS-resident otherwise)
bool morph_fused_supported(int w, const RowSpans *se, int count);
int launch_morph_fused(const uint32_t *src, uint32_t *dst, int n, int h,
                       int w, const int *ops, const RowSpans *se, int count, hipStream_t st);

// connected components on bit masks; labels doubles as the union-find forest
// workspace of the entry points that label a u8 mask: its packed bits, then launch_ccl's workspace
struct CclLayout { size_t bits, rows, rows_bytes, total; };
CclLayout ccl_layout(int n, int h, int w);
size_t ccl_rows_workspace_bytes(int n, int h);   // launch_ccl's workspace (the caller owns the bit mask)
int launch_ccl(const uint32_t *bits, int32_t *labels, int32_t *counts, int n, int h, int w,
               int connectivity, void *workspace, size_t ws_bytes, int64_t *stats, int max_labels,
               hipStream_t st, StageProfiler *prof = nullptr,
               bool paint = true);
// the same in two halves: the labelling itself, and the write of the label image (+ per-label
// statistics), which reads only what the plan names -- the final bit mask, the run tables in the
// workspace (or the sparse forest words in the label image) -- and may run on another stream
struct CclPaintPlan {
    const uint32_t *bits;
    int32_t *labels;
    int n, h, w;          // n == 0: nothing to paint
    int64_t *stats;
    int max_labels;
    const int32_t *run_table, *row_off, *frame_mode;
    int table_stride, xcd_frames;
    int persistent_grid;   // > 0: paint with this many workgroups (multiple of 8), each walking several row blocks
};
int launch_ccl_front(const uint32_t *bits, int32_t *labels, int32_t *counts, int n, int h, int w,
                     int connectivity, void *workspace, size_t ws_bytes, int64_t *stats, int max_labels,
                     hipStream_t st, StageProfiler *prof, CclPaintPlan *plan);
int launch_ccl_paint(const CclPaintPlan &plan, hipStream_t st, StageProfiler *prof = nullptr);
// what the geodesic default start borrows from va_contours.hip (which states the arguments)
int launch_outline_labels(const uint32_t *bits, uint32_t *inv, int32_t *forest, int32_t *bg_labels, int32_t *counts,
                          void *rows_ws, size_t rows_bytes, int n, int h, int w, hipStream_t st);
int edge_label_words(int h, int w);
int launch_longest_external_start(const uint32_t *bits, const int32_t *forest, const int32_t *bg_labels,
                                  uint32_t *edge_bits, int n, int h, int w, unsigned long long *keys,
                                  int32_t *p1, hipStream_t st);
// cv2.resize for float32 frames (va_resize.hip), as the optical flow's pyramid calls it; mode 0 nearest, 1 linear,
// 2 cubic, 3 area, 4 lanczos4; scratch: resize_scratch_bytes
size_t resize_scratch_bytes(int sh, int sw, int dh, int dw);
// stage: Upload puts the tables into scratch with a blocking copy and enqueues nothing; Launch then enqueues the
// kernel on them without copying -- a caller that runs several geometries on one stream uploads every table first,
// into disjoint scratch, so that no copy can overtake a kernel still reading its tables
enum class ResizeStage { Both, Upload, Launch };
int launch_resize_f32(const float *src, float *dst, int n, int sh, int sw, int c, int dh, int dw, int mode,
                      void *scratch, hipStream_t st, ResizeStage stage = ResizeStage::Both);
// the largest coordinate the rasterisers of va_polygon.hip and va_compose.hip take
constexpr int64_t kPolyMaxCoord = VA_FILL_MAX_COORD;

}  // namespace va
