// va_api.hip -- the runtime plumbing of libvideoanalysis_hip.so and the fused pipeline (include/videoanalysis_hip.h)
//
// Host code only: the error message, the device and the entry prologue; memory, streams and events; the fused
// pipeline; the lazy RCCL binding.  Every op's entry points are in the file of its kernels.  No exception
// crosses the ABI; every failure sets the thread-local message returned by va_last_error().
#include <dlfcn.h>
#include <stdarg.h>
#include <stdlib.h>

#include <new>
#include <utility>

#include "va_common.h"

namespace va {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char *get_error() { return g_err; }

// One device per process (one process per GPU): va_init records it, and every
// entry point that allocates or launches selects it for the calling thread first -- hipSetDevice
// is per thread, so a worker thread that never called va_init would otherwise run on device 0.
static int g_device = -1;
static thread_local int tl_device = -1;
int enter_device()
{
    if (g_device >= 0 && tl_device != g_device) {
        VA_HIP(hipSetDevice(g_device));
        tl_device = g_device;
    }
    return VA_OK;
}

}  // namespace va

using namespace va;

struct va_pipeline {
    va_config cfg;
    size_t px;         // elements per frame (H*W*C)
    size_t frame_px;   // pixels per frame (H*W)
    int w32;
    void *bg_state;
    void *bg_state_alt;   // fused float32 EMA: the kernel writes the new state here, then the two swap
    bool bg_in_u8_range;  // running mean: every state value is known to lie in [0, 255]
    size_t bg_bytes;
    int64_t n_seen;
    double *bg_recip;  // per-frame reciprocals of the running mean's divisor
    void *diff;        // background-subtracted frames (cfg.dtype)
    void *blur;        // blurred frames when the caller does not ask for them (Gaussians with scratch)
    void *gscratch;    // Gaussian scratch: gauss_scratch_bytes(gauss, max_batch)
    // Mask ping-pong and labelling workspace exist twice ("slots") once va_pipeline_overlap is on: the
    // paint pass of batch k reads slot k % 2 on the side stream while the stages of batch k + 1 fill the
    // other one.  slot 1 is allocated by va_pipeline_overlap.
    uint32_t *bits[2][2];
    void *ccl_ws[2];
    size_t ccl_ws_bytes;
    size_t bits_bytes;
    bool overlap;
    int slot;                       // slot of the next overlapped run
    hipStream_t side;               // paint passes of overlapped runs
    int paint_grid;                 // workgroups of the persistent paint pass of overlapped runs (0: one per row block)
    hipEvent_t ev_front;            // labelling of the current batch done (main stream)
    hipEvent_t ev_paint[2];         // paint pass that read slot s done (side stream)
    bool paint_pending[2];          // ev_paint[s] has been recorded and may still be running
    const char *paint_lo[2], *paint_hi[2];     // label image written by that paint pass
    const char *pstat_lo[2], *pstat_hi[2];     // statistics written by that paint pass
    int32_t *labels_scratch;
    int32_t *counts_scratch;
    GaussPlan gauss;   // family None: no blur
    RowSpans se[VA_MAX_MORPH_OPS];
    char desc[160];
    StageProfiler *prof;
};

extern "C" {

// ------------------------------------------------------------------------------ runtime
const char *va_version(void) { return "videoanalysis_hip 0.1 (gfx950)"; }
const char *va_last_error(void) { return get_error(); }

int va_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess)
        return 0;
    return n;
}

int va_init(int device)
{
    int n = va_device_count();
    if (n <= 0) {
        set_error("va_init: no HIP device visible");
        return VA_ERR_NODEV;
    }
    VA_REQUIRE(device >= 0 && device < n, "va_init: device %d out of range [0,%d)", device, n);
    VA_REQUIRE(g_device < 0 || g_device == device,
               "va_init: this process already runs on device %d (one device per process)", g_device);
    VA_HIP(hipSetDevice(device));
    VA_HIP(hipFree(nullptr));  // force context creation
    g_device = device;
    tl_device = device;
    return VA_OK;
}

int va_trim(size_t keep_bytes)
{
    VA_ENTER();
    VA_REQUIRE(g_device >= 0, "va_trim: va_init has not run");
    hipMemPool_t pool;
    VA_HIP(hipDeviceGetDefaultMemPool(&pool, g_device));
    VA_HIP(hipDeviceSynchronize());
    scratch_release_cached(keep_bytes);      // the cached scratch blocks of the stand-alone calls
    VA_HIP(hipMemPoolTrimTo(pool, keep_bytes));
    return VA_OK;
}

int va_malloc(void **dev_ptr, size_t bytes)
{
    VA_ENTER();
    VA_REQUIRE(dev_ptr, "va_malloc: NULL out pointer");
    *dev_ptr = nullptr;
    if (bytes == 0)
        return VA_OK;
    VA_HIP(hipMalloc(dev_ptr, bytes));
    return VA_OK;
}
int va_free(void *dev_ptr)
{
    VA_ENTER();
    if (dev_ptr)
        VA_HIP(hipFree(dev_ptr));
    return VA_OK;
}
int va_host_alloc(void **host_ptr, size_t bytes)
{
    VA_ENTER();
    VA_REQUIRE(host_ptr, "va_host_alloc: NULL out pointer");
    *host_ptr = nullptr;
    if (bytes == 0)
        return VA_OK;
    VA_HIP(hipHostMalloc(host_ptr, bytes, hipHostMallocDefault));
    return VA_OK;
}
int va_host_free(void *host_ptr)
{
    VA_ENTER();
    if (host_ptr)
        VA_HIP(hipHostFree(host_ptr));
    return VA_OK;
}
// Host memory that is neither hipHostMalloc'ed nor registered is pageable.  Large asynchronous copies to pageable
// memory were seen to leave a span of the destination unwritten after hipStreamSynchronize (64 x 1080p float32 =
// 531 MB into a fresh NumPy array: 28 MB of zeros, tools/debug notes in DESIGN.md 13.10), so pageable transfers are
// blocking copies here -- ordered after the stream's earlier work, complete on return -- and only pinned memory is
// copied asynchronously.
static bool host_is_pinned(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();                  // (unregistered host memory: not an error for us)
        return false;
    }
    return a.type == hipMemoryTypeHost;
}
int va_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream)
{
    VA_ENTER();
    if (!bytes)
        return VA_OK;
    if (host_is_pinned(src)) {
        VA_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, as_stream(stream)));
    } else {
        VA_HIP(hipStreamSynchronize(as_stream(stream)));
        VA_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
    }
    return VA_OK;
}
int va_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream)
{
    VA_ENTER();
    if (!bytes)
        return VA_OK;
    if (host_is_pinned(dst)) {
        VA_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, as_stream(stream)));
    } else {
        VA_HIP(hipStreamSynchronize(as_stream(stream)));
        VA_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    }
    return VA_OK;
}
int va_memcpy_d2d(void *dst, const void *src, size_t bytes, void *stream)
{
    VA_ENTER();
    if (bytes)
        VA_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, as_stream(stream)));
    return VA_OK;
}
int va_memset(void *dst, int value, size_t bytes, void *stream)
{
    VA_ENTER();
    if (bytes)
        VA_HIP(hipMemsetAsync(dst, value, bytes, as_stream(stream)));
    return VA_OK;
}
int va_stream_sync(void *stream)
{
    VA_ENTER();
    VA_HIP(hipStreamSynchronize(as_stream(stream)));
    return VA_OK;
}

int va_stream_create(void **stream_out)
{
    VA_ENTER();
    VA_REQUIRE(stream_out, "va_stream_create: NULL argument");
    hipStream_t s;
    VA_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *stream_out = (void *)s;
    return VA_OK;
}
int va_stream_destroy(void *stream)
{
    VA_ENTER();
    if (!stream)
        return VA_OK;
    // the cache is keyed by the handle, and a later stream may get the same one: its blocks go with it
    VA_HIP(hipStreamSynchronize(as_stream(stream)));
    scratch_purge_stream(as_stream(stream));
    VA_HIP(hipStreamDestroy(as_stream(stream)));
    return VA_OK;
}
int va_event_create(void **event_out)
{
    VA_ENTER();
    VA_REQUIRE(event_out, "va_event_create: NULL argument");
    hipEvent_t e;
    VA_HIP(hipEventCreate(&e));
    *event_out = (void *)e;
    return VA_OK;
}
int va_event_destroy(void *event)
{
    VA_ENTER();
    if (event)
        VA_HIP(hipEventDestroy((hipEvent_t)event));
    return VA_OK;
}
int va_event_record(void *event, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(event, "va_event_record: NULL event");
    VA_HIP(hipEventRecord((hipEvent_t)event, as_stream(stream)));
    return VA_OK;
}
int va_stream_wait_event(void *stream, void *event)
{
    VA_ENTER();
    VA_REQUIRE(event, "va_stream_wait_event: NULL event");
    VA_HIP(hipStreamWaitEvent(as_stream(stream), (hipEvent_t)event, 0));
    return VA_OK;
}
int va_event_sync(void *event)
{
    VA_ENTER();
    VA_REQUIRE(event, "va_event_sync: NULL event");
    VA_HIP(hipEventSynchronize((hipEvent_t)event));
    return VA_OK;
}
int va_event_elapsed_ms(void *start_event, void *stop_event, float *ms_out)
{
    VA_ENTER();
    VA_REQUIRE(start_event && stop_event && ms_out, "va_event_elapsed_ms: NULL argument");
    VA_HIP(hipEventElapsedTime(ms_out, (hipEvent_t)start_event, (hipEvent_t)stop_event));
    return VA_OK;
}

// test hook: -1 = off, 0..255 = every scratch lease and every plane of a pipeline created from now on starts
// out filled with that byte (undefined memory that is not zero)
int va_test_hook_fill(int byte)
{
    VA_REQUIRE(byte >= -1 && byte <= 255, "va_test_hook_fill: byte must be -1 (off) or 0..255");
    g_test_fill = byte;
    return VA_OK;
}

// ------------------------------------------------------------------------------ pipeline
static int pipeline_free(va_pipeline *p)
{
    void *ptrs[] = {p->bg_state, p->bg_state_alt, p->bg_recip, p->diff, p->blur, p->gscratch,
                    p->bits[0][0], p->bits[0][1], p->bits[1][0], p->bits[1][1],
                    p->ccl_ws[0], p->ccl_ws[1], p->labels_scratch, p->counts_scratch};
    for (void *q : ptrs)
        if (q)
            (void)hipFree(q);
    if (p->side)
        (void)hipStreamDestroy(p->side);
    if (p->ev_front)
        (void)hipEventDestroy(p->ev_front);
    for (hipEvent_t e : p->ev_paint)
        if (e)
            (void)hipEventDestroy(e);
    if (p->prof) {
        for (int i = 0; i < StageProfiler::kMaxMarks; i++)
            if (p->prof->created[i])
                (void)hipEventDestroy(p->prof->ev[i]);
        delete p->prof;
    }
    delete p;
    return VA_OK;
}

int va_pipeline_create(const va_config *cfg, va_pipeline_t **out)
{
    VA_ENTER();
    VA_REQUIRE(cfg && out, "va_pipeline_create: NULL argument");
    *out = nullptr;
    VA_REQUIRE(cfg->struct_size == (int32_t)sizeof(va_config),
               "va_pipeline_create: va_config.struct_size %d != %zu (ABI mismatch)",
               cfg->struct_size, sizeof(va_config));
    VA_REQUIRE(cfg->width > 0 && cfg->height > 0 && (cfg->channels == 1 || cfg->channels == 3),
               "va_pipeline_create: bad frame format %dx%dx%d", cfg->width, cfg->height,
               cfg->channels);
    VA_REQUIRE(cfg->dtype == VA_U8 || cfg->dtype == VA_F32, "va_pipeline_create: bad dtype %d",
               cfg->dtype);
    VA_REQUIRE(cfg->max_batch > 0, "va_pipeline_create: max_batch must be > 0");
    VA_REQUIRE(cfg->bg_mode >= VA_BG_NONE && cfg->bg_mode <= VA_BG_STATIC,
               "va_pipeline_create: bad bg_mode %d", cfg->bg_mode);
    VA_REQUIRE(cfg->morph_count >= 0 && cfg->morph_count <= VA_MAX_MORPH_OPS,
               "va_pipeline_create: morph_count %d out of range", cfg->morph_count);
    VA_REQUIRE(cfg->connectivity == 0 || cfg->connectivity == 4 || cfg->connectivity == 8,
               "va_pipeline_create: connectivity must be 0, 4 or 8");
    VA_REQUIRE(cfg->tap_rule == VA_TAPS_CV4 || cfg->tap_rule == VA_TAPS_CV3,
               "va_pipeline_create: tap_rule must be VA_TAPS_CV4 or VA_TAPS_CV3");
    const bool masks = cfg->thresh >= 0;
    if (cfg->dtype == VA_F32) {
        VA_REQUIRE(!masks, "va_pipeline_create: threshold/labelling need uint8 frames");
        VA_REQUIRE(cfg->bg_mode == VA_BG_NONE || cfg->bg_mode == VA_BG_EMA,
                   "va_pipeline_create: float32 frames support bg_mode NONE/EMA only");
    }
    if (masks)
        VA_REQUIRE(cfg->channels == 1, "va_pipeline_create: threshold/labelling need 1 channel");
    else
        VA_REQUIRE(cfg->morph_count == 0 && cfg->connectivity == 0,
                   "va_pipeline_create: morphology/labelling need a threshold (thresh >= 0)");
    VA_REQUIRE((size_t)cfg->width * cfg->height < kMaxFramePixels,
               "va_pipeline_create: frames of %dx%d exceed the supported 2^29 pixels (the kernels'"
               " 32-bit buffer descriptors address h*w*4 bytes)", cfg->width, cfg->height);

    va_pipeline *p = new (std::nothrow) va_pipeline();
    if (!p) {
        set_error("va_pipeline_create: out of host memory");
        return VA_ERR_NOMEM;
    }
    memset(p, 0, sizeof(*p));
    p->cfg = *cfg;
    if (p->cfg.maxval <= 0 || p->cfg.maxval > 255)
        p->cfg.maxval = 255;
    p->frame_px = (size_t)cfg->width * cfg->height;
    p->px = p->frame_px * cfg->channels;
    p->w32 = words_per_row(cfg->width);
    const size_t esz = cfg->dtype == VA_U8 ? 1 : 4;
    const size_t nb = (size_t)cfg->max_batch;
    int rc = VA_OK;
#define PIPE_TRY(expr)                    \
    do {                                  \
        rc = (expr);                      \
        if (rc) {                         \
            pipeline_free(p);             \
            return rc;                    \
        }                                 \
    } while (0)
#define PIPE_MALLOC(ptr, bytes)                                                          \
    do {                                                                                 \
        hipError_t _e = hipMalloc((void **)&(ptr), (bytes));                             \
        if (_e != hipSuccess) {                                                          \
            set_error("va_pipeline_create: hipMalloc(%zu) failed: %s", (size_t)(bytes),  \
                      hipGetErrorString(_e));                                            \
            pipeline_free(p);                                                            \
            return VA_ERR_NOMEM;                                                         \
        }                                                                                \
        if (g_test_fill >= 0)                                                            \
            (void)hipMemset((ptr), g_test_fill, (bytes));                                \
    } while (0)

    if (cfg->sigma > 0)
        PIPE_TRY(plan_gaussian(&p->gauss, cfg->dtype, cfg->height, cfg->width, cfg->channels, cfg->sigma,
                               cfg->tap_rule, true, g_gauss_u8_valu != 0));
    for (int i = 0; i < cfg->morph_count; i++) {
        if (cfg->morph_op[i] != VA_MORPH_ERODE && cfg->morph_op[i] != VA_MORPH_DILATE) {
            set_error("va_pipeline_create: bad morph_op[%d]=%d", i, cfg->morph_op[i]);
            pipeline_free(p);
            return VA_ERR_INVALID;
        }
        PIPE_TRY(make_row_spans(cfg->morph_shape[i], cfg->morph_ksize[i], &p->se[i]));
    }
    if (cfg->bg_mode != VA_BG_NONE) {
        p->bg_bytes = p->px * (cfg->bg_mode == VA_BG_EMA ? sizeof(float) : sizeof(double));
        PIPE_MALLOC(p->bg_state, p->bg_bytes);
        if (p->gauss.folds_ema() && cfg->bg_mode == VA_BG_EMA)
            PIPE_MALLOC(p->bg_state_alt, p->bg_bytes);
        p->bg_in_u8_range = true;                        // (zeros)
        hipError_t e = hipMemset(p->bg_state, 0, p->bg_bytes);
        if (e != hipSuccess) {
            set_error("va_pipeline_create: hipMemset failed: %s", hipGetErrorString(e));
            pipeline_free(p);
            return VA_ERR_HIP;
        }
        if (!p->gauss.folds_ema())      // (the fused float path never materialises the difference image)
            PIPE_MALLOC(p->diff, nb * p->px * esz);
        if (cfg->bg_mode == VA_BG_MEAN)
            PIPE_MALLOC(p->bg_recip, bg_scratch_bytes(cfg->max_batch));
    }
    if (cfg->sigma > 0 && !p->gauss.single_pass()) {
        PIPE_MALLOC(p->gscratch, gauss_scratch_bytes(p->gauss, nb));
        PIPE_MALLOC(p->blur, nb * p->px * esz);
    }
    if (masks) {
        size_t bb = Carve::up(nb * cfg->height * p->w32 * sizeof(uint32_t));
        p->bits_bytes = bb;
        PIPE_MALLOC(p->bits[0][0], bb);
        PIPE_MALLOC(p->bits[0][1], bb);
        if (cfg->connectivity) {
            p->ccl_ws_bytes = ccl_rows_workspace_bytes(cfg->max_batch, cfg->height);
            PIPE_MALLOC(p->ccl_ws[0], p->ccl_ws_bytes);
            PIPE_MALLOC(p->counts_scratch, Carve::up(nb * sizeof(int32_t)));
            // forest / label scratch for runs that do not ask for the label image (counts only:
            // sparse forest words, never painted; stats only: painted here).  Allocated now so
            // that an out-of-memory shows at create time and no run ever calls hipMalloc.
            PIPE_MALLOC(p->labels_scratch, nb * p->frame_px * sizeof(int32_t));
        }
    }
    snprintf(p->desc, sizeof(p->desc), "bg=%d gauss=%s(ksize=%d) thresh=%d morph=%d ccl=%d", cfg->bg_mode,
             gauss_plan_name(p->gauss), p->gauss.ksize(), cfg->thresh, cfg->morph_count, cfg->connectivity);
#undef PIPE_TRY
#undef PIPE_MALLOC
    *out = p;
    return VA_OK;
}

int va_pipeline_destroy(va_pipeline_t *p)
{
    VA_ENTER();
    if (!p)
        return VA_OK;
    (void)hipDeviceSynchronize();
    return pipeline_free(p);
}

const char *va_pipeline_describe(const va_pipeline_t *p) { return p ? p->desc : ""; }

int va_pipeline_overlap(va_pipeline_t *p, int enable)
{
    VA_ENTER();
    VA_REQUIRE(p, "va_pipeline_overlap: NULL pipeline");
    VA_HIP(hipDeviceSynchronize());                  // no paint pass in flight across the switch
    p->paint_pending[0] = p->paint_pending[1] = false;
    p->slot = 0;
    if (!enable) {
        p->overlap = false;
        return VA_OK;
    }
    VA_REQUIRE(p->cfg.thresh >= 0 && p->cfg.connectivity,
               "va_pipeline_overlap: only a labelling pipeline has a paint pass to overlap");
#define OV_MALLOC(ptr, bytes)                                                               \
    do {                                                                                    \
        if (!(ptr)) {                                                                       \
            hipError_t _e = hipMalloc((void **)&(ptr), (bytes));                            \
            if (_e != hipSuccess) {                                                         \
                (ptr) = nullptr;                                                            \
                set_error("va_pipeline_overlap: hipMalloc(%zu) failed: %s", (size_t)(bytes), \
                          hipGetErrorString(_e));                                           \
                return VA_ERR_NOMEM;                                                        \
            }                                                                               \
            if (g_test_fill >= 0)                                                           \
                (void)hipMemset((ptr), g_test_fill, (bytes));                               \
        }                                                                                   \
    } while (0)
    OV_MALLOC(p->bits[1][0], p->bits_bytes);
    OV_MALLOC(p->bits[1][1], p->bits_bytes);
    OV_MALLOC(p->ccl_ws[1], p->ccl_ws_bytes);
#undef OV_MALLOC
    if (!p->side) {
        // lowest priority: the dispatcher places the workgroups of the caller's stream (VALU-/latency-
        // bound kernels with large register and LDS footprints) first, and the paint pass -- tens of
        // thousands of small store-only workgroups that would otherwise take every slot that frees
        // up -- fills what is left of the CUs and of the HBM bandwidth.  enable == 2: default priority
        // (kept for A/B measurements).
        int lo = 0, hi = 0;
        VA_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));        // lo = numerically greatest = least urgent
        VA_HIP(hipStreamCreateWithPriority(&p->side, hipStreamNonBlocking, enable == 2 ? 0 : lo));
    }
    if (!p->ev_front)
        VA_HIP(hipEventCreateWithFlags(&p->ev_front, hipEventDisableTiming));
    for (int s = 0; s < 2; s++)
        if (!p->ev_paint[s])
            VA_HIP(hipEventCreateWithFlags(&p->ev_paint[s], hipEventDisableTiming));
    {
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g_device);
        // persistent paint pass, 4 workgroups per CU: bounded footprint beside the next batch's kernels
        // (measured best of 0 = one workgroup per row block, 1, 2, 4, 8: tools/overlap_probe.py);
        // $VA_PAINT_WGS_PER_CU overrides it for such measurements
        const char *e = getenv("VA_PAINT_WGS_PER_CU");
        const int per_cu = e ? atoi(e) : 4;
        p->paint_grid = per_cu > 0 ? ((cus * per_cu + 7) / 8) * 8 : 0;
    }
    p->overlap = true;
    return VA_OK;
}

int va_pipeline_fence(va_pipeline_t *p, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(p, "va_pipeline_fence: NULL pipeline");
    for (int s = 0; s < 2; s++)
        if (p->paint_pending[s])
            VA_HIP(hipStreamWaitEvent(as_stream(stream), p->ev_paint[s], 0));
    return VA_OK;
}

size_t va_bg_state_bytes(const va_pipeline_t *p) { return p ? p->bg_bytes : 0; }

int va_bg_get_state(va_pipeline_t *p, void *state_host, size_t bytes, int64_t *n_seen)
{
    VA_ENTER();
    VA_REQUIRE(p, "va_bg_get_state: NULL pipeline");
    if (n_seen)
        *n_seen = p->n_seen;
    if (state_host) {
        VA_REQUIRE(bytes == p->bg_bytes, "va_bg_get_state: %zu bytes given, state is %zu", bytes,
                   p->bg_bytes);
        if (bytes) {
            VA_HIP(hipDeviceSynchronize());
            VA_HIP(hipMemcpy(state_host, p->bg_state, bytes, hipMemcpyDeviceToHost));
        }
    }
    return VA_OK;
}

int va_bg_set_state(va_pipeline_t *p, const void *state_host, size_t bytes, int64_t n_seen)
{
    VA_ENTER();
    VA_REQUIRE(p, "va_bg_set_state: NULL pipeline");
    VA_REQUIRE(n_seen >= 0, "va_bg_set_state: n_seen must be >= 0");
    if (state_host) {
        VA_REQUIRE(bytes == p->bg_bytes, "va_bg_set_state: %zu bytes given, state is %zu", bytes,
                   p->bg_bytes);
        if (bytes) {
            VA_HIP(hipDeviceSynchronize());
            VA_HIP(hipMemcpy(p->bg_state, state_host, bytes, hipMemcpyHostToDevice));
        }
        p->bg_in_u8_range = false;
        if (p->cfg.bg_mode == VA_BG_MEAN) {              // (float64 state)
            const double *m = static_cast<const double *>(state_host);
            bool ok = true;
            for (size_t i = 0; i < bytes / sizeof(double) && ok; i++)
                ok = m[i] >= 0.0 && m[i] <= 255.0;       // (false for NaN)
            p->bg_in_u8_range = ok;
        }
    } else if (p->bg_bytes) {
        VA_HIP(hipDeviceSynchronize());
        VA_HIP(hipMemset(p->bg_state, 0, p->bg_bytes));
        p->bg_in_u8_range = true;
    }
    p->n_seen = n_seen;
    return VA_OK;
}

int va_pipeline_run(va_pipeline_t *p, const void *frames, int n, void *filtered_out,
                    uint8_t *mask_out, int32_t *labels_out, int32_t *counts_out,
                    int64_t *stats_out, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(p && frames, "va_pipeline_run: NULL argument");
    const va_config &c = p->cfg;
    VA_REQUIRE(n >= 0 && n <= c.max_batch, "va_pipeline_run: n=%d exceeds max_batch=%d", n,
               c.max_batch);
    if (n == 0)
        return VA_OK;
    hipStream_t st = as_stream(stream);
    const bool masks = c.thresh >= 0;
    VA_REQUIRE(masks || !(mask_out || labels_out || counts_out || stats_out),
               "va_pipeline_run: mask/label outputs requested but the pipeline has no threshold");
    VA_REQUIRE(c.connectivity || !(labels_out || counts_out || stats_out),
               "va_pipeline_run: label outputs requested but connectivity == 0");
    VA_REQUIRE(!stats_out || c.max_labels > 0, "va_pipeline_run: stats_out needs max_labels > 0");
    // 8-bit frames, single-pass Gaussian planned (with aligned = true, at creation): what its launcher will ask
    // of the caller's pointers is asked here, before the background model is updated or anything is counted.
    // With a background model the Gaussian reads the pipeline's own difference buffer, not frames_dev.
    if (p->gauss.single_pass()) {
        VA_REQUIRE(c.bg_mode != VA_BG_NONE || reinterpret_cast<uintptr_t>(frames) % 16 == 0,
                   "va_pipeline_run: frames_dev must be 16-byte aligned for the %s Gaussian of a pipeline "
                   "without a background model", gauss_plan_name(p->gauss));
        VA_REQUIRE(!p->gauss.byte_mask() || !filtered_out || reinterpret_cast<uintptr_t>(filtered_out) % 4 == 0,
                   "va_pipeline_run: filtered_out_dev must be 4-byte aligned for the %s Gaussian",
                   gauss_plan_name(p->gauss));
    }
    const size_t esz = c.dtype == VA_U8 ? 1 : 4;
    int rc;
    const void *cur = frames;
    StageProfiler *prof = (p->prof && p->prof->enabled && p->prof->runs++ % p->prof->every == 0) ? p->prof : nullptr;
    mark(prof, nullptr, st);

    // float32 frames: background update, difference and row pass in one kernel, then the columns
    // (16-byte aligned frame pointers: a contract of float32 pipelines, see the header)
    if (p->gauss.folds_ema()) {
        VA_REQUIRE(reinterpret_cast<uintptr_t>(frames) % 16 == 0 &&
                       (!filtered_out || reinterpret_cast<uintptr_t>(filtered_out) % 16 == 0),
                   "va_pipeline_run: float32 pipelines need 16-byte aligned frames_dev / filtered_out_dev "
                   "(hipMalloc'ed buffers and whole-frame offsets into them are)");
        void *dst = filtered_out ? filtered_out : p->blur;
        const bool ema = c.bg_mode == VA_BG_EMA;
        rc = launch_gaussian(p->gauss, frames, dst, nullptr, -1, 0, p->gscratch, n, st, prof,
                             ema ? (const float *)p->bg_state : nullptr, ema ? (float *)p->bg_state_alt : nullptr,
                             p->n_seen, (double)c.bg_rate);
        if (rc)
            return rc;
        if (ema && n > 0) {
            std::swap(p->bg_state, p->bg_state_alt);      // (stream order: later runs read what this one wrote)
            p->n_seen += n;
        }
        return VA_OK;
    }
    // 1. background subtraction (temporal, in frame order)
    if (c.bg_mode != VA_BG_NONE) {
        rc = launch_bg(c.bg_mode, c.dtype, cur, p->diff, p->bg_state, p->n_seen, (double)c.bg_rate,
                       n, p->px, st, p->bg_recip, p->bg_in_u8_range);
        if (rc)
            return rc;
        p->n_seen += n;
        cur = p->diff;
        mark(prof, "bg", st);
    }

    // Overlapped runs (va_pipeline_overlap): this batch's masks and run tables live in slot `slot`; the
    // paint pass that last read that slot (two runs ago) must be done before anything writes it.
    const bool want_ccl = masks && c.connectivity && (labels_out || counts_out || stats_out);
    const bool defer_paint = p->overlap && want_ccl && (labels_out != nullptr || stats_out != nullptr);
    const int slot = defer_paint ? p->slot : 0;
    if (p->overlap && p->paint_pending[slot])
        VA_HIP(hipStreamWaitEvent(st, p->ev_paint[slot], 0));
    uint32_t *const *bits = p->bits[slot];

    // 2. Gaussian blur (+ threshold + bit packing when fused)
    bool have_bits = false;
    if (c.sigma > 0) {
        if (p->gauss.byte_mask() && masks && mask_out && !filtered_out && c.morph_count == 0 && !want_ccl &&
            reinterpret_cast<uintptr_t>(mask_out) % 4 == 0) {
            // the chain ends at FilterThreshold's uint8 mask (BASELINE configs[1]): the Gaussian's
            // epilogue writes the 0 / maxval bytes itself -- no bit mask, no unpack pass
            return launch_gaussian(p->gauss, cur, mask_out, nullptr, c.thresh, c.maxval, p->gscratch, n, st, prof);
        }
        uint32_t *gbits = masks && p->gauss.single_pass() ? bits[0] : nullptr;
        void *dst = filtered_out ? filtered_out : p->blur;      // (a single pass has no blur buffer)
        rc = launch_gaussian(p->gauss, cur, dst, gbits, c.thresh, 0, p->gscratch, n, st, prof);
        if (rc)
            return rc;
        have_bits = gbits != nullptr;
        cur = dst;  // may be NULL after a single pass; not needed any more when have_bits
    } else if (filtered_out) {
        VA_HIP(hipMemcpyAsync(filtered_out, cur, (size_t)n * p->px * esz, hipMemcpyDeviceToDevice,
                              st));
    }
    if (!masks)
        return VA_OK;

    // 3. threshold -> bit mask
    int b = 0;
    if (!have_bits) {
        rc = launch_pack_bits((const uint8_t *)cur, bits[0], n, c.height, c.width, c.thresh, st);
        if (rc)
            return rc;
        mark(prof, "threshold_pack", st);
    }
    // 4. morphology on bits (one fused kernel when the sequence allows it)
    int32_t *labels = nullptr;
    if (want_ccl) {
        labels = labels_out ? labels_out : p->labels_scratch;
    }
    if (c.morph_count > 0 && morph_fused_supported(c.width, p->se, c.morph_count)) {
        rc = launch_morph_fused(bits[b], bits[b ^ 1], n, c.height, c.width, c.morph_op, p->se,
                                c.morph_count, st);
        if (rc)
            return rc;
        b ^= 1;
        mark(prof, "morph_fused", st);
    } else {
        for (int i = 0; i < c.morph_count; i++) {
            rc = launch_morph_bits(bits[b], bits[b ^ 1], n, c.height, c.width, c.morph_op[i],
                                   p->se[i], st);
            if (rc)
                return rc;
            b ^= 1;
            mark(prof, c.morph_op[i] == VA_MORPH_DILATE ? "morph_dilate" : "morph_erode", st);
        }
    }
    if (mask_out) {
        rc = launch_unpack_bits(bits[b], mask_out, n, c.height, c.width, c.maxval, st);
        if (rc)
            return rc;
        mark(prof, "mask_unpack", st);
    }
    // 5. labelling (+ statistics)
    if (want_ccl) {
        // counts alone come out of the labelling kernels; the label image (the chain's largest
        // write) is painted only for callers that read it or the per-label statistics
        const bool paint = labels_out != nullptr || stats_out != nullptr;
        int32_t *counts = counts_out ? counts_out : p->counts_scratch;
        // The labelling kernels may write the label image (sparse forest words: chip-wide passes,
        // frames beyond the LDS run table); a paint pass still in flight on the side stream that
        // writes the same image -- the caller reuses one label buffer for consecutive batches --
        // has to finish first.  Callers that alternate two label buffers never wait here.
        const char *lo = (const char *)labels, *hi = lo + (size_t)n * p->frame_px * sizeof(int32_t);
        const char *slo = (const char *)stats_out,
                   *shi = slo + (stats_out ? (size_t)n * c.max_labels * VA_STATS_STRIDE * sizeof(int64_t) : 0);
        for (int s = 0; s < 2 && p->overlap; s++)
            if (p->paint_pending[s] &&
                ((lo < p->paint_hi[s] && p->paint_lo[s] < hi) || (slo < p->pstat_hi[s] && p->pstat_lo[s] < shi)))
                VA_HIP(hipStreamWaitEvent(st, p->ev_paint[s], 0));
        if (!defer_paint) {
            rc = launch_ccl(bits[b], labels, counts, n, c.height, c.width, c.connectivity, p->ccl_ws[0],
                            p->ccl_ws_bytes, stats_out, c.max_labels, st, prof, paint);
            if (rc)
                return rc;
        } else {
            CclPaintPlan plan;
            rc = launch_ccl_front(bits[b], labels, counts, n, c.height, c.width, c.connectivity, p->ccl_ws[slot],
                                  p->ccl_ws_bytes, stats_out, c.max_labels, st, prof, &plan);
            if (rc)
                return rc;
            VA_HIP(hipEventRecord(p->ev_front, st));
            VA_HIP(hipStreamWaitEvent(p->side, p->ev_front, 0));
            mark(prof, nullptr, p->side);                // (start of the side stream's part of this run)
            plan.persistent_grid = p->paint_grid;
            rc = launch_ccl_paint(plan, p->side, prof);
            if (rc)
                return rc;
            VA_HIP(hipEventRecord(p->ev_paint[slot], p->side));
            p->paint_pending[slot] = true;
            p->paint_lo[slot] = lo;
            p->paint_hi[slot] = hi;
            p->pstat_lo[slot] = slo;
            p->pstat_hi[slot] = shi;
            p->slot = slot ^ 1;
        }
    }
    return VA_OK;
}

int va_pipeline_profile(va_pipeline_t *p, int enable)
{
    VA_ENTER();
    VA_REQUIRE(p, "va_pipeline_profile: NULL pipeline");
    if (!p->prof) {
        p->prof = new (std::nothrow) StageProfiler();
        if (!p->prof) {
            set_error("va_pipeline_profile: out of host memory");
            return VA_ERR_NOMEM;
        }
    }
    p->prof->enabled = enable != 0;
    p->prof->every = enable > 1 ? enable : 1;
    p->prof->runs = 0;
    p->prof->n = 0;
    p->prof->dropped = 0;
    return VA_OK;
}

int va_pipeline_stage_times(va_pipeline_t *p, int capacity, char *names, double *total_ms,
                            int32_t *launches, int *nstages_out)
{
    VA_ENTER();
    VA_REQUIRE(p && names && total_ms && launches && nstages_out && capacity > 0,
               "va_pipeline_stage_times: bad argument");
    *nstages_out = 0;
    if (!p->prof || p->prof->n == 0)
        return VA_OK;
    StageProfiler &pr = *p->prof;
    for (int i = 0; i < pr.n; i++)                  // (marks of overlapped runs sit on two streams)
        VA_HIP(hipEventSynchronize(pr.ev[i]));
    int ns = 0;
    for (int i = 1; i < pr.n; i++) {
        if (!pr.name[i])
            continue;  // start-of-run marker
        float ms = 0.f;
        VA_HIP(hipEventElapsedTime(&ms, pr.ev[i - 1], pr.ev[i]));
        int k = 0;
        for (; k < ns; k++)
            if (strncmp(names + (size_t)k * 32, pr.name[i], 31) == 0)
                break;
        if (k == ns) {
            if (ns == capacity)
                continue;
            strncpy(names + (size_t)k * 32, pr.name[i], 31);
            names[(size_t)k * 32 + 31] = 0;
            total_ms[k] = 0;
            launches[k] = 0;
            ns++;
        }
        total_ms[k] += ms;
        launches[k] += 1;
    }
    *nstages_out = ns;
    return VA_OK;
}

// ------------------------------------------------------------------------------ RCCL (lazy)
struct NcclId {
    char internal[128];
};
namespace {
struct NcclApi {
    void *handle = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, NcclId, int) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
}  // namespace
static NcclApi g_nccl;

static int nccl_load()
{
    if (g_nccl.handle)
        return VA_OK;
    const char *names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
    void *h = nullptr;
    for (const char *nm : names)
        if ((h = dlopen(nm, RTLD_NOW | RTLD_GLOBAL)))
            break;
    if (!h) {
        set_error("RCCL not found: %s", dlerror());
        return VA_ERR_NODEV;
    }
    g_nccl.GetUniqueId = (int (*)(void *))dlsym(h, "ncclGetUniqueId");
    g_nccl.CommInitRank = (int (*)(void **, int, NcclId, int))dlsym(h, "ncclCommInitRank");
    g_nccl.AllGather =
        (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(h, "ncclAllGather");
    g_nccl.CommDestroy = (int (*)(void *))dlsym(h, "ncclCommDestroy");
    g_nccl.GetErrorString = (const char *(*)(int))dlsym(h, "ncclGetErrorString");
    if (!g_nccl.GetUniqueId || !g_nccl.CommInitRank || !g_nccl.AllGather || !g_nccl.CommDestroy) {
        set_error("RCCL symbols missing in librccl.so");
        dlclose(h);
        return VA_ERR_NODEV;
    }
    g_nccl.handle = h;
    return VA_OK;
}
#define VA_NCCL(call)                                                                       \
    do {                                                                                    \
        int _r = (call);                                                                    \
        if (_r != 0) {                                                                      \
            set_error("%s failed: %s", #call,                                               \
                      g_nccl.GetErrorString ? g_nccl.GetErrorString(_r) : "rccl error");    \
            return VA_ERR_HIP;                                                              \
        }                                                                                   \
    } while (0)

int va_comm_unique_id(uint8_t id_out[128])
{
    VA_ENTER();
    VA_REQUIRE(id_out, "va_comm_unique_id: NULL argument");
    int rc = nccl_load();
    if (rc)
        return rc;
    NcclId id;
    VA_NCCL(g_nccl.GetUniqueId(&id));
    memcpy(id_out, id.internal, 128);
    return VA_OK;
}

int va_comm_init(void **comm_out, int world_size, int rank, const uint8_t id[128])
{
    VA_ENTER();
    VA_REQUIRE(comm_out && id, "va_comm_init: NULL argument");
    VA_REQUIRE(world_size >= 1 && rank >= 0 && rank < world_size, "va_comm_init: bad rank %d/%d",
               rank, world_size);
    int rc = nccl_load();
    if (rc)
        return rc;
    NcclId nid;
    memcpy(nid.internal, id, 128);
    VA_NCCL(g_nccl.CommInitRank(comm_out, world_size, nid, rank));
    return VA_OK;
}

int va_gather_counts(void *comm, const int32_t *send, int32_t *recv, int count_per_rank,
                     void *stream)
{
    VA_ENTER();
    VA_REQUIRE(comm && send && recv && count_per_rank >= 0, "va_gather_counts: bad argument");
    int rc = nccl_load();
    if (rc)
        return rc;
    VA_NCCL(g_nccl.AllGather(send, recv, (size_t)count_per_rank, /*ncclInt32*/ 2, comm,
                             as_stream(stream)));
    return VA_OK;
}

int va_comm_destroy(void *comm)
{
    VA_ENTER();
    if (!comm)
        return VA_OK;
    int rc = nccl_load();
    if (rc)
        return rc;
    VA_NCCL(g_nccl.CommDestroy(comm));
    return VA_OK;
}

}  // extern "C"
