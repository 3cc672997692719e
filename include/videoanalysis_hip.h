/*
 * videoanalysis_hip.h -- C ABI of libvideoanalysis_hip.so (MI355X / gfx950)
 *
 * The drop-in boundary for the data-parallel hot path of david-zwicker/video-analysis:
 * the `video.filters` chain (background subtraction, Gaussian blur, threshold, morphology)
 * and the per-frame `video.analysis` image ops (labelling, areas, bounding boxes, moments).
 *
 * The reference is pure Python and has no FFI of its own; its boundary for this path is the
 * `VideoFilterBase._process_frame(frame) -> frame` protocol (video/io/base.py:182-189,
 * 369-380) plus the free functions of the video/analysis modules.  Each entry point below names the
 * reference call it replaces (paths relative to the reference checkout).  The ctypes stubs a
 * maintainer would add to the reference are shown in INTEGRATION.md; the build's own Python
 * host (video-analysis_amd/video/_hip.py) binds exactly these symbols.
 *
 * Conventions
 *   - plain C types only; every function returns 0 (VA_OK) or a negative errno-style code and
 *     never throws; va_last_error() gives the message of the calling thread's last failure.
 *   - "dev" pointers are HIP device pointers owned by the caller (e.g. torch tensors'
 *     data_ptr()); `stream` is a hipStream_t passed as void* (NULL = default stream).  All
 *     kernels are enqueued asynchronously on `stream`; nothing synchronises unless stated.
 *   - frames are row-major contiguous (N, H, W[, C]); size=(W,H) as in video/io/base.py:119-125.
 *   - bit masks ("bits") are (N, H, ceil(W/32)) uint32, pixel x <-> bit (x & 31) of word x>>5,
 *     padding bits are 0.
 *   - threads: one device per process (va_init fixes it; every entry point selects it for the
 *     calling thread).  The stand-alone entry points keep no results between calls: each call
 *     leases its device scratch for itself, and a returned block is cached for later calls on the
 *     same `stream` only (va_trim and va_stream_destroy free it), so different threads may call
 *     them concurrently on different streams (the reference's VideoPreprocessor workers,
 *     video/io/parallel.py:398-400).  va_resize_u8 / va_resize_f32 upload their tables with a
 *     blocking copy and wait for `stream` first.  A va_pipeline_t handle owns its scratch and
 *     background state and must be used by one thread / one stream at a time.
 *   - sizes: frames of up to 2^29 - 1 pixels (the kernels address h*w*4 bytes through 32-bit
 *     buffer descriptors); larger frames are refused with VA_ERR_INVALID.
 *   - shape envelope ("Shape envelope"): unless an entry point says otherwise it takes any n >= 0
 *     (n = 0 enqueues nothing and writes nothing) and any h, w >= 1 below the pixel limit: a frame may be a single
 *     pixel, row or column, narrower than the filter (borders reflect or clip as often as needed), or longer than
 *     65535 rows or columns.  No launch puts more than 65535 into gridDim.y or gridDim.z: a longer batch goes out
 *     in pieces of 65535 frames, a taller frame takes a kernel with a one-dimensional grid, and where neither is
 *     possible the entry point states the limit and refuses beyond it with VA_ERR_INVALID and a message that names
 *     it, before anything is enqueued or written.  Ragged entry points count their m items in gridDim.x: any
 *     m >= 0 below 2^31.
 */
#ifndef VIDEOANALYSIS_HIP_H
#define VIDEOANALYSIS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VA_OK 0
#define VA_ERR_INVALID (-22) /* EINVAL  bad argument                     */
#define VA_ERR_NOMEM (-12)   /* ENOMEM  device/host allocation failed   */
#define VA_ERR_HIP (-5)      /* EIO     a HIP runtime call failed       */
#define VA_ERR_NODEV (-19)   /* ENODEV  no usable GPU                   */
#define VA_ERR_RANGE (-34)   /* ERANGE  capacity (max_labels, ...) exceeded */

/* dtypes */
#define VA_U8 0
#define VA_F32 1
#define VA_F64 2 /* targets of va_normalize / va_gaussian_noise; frames of va_mean_any / va_welford_any */
#define VA_I16 3 /* int16 frames (FilterTimeDifference's output): va_mean_any / va_welford_any only */
/* background modes (BUILD-DEFINED FilterBackground; arithmetic of video/analysis/video.py) */
#define VA_BG_NONE 0
#define VA_BG_MEAN 1   /* cumulative mean, float64 state: measure_mean, video/analysis/video.py:33 */
#define VA_BG_EMA 2    /* bg += rate*(frame-bg), float32 state (no reference counterpart)        */
#define VA_BG_STATIC 3 /* fixed float64 background image (e.g. a measure_mean() result)          */
/* morphology */
/* which OpenCV's 8-bit Gaussian taps (both written from upstream knowledge, unverifiable offline):
 * CV4: unsigned 8.8 fixed point with error diffusion, sum forced to 256 (OpenCV >= 4.x; default);
 * CV3: float32 getGaussianKernel, every tap cvRound(k * 256) on its own, sum not forced -- OpenCV 2.4 / 3.x,
 *      the era of the reference (cv2.findContours(...)[1], video/analysis/regions.py:180-182) */
#define VA_TAPS_CV4 0
#define VA_TAPS_CV3 1

#define VA_MORPH_ERODE 0
#define VA_MORPH_DILATE 1
#define VA_SHAPE_RECT 0    /* cv2.MORPH_RECT    */
#define VA_SHAPE_CROSS 1   /* cv2.MORPH_CROSS   (video/analysis/image.py:248) */
#define VA_SHAPE_ELLIPSE 2 /* cv2.MORPH_ELLIPSE */
#define VA_MAX_MORPH_OPS 4
#define VA_STATS_STRIDE 16 /* int64 per label, see va_moments_i64 */

/* ------------------------------------------------------------------ runtime / errors */
int va_init(int device);               /* select + warm up the GPU; VA_ERR_NODEV if none;
                                          a second, different device is VA_ERR_INVALID        */
int va_device_count(void);             /* number of visible GPUs (0 if none / no driver)     */
const char *va_version(void);
const char *va_last_error(void);       /* message for the calling thread's last failure      */

/* device memory helpers, so that a host without torch can drive the library */
/* The stand-alone entry points keep their device scratch between calls (a per-stream cache of blocks, at most
 * 6 GiB); va_trim synchronises the device and hands the cache (when it holds more than keep_bytes) and the default
 * memory pool's pages above keep_bytes back -- e.g. before another library in the process needs the memory. */
int va_trim(size_t keep_bytes);
int va_malloc(void **dev_ptr, size_t bytes);
int va_free(void *dev_ptr);
int va_host_alloc(void **host_ptr, size_t bytes); /* pinned host memory */
int va_host_free(void *host_ptr);
/* Host <-> device copies.  Pinned host memory (va_host_alloc, or registered by the caller): asynchronous on `stream`.
 * Pageable host memory (a NumPy array): the call waits for the stream's earlier work and returns when the copy is
 * complete -- large asynchronous copies to pageable memory were seen to leave part of the destination unwritten
 * after the stream had been synchronised.  So with pageable memory each of the two synchronises
 * `stream`, in front of the copy; the copy sees, or delivers, what the stream's earlier work has written. */
int va_memcpy_h2d(void *dst_dev, const void *src_host, size_t bytes, void *stream);
int va_memcpy_d2h(void *dst_host, const void *src_dev, size_t bytes, void *stream);
/* device to device, and a byte fill: enqueued on `stream`, never waited for */
int va_memcpy_d2d(void *dst_dev, const void *src_dev, size_t bytes, void *stream);
int va_memset(void *dst_dev, int value, size_t bytes, void *stream);
/* synchronises `stream`: returns when everything enqueued on it so far is complete */
int va_stream_sync(void *stream);

/* streams and events, for hosts that overlap uploads, the chain and downloads (the role of the
 * reference's reader process / VideoPreprocessor threads, video/io/parallel.py:345-488) */
int va_stream_create(void **stream_out);
/* synchronises `stream`, then frees the scratch cached for it and the stream */
int va_stream_destroy(void *stream);
/* events: recording and waiting are enqueued, only va_event_sync blocks the host */
int va_event_create(void **event_out);
int va_event_destroy(void *event);
int va_event_record(void *event, void *stream);
int va_stream_wait_event(void *stream, void *event);
int va_event_sync(void *event);
int va_event_elapsed_ms(void *start_event, void *stop_event, float *ms_out);

/* ------------------------------------------------------------------ A1 Gaussian blur
 * replaces  cv2.GaussianBlur(frame.astype(np.uint8), (0, 0), sigma)
 *           FilterBlur._process_frame, video/filters.py:388-392
 * 8-bit: ksize = cvRound(6 sigma + 1)|1, unsigned 8.8 fixed-point taps, BORDER_REFLECT_101,
 * each of the `c` interleaved channels independently.  src != dst.
 * Shape: any n >= 0, h, w >= 1 (frames smaller than the filter reflect repeatedly, as cv::borderInterpolate does). */
int va_gaussian_u8(const uint8_t *src_dev, uint8_t *dst_dev, int n, int h, int w, int c,
                   double sigma, void *stream);
/* replaces  cv2.GaussianBlur(float_image, (0, 0), sigma), video/analysis/active_contour.py:108
 * ksize = cvRound(8 sigma + 1)|1, float32 taps and fmaf accumulation.  Shape: any n >= 0, h, w >= 1. */
int va_gaussian_f32(const float *src_dev, float *dst_dev, int n, int h, int w, int c,
                    double sigma, void *stream);
/* the same with the tap set named explicitly (VA_TAPS_CV4 = va_gaussian_u8's, VA_TAPS_CV3 = the
 * reference-era definition; same row/column arithmetic: integer row sums, (acc + 2^15) >> 16 saturated) */
int va_gaussian_u8_rule(const uint8_t *src_dev, uint8_t *dst_dev, int n, int h, int w, int c,
                        double sigma, int tap_rule, void *stream);
/* analytic taps (host side, no GPU needed): q8.8 taps sum to 256 */
int va_gauss_taps_q8(double sigma, int *ksize_out, uint16_t *taps_out, int capacity);
int va_gauss_taps_q8_rule(double sigma, int tap_rule, int *ksize_out, uint16_t *taps_out, int capacity);
int va_gauss_taps_f32(double sigma, int *ksize_out, float *taps_out, int capacity);

/* ------------------------------------------------------------------ A2 background model
 * replaces  mean = mean*n/(n + 1) + frame/(n + 1)       measure_mean, video/analysis/video.py:33
 * and implements the BUILD-DEFINED FilterBackground: for each of the n frames IN ORDER
 *     diff = sat_u8(trunc(|frame - bg|))   (f32 frames: |frame - bg|)     then update bg.
 * mode VA_BG_MEAN  : state = float64[px], n_seen = frames already folded into it
 * mode VA_BG_EMA   : state = float32[px], rate; the very first frame initialises bg = frame
 * mode VA_BG_STATIC: state = float64[px], read only
 * dtype VA_U8 (all modes) or VA_F32 (EMA only).  diff_out may be NULL (state update only).
 * Values: the state is the caller's and may hold anything -- NaN, infinities, subnormals, 1e308: the new state is the
 * IEEE result of the expressions above, operation by operation (a NaN it generates may differ in sign and payload
 * from another machine's).  The uint8 difference of a pixel whose state is NaN is unspecified (C leaves the
 * conversion undefined); the state update of that pixel is not.
 * Shape (this call and the three below): any n >= 0, px >= 1 (px = h*w*c: the frame's shape does not matter). */
int va_bg_update(int mode, int dtype, const void *frames_dev, void *diff_out_dev,
                 void *state_dev, int64_t n_seen, double rate, int n, size_t px, void *stream);
/* measure_mean / measure_mean_std over frames of any dtype the reference meets (video/analysis/video.py:26-55):
 * dtype VA_U8, VA_I16 (FilterTimeDifference's int16), VA_F32 or VA_F64 (FilterNormalize's float64 target).
 * NumPy's promotions are kept:
 * `frame/(n + 1)` is rounded to float32 first for float32 frames, float64 otherwise. */
int va_mean_any(const void *frames_dev, int dtype, double *mean_dev, int64_t n_seen, int n, size_t px,
                void *stream);
int va_welford_any(const void *frames_dev, int dtype, double *mean_dev, double *m2_dev, int64_t n_seen,
                   int n, size_t px, void *stream);
/* replaces  measure_mean_std's Welford update, video/analysis/video.py:48-50 (float64 state) */
int va_welford_u8(const uint8_t *frames_dev, double *mean_dev, double *m2_dev, int64_t n_seen,
                  int n, size_t px, void *stream);

/* ------------------------------------------------------------------ A2b temporal median and rank planes
 * replaces  np.median(stack, axis=0) / np.percentile(stack, q, axis=0) on a downloaded uint8 stack; the reference
 *           has no counterpart (its only static background image is measure_mean, video/analysis/video.py:26-35).
 * frames_dev: t planes of px bytes, plane i at frames_dev + i * frame_stride (1 <= t <= 255, px >= 1,
 * frame_stride >= px: a stride of several frames samples a longer stack without a gather).  ranks_host: nranks
 * integers in HOST memory, 1 <= nranks <= 8, each 0 .. t - 1, in any order, repeats allowed.
 *   out_dev[j * px + p] = sort(frames[:, p])[ranks_host[j]]        (nranks, px) uint8, exact
 * Exactly nranks * px bytes are written, every one of them; nothing beyond byte px - 1 of a plane is read; two calls
 * write identical bytes.  t <= 64: the stack is read once, whatever nranks.  t >= 65: eight passes over it.  Dword
 * loads and stores where frames_dev, out_dev, frame_stride and px are all multiples of 4, byte accesses otherwise.
 * Anything outside the ranges above is VA_ERR_INVALID, and nothing is written. */
int va_temporal_ranks_u8(const uint8_t *frames_dev, int t, size_t px, size_t frame_stride,
                         const int32_t *ranks_host, int nranks, uint8_t *out_dev, void *stream);

/* ------------------------------------------------------------------ A2c sliding-window median
 * replaces  one va_temporal_ranks_u8 call per emitted frame on the window of the `window` frames before it
 *           (np.median over a sliding_window_view of a downloaded stack); the reference has no counterpart.
 * For every pixel and absolute frame index k = n_seen + j, j = 0 .. n - 1, with cnt = min(k, window):
 *   lower[j] = sort(frames[max(0, k - window) .. k - 1])[(cnt - 1) / 2],  upper[j] = the same at rank cnt / 2
 *   (both 0 at k = 0, the empty window);  diff[j] = min(255, |2 frame[k] - lower[j] - upper[j]| >> 1),
 *   which is sat_u8(trunc(|frame - median|)) for the float median (lower + upper) / 2.  All integer, all exact.
 * After its outputs are taken, frame k enters the window and frame k - window leaves it.
 * frames_dev: n planes of px bytes, plane j at frames_dev + j * frame_stride.  1 <= window <= 65535, px >= 1, n >= 0
 * (n = 0 writes nothing), frame_stride >= px, n_seen >= 0: the frames folded into the state so far, which the caller
 * counts (as for va_bg_update).  state_dev: va_sliding_median_state_bytes(px, window) bytes of the caller's device
 * memory on a 16-byte boundary, opaque between calls; all zeros (va_memset) is the empty state of n_seen = 0.  Per
 * tile of 128 pixels it holds a bin-major histogram [256][128] (uint8 counters for window <= 255, uint16 above),
 * the tracker planes lower, upper (u8) and below (u16), and behind the tiles a ring of the last `window` frames,
 * frame k in slot k % window: 260 + window bytes a pixel (516 + window above 255), in whole tiles.  A state belongs
 * to one (px, window); state_bytes is 0 for arguments outside the ranges above.
 * Each of lower / upper / diff_out_dev is (n, px) uint8 or NULL: exactly n * px bytes are written per non-NULL output,
 * nothing beyond byte px - 1 of a plane is read, and two identical call sequences from a zero state leave identical
 * outputs and identical state bytes, however the frames are split into calls.  Dword accesses where frames_dev,
 * frame_stride, px and the outputs are all multiples of 4, byte accesses otherwise.  One launch a call.
 * va_sliding_median_current writes the planes of the window as it stands (what the next frame would get as lower /
 * upper), (px) uint8 each or NULL.  Anything outside the ranges above is VA_ERR_INVALID, and nothing is written. */
size_t va_sliding_median_state_bytes(size_t px, int window);
int va_sliding_median_u8(const uint8_t *frames_dev, int n, size_t px, size_t frame_stride, int window,
                         int64_t n_seen, void *state_dev, uint8_t *lower_out_dev, uint8_t *upper_out_dev,
                         uint8_t *diff_out_dev, void *stream);
int va_sliding_median_current(const void *state_dev, size_t px, int window, int64_t n_seen,
                              uint8_t *lower_out_dev, uint8_t *upper_out_dev, void *stream);

/* ------------------------------------------------------------------ A3 / A4 / A5 pointwise
 * Shape: the calls that take `count` or `pixels` see one flat array of any length >= 0; va_prepare_u8,
 * va_rot90: any n >= 0 and frames of any h, w >= 1 (a crop must lie inside its source frame).
 * replaces  this_frame.astype(np.int16) - prev_frame, FilterTimeDifference._compare_frames,
 *           video/filters.py:564-568 */
int va_time_difference_u8(const uint8_t *this_dev, const uint8_t *prev_dev, int16_t *out_dev,
                          size_t count, void *stream);
/* BUILD-DEFINED FilterThreshold; the reference idiom is `frame > t` boolean masks
 * (video/analysis/image.py:282,288,304):  out = src > thresh ? maxval : 0 */
int va_threshold_u8(const uint8_t *src_dev, uint8_t *dst_dev, size_t count, int thresh,
                    int maxval, void *stream);
/* replaces  np.mean(frame, axis=2).astype(frame.dtype), FilterMonochrome._process_frame,
 *           video/filters.py:365-366 (float64 mean of 3 channels, truncated) */
int va_mono_mean_u8(const uint8_t *src_dev, uint8_t *dst_dev, size_t pixels, void *stream);
/* replaces  FilterNormalize._process_frame, video/filters.py:126-132, for u8 -> u8:
 *           clip to [fmin,fmax]; (f - fmin)*alpha + tmin in float64; astype(uint8) */
int va_normalize_u8(const uint8_t *src_dev, uint8_t *dst_dev, size_t count, double fmin,
                    double fmax, double alpha, double tmin, void *stream);
/* the same for float32 or uint8 frames and uint8 / float32 / float64 targets (the reference takes
 * any dtype, video/filters.py:101-135): clip, affine map, C cast to the target, with NumPy's types: uint8 frames are
 * mapped in float64; float32 frames stay float32 throughout (fmin, fmax, alpha and tmin are rounded to float32 first),
 * whatever the target.  A NaN pixel stays NaN in a float target; in a uint8 target, NaN and values beyond int32 are
 * unspecified (C leaves the conversion undefined). */
int va_normalize(const void *src_dev, int src_dtype, void *dst_dev, int dst_dtype, size_t count,
                 double fmin, double fmax, double alpha, double tmin, void *stream);
/* FilterCrop -> FilterMonochrome -> FilterNormalize in ONE pass over the source frames, on the device
 * (A5: the pointwise pre-stages of a chain, video/filters.py:238-248, 359-374, 126-132), so that a
 * chain which starts with them feeds the engine without a host round trip:
 *   crop = frame[top:top+height, left:left+width]; mono: -1 keep the channels, 0..2 that channel,
 *   3 np.mean(axis=2).astype(uint8); normalize != 0: clip, (f - fmin)*alpha + tmin, astype(uint8).
 * src (n, src_h, src_w, src_c) uint8 -> dst (n, height, width[, src_c when mono == -1]). */
#define VA_MONO_KEEP (-1)
#define VA_MONO_MEAN 3
int va_prepare_u8(const uint8_t *src_dev, uint8_t *dst_dev, int n, int src_h, int src_w, int src_c, int left,
                  int top, int width, int height, int mono, int normalize, double fmin, double fmax,
                  double alpha, double tmin, void *stream);
/* replaces  self.mean + self.std*np.random.randn(*self._frame_shape), VideoGaussianNoise.get_frame,
 *           video/io/computed.py:36-41, on the device (N4): sample i of the stream is a pure
 * function of (seed, i) -- Philox4x32-10 counter, Box-Muller in float64 -- so any frame can be
 * produced on its own: count samples starting at absolute sample index first_index
 * (= frame_index * samples_per_frame).  dtype VA_U8 (saturated to [0, 255], truncated), VA_F32
 * or VA_F64.  The reference's stream is unseeded NumPy state: agreement is statistical. */
int va_gaussian_noise(void *dst_dev, int dtype, size_t count, double mean, double stdev, uint64_t seed,
                      uint64_t first_index, void *stream);
/* replaces  np.rot90(frame, angle // 90), FilterRotate._process_frame, video/filters.py:339-344
 * (N4): n frames (h, w) of opaque elem_bytes-byte pixels (channels x dtype: 1, 2, 3, 4, 6, 8 or
 * 12 bytes) turned k quarter turns counter-clockwise; output frames are (w, h) for odd k. */
int va_rot90(const void *src_dev, void *dst_dev, int n, int h, int w, int elem_bytes, int k,
             void *stream);

/* replaces  cv2.resize(frame, self.size, interpolation=...), FilterResize._process_frame,
 *           video/filters.py:310-314 (N4).  uint8 frames (n, src_h, src_w[, c]) -> (n, dst_h, dst_w[, c]),
 * c <= 4 interleaved channels.  OpenCV's 8-bit definitions: nearest = floor(x * src/dst); linear and
 * cubic (A = -0.75) with 11-bit fixed-point weights and OpenCV's rounding steps (an exact 2x2
 * linear shrink is the area mean, as there); area = block means for integer shrink factors,
 * float cell-overlap weights for other shrinks, linear with area-style positions when growing;
 * lanczos4 (video/filters.py:293-294) = 8 x 8 taps, 11-bit fixed point, int32 accumulation.  src != dst.
 * va_resize_f32: float32 frames (FilterResize takes the video's dtype): the float instantiations of the
 * same algorithms -- float coefficients, products summed from the first tap to the last, no rounding.
 * Shape: any n >= 0 (more than 65535 frames go out in pieces); source frames of any src_h, src_w >= 1; targets of
 * dst_w >= 1 and 1 <= dst_h <= 65535 (the kernels count target rows in gridDim.y): a taller target is refused
 * with VA_ERR_INVALID before the tables are uploaded.
 * Each call synchronises `stream` once, before it uploads its coefficient tables: the upload is a blocking copy from
 * the host into leased scratch, which the stream's earlier kernels may still read.  The kernels are then enqueued
 * on `stream` and the call returns without waiting for them.  (An area shrink by integer factors, which the exact
 * 2 x 2 linear shrink is too, has no tables and waits for nothing.) */
#define VA_INTER_NEAREST 0
#define VA_INTER_LINEAR 1
#define VA_INTER_CUBIC 2
#define VA_INTER_AREA 3
#define VA_INTER_LANCZOS4 4
int va_resize_u8(const uint8_t *src_dev, uint8_t *dst_dev, int n, int src_h, int src_w, int c, int dst_h,
                 int dst_w, int interpolation, void *stream);
int va_resize_f32(const float *src_dev, float *dst_dev, int n, int src_h, int src_w, int c, int dst_h,
                  int dst_w, int interpolation, void *stream);

/* ------------------------------------------------------------------ A6 morphology
 * replaces  cv2.erode / cv2.dilate(img, cv2.getStructuringElement(shape, (k, k))),
 *           video/analysis/image.py:248-251; anchor = centre, pixels outside the image never
 *           win (OpenCV's default border).  src != dst.  (n, h, w) u8.
 * Shape: any n >= 0, h, w >= 1, elements larger than the frame included (rows of whole dwords with h, n <= 65535
 * take the four-samples-per-thread kernels, everything else the one-sample kernels: the same bytes). */
int va_morph_u8(const uint8_t *src_dev, uint8_t *dst_dev, int n, int h, int w, int op,
                int shape, int ksize, void *stream);

/* ------------------------------------------------------------------ A7 labelling
 * replaces  labels, num = ndimage.measurements.label(mask), video/analysis/regions.py:162
 * any non-zero mask byte is foreground; connectivity 4 (SciPy default) or 8; int32 labels
 * 1..L numbered in raster order of each component's first pixel; counts[f] = L of frame f.
 * labels_dev: (n,h,w) int32 (also used as the union-find forest while running).
 * workspace: va_label_workspace_bytes(n,h,w) bytes of device scratch.
 * Shape: any n >= 0, h, w >= 1 below 2^29 pixels. */
size_t va_label_workspace_bytes(int n, int h, int w);
int va_label_i32(const uint8_t *mask_dev, int32_t *labels_dev, int32_t *counts_dev, int n,
                 int h, int w, int connectivity, void *workspace_dev, size_t workspace_bytes,
                 void *stream);

/* ------------------------------------------------------------------ A7/A8/A9 per-label stats
 * replaces  [np.sum(labels == l) ...], video/analysis/regions.py:165-166;
 *           find_bounding_box, video/analysis/regions.py:113-149;
 *           cv2.moments(mask.astype(np.uint8)) spatial moments, video/analysis/image.py:353
 * stats_dev: (n, max_labels, 16) int64, for label l at [l-1]:
 *   0 area(m00) 1 m10 2 m01 3 m20 4 m11 5 m02 6 m30 7 m21 8 m12 9 m03
 *   10 xmin 11 ymin 12 xmax 13 ymax 14,15 reserved
 * labels above max_labels are ignored (check counts against max_labels on the host).
 * Shape (va_moments_i64, va_largest_region): any n >= 0, h, w >= 1, max_labels >= 1. */
int va_moments_i64(const int32_t *labels_dev, int n, int h, int w, int max_labels,
                   int64_t *stats_dev, void *stream);
/* replaces  label_max = np.argmax(areas) + 1; labels == label_max,
 *           get_largest_region, video/analysis/regions.py:169-174 (first maximum wins).
 * largest_dev[f] = label_max (0 when the frame is empty); mask_out_dev (nullable) = 0/1 u8. */
int va_largest_region(const int32_t *labels_dev, const int32_t *counts_dev,
                      const int64_t *stats_dev, int n, int h, int w, int max_labels,
                      int32_t *largest_dev, int64_t *largest_area_dev, uint8_t *mask_out_dev,
                      void *stream);

/* ------------------------------------------------------------------ A8 contour of the largest region
 * replaces  contours = cv2.findContours(mask.astype(np.uint8), cv2.RETR_EXTERNAL,
 *                                       cv2.CHAIN_APPROX_SIMPLE)[1]
 *           contour_id = np.argmax([cv2.contourArea(c) for c in contours])
 *           get_contour_from_largest_region, video/analysis/regions.py:178-197
 * 8-connected foreground (any non-zero byte), Suzuki-Abe outer border following from each
 * component's first raster pixel, points kept only where the direction changes, OpenCV's
 * most-recent-first contour order for the argmax tie rule.
 * points_dev: (n, max_points, 2) int32 (x, y); npoints_dev[f] = points of the winning contour
 * (if > max_points only the first max_points were stored); area_dev[f] = cv2.contourArea of it;
 * ncomponents_dev[f] = number of 8-connected components (0 -> "Could not find any contour").
 * Shape: any n >= 0 (the per-frame passes go out in pieces of 65535 frames), h, w >= 1 below 2^29 pixels. */
size_t va_contour_workspace_bytes(int n, int h, int w);
int va_largest_contour(const uint8_t *mask_dev, int n, int h, int w, int32_t *points_dev,
                       int max_points, int32_t *npoints_dev, double *area_dev,
                       int32_t *ncomponents_dev, void *workspace_dev, size_t workspace_bytes,
                       void *stream);

/* ------------------------------------------------------------------ A8 all outer contours
 * replaces  contours = cv2.findContours(mask.astype(np.uint8), cv2.RETR_EXTERNAL,
 *                                       cv2.CHAIN_APPROX_SIMPLE)[1]   used as a whole list:
 *           video/analysis/regions.py:180-182, :229-231 (get_external_contour), :575-576,
 *           video/io/composer.py:228
 * Every outer contour of n frames of h x w uint8 (any non-zero byte is foreground) as one ragged list.
 * A contour is the outer border (the walk of va_largest_contour, point for point) of an 8-connected
 * component that lies in no hole of another: the 4-connected background component left of its first
 * raster pixel reaches the frame edge, or that pixel is in column 0.  Within a frame the contours come
 * in OpenCV's order, most recently found first = descending first-pixel index; frames follow each
 * other, so contour k of frame f is global slot (sum of ncontours_dev[0 .. f)) + k.
 *   ncontours_dev[n]                 contours of each frame
 *   totals_dev[2]                    contours and points of the whole batch, always the true totals
 *   info_dev[cap_contours]           one record per slot
 *   point_off_dev[cap_contours + 1]  exclusive scan of the records' npoints: slot s owns the points
 *                                    point_off[s] .. point_off[s + 1]
 *   points_dev[cap_points][2]        int32 (x, y), 8-byte aligned
 * Nothing is written beyond a capacity: slots 0 .. min(total, cap_contours) - 1 have their record and
 * offsets, and a slot has its points when all of them lie below cap_points (such slots form a
 * prefix).  Exceeding a capacity is no error: compare totals_dev with the capacities and call again
 * with room.  Slots and positions come from counts and scans, never from the order of atomics: two
 * calls write identical bytes.  Everything is enqueued on `stream`, in the caller's workspace only.
 * Frames stay below 2^29 pixels, as for va_largest_contour.  Shape: any n >= 0 (pieces of 65535 frames where a
 * pass counts frames in its grid), h, w >= 1. */
typedef struct va_contour_info {
    int32_t frame, npoints;                     /* frame index; points of the contour */
    int32_t start_x, start_y;                   /* its first point = the component's first raster pixel */
    int32_t rect_x, rect_y, rect_w, rect_h;     /* cv2.boundingRect */
    double area;                                /* cv2.contourArea */
    double perimeter;                           /* cv2.arcLength(contour, closed=True) */
} va_contour_info;
size_t va_find_contours_workspace_bytes(int n, int h, int w);
int va_find_contours(const uint8_t *mask_dev, int n, int h, int w, int32_t *ncontours_dev, int64_t *totals_dev,
                     va_contour_info *info_dev, int64_t *point_off_dev, int64_t cap_contours,
                     int32_t *points_dev, int64_t cap_points, void *workspace_dev, size_t workspace_bytes,
                     void *stream);

/* ------------------------------------------------------------------ A8b region links between consecutive frames
 * replaces  no call of the reference.  It is what a tracker does first with the labels of
 *           video/analysis/regions.py:159-174 on consecutive frames -- which region of frame t is which region of
 *           frame t - 1 -- computed where the labels lie, so that no label plane crosses to the host.
 * labels_dev: (n, h, w) int32; prev_dev: (h, w) int32 or NULL.  A value <= 0 is background, any value >= 1 a
 * region label (the planes need not be a connected-component labelling).  Pair t = (E, L) with L = labels[t] and
 * E = labels[t - 1], or prev for t = 0; without prev pair 0 has no links.  The links of pair t are all
 * (a, b, count) with a >= 1, b >= 1 and count = #{pixels: E = a and L = b} > 0, ordered by the raster index of the
 * first such pixel; the links of pair t follow those of pair t - 1.
 *   nlinks_dev[n]         links of each pair, always the true numbers
 *   totals_dev[2]         [0] links of the batch, always the true total; [1] `need`: a capacity that is sure to
 *                         suffice
 *   links_dev[cap_links]  the records, 16-byte aligned
 * need is always computed, without the tables: the number of pixels with a key (a, b) whose left and upper
 * neighbours carry another key or do not exist, so links <= need <= #{pixels with both labels >= 1}.
 * need <= cap_links: every record is written.  Otherwise nothing is stored in links_dev, the counts and both totals
 * still report, and one more call with cap_links = need succeeds.  Exceeding the capacity is no error.  Nothing is
 * written beyond the capacity or outside the caller's buffers.  Slots come from counts and scans, never from the
 * order of atomics: two calls write identical bytes.  The workspace (16-byte aligned) holds the per-pair hash
 * tables: 32 bytes a link of capacity, and never less than 32 bytes a pixel of one frame.  Where the tables of all
 * pairs fit it together -- always when need <= cap_links -- the pairs are counted side by side; below that the
 * links are still counted exactly, a table at a time, which takes longer.  A workspace_bytes above what the size
 * function asks for is used: 32 bytes more hold one more candidate side by side.  n == 0 writes two zero totals.
 * Shape: any n >= 0 (pieces of 65535 pairs in a grid), h, w >= 1, frames below 2^29 pixels, batches below 2^37. */
typedef struct va_region_link {
    int32_t frame, a, b, count;
} va_region_link;
size_t va_region_links_workspace_bytes(int n, int h, int w, int64_t cap_links);
int va_region_links(const int32_t *prev_dev, const int32_t *labels_dev, int n, int h, int w, int32_t *nlinks_dev,
                    int64_t *totals_dev, va_region_link *links_dev, int64_t cap_links, void *workspace_dev,
                    size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ A8c template matching
 * replaces  cv2.matchTemplate(frame, template, method) and cv2.minMaxLoc on its result, for a batch of (frame,
 *           template, search window) queries, and the slicing that regions.get_overlapping_slices
 *           (video/analysis/regions.py) does for a caller that compares a template with part of a frame.
 * Frames are (n, h, w) uint8, frame f at frames_dev + f * frame_stride (frame_stride >= h * w bytes).  Templates are
 * a ragged batch: template t is template_shapes_dev[2 t] rows x template_shapes_dev[2 t + 1] columns of uint8,
 * row-major at templates_dev + template_offsets_dev[t]; the m + 1 offsets are in order.  1 <= th, tw and
 * th * tw <= 65536, so that every sum below fits 32 unsigned bits (255 * 255 * 65536 < 2^32).
 * Query k = (frame, templ, x0, y0, nx, ny) asks for the template's top-left corner at (x0 + i, y0 + j), 0 <= i < nx,
 * 0 <= j < ny; every position must hold the whole template inside the frame.  With the exact integers S_it = sum I T,
 * S_i = sum I, S_ii = sum I I over the window, S_t = sum T, S_tt = sum T T and N = th * tw, the float64 score is
 *   VA_MATCH_SQDIFF         (double)(S_ii - 2 S_it + S_tt)
 *   VA_MATCH_SQDIFF_NORMED  that / sqrt((double)S_ii * (double)S_tt)            (1.0 where the denominator is 0.0)
 *   VA_MATCH_CCORR          (double)S_it
 *   VA_MATCH_CCORR_NORMED   (double)S_it / sqrt((double)S_ii * (double)S_tt)    (0.0 where the denominator is 0.0)
 *   VA_MATCH_CCOEFF         (double)(N S_it - S_i S_t) / (double)N
 *   VA_MATCH_CCOEFF_NORMED  (double)(N S_it - S_i S_t) / sqrt((double)(N S_ii - S_i S_i) * (double)(N S_tt - S_t S_t))
 *                           (0.0 where the denominator is 0.0)
 * with int64 numerators and each multiply, sqrt and divide rounded once.  The codes are cv2.TM_*'s.  cv2 itself returns
 * float32 from a DFT and thresholds small denominators; agreement is expected up to that rounding only.
 *   best_out_dev[k]   (NULL: not wanted) the minimum (SQDIFF methods) or maximum score of query k and its frame
 *                     position (x, y); at equal scores the first position in raster order (j, then i)
 *   maps_out_dev      (NULL: not wanted) the scores of query k, (ny, nx) float64 row-major, at
 *                     maps_out_dev + map_offsets_dev[k] (k + 1 offsets in elements; the caller lays them out)
 * status of a query: 0, or VA_MATCH_STATUS_* bits.  A flagged query writes its status into best_out_dev[k].status and
 * nothing else, neither the rest of its record nor its map, and the entry point still returns 0.
 * total_positions: the sum of nx * ny over the valid queries, as the caller computed it; it sizes the workspace.  A
 * call whose queries need more than it allows flags every query with VA_MATCH_STATUS_WORKSPACE and writes no score.
 * Envelope: n_queries >= 0 (0 enqueues nothing); n_queries, n_templates and the tile bound of total_positions below
 * 2^31; frames below 2^29 pixels; queries and tiles are counted in gridDim.x, never in gridDim.y or z.
 * Alignment: every typed pointer may start at any multiple of its element size (queries and shapes 4, offsets, bests,
 * maps and the workspace 8), frames and templates at any byte; a misaligned pointer is VA_ERR_INVALID.
 * Refused with VA_ERR_INVALID and a message that names the limit, before anything is enqueued: a struct_size that is
 * not sizeof(va_match_args), an unknown method, counts outside the envelope, a workspace below
 * va_template_match_workspace_bytes (0 for counts outside the envelope), a misaligned pointer.  Template shapes live
 * on the device: one beyond 65536 pixels is the status bit VA_MATCH_STATUS_TEMPLATE_SHAPE of the queries that name it.
 * Asynchronous on args->stream; leases nothing: the workspace is the caller's.  Slots come from a scan and the bests
 * from a rule that is a total order, never from the order of atomics: two calls write identical bytes. */
#define VA_MATCH_SQDIFF 0
#define VA_MATCH_SQDIFF_NORMED 1
#define VA_MATCH_CCORR 2
#define VA_MATCH_CCORR_NORMED 3
#define VA_MATCH_CCOEFF 4
#define VA_MATCH_CCOEFF_NORMED 5
#define VA_MATCH_MAX_TEMPLATE_PIXELS 65536
#define VA_MATCH_STATUS_FRAME 1           /* frame index outside 0 .. n - 1 */
#define VA_MATCH_STATUS_TEMPLATE 2        /* template index outside 0 .. n_templates - 1 */
#define VA_MATCH_STATUS_EMPTY 4           /* nx < 1 or ny < 1 */
#define VA_MATCH_STATUS_OUTSIDE 8         /* a position puts the template outside the frame */
#define VA_MATCH_STATUS_TEMPLATE_SHAPE 16 /* th or tw < 1, th * tw > 65536, or offsets that do not hold the template */
#define VA_MATCH_STATUS_WORKSPACE 32      /* total_positions was below what the queries need */
#define VA_MATCH_TILE 32                  /* positions of a tile, each way */
#define VA_MATCH_CHUNK_ROWS 16            /* template rows and columns in LDS at a time */
#define VA_MATCH_CHUNK_COLS 64
typedef struct va_match_query {
    int32_t frame, templ, x0, y0, nx, ny;
} va_match_query; /* 24 bytes */
typedef struct va_match_best {
    double score;
    int32_t x, y, status, reserved;
} va_match_best; /* 24 bytes */
typedef struct va_match_args {
    int32_t struct_size; /* = sizeof(va_match_args), as va_config */
    int32_t method;      /* VA_MATCH_SQDIFF ... VA_MATCH_CCOEFF_NORMED */
    const uint8_t *frames_dev;
    int32_t n, h, w, reserved;
    int64_t frame_stride;
    const uint8_t *templates_dev;
    const int32_t *template_shapes_dev;  /* (n_templates, 2): rows, columns */
    const int64_t *template_offsets_dev; /* n_templates + 1 */
    int64_t n_templates;
    const va_match_query *queries_dev;
    int64_t n_queries, total_positions;
    va_match_best *best_out_dev;
    double *maps_out_dev;
    const int64_t *map_offsets_dev; /* n_queries + 1 */
    void *workspace_dev;
    size_t workspace_bytes;
    void *stream;
} va_match_args; /* 144 bytes */
size_t va_template_match_workspace_bytes(int64_t n_queries, int64_t total_positions, int64_t n_templates);
int va_template_match_u8(const va_match_args *args);

/* ------------------------------------------------------------------ A10 geodesic distance maps
 * 8-neighbour geodesics inside masks: straight steps cost 1, diagonal steps sqrt2 (a diagonal step may
 * pass between two wall pixels).  A distance d = a + b*sqrt2 is kept as the exact pair (a, b) and
 * written as 2 + a + floor(b*sqrt2), the reference's int(2 + d); maps are relaxed to their fixpoint
 * with one workgroup per frame.  Frames up to 8192 columns wide (wider: VA_ERR_INVALID), any h >= 1, any
 * n >= 0 (the frame is the workgroup index, gridDim.x).  All three entry points work only
 * in `workspace_dev` (va_geodesic_workspace_bytes) and on `stream`. */
size_t va_geodesic_workspace_bytes(int n, int h, int w);
/* replaces  make_distance_map(mask, start_points, end_points), video/analysis/regions.py:455-509
 * fillable_dev: (n, h, w) u8, non-zero where the map may be filled (the reference's pixels equal to 1).
 * starts_dev: (n, max_starts, 2) int32 (x, y), nstarts_dev[f] of them used; starts outside the frame
 * or on a pixel that is not fillable are ignored.  ends_dev (nullable): (n, max_ends, 2) int32 (x, y),
 * nends_dev[f] of them used: the fill stops at the nearest reachable end point -- pixels closer than
 * it are filled, and it itself (the first listed among equally near ones); other pixels at exactly its
 * distance stay unfilled, where the reference's choice depends on its float keys and set order.
 * map_out_dev: (n, h, w) int32, 0 = not fillable, 1 = fillable but not reached, >= 2 = filled. */
int va_distance_map_i32(const uint8_t *fillable_dev, int n, int h, int w, const int32_t *starts_dev,
                        const int32_t *nstarts_dev, int max_starts, const int32_t *ends_dev,
                        const int32_t *nends_dev, int max_ends, int32_t *map_out_dev, void *workspace_dev,
                        size_t workspace_bytes, void *stream);
/* replaces  shortest_path_in_distance_map(distance_map, end_point), video/analysis/regions.py:513-565
 * The reference's walk, literally: values <= 1 and the one-pixel frame around the map read as INT64_MAX,
 * each step moves to the first minimum (row-major) of (D - d) * weight over the 3x3 window (int64
 * differences, float64 weights 1 / (1/sqrt2 at the corners)), continuing while the value falls or stays
 * on an unvisited pixel.  map_dev: (n, h, w) int32; end_points_dev: (n, 2) int32 (x, y).
 * path_out_dev: (n, max_points, 2) int32 (x, y); npath_out_dev[f] = full path length (only the first
 * max_points stored); 0 when the end point is outside the frame or its value is <= 1 (the reference
 * walks through its sentinels there). */
int va_distance_map_path(const int32_t *map_dev, int n, int h, int w, const int32_t *end_points_dev,
                         int32_t *path_out_dev, int max_points, int32_t *npath_out_dev, void *workspace_dev,
                         size_t workspace_bytes, void *stream);
/* replaces  get_farthest_points(mask, p1, ret_path), video/analysis/regions.py:568-611
 * mask_dev: (n, h, w) u8, foreground = non-zero.  p1_dev (nullable): (n, 2) int32 (x, y) start points;
 * NULL: the first point of the longest (cv2.arcLength, closed) cv2.findContours RETR_EXTERNAL /
 * CHAIN_APPROX_SIMPLE contour, ties to the contour OpenCV lists first (the component whose first
 * pixel comes last in raster order); with p1_dev NULL, p1_out = (-1, -1) marks a frame without a
 * component (nothing else is computed for it).  A given start outside the frame or off the mask is
 * ignored by the first map, as in the reference, so p2 becomes the first foreground pixel.  The whole loop -- map from p1, first raster argmax p2, stop when its value
 * does not grow, else p1 = p2 -- runs on the device.  p1_out_dev, p2_out_dev: (n, 2) int32;
 * dist_out_dev: (n) int32, the map value at p2; rounds_out_dev: (n, 2) int32, maps built and sweeps
 * over all of them.  path_out_dev (nullable): (n, max_points, 2) int32, the walk of
 * va_distance_map_path from p2 through the last map, npath_out_dev[f] its full length. */
int va_farthest_points(const uint8_t *mask_dev, int n, int h, int w, const int32_t *p1_dev,
                       int32_t *p1_out_dev, int32_t *p2_out_dev, int32_t *dist_out_dev, int32_t *rounds_out_dev,
                       int32_t *path_out_dev, int max_points, int32_t *npath_out_dev, void *workspace_dev,
                       size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ A11 dense optical flow
 * replaces  cv2.calcOpticalFlowFarneback(prev, next, None, pyr_scale, levels, winsize, iterations, poly_n,
 *           poly_sigma, flags) and the magnitude of cv2.cartToPolar, FilterOpticalFlow, video/filters.py:572-589
 * OpenCV's algorithm with flags = 0, bit for bit as DESIGN.md "Optical flow" pins it (no fused multiply-add).
 * va_farneback_poly_consts (host only, no GPU needed): FarnebackPrepareGaussian's float g, xg, xxg
 * (2 poly_n + 1 each, offsets -poly_n..poly_n) and ig_out = ig11, ig03, ig33, ig55. */
int va_farneback_poly_consts(int poly_n, double poly_sigma, float *g_out, float *xg_out, float *xxg_out,
                             double *ig_out);
/* device workspace of va_optical_flow_farneback (0 for arguments it refuses) */
size_t va_farneback_workspace_bytes(int n, int h, int w, double pyr_scale, int levels, int winsize,
                                    int iterations, int poly_n);
/* frames_dev: n >= 2 consecutive (h, w) frames, dtype VA_U8 or VA_F32; pair k is (frame k, frame k + 1).
 * flow_out_dev (nullable): (n - 1, h, w, 2) float32 (dx, dy); mag_out_dev (nullable): (n - 1, h, w) float32
 * sqrt(dx^2 + dy^2); not both NULL.  pyr_scale in (0, 1), levels >= 0, winsize >= 1, iterations >= 1,
 * poly_n 5 or 7, flags 0 (OPTFLOW_USE_INITIAL_FLOW and OPTFLOW_FARNEBACK_GAUSSIAN are not supported), else
 * VA_ERR_INVALID; a workspace smaller than va_farneback_workspace_bytes is VA_ERR_RANGE.  Shape: 2 <= n, at most
 * 65535 frames and at most 65535 rows in one call (both count in gridDim.y / gridDim.z of the pyramid kernels, and
 * a pair needs both of its frames in one call), any w >= 1; beyond: VA_ERR_INVALID, nothing enqueued.  The call
 * synchronises `stream` before it uploads its resize tables (a blocking copy from the host into leased scratch that
 * the stream's earlier kernels may still read), then enqueues its kernels on it. */
int va_optical_flow_farneback(const void *frames_dev, int dtype, int n, int h, int w, double pyr_scale,
                              int levels, int winsize, int iterations, int poly_n, double poly_sigma, int flags,
                              float *flow_out_dev, float *mag_out_dev, void *workspace_dev,
                              size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ A12 active contours
 * replaces  cv2.Sobel(p, cv2.CV_64F, 1, 0, ksize=5) and cv2.Sobel(p, cv2.CV_64F, 0, 1, ksize=5),
 *           ActiveContour.set_potential, video/analysis/active_contour.py:109-110
 * src_dev: (n, h, w) frames of dtype VA_U8 or VA_F32 (the blurred potential: va_gaussian_u8 / va_gaussian_f32
 * before it).  fx_out_dev, fy_out_dev (nullable, not both): (n, h, w) float64, OpenCV's FilterEngine
 * arithmetic with a CV_64F kernel and BORDER_REFLECT_101, -0.0 and +0.0 as it gives them.
 * Shape: any n >= 0 (pieces of 65535 frames), h, w >= 1. */
int va_sobel5_f64(const void *src_dev, int dtype, double *fx_out_dev, double *fy_out_dev, int n, int h, int w,
                  void *stream);
/* replaces  the iteration of ActiveContour.find_contour, video/analysis/active_contour.py:160-191
 * m contours on an (n, h, w) stack of float64 gradients (h, w >= 2: smaller frames are VA_ERR_INVALID; any
 * n >= 1, any m >= 0), every iteration of every contour in one launch.  Per contour c: npts_dev[c] points (<= max_points <= 1024; <= 2 leaves the contour as it is with
 * 0 iterations), frame_dev[c] its frame, mat_offset_dev[c] the element offset in mats_dev (mats_count
 * doubles) of its inverse evolution matrix stored TRANSPOSED (element (j, i) = Pinv[i, j]).
 * anchor_flags_dev (nullable): (m, max_points) u8, bit 0 = x fixed, bit 1 = y fixed, at the value in
 * anchor_vals_dev (m, max_points, 2) float64.  pts_inout_dev: (m, max_points, 2) float64 (x, y), the
 * equidistant curve in, the contour out.  An iteration stops the contour when its residual is below
 * tol_gamma (residual_tolerance*gamma); iterations_out_dev[c] (int32) counts them (-1: an entry out of
 * range, contour untouched), total_variation_out_dev[c] (float64) = sum |clipped start - end|.  The
 * matrices of calls whose max_points <= 128 are staged in LDS, longer ones are read from global memory.
 * Nothing is copied: the call enqueues one kernel on `stream`. */
int va_active_contour(const double *fx_dev, const double *fy_dev, int n, int h, int w, int m, int max_points,
                      const int32_t *npts_dev, const int32_t *frame_dev, const double *mats_dev,
                      const int64_t *mat_offset_dev, int64_t mats_count, const uint8_t *anchor_flags_dev,
                      const double *anchor_vals_dev, double gamma, double tol_gamma, int max_iterations,
                      double *pts_inout_dev, int32_t *iterations_out_dev, double *total_variation_out_dev,
                      void *stream);
/* replaces  cv2.GaussianBlur(potential, (0, 0), sigma) and both cv2.Sobel calls of ActiveContour.set_potential,
 *           video/analysis/active_contour.py:104-110, for the potentials of many polygons at once
 *           (Polygon.get_centerline_optimized, video/analysis/shapes.py:735-743)
 * m items of a ragged packed buffer, laid out as for va_distance_transform_l2_5: item i is (shapes_dev[2i],
 * shapes_dev[2i + 1]) = (h, w) at element offset offsets_dev[i] (int64) of src_dev, and its two float64 planes
 * go to the same element offset of fx_out_dev and fy_out_dev; every buffer holds `total` elements.  Each item
 * is an image of its own: blur and Sobel reflect (BORDER_REFLECT_101) at the item's edges, and the Sobel
 * reflects the blurred image ("Batched centre lines").  dtype: VA_F32, blurred as
 * va_gaussian_f32 blurs when sigma > 0, or VA_U8 with sigma == 0 (the 8-bit blur is a different, fixed-point
 * arithmetic: VA_U8 with sigma > 0 is VA_ERR_INVALID).  One workgroup keeps an item in LDS at 8 bytes per
 * pixel; max_pixels is the largest h * w of the call (<= VA_GRAD_RESIDENT_MAX_PIXELS: 64 KiB; it sizes the
 * LDS).  status_dev[i] (int32): VA_OK, or VA_ERR_RANGE for an item above max_pixels or outside `total` (not
 * written); an empty item is VA_OK.  Nothing is copied: the call enqueues one kernel on `stream`. */
#define VA_GRAD_RESIDENT_MAX_PIXELS 8192
int va_potential_gradients_ragged(const void *src_dev, int dtype, const int32_t *shapes_dev,
                                  const int64_t *offsets_dev, int64_t total, int m, int max_pixels, double sigma,
                                  double *fx_out_dev, double *fy_out_dev, int32_t *status_dev, void *stream);
/* replaces  the iteration of ActiveContour.find_contour, video/analysis/active_contour.py:160-191, on
 *           potentials of different sizes
 * va_active_contour on the planes va_potential_gradients_ragged writes: contour c runs on item item_dev[c]
 * of the n_items items, whose plane starts at offsets_dev[item] with a row stride of its own w and is clipped
 * to its own (w - 2, h - 2).  An item index out of range, an item with h < 2 or w < 2 or a plane that does not
 * fit in `total` gives iterations -1 and leaves the contour untouched.  Everything else is as for
 * va_active_contour. */
int va_active_contour_ragged(const double *fx_dev, const double *fy_dev, const int32_t *shapes_dev,
                             const int64_t *offsets_dev, int64_t total, int n_items, int m, int max_points,
                             const int32_t *npts_dev, const int32_t *item_dev, const double *mats_dev,
                             const int64_t *mat_offset_dev, int64_t mats_count, const uint8_t *anchor_flags_dev,
                             const double *anchor_vals_dev, double gamma, double tol_gamma, int max_iterations,
                             double *pts_inout_dev, int32_t *iterations_out_dev,
                             double *total_variation_out_dev, void *stream);

/* ------------------------------------------------------------------ A13 polygons
 * Limits of one polygon / mask of the two calls below (beyond them its status is VA_ERR_RANGE):
 * fill: 1 .. VA_FILL_MAX_VERTS vertices, box sides 0 .. VA_FILL_MAX_SIDE, every vertex within
 * +-VA_FILL_MAX_COORD of its box's origin (so that x << 16 and (y - y0)*dx stay far inside int64);
 * distance transform: width 0 .. VA_DT_MAX_WIDTH, height 0 .. VA_DT_MAX_HEIGHT (its unsigned sums
 * INIT_DIST0 + (rows + 1)*65536 + 143976 stay below 2^32). */
#define VA_FILL_MAX_VERTS 1024
#define VA_FILL_MAX_SIDE 16384
#define VA_FILL_MAX_COORD (1 << 20)
#define VA_DT_MAX_WIDTH 4096
#define VA_DT_MAX_HEIGHT 16384
/* replaces  cv2.fillPoly(mask, [contour], color=1, offset=(-x, -y)) with lineType LINE_8, shift 0,
 *           Polygon.get_mask, video/analysis/shapes.py:577-597
 * m polygons, each drawn into its own (h, w) box of a ragged packed buffer.  verts_dev: int32 (x, y)
 * vertices of all polygons; polygon i owns vertices vert_off_dev[i] .. vert_off_dev[i + 1] - 1
 * (int64, m + 1 entries, within 0 .. nverts).  boxes_dev: (m, 4) int32 (x, y, w, h): the box's origin
 * in vertex coordinates and its size.  out_off_dev[i] (int64): element offset of box i in out_dev,
 * which holds out_elems elements of elem_size bytes (1: uint8, 4: int32).  Every pixel of a box is
 * written: 1 inside (OpenCV's scanline fill and the edges' 8-connected lines), 0 else.
 * status_dev[i] (int32): VA_OK, or VA_ERR_RANGE for a polygon beyond the limits (its box is not
 * written).  Nothing is copied: the call enqueues one kernel on `stream`. */
int va_fill_poly(const int32_t *verts_dev, const int64_t *vert_off_dev, int64_t nverts, const int32_t *boxes_dev,
                 const int64_t *out_off_dev, int64_t out_elems, int m, int elem_size, void *out_dev,
                 int32_t *status_dev, void *stream);
/* replaces  cv2.distanceTransform(mask, cv2.DIST_L2, 5) (float32 output),
 *           Polygon.get_centerline_optimized, video/analysis/shapes.py:742
 * m uint8 masks (non-zero = foreground) of a ragged packed buffer: mask i is (shapes_dev[2i],
 * shapes_dev[2i + 1]) = (h, w) at element offset offsets_dev[i] (int64) of masks_dev, and its
 * float32 distances go to the same offset of out_dev; both buffers hold `total` elements.  max_w:
 * the widest mask of the call (<= VA_DT_MAX_WIDTH; it sizes the LDS).  OpenCV's
 * distanceTransform_5x5, both passes in its order; a mask without background gives
 * DIST_MAX / 65536 everywhere.  status_dev[i]: VA_OK or VA_ERR_RANGE (mask not written). */
int va_distance_transform_l2_5(const uint8_t *masks_dev, const int32_t *shapes_dev, const int64_t *offsets_dev,
                               int64_t total, int m, int max_w, float *out_dev, int32_t *status_dev, void *stream);

/* ------------------------------------------------------------------ A14 Guo-Hall thinning
 * replaces  thinning.guo_hall_thinning(img), the `guo-hall` method of mask_thinning,
 *           video/analysis/image.py:236-241
 * The definition ("Guo-Hall thinning"): foreground is img != 0; with p2 .. p9 the neighbours
 * N, NE, E, SE, S, SW, W, NW of a pixel, a foreground pixel with 1 <= y <= h - 2 and 1 <= x <= w - 2 is
 * deleted by a sub-iteration iff C == 1, 2 <= min(N1, N2) <= 3 and m == 0, where
 *   C  = (!p2 & (p3|p4)) + (!p4 & (p5|p6)) + (!p6 & (p7|p8)) + (!p8 & (p9|p2)),
 *   N1 = (p9|p2) + (p3|p4) + (p5|p6) + (p7|p8),   N2 = (p2|p3) + (p4|p5) + (p6|p7) + (p8|p9),
 *   m  = (p6 | p7 | !p9) & p8 in sub-iteration 0,  (p2 | p3 | !p5) & p4 in sub-iteration 1,
 * all of the state before the sub-iteration (parallel deletion).  An iteration is sub-iteration 0 then 1;
 * iterations repeat until one deletes nothing, and the count includes that last one.  Pixels of the first
 * and last row and column are never deleted (a mask with h < 3 or w < 3 comes back unchanged, 1 iteration).
 * The output holds the input's own value where the pixel survives and 0 elsewhere; the input is not
 * modified (the module thins in place).
 * Limits: the resident call keeps a mask in LDS at one bit per pixel, rows padded to 32-bit words:
 * h * ((w + 31) / 32) <= VA_THIN_RESIDENT_MAX_WORDS (60 KiB, so that two workgroups of the largest size
 * still share a CU's 160 KiB); beyond it the item's status is VA_ERR_RANGE and its box is not written.
 * The tiled call takes 1 .. 65535 frames of fewer than 2^29 pixels and at most VA_THIN_MAX_ROWS rows (its
 * grid has one row of tiles per 32 .. 60 image rows), fewer than 2^31 packed words in all; beyond that it
 * returns VA_ERR_INVALID (va_guo_hall_thinning_scratch_bytes returns 0). */
#define VA_THIN_RESIDENT_MAX_WORDS 15360
#define VA_THIN_MAX_SUB_ITERATIONS 16
#define VA_THIN_MAX_POLL 64
#define VA_THIN_MAX_ROWS (65535 * 32)
/* m uint8 masks of a ragged packed buffer, laid out as for va_distance_transform_l2_5: mask i is
 * (shapes_dev[2i], shapes_dev[2i + 1]) = (h, w) at element offset offsets_dev[i] (int64) of masks_dev,
 * and its skeleton goes to the same offset of out_dev; both buffers hold `total` elements.  max_words:
 * the largest h * ((w + 31) / 32) of the call (<= VA_THIN_RESIDENT_MAX_WORDS; it sizes the LDS).  One
 * workgroup runs a mask to its fixed point; iterations_out_dev[i] (int32) is its iteration count,
 * status_dev[i] VA_OK or VA_ERR_RANGE.  Nothing is copied: the call enqueues one kernel on `stream`. */
int va_guo_hall_thinning_batch(const uint8_t *masks_dev, const int32_t *shapes_dev, const int64_t *offsets_dev,
                               int64_t total, int m, int max_words, uint8_t *out_dev,
                               int32_t *iterations_out_dev, int32_t *status_dev, void *stream);
/* scratch of the call below: two bit planes of the stack and the iteration flags */
size_t va_guo_hall_thinning_scratch_bytes(int n, int h, int w);
/* the same definition (video/analysis/image.py:236-241) for an (n, h, w) stack of equal-sized uint8
 * frames of any size: bit planes ping-pong in scratch_dev (va_guo_hall_thinning_scratch_bytes), every
 * launch advances all tiles by sub_iterations (even, 2 .. VA_THIN_MAX_SUB_ITERATIONS; 0: the default 16)
 * sub-iterations, and the host reads one changed flag per iteration and frame after every poll_period
 * (1 .. VA_THIN_MAX_POLL; 0: the default 2) launches -- it synchronises `stream` that often, and stops
 * after an iteration that deleted nothing in any frame.  dst_dev: (n, h, w) skeletons (enqueued; complete
 * when `stream` is).  iterations_out (host, nullable): n int32 iteration counts as the definition gives
 * them.  stats_out (host, nullable): 2 int32, the tile launches and the host reads of this call.
 * Because it waits for `stream` and copies the flags to the host inside the call, it cannot be captured
 * into a graph (va_guo_hall_thinning_batch can: it only enqueues). */
int va_guo_hall_thinning_u8(const uint8_t *src_dev, void *scratch_dev, size_t scratch_bytes, uint8_t *dst_dev,
                            int n, int h, int w, int sub_iterations, int poll_period, int32_t *iterations_out,
                            int32_t *stats_out, void *stream);

/* ------------------------------------------------------------------ A16 skeleton graphs
 * replaces  MorphologicalGraph.from_skeleton(skeleton, post_process=False), video/analysis/morphological_graph.py:
 *           287-378, by a definition that depends on no visiting order (the reference pops from a dict and a set)
 * The definition ("Skeleton graphs"): foreground is img != 0, everything outside an item is
 * background, pixel index i = y * w + x.  m-adjacency: two foreground pixels that share an edge are adjacent; two
 * that touch only at a corner are adjacent iff neither of the two pixels that share an edge with both is
 * foreground.  d(p) = number of pixels adjacent to p (0 .. 4).  Node pixels: d != 2, and the pixel of smallest
 * index of a connected component whose pixels all have d == 2 (a pure ring).  A node is a maximal set of node
 * pixels connected by adjacency; its anchor, which gives its coordinates, is its pixel of largest d, smallest
 * index on ties; nodes of an item are numbered by ascending smallest pixel index.  Every other foreground pixel is
 * a chain pixel (exactly two adjacent pixels).  An edge is a maximal path c1 .. ck (k >= 1) of chain pixels from a
 * node pixel a adjacent to c1 to a node pixel b adjacent to ck; it starts at the end whose pair (index(a),
 * index(c1)) is lexicographically smaller, and the edges of an item are ordered by that pair.  Its curve:
 * anchor(A), a unless it is the anchor, c1 .. ck, b unless it is the anchor, anchor(B); its length: every segment
 * the float32 sqrt(dx * dx + dy * dy) (correctly rounded), the roots summed in double in point order.
 * Input: m uint8 items of a ragged packed buffer, laid out as for va_guo_hall_thinning_batch (an (n, h, w) stack
 * is the same layout with equal shapes); offsets ascend and items do not overlap; total < 2^31 - 2 elements.
 * An item of 2^29 elements or more, or one that would reach beyond `total`, is treated as empty (no nodes).
 *   counts_dev[m][2]                 (nodes, edges) of each item
 *   totals_dev[3]                    nodes, edges and points of the whole batch, always the true totals
 *   nodes_dev[cap_nodes]             one record per node; item i's nodes follow those of items 0 .. i - 1
 *   edges_dev[cap_edges]             one record per edge, in the same order; node_a, node_b are item-local numbers
 *   point_off_dev[cap_edges + 1]     exclusive scan of the records' npoints
 *   points_dev[cap_points][2]        int32 (x, y) in item coordinates, 8-byte aligned
 * Nothing is written beyond a capacity: slots 0 .. min(total, cap) - 1 have their records and offsets, and an
 * edge has its points when all of them lie below cap_points (such edges form a prefix).  Exceeding a capacity is
 * no error: compare totals_dev with the capacities and call again with room.  Slots and positions come from
 * counts and scans, never from the order of atomics: two calls write identical bytes.  Everything is enqueued on
 * `stream`, in the caller's workspace only (va_skeleton_graph_workspace_bytes, 30 bytes per packed element). */
typedef struct va_skeleton_node {
    int32_t item, x, y;                         /* item index; the anchor */
    int32_t degree;                             /* edge ends at the node (a loop counts twice) */
    int32_t pixels;                             /* pixels of the node's set */
} va_skeleton_node;
typedef struct va_skeleton_edge {
    int32_t item, node_a, node_b, npoints;      /* node numbers within the item, points of the curve */
    double length;
} va_skeleton_edge;
size_t va_skeleton_graph_workspace_bytes(int64_t total, int m);
int va_skeleton_graph(const uint8_t *masks_dev, const int32_t *shapes_dev, const int64_t *offsets_dev, int64_t total,
                      int m, int32_t *counts_dev, int64_t *totals_dev, va_skeleton_node *nodes_dev,
                      int64_t cap_nodes, va_skeleton_edge *edges_dev, int64_t *point_off_dev, int64_t cap_edges,
                      int32_t *points_dev, int64_t cap_points, void *workspace_dev, size_t workspace_bytes,
                      void *stream);

/* ------------------------------------------------------------------ A15 affine warps and line scans
 * replaces  cv2.warpAffine(img, matrix, dsize) of single-channel uint8 images (INTER_LINEAR, BORDER_CONSTANT 0) in
 *           line_scan, video/analysis/image.py:102-106 (the strip and its mean over the rows), and
 *           get_subimage, video/analysis/image.py:81-82
 * The definition ("Affine warps and line scans") is the classical fixed-point path of OpenCV
 * 2.4 .. 4.10, not the float kernels of 4.11 and later.  Unless VA_WARP_INVERSE_MAP is set, the forward 2x3
 * float64 matrix M is inverted in float64 as cv::warpAffine does: D = M0 M4 - M1 M3; D = D != 0 ? 1/D : 0;
 * A11 = M4 D; A22 = M0 D; M0 = A11; M1 *= -D; M3 *= -D; M4 = A22; b1 = -M0 M2 - M1 M5; b2 = -M3 M2 - M4 M5;
 * M2 = b1; M5 = b2.  Destination pixel (x, y) then reads the source at (R: nearest integer, halves to even)
 *   X = (R((M1 y + M2) 1024) + 16 + R(M0 x 1024)) >> 5,   Y = (R((M4 y + M5) 1024) + 16 + R(M3 x 1024)) >> 5,
 *   sx = X >> 5, sy = Y >> 5, fx = X & 31, fy = Y & 31 (arithmetic shifts), and with v00, v01, v10, v11 the
 *   source at (sy, sx), (sy, sx + 1), (sy + 1, sx), (sy + 1, sx + 1), 0 outside the image,
 *   out = ((32 - fx)(32 - fy) v00 + fx (32 - fy) v01 + (32 - fx) fy v10 + fx fy v11 + 512) >> 10.
 * Limits of one item (beyond them its status is VA_ERR_RANGE and nothing of it is written; the other items
 * run): sides 0 .. VA_WARP_MAX_SIDE, and (|M0| (w - 1) + |M1| (h - 1) + |M2|) 1024 < VA_WARP_COORD_LIMIT for
 * the inverted matrix and the destination's size, likewise for its second row (OpenCV saturates there); a
 * frame index outside 0 .. n_frames - 1 or an output range outside 0 .. total_out are refused the same way.
 * Frames: n_frames uint8 frames of h x w, fewer than 2^29 pixels each. */
#define VA_WARP_MAX_SIDE 32767
#define VA_WARP_COORD_LIMIT (1 << 30)
#define VA_WARP_INVERSE_MAP 1 /* flag bit: the matrix maps destination to source (cv2.WARP_INVERSE_MAP) */
#define VA_WARP_CHUNK 64      /* columns of a strip per work item of va_line_scan_u8 */
#define VA_WARP_TILE_W 64     /* tile of va_warp_affine_u8 */
#define VA_WARP_TILE_H 16
/* m line scans in one launch.  Scan i warps frame frame_dev[i] (int32) with the forward matrix
 * matrices_dev[6 i .. 6 i + 5] (float64) into a strip of shapes_dev[2 i] rows and shapes_dev[2 i + 1] columns
 * (int32) that is never stored: sums_out_dev[out_off_dev[i] + x] (int32; out_off_dev int64, element offsets
 * into total_out elements) receives the sum of column x over the rows, which is exact in any order; the
 * profile of line_scan is that sum divided by the rows.  chunk_prefix_dev (int32, m entries): entry i is the
 * number of work items before scan i, a scan of c columns having max(1, ceil(c / VA_WARP_CHUNK)) of them;
 * total_chunks: their total.  A table that disagrees with the shapes leaves columns unwritten, never writes
 * outside a scan's range.  status_dev[i] (int32): VA_OK or VA_ERR_RANGE.  Nothing is copied: the call
 * enqueues one kernel on `stream`. */
int va_line_scan_u8(const uint8_t *frames_dev, int n_frames, int h, int w, int m, const int32_t *frame_dev,
                    const double *matrices_dev, const int32_t *shapes_dev, const int64_t *out_off_dev,
                    const int32_t *chunk_prefix_dev, int total_chunks, int64_t total_out, int32_t *sums_out_dev,
                    int32_t *status_dev, void *stream);
/* m warps in one launch, the same per-item tables; shapes_dev[2 i], shapes_dev[2 i + 1] = (dh, dw) of
 * destination i, written row-major as uint8 at byte offset out_off_dev[i] of out_dev (total_out bytes);
 * flags_dev[i] (int32): VA_WARP_INVERSE_MAP or 0.  tile_prefix_dev (int32, m entries): the number of work
 * items before item i, an item having max(1, ceil(dw / VA_WARP_TILE_W) * ceil(dh / VA_WARP_TILE_H)) of them;
 * total_tiles: their total.  One kernel on `stream`, nothing copied. */
int va_warp_affine_u8(const uint8_t *frames_dev, int n_frames, int h, int w, int m, const int32_t *frame_dev,
                      const double *matrices_dev, const int32_t *shapes_dev, const int32_t *flags_dev,
                      const int64_t *out_off_dev, const int32_t *tile_prefix_dev, int total_tiles, int64_t total_out,
                      uint8_t *out_dev, int32_t *status_dev, void *stream);

/* ------------------------------------------------------------------ A17 outline queries
 * replaces  line_string.intersection(ray) and the choice of the nearest point in get_ray_hitpoint,
 *           video/analysis/regions.py:353-391, once per ray of the angle loops of get_ray_intersections, :395-405,
 *           and get_farthest_ray_intersection, :409-426, and
 *           Polygon.contains (shapely's contains), video/analysis/shapes.py:552-554
 * The definition is pinned in DESIGN.md §9, "Outline queries".  All arithmetic is float64, every product, sum and
 * quotient rounded on its own.  Outlines: m of them in one packed buffer, points_dev[npoints][2] float64 (x, y);
 * outline o owns points point_off_dev[o] .. point_off_dev[o + 1] - 1 (int64, m + 1 entries, ascending).  Query k
 * names its outline in index_dev[k] (int32).  A group of `lanes` lanes takes one query and strides over the
 * outline's edges: lanes = 8 or 64, or 0 for the library's choice (64 when the outlines hold
 * VA_OUTLINE_WIDE_MIN_POINTS points or more on average, else 8); anything else is VA_ERR_INVALID.  Both widths
 * write identical bytes.  Limits: an outline of at most 2^31 - 2 points; at most (2^31 - 1) * 256 / lanes
 * queries (more: VA_ERR_INVALID).  A query whose index is outside 0 .. m - 1, whose outline's offsets are not
 * inside 0 .. npoints in order, or whose outline has more points, is refused: it reads nothing else and writes
 * the refused markers below; the other queries run.  q == 0 or m == 0 enqueues nothing and returns VA_OK; a NULL
 * pointer with q > 0 is VA_ERR_INVALID.  Each call enqueues one kernel on `stream`, copies nothing and needs no
 * workspace. */
#define VA_OUTLINE_WIDE_MIN_POINTS 384
/* q rays.  Ray k runs from A = anchors_dev[k] to F = fars_dev[k] (float64 (x, y) each), d = F - A.  Edge i of its
 * outline runs from P = point i to Q = point i + 1; closed_dev[o] != 0 adds the edge from the last point to the
 * first.  With e = Q - P and w = P - A:
 *   den = d.x e.y - d.y e.x   tn = w.x e.y - w.y e.x   un = w.x d.y - w.y d.x   t = tn / den   u = un / den
 * and edge i is hit iff den != 0, 0 <= t <= 1 and 0 <= u <= 1 (a NaN fails; -0.0 passes).  The ray's hit is the
 * hitting edge with the smallest pair (t, i), -0.0 and +0.0 being equal:
 *   t_out_dev[k] = its t, hits_out_dev[k] = (A.x + t d.x, A.y + t d.y), edge_out_dev[k] = i (int32),
 *   count_out_dev[k] = the number of hitting edges (int32).
 * Without a hit t and both coordinates are the quiet NaN 0x7FF8000000000000, edge = -1 and count = 0; a refused
 * query has the same NaNs, edge = -1 and count = -1.  No root and no trigonometric function is evaluated:
 * distances and the far points of the angle forms are the host's. */
int va_ray_hits(const double *points_dev, const int64_t *point_off_dev, const uint8_t *closed_dev, int64_t npoints,
                int m, const double *anchors_dev, const double *fars_dev, const int32_t *index_dev, int64_t q,
                int lanes, double *t_out_dev, double *hits_out_dev, int32_t *edge_out_dev, int32_t *count_out_dev,
                void *stream);
/* q points.  Point k is X = query_dev[k] (float64 (x, y)); its outline is a ring, always closed.  For every edge
 * P -> Q, c = (Q.x - P.x)(X.y - P.y) - (Q.y - P.y)(X.x - P.x).  If c == 0 and X lies in the edge's coordinate box
 * (comparisons that a NaN fails), X is on the boundary and the result is 0.  Otherwise the edge toggles the
 * answer iff (P.y > X.y) != (Q.y > X.y) and (c > 0 if Q.y > P.y, else c < 0).  inside_out_dev[k] (uint8) = 1 iff
 * no edge reported the boundary and the number of toggles is odd, else 0; a ring of fewer than three points and a
 * non-finite point give 0; a refused query gives 2. */
int va_points_in_outlines(const double *points_dev, const int64_t *point_off_dev, int64_t npoints, int m,
                          const double *query_dev, const int32_t *index_dev, int64_t q, int lanes,
                          uint8_t *inside_out_dev, void *stream);

/* ------------------------------------------------------------------ A18 equidistant curves
 * replaces  make_curve_equidistant, video/analysis/curves.py:103-148, once per curve: the three calls per polygon
 *           of Polygon.get_centerline_optimized, video/analysis/shapes.py:727-757, and the one per curve of
 *           ActiveContour.find_contour, video/analysis/active_contour.py
 * The definition is pinned in DESIGN.md §9, "Equidistant curves".  Curves: m of them in one packed buffer,
 * points_dev[npoints][2] float64 (x, y); curve k owns points point_off_dev[k] .. point_off_dev[k + 1] - 1 (int64,
 * m + 1 entries, ascending).  spacing_dev[k] (float64) > 0: the curve is walked and a point dropped every
 * L / rint(L / spacing) of its float32-rule length L (L < spacing: the result is the input); spacing_dev[k] == 0:
 * count_dev[k] (int32, >= 1) points at equal arc length (count_dev is read only for such curves, and may be NULL
 * when there are none).  translate_dev: NULL, or (tx, ty) float64 per curve, added to every coordinate of the
 * result, one rounded add each.
 * Three launches on `stream`, one lane per curve, nothing copied, no workspace:
 *   out_count_dev[k] (int32)   the number of points of curve k's result
 *   out_off_dev[k]   (int64, m + 1 entries)  its first slot in out_points_dev; out_off_dev[m] = the total
 *   in_length_dev[k] (float64) L in spacing mode, the arc total s[-1] in count mode
 *   status_dev[k]    (int32)   VA_OK, or VA_ERR_RANGE for a curve that is not run: fewer than 2 or more than
 *                    VA_CURVES_MAX_POINTS points, offsets out of order or outside 0 .. npoints, a negative or NaN
 *                    spacing, a count < 1, rint(L / spacing) above VA_CURVES_MAX_STEPS, or a walk that drops more
 *                    than 2 rint(L / spacing) + n + 2 points; such a curve has count 0 and lengths 0
 *   totals_dev[0]    (int64)   the total number of points
 *   out_points_dev[cap_points][2] (float64)  the results, curve after curve, written only when the total is at
 *                    most cap_points: a caller that reads a larger total runs again with that much room
 *   out_length_dev[k] (float64) the float32-rule length (cv2.arcLength of the float32 casts) of what was written
 *                    for curve k, 0 when nothing was
 * Two runs write identical bytes.  m == 0 enqueues nothing; a NULL pointer with m > 0 (translate_dev and, without
 * a count-mode curve, count_dev apart), a negative count or capacity and a misaligned pointer are VA_ERR_INVALID. */
#define VA_CURVES_MAX_POINTS (1 << 24)
#define VA_CURVES_MAX_STEPS (1 << 20)
int va_curves_equidistant(const double *points_dev, const int64_t *point_off_dev, int64_t npoints, int m,
                          const double *spacing_dev, const int32_t *count_dev, const double *translate_dev,
                          int32_t *out_count_dev, int64_t *out_off_dev, double *in_length_dev, int32_t *status_dev,
                          int64_t *totals_dev, double *out_points_dev, int64_t cap_points, double *out_length_dev,
                          void *stream);

/* ------------------------------------------------------------------ A23 simplification
 * replaces  simplify_curve, video/analysis/curves.py:22 (the rdp of external/simplify_polygon_rdp.py), once per
 *           curve, and simplify_contour, video/analysis/regions.py:307-325 (simplify_ring and simplify_line of
 *           external/simplify_polygon_visvalingam.py), once per ring
 * The two definitions are pinned in DESIGN.md §9, "Simplification".  Curves: m of them in one packed buffer, laid
 * out as for va_curves_equidistant: points_dev[npoints][2] float64 (x, y); curve k owns points point_off_dev[k] ..
 * point_off_dev[k + 1] - 1 (int64, m + 1 entries, ascending).  One tolerance per curve (float64).  Both calls write
 *   keep_dev[npoints]  (uint8)  1 for a point that is kept, 0 for one that is dropped; the simplified curve k is its
 *                      points with flag 1, in order.  Only the slots of the m curves are written.
 *   out_count_dev[k]   (int32)  the number of points kept; 0 for a ring that vanishes
 *   status_dev[k]      (int32)  VA_OK, or VA_ERR_RANGE for a curve that is not run: offsets out of order or outside
 *                      0 .. npoints, a NaN tolerance, or more than VA_SIMPLIFY_MAX_POINTS points.  Such a curve has
 *                      the count 0 and, where its offsets lie inside the buffer, all its flags 0.
 *
 * va_simplify_rdp: Ramer-Douglas-Peucker on open curves, one wave per curve (in launches of 65535 curves).  Points
 * 0 and n - 1 are kept.  A span (i0, i1) with i1 - i0 >= 2 measures every point strictly between its ends against
 * its chord: |x0.x - x1.x| when both ends have the same x, else |a x b| / |a| with a = x2 - x1, b = x1 - x0, every
 * operation rounded on its own; the first point of largest distance is kept and splits the span when that
 * distance exceeds max(eps_dev[k], 0).  A curve of fewer than 3 points keeps all its points.
 *
 * va_simplify_visvalingam: the reference's heap procedure, one lane per curve.  closed = 1: every curve is a ring
 * without a closing duplicate; points go while more than 2 are left and the smallest triangle area is below
 * thr_dev[k]; a ring that ends with fewer than 3 points, or has fewer than 3, keeps none (count 0: the reference's
 * None).  closed = 0: open lines, both ends fixed; a line of fewer than 3 points keeps all its points.
 * workspace_dev: va_simplify_visvalingam_workspace_bytes(npoints) bytes, 12 per point (heap, prev, next, int32);
 * what it holds before the call does not matter.
 *
 * Two runs write identical bytes.  m == 0 enqueues nothing; a NULL pointer with m > 0, a negative count, a
 * misaligned pointer, closed other than 0 or 1 and a workspace that is too small are VA_ERR_INVALID. */
#define VA_SIMPLIFY_MAX_POINTS (1 << 24)
int va_simplify_rdp(const double *points_dev, const int64_t *point_off_dev, int64_t npoints, int m,
                    const double *eps_dev, uint8_t *keep_dev, int32_t *out_count_dev, int32_t *status_dev,
                    void *stream);
size_t va_simplify_visvalingam_workspace_bytes(int64_t npoints);
int va_simplify_visvalingam(const double *points_dev, const int64_t *point_off_dev, int64_t npoints, int m,
                            const double *thr_dev, int closed, uint8_t *keep_dev, int32_t *out_count_dev,
                            int32_t *status_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ A19 composer
 * replaces  VideoComposer, video/io/composer.py: set_frame's copy of a monochrome frame into a colour video
 *           (:103-105, :119-123), highlight_mask (:131-154), add_image (:168-186), blend_image (:190-210) by
 *           va_compose_layers_u8; cv2.drawContours (:236), cv2.polylines (:257), cv2.rectangle (:284) and
 *           cv2.circle (:298), all with thickness 1 or, for the circle, -1, by va_draw_u8
 * The definitions are pinned in DESIGN.md §9, "Composer".  Frames are uint8, (n, h, w) or (n, h, w, 3) with RGB
 * interleaved.
 *
 * va_compose_layers_u8: dst frame f = src frame f (c_src channels; a monochrome source is copied into the three
 * channels of a colour destination) with the layers layer_off_dev[f] .. layer_off_dev[f + 1] - 1 (int64, n + 1
 * entries) of layers_dev applied in order.  A layer reads an image of image_channels (1, or 3 on a colour
 * destination; a monochrome image counts for all three channels) at byte image_off of images_dev and, with
 * mask_off >= 0, a (h, w) uint8 mask at byte mask_off of masks_dev: it changes the pixels whose mask byte is non-zero,
 * every pixel with mask_off == -1.
 *   VA_COMPOSE_HIGHLIGHT  v = (uint8) trunc((double) alpha + factor * v) in float64, product and sum rounded
 *                         separately; on channel `channel` of a colour frame, on all three for channel == -1
 *                         (alpha: the strength 0 .. 255, factor: (255 - strength) / 255; no image)
 *   VA_COMPOSE_ADD        v = min(255, v + u)
 *   VA_COMPOSE_BLEND      v = the float32 alpha * v + beta * u, two rounded products and one rounded sum, rounded
 *                         to the nearest integer with ties to even and saturated to 0 .. 255
 * One launch, 16 pixels of a row per lane; src_dev == dst_dev is allowed when c_src == c, and then a frame without
 * layers is not touched.  A layer whose kind, channels or offsets are not valid for the buffers' sizes is not
 * applied, and a frame whose layer range leaves the table gets none: nothing outside the buffers is read.
 * n == 0, h == 0, w == 0, and nlayers == 0 in place enqueue nothing.  c_src, c outside {1, 3}, c_src > c, distinct
 * pointers required for c_src != c, negative counts, NULL pointers and frames of 2^29 pixels or more are
 * VA_ERR_INVALID.
 *
 * va_draw_u8: the commands cmd_off_dev[f] .. cmd_off_dev[f + 1] - 1 (int64, n + 1 entries) of cmds_dev drawn into
 * frame f in order, one workgroup per frame: the final value of a pixel is the colour of the last command in list
 * order that covers it.  Lines are 8-connected (clipLine, then the left-to-right LineIterator), thickness 1, shift 0.
 *   VA_DRAW_POLYLINE  the points first .. first + count - 1 of points_dev[npoints][2] (int32 x, y): the segments
 *                     v[i - 1] -> v[i], and v[count - 1] -> v[0] with flags & 1 (closed); a closed polyline of
 *                     one point is that pixel, an open one and an empty one nothing
 *   VA_DRAW_CIRCLE    OpenCV's integer Circle around (cx, cy): the outline, or the filled disc with flags & 1;
 *                     radius 0 is one pixel, a negative radius nothing
 * color: byte 0 on a monochrome frame, bytes 0, 1, 2 = R, G, B on a colour one.
 * status_dev[f] (int32): VA_OK, or VA_ERR_RANGE for a frame that is left untouched: a command range outside
 * 0 .. ncmds, an unknown kind, a point range outside 0 .. npoints, a coordinate beyond +-VA_FILL_MAX_COORD or a
 * radius above it.  n == 0 and ncmds == 0 enqueue nothing (status_dev is not written).  c outside {1, 3}, negative
 * counts, NULL pointers and frames of 2^29 pixels or more are VA_ERR_INVALID. */
#define VA_COMPOSE_HIGHLIGHT 1
#define VA_COMPOSE_ADD 2
#define VA_COMPOSE_BLEND 3
#define VA_DRAW_POLYLINE 1
#define VA_DRAW_CIRCLE 2
typedef struct va_compose_layer {
    int32_t kind;           /* VA_COMPOSE_* */
    int32_t image_channels; /* 1 or 3 (0 for a highlight) */
    int32_t channel;        /* highlight: 0 .. 2, or -1 for all */
    int32_t reserved;
    int64_t image_off;      /* bytes into images_dev */
    int64_t mask_off;       /* bytes into masks_dev, or -1 */
    double factor;          /* highlight: (255 - strength) / 255 */
    float alpha;            /* highlight: strength; blend: (float)(1 - weight) */
    float beta;             /* blend: (float) weight */
} va_compose_layer;         /* 48 bytes */
typedef struct va_draw_cmd {
    int32_t kind;   /* VA_DRAW_* */
    int32_t flags;  /* bit 0: closed (polyline), filled (circle) */
    uint32_t color; /* R | G << 8 | B << 16, or the grey value */
    int32_t radius;
    int32_t cx, cy;
    int32_t count;  /* points of the polyline */
    int32_t reserved;
    int64_t first;  /* its first point in points_dev */
} va_draw_cmd;      /* 40 bytes */
int va_compose_layers_u8(const uint8_t *src_dev, int c_src, uint8_t *dst_dev, int n, int h, int w, int c,
                         const va_compose_layer *layers_dev, const int64_t *layer_off_dev, int64_t nlayers,
                         const uint8_t *images_dev, int64_t images_bytes, const uint8_t *masks_dev,
                         int64_t masks_bytes, void *stream);
int va_draw_u8(uint8_t *frames_dev, int n, int h, int w, int c, const va_draw_cmd *cmds_dev,
               const int64_t *cmd_off_dev, int64_t ncmds, const int32_t *points_dev, int64_t npoints,
               int32_t *status_dev, void *stream);
/* replaces  the cv2.findContours -> cv2.drawContours pair of add_contour given a mask, video/io/composer.py:228-237,
 *           without the host lists in between
 * va_draw_contours_u8: a result of va_find_contours, as it lies in device memory, drawn into a frame stack of n_out
 * frames: every contour a closed polyline of thickness 1, all in one colour (packed as in va_draw_cmd).  ncontours
 * and npoints are the valid slots and points: min(total, capacity) of the va_find_contours call.
 * Slot s owns the points v[0 .. k - 1] at point_off_dev[s] .. point_off_dev[s + 1] of points_dev; for k >= 1 its k
 * segments v[i] -> v[(i + 1) mod k] are drawn as va_draw_u8 draws a closed VA_DRAW_POLYLINE (a contour of one point
 * is that pixel, a slot with k == 0 draws nothing), into frame info_dev[s].frame, or, with frame_map_dev (int32,
 * n_src entries), into frame frame_map_dev[info_dev[s].frame]; a mapped value of -1 means that the source frame is
 * not drawn and is no error.  All stores carry one value: two calls write identical bytes.
 * Nothing outside the buffers is read or written.  A segment is not drawn, and status_dev[0] (int32) becomes
 * VA_ERR_RANGE, when its slot has info.frame outside 0 .. n_src - 1, a target that is neither -1 nor in
 * 0 .. n_out - 1, or offsets that are not 0 <= point_off[s] <= point_off[s + 1] <= npoints, or when one of its two
 * end points is beyond +-VA_FILL_MAX_COORD.  The slot of a point is found by binary search in point_off_dev; on a
 * table that is not sorted (at least one slot is refused then) a point is drawn only with the slot the search
 * finds for it.  Otherwise status_dev[0] is VA_OK; it is written on every call, ncontours == 0 included.
 * One launch per 2^30 lanes, a lane per slot and a lane per point; no workspace.  c outside {1, 3}, negative counts,
 * NULL pointers where data is required (frame_map_dev may be NULL) and frames of 2^29 pixels or more are
 * VA_ERR_INVALID. */
int va_draw_contours_u8(uint8_t *frames_dev, int n_out, int h, int w, int c,
                        const va_contour_info *info_dev, const int64_t *point_off_dev, int64_t ncontours,
                        const int32_t *points_dev, int64_t npoints,
                        const int32_t *frame_map_dev, int n_src, uint32_t color,
                        int32_t *status_dev, void *stream);

/* ------------------------------------------------------------------ A20 Motion-JPEG
 * replaces  the frame-by-frame cv2.VideoWriter.write of VideoWriterOpenCV, video/io/backend_opencv.py:240-242, behind
 *           write_video, video/io/file.py:50-64, by one baseline JFIF file per frame (the payload of an AVI's MJPG
 *           stream, video/io/backend_mjpeg.py here)
 * The stream is pinned in DESIGN.md §9, "Motion-JPEG": frames_dev uint8 (n, h, w) or (n, h, w, 3) RGB interleaved;
 * 4:4:4 or monochrome, the Annex K Huffman tables, one restart interval per MCU row.  qtables_dev: 128 bytes, the
 * luma and the chroma quantisation table in natural order (the chroma table is not read for c == 1).  header_dev:
 * the header_bytes bytes SOI .. SOS that every frame's file starts with (video.ops.jpeg_header builds them).
 *   sizes_out_dev[k]   (int64, n entries)      the bytes of frame k's file
 *   offsets_out_dev[k] (int64, n + 1 entries)  where it starts in bytes_out_dev; offsets_out_dev[n] = the total
 *   totals_dev[0]      (int64)                 the bytes needed, always
 *   bytes_out_dev[cap_bytes]                   frame k's file is bytes offsets[k] .. offsets[k + 1] - 1, written only
 *                      when the total is at most cap_bytes: a caller that reads a larger total runs again with that
 *                      much room (bytes_out_dev may be NULL with cap_bytes == 0)
 * Three launches on `stream` (count, scan, write), one workgroup per MCU row; every frame's bytes depend on that
 * frame alone and two runs write identical bytes.  n == 0 enqueues nothing.  VA_ERR_INVALID, before anything is
 * enqueued, in this order: a negative n or capacity, h, w or header_bytes below 1; c outside {1, 3}; a NULL
 * pointer; an int64 buffer that is not 8-byte aligned; h or w above 65535 (SOF0 holds 16 bits); more than 2^31 - 1
 * MCU rows in the stack. */
int va_jpeg_encode_u8(const uint8_t *frames_dev, int n, int h, int w, int c, const uint8_t *qtables_dev,
                      const uint8_t *header_dev, int header_bytes, int64_t *sizes_out_dev, int64_t *offsets_out_dev,
                      int64_t *totals_dev, uint8_t *bytes_out_dev, int64_t cap_bytes, void *stream);
/* The same with a luma sampling of luma_h x luma_v ("Subsampled Motion-JPEG encoding"): 1 x 1 writes
 * the bytes of va_jpeg_encode_u8; 2 x 1 (4:2:2) and 2 x 2 (4:2:0) take c == 3 and write MCUs of luma_h luma_v luma
 * blocks, Cb and Cr, whose chroma is the rounded box average, one restart interval and one workgroup per MCU row of
 * 8 luma_v pixel rows.  header_dev is video.ops.jpeg_header(h, w, 3, quality, (luma_h, luma_v)).  VA_ERR_INVALID as
 * above and in that order, then: a sampling other than 1 x 1, 2 x 1 and 2 x 2; a subsampled layout with c == 1. */
int va_jpeg_encode_sampled_u8(const uint8_t *frames_dev, int n, int h, int w, int c, int luma_h, int luma_v,
                              const uint8_t *qtables_dev, const uint8_t *header_dev, int header_bytes,
                              int64_t *sizes_out_dev, int64_t *offsets_out_dev, int64_t *totals_dev,
                              uint8_t *bytes_out_dev, int64_t cap_bytes, void *stream);
/* The same with Huffman tables made for the call ("Optimised Huffman tables"): one set of tables from
 * the symbol counts of all n frames, as libjpeg's jpeg_gen_optimal_table builds them, in the DHT segments of every
 * frame's header and in its entropy segments; every other byte is the plain call's.  The header is given in two
 * pieces: header_pre_dev, the pre_bytes bytes in front of the DHT segments (SOI .. SOF0), and header_post_dev, the
 * post_bytes bytes behind them (DRI, SOS); video.ops.jpeg_header_pieces cuts them from video.ops.jpeg_header.
 *   bits_vals_out_dev  uint8 [c == 1 ? 2 : 4][272]: per table, in the order DC0, AC0, DC1, AC1 of the header, BITS
 *                      (16) and HUFFVAL (256, the unused entries 0)
 * The other outputs, the capacity rule (a total above cap_bytes stores no file and reports the total) and n == 0
 * are the plain call's.  The counts are zeroed by the call; then five launches on `stream` (histogram, tables, count,
 * scan, write) with no host synchronisation between them; integer atomics only: two runs write identical bytes.
 * VA_ERR_INVALID as above and in that order, pre_bytes and post_bytes below 1 among the sizes and header_post_dev
 * and bits_vals_out_dev among the pointers. */
int va_jpeg_encode_optimized_u8(const uint8_t *frames_dev, int n, int h, int w, int c, int luma_h, int luma_v,
                                const uint8_t *qtables_dev, const uint8_t *header_pre_dev, int pre_bytes,
                                const uint8_t *header_post_dev, int post_bytes, uint8_t *bits_vals_out_dev,
                                int64_t *sizes_out_dev, int64_t *offsets_out_dev, int64_t *totals_dev,
                                uint8_t *bytes_out_dev, int64_t cap_bytes, void *stream);
/* The table construction alone: freq_dev int64 [t][256] symbol counts (non-negative, the sum of a table's 256 counts
 * at most 2^63 - 1: the merges add them in 64 bits, which the call cannot check; 8-byte aligned) ->
 * bits_vals_out_dev uint8 [t][272] as above, one wave per table.  A row of zeros gives an empty table.  t == 0
 * enqueues nothing; VA_ERR_INVALID for a negative t, a NULL pointer, counts that are not 8-byte aligned. */
int va_jpeg_optimal_tables(const int64_t *freq_dev, int t, uint8_t *bits_vals_out_dev, void *stream);

/* ------------------------------------------------------------------ A21 Motion-JPEG decoding
 * replaces  the frame-by-frame cv2.VideoCapture.read of VideoOpenCV.get_frame, video/io/backend_opencv.py, behind
 *           load_any_video, video/io/file.py:37-46, by one call per batch of stored baseline JPEG files (the chunks
 *           of an AVI's MJPG stream, video/io/backend_mjpeg.py here)
 * The decoder is pinned in DESIGN.md §9, "Motion-JPEG decoding".  All frames of a call share h, w, c, ri and the
 * tables; video.ops.jpeg_decode parses the headers, refuses what the decoder does not take and groups the frames.
 *   bytes_dev        the stored files, one behind the other
 *   offsets_dev      int64 (n + 1): file k is bytes offsets[k] .. offsets[k + 1] - 1
 *   scan_begin_dev   int64 (n): where file k's entropy data begins (the byte behind its SOS header), from the
 *                    file's start; a value outside the file is clamped into it
 *   c, ri            1 or 3 components (Y, or Y Cb Cr, all 1 x 1); the restart interval in MCUs, at least 1 (a
 *                    stream without DRI: the MCUs of a frame); a frame has ceil(MCUs / ri) segments
 *   qtables_dev      c * 64 bytes: the quantisation table of each component in natural order
 *   huff_dev         2 * c tables of VA_JPEG_HUFF_DECODE_BYTES bytes: the DC and the AC table of each component as
 *                    video.ops builds them from the DHT segments (va_jpeg_decode_math.h, HuffDecode); huff_bytes
 *                    is their size.  Whatever they hold, nothing outside them is read.
 *   frames_out_dev   uint8 (n, h, w) or (n, h, w, 3) RGB interleaved; every pixel is written, nothing else
 *   status_out_dev   int32 (n): 0 or the VA_JPEG_STATUS_* bits; blocks at and behind an error in their segment, and
 *                    the blocks of a missing segment, decode as zero coefficients (sample 128)
 *   workspace_dev    workspace_bytes bytes, 16-byte aligned.  va_jpeg_decode_workspace_bytes(n, h, w, c, ri) holds the
 *                    whole batch (2 bytes per padded sample and 16 bytes per segment; 0 for arguments the call would
 *                    refuse); with less the call runs in chunks of as many frames as fit, with the same result.
 * Three launches on `stream` per chunk (locate, entropy, reconstruct).  Nothing is read outside a file's bytes or
 * written outside its pixels whatever the bytes are, a hostile stream costs no more than a valid one of its
 * length, and two runs write identical bytes.  n == 0 enqueues nothing.  VA_ERR_INVALID, before anything is
 * enqueued, in this order: a negative n or workspace_bytes, h, w or ri below 1; c outside {1, 3}; a NULL pointer;
 * offsets_dev or scan_begin_dev not 8-byte, huff_dev or status_out_dev not 4-byte, workspace_dev not 16-byte
 * aligned; h or w above 65535 (SOF0 holds 16 bits); huff_bytes other than 2 * c * VA_JPEG_HUFF_DECODE_BYTES.  Then
 * VA_ERR_RANGE for a workspace that does not hold one frame. */
#define VA_JPEG_STATUS_BAD_CODE 1  /* a code in no table, a DC category > 11, an AC size > 10, a DC value outside
                                      -2048 .. 2047 */
#define VA_JPEG_STATUS_OVERRUN 2   /* a coefficient index beyond 63 */
#define VA_JPEG_STATUS_TRUNCATED 4 /* bits are needed beyond the segment's end */
#define VA_JPEG_STATUS_MARKER 8    /* the scan did not end on EOI, or has another number of segments */
#define VA_JPEG_HUFF_DECODE_BYTES 1416
size_t va_jpeg_decode_workspace_bytes(int n, int h, int w, int c, int ri);
int va_jpeg_decode_u8(const uint8_t *bytes_dev, const int64_t *offsets_dev, const int64_t *scan_begin_dev, int n, int h,
                      int w, int c, int ri, const uint8_t *qtables_dev, const void *huff_dev, int huff_bytes,
                      uint8_t *frames_out_dev, int32_t *status_out_dev, void *workspace_dev, int64_t workspace_bytes,
                      void *stream);

/* ------------------------------------------------------------------ A22 Motion-JPEG decoding, 4:2:0 and 4:2:2
 * replaces  the same cv2.VideoCapture.read of VideoOpenCV.get_frame, video/io/backend_opencv.py, behind
 *           load_any_video, video/io/file.py:37-46, for the files that cameras and other encoders write: chroma at
 *           half resolution
 * The arguments and the contract of va_jpeg_decode_u8, and behind ri the sampling factors of the luma component
 * ("Subsampled Motion-JPEG decoding"):
 *   luma_h, luma_v   1, 1: the bytes va_jpeg_decode_u8 writes.  2, 1 (4:2:2) or 2, 2 (4:2:0) with c == 3: Cb and Cr are
 *                    1 x 1, an MCU covers 8 luma_h x 8 luma_v pixels and holds the Y blocks row by row, then Cb, Cr;
 *                    ri and the segments count these MCUs; the chroma planes are upsampled with libjpeg's triangle
 *                    filter in integers (replicated where the frame has at most 4 columns) before the colour
 *                    conversion.  After an error the MCU's earlier blocks keep their coefficients.
 *   workspace_dev    va_jpeg_decode_sampled_workspace_bytes(n, h, w, c, ri, luma_h, luma_v) holds the whole batch: as
 *                    above, and for a subsampled file 1 byte per padded chroma sample more
 * Four launches per chunk of subsampled frames (locate, entropy, chroma planes, pixels).  VA_ERR_INVALID in the order
 * of va_jpeg_decode_u8, with sampling factors other than these three, or 2 x 1 / 2 x 2 with c == 1, refused behind
 * "c outside {1, 3}"; then VA_ERR_RANGE. */
size_t va_jpeg_decode_sampled_workspace_bytes(int n, int h, int w, int c, int ri, int luma_h, int luma_v);
int va_jpeg_decode_sampled_u8(const uint8_t *bytes_dev, const int64_t *offsets_dev, const int64_t *scan_begin_dev, int n,
                              int h, int w, int c, int ri, int luma_h, int luma_v, const uint8_t *qtables_dev,
                              const void *huff_dev, int huff_bytes, uint8_t *frames_out_dev, int32_t *status_out_dev,
                              void *workspace_dev, int64_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------ A24 Motion-JPEG decoding, frames without restart markers
 * replaces  the same cv2.VideoCapture.read of VideoOpenCV.get_frame, video/io/backend_opencv.py, behind
 *           load_any_video, video/io/file.py:37-46, for the files that cameras, libjpeg and Pillow write by default: no
 *           DRI, so a frame is one entropy segment, which the entries above decode with one lane
 * The arguments and the contract of va_jpeg_decode_sampled_u8 without ri (a frame is one segment; a restart marker in
 * it is a marker-sequence error as there), and behind workspace_bytes ("Split Motion-JPEG decoding"):
 *   sub_bytes        the raw bytes of a subsequence, a multiple of 16 in 16 .. 65536: a frame's segment is decoded by
 *                    one lane per subsequence, which find the serial decoder's states by self-synchronisation
 *   max_rounds       0 or more rounds of the scan; a frame that has not converged behind them falls back to the one
 *                    lane of the entries above (0: every frame)
 *   max_scan_bytes   sizes the scan's grid: ceil(max_scan_bytes / sub_bytes) lanes a frame; a frame with more entropy
 *                    bytes falls back
 *   rounds_out_dev   int32 (n) or NULL: the last round in which a lane of the frame ran, -1 where the frame fell back
 *   workspace_dev    va_jpeg_decode_split_workspace_bytes(n, h, w, c, luma_h, luma_v, sub_bytes, max_scan_bytes) holds
 *                    the whole batch: as above, and 88 bytes per lane more; with less the call runs in chunks
 * Every output byte and status word is the one va_jpeg_decode_sampled_u8 writes for the same file with ri = its MCUs.
 * Per chunk: locate, max_rounds scan launches, check, a memset of the coefficients, write, seal, the fallback, and the
 * reconstruction launches; no host synchronisation.  Nothing is read outside a file's bytes or written outside its
 * pixels whatever the bytes are; a hostile stream costs at most what it costs the entries above plus max_rounds
 * rounds; two runs write identical bytes.  VA_ERR_INVALID in the order of va_jpeg_decode_sampled_u8 (rounds_out_dev
 * not 4-byte aligned with the other alignments), then sub_bytes, a negative max_rounds, max_scan_bytes outside
 * 0 .. 2^40; then VA_ERR_RANGE for a workspace that does not hold one frame. */
size_t va_jpeg_decode_split_workspace_bytes(int n, int h, int w, int c, int luma_h, int luma_v, int sub_bytes,
                                            int64_t max_scan_bytes);
int va_jpeg_decode_split_u8(const uint8_t *bytes_dev, const int64_t *offsets_dev, const int64_t *scan_begin_dev, int n,
                            int h, int w, int c, int luma_h, int luma_v, const uint8_t *qtables_dev,
                            const void *huff_dev, int huff_bytes, uint8_t *frames_out_dev, int32_t *status_out_dev,
                            void *workspace_dev, int64_t workspace_bytes, int sub_bytes, int max_rounds,
                            int64_t max_scan_bytes, int32_t *rounds_out_dev, void *stream);

/* ------------------------------------------------------------------ A9 contour moments
 * replaces  cv2.moments(contour), regionprops(contour=...), video/analysis/image.py:355, and
 *           cv2.moments(np.asarray(self.contour, np.float32)), Polygon.moments,
 *           video/analysis/shapes.py:527-533
 * Green's-theorem moments of n closed polygons, accumulated in float64 in OpenCV's point order
 * (bit-identical to its contourMoments; m00 >= 0 for either orientation; a degenerate contour
 * gives zeros; any n >= 0, one wave per contour in gridDim.x).  points_dev: (n, max_points, 2) int32 (is_float == 0) or float32 (x, y) -- e.g.
 * the output of va_largest_contour; npoints_dev[f] = points of contour f (NULL: max_points each).
 * moments_out_dev: (n, 10) float64 = m00 m10 m01 m20 m11 m02 m30 m21 m12 m03; the central and
 * normalised moments follow on the host (completeMomentState). */
int va_contour_moments(const void *points_dev, const int32_t *npoints_dev, int n, int max_points,
                       int is_float, double *moments_out_dev, void *stream);
/* the same for m contours of a ragged list, contour i = points point_off_dev[i] .. point_off_dev[i + 1]
 * (m + 1 offsets) -- the layout va_find_contours writes, so that the moments of every blob come from the
 * device-resident points.  The same sequential per-contour code, one wave per contour. */
int va_contour_moments_ragged(const void *points_dev, const int64_t *point_off_dev, int64_t m, int is_float,
                              double *moments_out_dev, void *stream);

/* ------------------------------------------------------------------ N2 small stencils
 * replaces  detect_peaks(img, include_plateaus), video/analysis/image.py:267-306:
 *           ndimage.maximum_filter(img, footprint=8-neighbourhood) == img, minus the
 *           binary_erosion(img == 0, 8-neighbourhood, border_value=1) background (plateaus), or
 *           img > maximum over the 8 neighbours.  dst: 0/1 u8 mask.
 * Shape (all of this section): any n >= 0, h, w >= 1 -- one-dimensional grids over all pixels, except the
 * four-samples-per-thread tail of va_mask_thinning_u8, which frames of more than 65535 rows do not take. */
int va_detect_peaks_u8(const uint8_t *src_dev, uint8_t *dst_dev, int n, int h, int w,
                       int include_plateaus, void *stream);
/* the same on float32 maps (the reference calls it on distance / correlation maps): comparisons in float,
 * background = (img == 0) */
int va_detect_peaks_f32(const float *src_dev, uint8_t *dst_dev, int n, int h, int w, int include_plateaus,
                        void *stream);
/* replaces  the python fallback of mask_thinning, video/analysis/image.py:243-258 (3x3 cross):
 *           eroded = cv2.erode(img); temp = cv2.dilate(eroded); cv2.subtract(img, temp, temp);
 *           cv2.bitwise_or(skel, temp, skel); img = eroded   ... until img is empty.
 * img_dev is consumed (used as ping-pong scratch with scratch_dev); skel_dev receives the
 * skeleton.  Synchronises `stream` once per 16 iterations (the loop's exit test reads one
 * survivor counter per iteration; steps past the emptying one change nothing). */
int va_mask_thinning_u8(uint8_t *img_dev, uint8_t *scratch_dev, uint8_t *skel_dev, int h, int w,
                        int *iterations_out, void *stream);
/* replaces  get_image_statistics, video/analysis/image.py:131-201: local mean and variance in a
 *           (2*ksize+1)^2 box or ellipse window of (img - prior), zero border.
 * kernel: 0 box, 1 ellipse.  mean_out_dev / var_out_dev: (n,h,w) float64; var_out may be NULL.
 * ksize >= 0; a window of one sample (ksize 0) has the variance 0/0 = NaN, as in the reference. */
int va_image_statistics_u8(const uint8_t *src_dev, double *mean_out_dev, double *var_out_dev, int n,
                           int h, int w, int kernel, int ksize, double prior, int exclude_center,
                           void *stream);

/* float32 images: truncated towards zero like the reference's `img.astype(np.int) - prior`
 * (video/analysis/image.py:175), then direct window sums in float64 */
int va_image_statistics_f32(const float *src_dev, double *mean_out_dev, double *var_out_dev, int n,
                            int h, int w, int kernel, int ksize, double prior, int exclude_center,
                            void *stream);

/* ------------------------------------------------------------------ fused pipeline
 * One handle per filter chain (not thread-safe; the reference's pull model is single-threaded,
 * video/io/base.py:207-223).  Runs, for a batch of n <= max_batch frames resident in HBM:
 *   bg-sub -> Gaussian -> threshold -> morphology ops -> labelling (+ stats)
 * i.e. FilterBackground -> FilterBlur -> FilterThreshold -> FilterMorphology ->
 * get_largest_region's label/areas, with bit-packed masks between the stages. */
typedef struct va_config {
    int32_t struct_size; /* = sizeof(va_config) */
    int32_t width, height, channels;
    int32_t dtype;     /* VA_U8 | VA_F32 */
    int32_t max_batch; /* frames per va_pipeline_run call, upper bound */
    int32_t bg_mode;   /* VA_BG_* */
    float bg_rate;     /* EMA rate */
    double sigma;      /* <= 0: no blur */
    int32_t thresh;    /* < 0: stop after the blur (no mask / labels) */
    int32_t maxval;    /* mask value written to mask_out (default 255) */
    int32_t morph_count;
    int32_t morph_op[VA_MAX_MORPH_OPS];
    int32_t morph_shape[VA_MAX_MORPH_OPS];
    int32_t morph_ksize[VA_MAX_MORPH_OPS];
    int32_t connectivity; /* 0: no labelling, 4, 8 */
    int32_t max_labels;   /* > 0: per-label stats capacity per frame */
    int32_t tap_rule;     /* VA_TAPS_CV4 (0, default) | VA_TAPS_CV3: the 8-bit Gaussian's tap set */
} va_config;

typedef struct va_pipeline va_pipeline_t;

int va_pipeline_create(const va_config *cfg, va_pipeline_t **out);
int va_pipeline_destroy(va_pipeline_t *p);
/* frames_dev: (n,H,W[,C]) of cfg.dtype (float32 pipelines: 16-byte aligned, as is filtered_out_dev;
 * VA_ERR_INVALID otherwise).  8-bit pipelines whose Gaussian is a single-launch kernel (va_pipeline_describe:
 * "mfma-i8" or "fused-lds") need frames_dev 16-byte aligned when there is no background model (with one, the
 * Gaussian reads the pipeline's own difference image and frames_dev may start anywhere), and "mfma-i8" needs
 * filtered_out_dev 4-byte aligned; VA_ERR_INVALID otherwise, checked before anything is enqueued: a rejected
 * run leaves the background model and n_seen as they were.  mask_out_dev may start at any byte, labels_out_dev
 * at any int32.  Any output may be NULL:
 *   filtered_out_dev : (n,H,W[,C]) cfg.dtype, the blurred background-subtracted frames
 *   mask_out_dev     : (n,H,W) u8 0/maxval after threshold + morphology
 *   labels_out_dev   : (n,H,W) int32
 *   counts_out_dev   : (n) int32 components per frame
 *   stats_out_dev    : (n,max_labels,16) int64
 * Shape: width, height >= 1 (a chain on frames too small for the single-launch Gaussians runs the generic
 * kernels: the same bytes), 0 <= n <= max_batch per run. */
int va_pipeline_run(va_pipeline_t *p, const void *frames_dev, int n, void *filtered_out_dev,
                    uint8_t *mask_out_dev, int32_t *labels_out_dev, int32_t *counts_out_dev,
                    int64_t *stats_out_dev, void *stream);
/* Overlapped runs (off by default).  The chain's last kernel -- the write of the int32 label image and
 * the per-label statistics, which get_largest_region / regionprops consume
 * (video/analysis/regions.py:159-174) -- is bound by HBM stores, the stages before it by VALU and
 * latency.  With enable != 0 va_pipeline_run enqueues that write on a stream the pipeline owns, ordered
 * after the labelling, and returns; the next va_pipeline_run starts its background / blur / morphology /
 * labelling stages on the caller's stream at once, beside it (mask buffers and run tables exist twice).
 * Contract while enabled: labels_out / stats_out of a run are complete on a stream only after
 * va_pipeline_fence(p, that stream) (or a device synchronisation); counts_out / mask_out /
 * filtered_out stay ordered on the run's own stream as before.  A caller that hands consecutive runs
 * the same labels_out / stats_out buffer stays correct (the run's labelling stage then waits for the
 * previous write); alternate two buffers to overlap that stage as well.
 * va_pipeline_overlap synchronises the device; it allocates the second buffer set on first use.  The
 * deferred write runs as a persistent kernel of 4 workgroups per CU on a lowest-priority stream (bounded
 * footprint beside the caller's kernels); $VA_PAINT_WGS_PER_CU overrides the 4 for measurements (0: one
 * workgroup per row block), enable == 2 gives the stream default priority. */
int va_pipeline_overlap(va_pipeline_t *p, int enable);
/* make `stream` wait for every label-image write this pipeline has enqueued so far (asynchronous:
 * enqueues waits, never blocks the host) */
int va_pipeline_fence(va_pipeline_t *p, void *stream);
/* background-model state, so that a shard can start mid-video (SURVEY.md 5 "checkpoint") */
int va_bg_get_state(va_pipeline_t *p, void *state_host, size_t bytes, int64_t *n_seen);
int va_bg_set_state(va_pipeline_t *p, const void *state_host, size_t bytes, int64_t n_seen);
size_t va_bg_state_bytes(const va_pipeline_t *p);
/* name of the implementation used for the Gaussian stage ("fused-lds" / "generic") */
const char *va_pipeline_describe(const va_pipeline_t *p);

/* per-stage device time, measured with HIP events recorded on the run's own stream (what
 * bench.py's `roofline` object is computed from).  enable != 0 starts/reset recording; every
 * va_pipeline_run (enable > 1: every enable-th run, the first one included -- an event per stage costs
 * the stream about 2 % of the chain) then records one event per stage (never waits).  stage_times waits for the
 * last event and sums, per stage name, the elapsed ms and the number of launches.
 * names: capacity x 32 chars. */
int va_pipeline_profile(va_pipeline_t *p, int enable);
int va_pipeline_stage_times(va_pipeline_t *p, int capacity, char *names, double *total_ms,
                            int32_t *launches, int *nstages_out);

/* ------------------------------------------------------------------ test hooks
 * Same contracts as va_gaussian_u8 / va_morph_u8, but forcing one implementation so that the
 * parity tests can compare the generic two-pass Gaussian with the single-launch kernels, and the
 * bit-packed morphology used inside the pipeline with the u8 one (binary masks: != 0 -> 255). */
int va_gaussian_u8_generic(const uint8_t *src_dev, uint8_t *dst_dev, int n, int h, int w, int c,
                           double sigma, void *stream);
/* the LDS/VALU (dot4/dot2) single-launch kernel that va_gaussian_u8 falls back to when the tap
 * set does not fit the matrix-core kernel (taps > 127); c must be 1 */
int va_gaussian_u8_valu(const uint8_t *src_dev, uint8_t *dst_dev, int n, int h, int w, int c,
                        double sigma, void *stream);
int va_morph_bits_u8(const uint8_t *src_dev, uint8_t *dst_dev, int n, int h, int w, int op,
                     int shape, int ksize, void *stream);
/* pins the labelling code path of every later va_label_i32 / va_largest_contour / pipeline call
 * of this process: path 0 = library's choice (per-frame LDS kernel when its cost model beats the
 * chip-wide passes: frames up to 1080p in batches of about 16 frames or more, 4K frames from
 * about 64, small frames in any batch; chip-wide passes otherwise), 1 = chip-wide passes, 2 = per-frame kernel,
 * 3 = the library's choice, but the per-frame kernel hands its labels to the paint pass as sparse words in the
 * label image (round 1's convention) instead of compact run tables; 4 = the per-frame kernel (as 2),
 * staging the mask rows in LDS even where it could read its spans straight from global memory;
 * 5 = the per-frame kernel (as 2), linking rows with the dense sweep over every span even where it would
 * walk its list of non-empty spans (16-byte aligned rows; frames up to 2048 pixels wide, wider ones up to 685 rows);
 * lds_runs > 0 caps the per-frame kernel's run table (frames above it take its large-frame mode) */
int va_test_hook_labelling(int path, int lds_runs);
/* force_valu != 0: pipelines created from now on run their 8-bit Gaussian in the LDS/VALU (dot4/dot2)
 * kernel instead of the matrix-core one (same bits; bench.py times the chain both ways) */
int va_test_hook_gaussian_u8(int force_valu);
/* bit 0: every later float32 Gaussian of this process runs its column pass in the runtime-radius
 * kernel, also for the radii (r = 4, 8, ... 36) that have an unrolled one; bit 1: the same for the
 * row pass (compile-time-radius kernels exist for the same radii) */
int va_test_hook_gaussian_f32(int generic);
/* byte = 0..255: from now on every block of library scratch (fresh or cached) is filled with that byte on the
 * call's stream before the call uses it, and every plane a pipeline allocates (va_pipeline_create,
 * va_pipeline_overlap) is filled before its own clears run: undefined memory that is not the zeros of a fresh
 * page.  -1 = off (the default; the initial value is $VA_TEST_FILL, decimal 0..255).  Off costs one branch per
 * scratch lease and per pipeline creation and nothing in va_pipeline_run. */
int va_test_hook_fill(int byte);

/* ------------------------------------------------------------------ multi-GPU (RCCL)
 * Frames shard across ranks with no data-path collective; the only exchange is the final
 * gather of per-frame object counts.  librccl is resolved lazily (dlopen) on first use.
 * id_out/id: 128-byte ncclUniqueId produced on rank 0 and distributed by the host. */
int va_comm_unique_id(uint8_t id_out[128]);
int va_comm_init(void **comm_out, int world_size, int rank, const uint8_t id[128]);
int va_gather_counts(void *comm, const int32_t *send_dev, int32_t *recv_dev,
                     int count_per_rank, void *stream);
int va_comm_destroy(void *comm);

#ifdef __cplusplus
}
#endif
#endif /* VIDEOANALYSIS_HIP_H */
