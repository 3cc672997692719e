// va_sliding_median.hip -- the exact median of the `window` frames before each frame of a uint8 stream (DESIGN.md §9,
// "Sliding median"): lower[k], upper[k] = the sorted window max(0, k - W) .. k - 1 of every pixel at ranks
// (cnt - 1) / 2 and cnt / 2, diff[k] = min(255, |2 frame[k] - lower[k] - upper[k]| >> 1).  This is what one
// va_temporal_ranks_u8 call per emitted frame gives on the W-plane window (np.median over a sliding_window_view on a
// downloaded stack); the reference has no counterpart.  The state layout and the per-pixel step are
// va_sliding_median_math.h, the same text the host test compiles.
//
// One launch a call.  A workgroup of two waves owns a tile of 128 pixels, one lane a pixel: it copies the tile's
// bin-major histogram (32 KiB of uint8 counters, 64 KiB of uint16 counters: one contiguous block) from the state into
// LDS with 16-byte loads, walks the n frames of the call with the histogram resident, and writes it back once.  Each
// counter belongs to one lane and is touched with an access of its own size (ds_read_u8 / ds_write_b8 for the byte
// counters: four lanes share a dword), so there are no atomics; the column of a pixel (va_slide::column) gives the 32
// lanes the LDS serves together 32 different banks whatever bins they touch.
// Frames go four at a time: a wave's 64 pixels of four planes are 64 dwords, one a lane, and four ds_bpermute turn
// them into each lane's own four bytes (and back for the ring and the outputs); the loads of the next four frames are
// issued before these four are walked.  The dword form is used for the caller's planes where frames, frame_stride, px
// and the outputs are all multiples of four, byte accesses otherwise; the ring always takes dwords (its planes are
// padded to whole tiles, the state is 16-byte aligned).  The leaving value of frame j of the call comes from the
// call's own frame j - W where there is one, and from the ring -- slots that an earlier call wrote -- otherwise; only
// the last W frames of a call are stored into the ring.  Every read of a ring slot comes before the one write to it
// in the program order of the wave that owns the pixels.
#include "va_common.h"
#include "va_sliding_median_math.h"

namespace va {

namespace {

using va_slide::kTilePixels;
constexpr size_t kSlideMaxPixels = (size_t)1 << 36;      // tiles of a plane go into gridDim.x (below 2^31)

struct SlideArgs {
    const uint8_t *frames;
    uint8_t *state, *ring;
    uint8_t *lower, *upper, *diff;
    size_t px, stride, ring_stride, tile_bytes;
    int n, window;
    uint32_t seen0;         // min(n_seen, window): the values in the window before the call's first frame
    uint32_t slot0;         // n_seen % window: the ring slot of the call's first frame
};

__device__ __forceinline__ uint32_t lane_shuffle(uint32_t v, int src)
{
    return (uint32_t)__builtin_amdgcn_ds_bpermute(src << 2, (int)v);
}

template <class P>
__device__ __forceinline__ P *pick_plane(P *const (&planes)[4], int f)
{
    return f == 0 ? planes[0] : f == 1 ? planes[1] : f == 2 ? planes[2] : planes[3];
}

// The wave's 64 bytes at `base` of up to four planes (a missing plane is nullptr and reads as 0, as does a byte at or
// beyond `limit`), in two steps so that the loads of the next four frames are in flight while these four are walked.
// fetch: what this lane loads -- kWide (every plane starts on a dword, limit is a multiple of four; base is one of
// 64): the dword (lane & 15) of plane lane >> 4; otherwise this lane's byte of each plane, byte f from plane f.
// spread: byte f of the result is this lane's byte of plane f (kWide: four ds_bpermute; otherwise it is that already).
template <bool kWide>
__device__ __forceinline__ uint32_t fetch(const uint8_t *const (&planes)[4], size_t base, size_t limit, int lane)
{
    uint32_t d = 0;
    if (kWide) {
        const uint8_t *plane = pick_plane(planes, lane >> 4);
        const size_t at = base + 4 * (size_t)(lane & 15);
        if (plane && at < limit)
            d = *reinterpret_cast<const uint32_t *>(plane + at);
    } else {
#pragma unroll
        for (int f = 0; f < 4; f++)
            if (planes[f] && base + lane < limit)
                d |= (uint32_t)planes[f][base + lane] << (8 * f);
    }
    return d;
}
template <bool kWide>
__device__ __forceinline__ uint32_t spread(uint32_t d, int lane)
{
    if (!kWide)
        return d;
    uint32_t packed = 0;
#pragma unroll
    for (int f = 0; f < 4; f++)
        packed |= ((lane_shuffle(d, f * 16 + (lane >> 2)) >> (8 * (lane & 3))) & 0xffu) << (8 * f);
    return packed;
}

// the reverse: byte f of `packed` goes to this lane's byte of plane f (no store for a missing plane or beyond limit)
template <bool kWide>
__device__ __forceinline__ void stage_out(uint8_t *const (&planes)[4], size_t base, size_t limit, int lane,
                                          uint32_t packed)
{
    if (kWide) {
        const int f = lane >> 4;
        uint32_t d = 0;
#pragma unroll
        for (int c = 0; c < 4; c++)
            d |= ((lane_shuffle(packed, 4 * (lane & 15) + c) >> (8 * f)) & 0xffu) << (8 * c);
        uint8_t *plane = pick_plane(planes, f);
        const size_t at = base + 4 * (size_t)(lane & 15);
        if (plane && at < limit)
            *reinterpret_cast<uint32_t *>(plane + at) = d;
    } else {
#pragma unroll
        for (int f = 0; f < 4; f++)
            if (planes[f] && base + lane < limit)
                planes[f][base + lane] = (uint8_t)(packed >> (8 * f));
    }
}

template <class T, bool kWide>
__global__ void __launch_bounds__(kTilePixels)
sliding_median_kernel(SlideArgs a)
{
    __shared__ __attribute__((aligned(16))) T hist[va_slide::kBins * kTilePixels];
    constexpr int kHistVectors = va_slide::kBins * kTilePixels * (int)sizeof(T) / 16;
    const int q = threadIdx.x, lane = q & (kWave - 1);
    uint8_t *tile = a.state + (size_t)blockIdx.x * a.tile_bytes;
    uint8_t *track = tile + sizeof(hist);
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(tile);
        uint4 *dst = reinterpret_cast<uint4 *>(hist);
        for (int i = q; i < kHistVectors; i += kTilePixels)
            dst[i] = src[i];
    }
    uint32_t lower = track[q], upper = track[kTilePixels + q];
    uint32_t below = reinterpret_cast<const uint16_t *>(track + 2 * kTilePixels)[q];
    __syncthreads();

    T *h = hist + va_slide::column((uint32_t)q, sizeof(T));
    const size_t base = (size_t)blockIdx.x * kTilePixels + (size_t)(q - lane);      // the wave's first pixel
    const uint32_t window = (uint32_t)a.window;
    // what the four frames from j0 on read: the entering planes, and the leaving ones from the call or from the ring
    struct Reads {
        uint32_t entering, leave_call, leave_ring;
    };
    auto fetch_group = [&](int64_t j0) {
        const uint8_t *in[4], *leave_in[4], *leave_ring[4];
#pragma unroll
        for (int f = 0; f < 4; f++) {
            const int64_t j = j0 + f;
            const bool leaves = j < a.n && a.seen0 + (uint32_t)j >= window;
            const size_t slot = (a.slot0 + (uint32_t)j) % window;
            in[f] = j < a.n ? a.frames + (size_t)j * a.stride : nullptr;
            leave_in[f] = leaves && j >= a.window ? a.frames + (size_t)(j - a.window) * a.stride : nullptr;
            leave_ring[f] = leaves && j < a.window ? a.ring + slot * a.ring_stride : nullptr;
        }
        Reads r;
        r.entering = fetch<kWide>(in, base, a.px, lane);
        r.leave_call = fetch<kWide>(leave_in, base, a.px, lane);
        r.leave_ring = fetch<true>(leave_ring, base, a.ring_stride, lane);
        return r;
    };
    // A ring slot that group j0 + 4 reads is not one that group j0 writes: a read is of a frame j < window, the
    // write to the same slot of a frame j - m window.
    Reads now = fetch_group(0);
    for (int64_t j0 = 0; j0 < a.n; j0 += 4) {      // (64 bits: n may be close to 2^31)
        Reads next = {0, 0, 0};
        if (j0 + 4 < a.n)
            next = fetch_group(j0 + 4);
        uint8_t *keep[4], *out_lower[4], *out_upper[4], *out_diff[4];
        bool leaves[4], any_keep = false;
#pragma unroll
        for (int f = 0; f < 4; f++) {
            const int64_t j = j0 + f;
            const bool valid = j < a.n;
            const size_t slot = (a.slot0 + (uint32_t)j) % window;
            leaves[f] = valid && a.seen0 + (uint32_t)j >= window;
            const bool kept = valid && j + a.window >= a.n;
            keep[f] = kept ? a.ring + slot * a.ring_stride : nullptr;
            out_lower[f] = valid && a.lower ? a.lower + (size_t)j * a.px : nullptr;
            out_upper[f] = valid && a.upper ? a.upper + (size_t)j * a.px : nullptr;
            out_diff[f] = valid && a.diff ? a.diff + (size_t)j * a.px : nullptr;
            any_keep |= kept;
        }
        const uint32_t entering = spread<kWide>(now.entering, lane);
        const uint32_t leaving = spread<kWide>(now.leave_call, lane) | spread<true>(now.leave_ring, lane);
        uint32_t lowers = 0, uppers = 0, diffs = 0;
#pragma unroll
        for (int f = 0; f < 4; f++) {
            if (j0 + f < a.n) {
                const uint32_t seen = a.seen0 + (uint32_t)(j0 + f);
                uint32_t lo, up, df;
                va_slide::step<T>(h, lower, upper, below, seen < window ? seen : window, (entering >> (8 * f)) & 0xffu,
                                  leaves[f], (leaving >> (8 * f)) & 0xffu, lo, up, df);
                lowers |= lo << (8 * f);
                uppers |= up << (8 * f);
                diffs |= df << (8 * f);
            }
        }
        if (a.lower)
            stage_out<kWide>(out_lower, base, a.px, lane, lowers);
        if (a.upper)
            stage_out<kWide>(out_upper, base, a.px, lane, uppers);
        if (a.diff)
            stage_out<kWide>(out_diff, base, a.px, lane, diffs);
        if (any_keep)
            stage_out<true>(keep, base, a.ring_stride, lane, entering);
        now = next;
    }

    __syncthreads();
    {
        const uint4 *src = reinterpret_cast<const uint4 *>(hist);
        uint4 *dst = reinterpret_cast<uint4 *>(tile);
        for (int i = q; i < kHistVectors; i += kTilePixels)
            dst[i] = src[i];
    }
    track[q] = (uint8_t)lower;
    track[kTilePixels + q] = (uint8_t)upper;
    reinterpret_cast<uint16_t *>(track + 2 * kTilePixels)[q] = (uint16_t)below;
}

// the tracker planes of the state, pixel by pixel
__global__ void __launch_bounds__(256)
sliding_median_current_kernel(const uint8_t *state, size_t px, size_t tile_bytes, size_t lower_at, uint8_t *lower,
                              uint8_t *upper)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= px)
        return;
    const uint8_t *track = state + (p / kTilePixels) * tile_bytes + lower_at + p % kTilePixels;
    if (lower)
        lower[p] = track[0];
    if (upper)
        upper[p] = track[kTilePixels];
}

template <class T>
void launch_slide(const SlideArgs &a, bool wide, hipStream_t st)
{
    const dim3 grid((unsigned)va_slide::tiles(a.px)), block(kTilePixels);
    if (wide)
        hipLaunchKernelGGL((sliding_median_kernel<T, true>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((sliding_median_kernel<T, false>), grid, block, 0, st, a);
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

size_t va_sliding_median_state_bytes(size_t px, int window)
{
    if (px < 1 || px > kSlideMaxPixels || window < 1 || window > va_slide::kMaxWindow)
        return 0;
    return va_slide::state_bytes(px, window);
}

int va_sliding_median_u8(const uint8_t *frames, int n, size_t px, size_t frame_stride, int window, int64_t n_seen,
                         void *state, uint8_t *lower_out, uint8_t *upper_out, uint8_t *diff_out, void *stream)
{
    VA_REQUIRE(state && (frames || n == 0), "va_sliding_median_u8: NULL argument");
    VA_REQUIRE(aligned(state, 16), "va_sliding_median_u8: the state starts on a 16-byte boundary");
    VA_REQUIRE(window >= 1 && window <= va_slide::kMaxWindow, "va_sliding_median_u8: a window of 1 .. %d frames, got %d",
               va_slide::kMaxWindow, window);
    VA_REQUIRE(px >= 1 && px <= kSlideMaxPixels, "va_sliding_median_u8: planes of 1 .. 2^36 bytes, got %zu", px);
    VA_REQUIRE(n >= 0, "va_sliding_median_u8: a negative number of frames (%d)", n);
    VA_REQUIRE(frame_stride >= px, "va_sliding_median_u8: frame stride %zu below the plane size %zu", frame_stride, px);
    VA_REQUIRE(n_seen >= 0, "va_sliding_median_u8: a negative n_seen (%lld)", (long long)n_seen);
    if (n == 0)
        return VA_OK;
    VA_ENTER();
    uint8_t *bytes = static_cast<uint8_t *>(state);
    const SlideArgs a = {frames, bytes, bytes + va_slide::ring_offset(px, window), lower_out, upper_out, diff_out,
                         px, frame_stride, va_slide::ring_stride(px), va_slide::tile_bytes(window), n, window,
                         (uint32_t)(n_seen < window ? n_seen : window), (uint32_t)(n_seen % window)};
    const bool wide = aligned(frames, 4) && frame_stride % 4 == 0 && px % 4 == 0 && aligned(lower_out, 4) &&
                      aligned(upper_out, 4) && aligned(diff_out, 4);
    if (va_slide::counter_bytes(window) == 1)
        launch_slide<uint8_t>(a, wide, as_stream(stream));
    else
        launch_slide<uint16_t>(a, wide, as_stream(stream));
    VA_LAUNCH_CHECK("sliding_median_kernel");
    return VA_OK;
}

int va_sliding_median_current(const void *state, size_t px, int window, int64_t n_seen, uint8_t *lower_out,
                              uint8_t *upper_out, void *stream)
{
    VA_REQUIRE(state, "va_sliding_median_current: NULL argument");
    VA_REQUIRE(window >= 1 && window <= va_slide::kMaxWindow,
               "va_sliding_median_current: a window of 1 .. %d frames, got %d", va_slide::kMaxWindow, window);
    VA_REQUIRE(px >= 1 && px <= kSlideMaxPixels, "va_sliding_median_current: planes of 1 .. 2^36 bytes, got %zu", px);
    VA_REQUIRE(n_seen >= 0, "va_sliding_median_current: a negative n_seen (%lld)", (long long)n_seen);
    if (!lower_out && !upper_out)
        return VA_OK;
    VA_ENTER();
    hipLaunchKernelGGL(sliding_median_current_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0,
                       as_stream(stream), static_cast<const uint8_t *>(state), px, va_slide::tile_bytes(window),
                       va_slide::lower_offset(window), lower_out, upper_out);
    VA_LAUNCH_CHECK("sliding_median_current_kernel");
    return VA_OK;
}

}  // extern "C"
