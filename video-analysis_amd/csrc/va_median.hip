// va_median.hip -- rank planes of a uint8 frame stack over time ("Temporal median"):
// out[j, p] = sort(frames[:, p])[ranks[j]] for t <= 255 planes of px bytes and up to eight ranks, exact.  This is what
// np.median / np.percentile(axis=0) do on a downloaded stack; the reference has no counterpart (its only static
// background is the mean of video/analysis/video.py:26-35).  The arithmetic is va_median_math.h, the same text the
// host test compiles.
//
// One lane per dword column (four adjacent pixels), 256 lanes a workgroup, so a wave reads 256 consecutive bytes of
// each plane.  Two paths, chosen by t alone, with no gap between them:
//   t <= 64   ranks_sort_kernel<N>, N = 8, 16, 32, 64: the column's dwords in N registers; their even bytes, then their
//             odd bytes, as N packed pairs of 16-bit halves through Batcher's odd-even merge sort with v_pk_min_u16 /
//             v_pk_max_u16, then a pick per rank.  The stack is read once, however many ranks are asked for.
//   t >= 65   ranks_count_kernel<K>, K = 2 or 8 ranks a pass: the value of each rank is built bit by bit; every bit
//             is a pass over the column that counts the planes at or above the trial value.  Eight reads of the stack,
//             whatever K.
// Each has an aligned variant (frames, frame_stride, px and out all multiples of four: one dword load a plane, one
// dword store a rank) and a safe variant (byte loads and stores, each checked against px).  Every lane writes its own
// bytes of every rank plane and nothing else, from values that depend on the stack alone: two calls write the same
// bytes.
#include "va_common.h"
#include "va_median_math.h"

namespace va {

namespace {

constexpr int kMedianBlock = 256;
constexpr size_t kMedianMaxPixels = (size_t)1 << 40;     // columns of a plane go into gridDim.x (below 2^31)

// waves per SIMD the sorting kernels are compiled for: the dwords of a column and one of its two sorted arrays are
// live together, and the compiler's schedule of the network takes about 3 N registers in all; a tighter bound spills
template <int kN> constexpr int kSortWaves = kN == 64 ? 2 : kN == 32 ? 4 : 8;

struct RankArgs {
    const uint8_t *frames;
    uint8_t *out;
    size_t px, stride;
    uint64_t ranks;         // va_median::pack_ranks
    int t, k;
};

template <int kN, bool kAligned>
__global__ void __launch_bounds__(kMedianBlock, kSortWaves<kN>)
ranks_sort_kernel(RankArgs a)
{
    const size_t p = ((size_t)blockIdx.x * kMedianBlock + threadIdx.x) * 4;
    if (p < a.px)
        va_median::ranks_sorted<kN, kAligned>(a.frames, a.t, a.px, a.stride, a.ranks, a.k, a.out, p);
}

template <int kK, bool kAligned>
__global__ void __launch_bounds__(kMedianBlock)
ranks_count_kernel(RankArgs a)
{
    const size_t p = ((size_t)blockIdx.x * kMedianBlock + threadIdx.x) * 4;
    if (p < a.px)
        va_median::ranks_counted<kK, kAligned>(a.frames, a.t, a.px, a.stride, a.ranks, a.k, a.out, p);
}

template <bool kAligned>
void launch_ranks(const RankArgs &a, hipStream_t st)
{
    const dim3 grid((unsigned)((a.px + 4 * kMedianBlock - 1) / (4 * kMedianBlock))), block(kMedianBlock);
    if (a.t > va_median::kSortMaxPlanes) {
        if (a.k <= 2)
            hipLaunchKernelGGL((ranks_count_kernel<2, kAligned>), grid, block, 0, st, a);
        else
            hipLaunchKernelGGL((ranks_count_kernel<8, kAligned>), grid, block, 0, st, a);
        return;
    }
    switch (va_median::sort_class(a.t)) {
    case 8: hipLaunchKernelGGL((ranks_sort_kernel<8, kAligned>), grid, block, 0, st, a); break;
    case 16: hipLaunchKernelGGL((ranks_sort_kernel<16, kAligned>), grid, block, 0, st, a); break;
    case 32: hipLaunchKernelGGL((ranks_sort_kernel<32, kAligned>), grid, block, 0, st, a); break;
    default: hipLaunchKernelGGL((ranks_sort_kernel<64, kAligned>), grid, block, 0, st, a); break;
    }
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

int va_temporal_ranks_u8(const uint8_t *frames, int t, size_t px, size_t frame_stride, const int32_t *ranks, int nranks,
                         uint8_t *out, void *stream)
{
    VA_REQUIRE(frames && ranks && out, "va_temporal_ranks_u8: NULL argument");
    VA_REQUIRE(t >= 1 && t <= va_median::kMaxPlanes, "va_temporal_ranks_u8: 1 .. %d planes a call, got %d",
               va_median::kMaxPlanes, t);
    VA_REQUIRE(px >= 1 && px <= kMedianMaxPixels, "va_temporal_ranks_u8: planes of 1 .. 2^40 bytes, got %zu", px);
    VA_REQUIRE(frame_stride >= px, "va_temporal_ranks_u8: frame stride %zu below the plane size %zu", frame_stride, px);
    VA_REQUIRE(nranks >= 1 && nranks <= va_median::kMaxRanks, "va_temporal_ranks_u8: 1 .. %d ranks a call, got %d",
               va_median::kMaxRanks, nranks);
    for (int j = 0; j < nranks; j++)
        VA_REQUIRE(ranks[j] >= 0 && ranks[j] < t, "va_temporal_ranks_u8: rank %d of %d planes (ranks[%d])", ranks[j], t, j);
    VA_ENTER();
    const RankArgs a = {frames, out, px, frame_stride, va_median::pack_ranks(ranks, nranks), t, nranks};
    const bool dwords = aligned(frames, 4) && aligned(out, 4) && frame_stride % 4 == 0 && px % 4 == 0;
    if (dwords)
        launch_ranks<true>(a, as_stream(stream));
    else
        launch_ranks<false>(a, as_stream(stream));
    VA_LAUNCH_CHECK("ranks_sort_kernel / ranks_count_kernel");
    return VA_OK;
}

}  // extern "C"
