// va_thinning.hip -- Guo-Hall thinning (the `guo-hall` method of mask_thinning, video/analysis/image.py:236-241,
// which calls guo_hall_thinning of the external `thinning` module); the definition is pinned in DESIGN.md §9,
// "Guo-Hall thinning".
//
// Both paths keep a mask as one bit per pixel, bit i of word k of a row = pixel x = 32 k + i, and evaluate a
// sub-iteration's deletion predicate on whole words: the eight neighbour planes p2 .. p9 are the words of the rows
// above, at and below, shifted by one bit with the carry of the adjacent word, and
//   C == 1              exactly one of the four terms  !p2 & (p3|p4), !p4 & (p5|p6), !p6 & (p7|p8), !p8 & (p9|p2)
//   2 <= min(N1, N2) <= 3   (N1 >= 2) & (N2 >= 2) & !((N1 == 4) & (N2 == 4)), each a sum of four one-bit terms
//   m == 0              (p6 | p7 | !p9) & p8 in sub-iteration 0, (p2 | p3 | !p5) & p4 in sub-iteration 1
// are boolean expressions of them.  Pixels of the first and last row and column are never tested (an eligibility
// mask per word), so no carry from outside a row is ever needed.
//
// resident : one workgroup per mask of a ragged packed buffer.  The mask is packed into LDS (one wave ballot per
//            64 pixels), iterated there until one whole iteration deletes nothing (flags of all words into
//            registers, barrier, store: a single plane), and the survivors are written out with the input's own
//            values.  No host round trip; the iteration count goes to a per-item int32.
// tiled    : an (n, h, w) stack.  Bit planes ping-pong in HBM; one launch advances every 32 x 448-pixel tile
//            (at the default K = 16) by K sub-iterations in LDS on a 64 x 512-pixel window: a sub-iteration depends on the 3x3
//            of the state before it, so after K of them the window is still exact K pixels inside its edge.
//            Every iteration ORs one flag per frame (set iff it deleted a pixel of some tile's own region); the host
//            reads the flags of `poll` launches at a time and stops after an iteration that is clear for every frame.
#include <vector>

#include "va_common.h"

namespace va {

namespace {

constexpr int kThinResidentMaxWords = VA_THIN_RESIDENT_MAX_WORDS;
constexpr int kThinMaxK = VA_THIN_MAX_SUB_ITERATIONS;
constexpr int kThinMaxPoll = VA_THIN_MAX_POLL;
constexpr int kThinBlock = 256;
constexpr int kThinWaves = kThinBlock / kWave;
constexpr int kTileRows = 64, kTileWordsX = 16;                 // the LDS window of the tiled path
constexpr int kTileWords = kTileRows * kTileWordsX;
constexpr int kTilePer = kTileWords / kThinBlock;
constexpr int kTileOwnX = kTileWordsX - 2;                      // one halo word (32 px >= K) on either side

// deletion flags of the 32 pixels of word c; l / r are the words left / right of it, u / d the rows above / below
__device__ __forceinline__ uint32_t gh_flags(uint32_t ul, uint32_t u, uint32_t ur, uint32_t cl, uint32_t c,
                                             uint32_t cr, uint32_t dl, uint32_t d, uint32_t dr, int sub)
{
    const uint32_t p2 = u, p6 = d;
    const uint32_t p9 = (u << 1) | (ul >> 31), p3 = (u >> 1) | (ur << 31);
    const uint32_t p8 = (c << 1) | (cl >> 31), p4 = (c >> 1) | (cr << 31);
    const uint32_t p7 = (d << 1) | (dl >> 31), p5 = (d >> 1) | (dr << 31);
    const uint32_t a1 = p9 | p2, a2 = p3 | p4, a3 = p5 | p6, a4 = p7 | p8;      // the terms of N1
    const uint32_t b1 = p2 | p3, b2 = p4 | p5, b3 = p6 | p7, b4 = p8 | p9;      // the terms of N2
    const uint32_t t1 = ~p2 & a2, t2 = ~p4 & a3, t3 = ~p6 & a4, t4 = ~p8 & a1;  // the terms of C
    const uint32_t c_is_1 = ((t1 ^ t2) ^ (t3 ^ t4)) & ~((t1 & t2) | (t3 & t4));
    const uint32_t n1_ge2 = (a1 & a2) | (a3 & a4) | ((a1 ^ a2) & (a3 ^ a4));
    const uint32_t n2_ge2 = (b1 & b2) | (b3 & b4) | ((b1 ^ b2) & (b3 ^ b4));
    const uint32_t both4 = (a1 & a2 & a3 & a4) & (b1 & b2 & b3 & b4);
    const uint32_t m = sub ? (p2 | p3 | ~p5) & p4 : (p6 | p7 | ~p9) & p8;
    return c & c_is_1 & n1_ge2 & n2_ge2 & ~both4 & ~m;
}

// the pixels of word k of a row of width w that may be tested: 1 <= x <= w - 2
__device__ __forceinline__ uint32_t gh_eligible(int k, int w)
{
    const int hi = w - 2 - 32 * k;                   // the last eligible bit of this word
    uint32_t m = hi < 0 ? 0u : hi >= 31 ? 0xffffffffu : (2u << hi) - 1u;
    return k == 0 ? m & ~1u : m;
}

// one sub-iteration over the words a thread owns (word j at s[idx[j]], row stride `stride`); em[j] == 0 marks a word
// that is not the thread's, lies in the first or last row, or has no eligible pixel.  Returns the OR of the flags
// selected by `count[j]`.
template <int PER>
__device__ __forceinline__ uint32_t gh_sub_iteration(uint32_t *s, const int (&idx)[PER], const uint32_t (&em)[PER],
                                                     const uint32_t (&count)[PER], int stride, int sub)
{
    uint32_t del[PER];
#pragma unroll
    for (int j = 0; j < PER; j++) {
        del[j] = 0;
        if (em[j]) {
            const uint32_t *q = s + idx[j];
            del[j] = em[j] & gh_flags(q[-stride - 1], q[-stride], q[-stride + 1], q[-1], q[0], q[1], q[stride - 1],
                                      q[stride], q[stride + 1], sub);
        }
    }
    __syncthreads();                                 // every flag is computed before any word is rewritten
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < PER; j++)
        if (del[j]) {
            s[idx[j]] &= ~del[j];
            any |= del[j] & count[j];
        }
    return any;
}

template <int PER>
__global__ void __launch_bounds__(kThinBlock)
gh_resident_kernel(const uint8_t *__restrict__ src, const int32_t *__restrict__ shapes,
                   const int64_t *__restrict__ offsets, int64_t total, int max_words, uint8_t *__restrict__ dst,
                   int32_t *__restrict__ iterations, int32_t *__restrict__ status)
{
    extern __shared__ uint32_t s_dyn[];              // max_words + 2: one pad word before and after the plane
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int h = shapes[2 * p], w = shapes[2 * p + 1];
    const int64_t o = offsets[p];
    const int wpr = h >= 0 && w >= 0 ? (int)(((int64_t)w + 31) >> 5) : 0;
    const int64_t words = (int64_t)h * wpr;
    if (!(h >= 0 && w >= 0 && words <= max_words && words <= (int64_t)PER * kThinBlock && o >= 0 &&
          o + (int64_t)h * w <= total)) {            // workgroup-uniform: nothing of the item is read or written
        if (tid == 0)
            status[p] = VA_ERR_RANGE;
        return;
    }
    uint32_t *s = s_dyn + 1;
    const uint8_t *in = src + o;
    uint8_t *out = dst + o;
    if (tid == 0)
        s[-1] = 0, s[words] = 0;
    for (int r = wave; r < h; r += kThinWaves)
        for (int x0 = 0; x0 < w; x0 += kWave) {
            const int x = x0 + lane;
            const unsigned long long b = __ballot(x < w && in[(int64_t)r * w + x] != 0);
            const int k = (x0 >> 5) + lane;
            if (lane < 2 && k < wpr)
                s[r * wpr + k] = lane ? (uint32_t)(b >> 32) : (uint32_t)b;
        }
    // the words of rows 1 .. h - 2, PER per thread
    int idx[PER];
    uint32_t em[PER], count[PER];
    const int first = wpr, last = (h - 1) * wpr;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        idx[j] = first + tid + j * kThinBlock;
        em[j] = idx[j] < last ? gh_eligible(idx[j] % wpr, w) : 0u;
        count[j] = 0xffffffffu;
    }
    __syncthreads();
    int it = 0;
    for (;;) {
        it++;
        uint32_t any = gh_sub_iteration<PER>(s, idx, em, count, wpr, 0);
        __syncthreads();
        any |= gh_sub_iteration<PER>(s, idx, em, count, wpr, 1);
        if (!__syncthreads_or(any != 0))             // also the barrier before the next iteration's reads
            break;
    }
    for (int r = wave; r < h; r += kThinWaves)
        for (int x = lane; x < w; x += kWave) {
            const int64_t i = (int64_t)r * w + x;
            out[i] = (s[r * wpr + (x >> 5)] >> (x & 31)) & 1u ? in[i] : (uint8_t)0;
        }
    if (tid == 0) {
        iterations[p] = it;
        status[p] = VA_OK;
    }
}

// ------------------------------------------------------------------------------------------ tiled
// one thread per word: 32 pixels of a row -> their bits (FAST: w % 4 == 0 and aligned buffers, dword loads)
template <bool FAST>
__global__ void __launch_bounds__(kThinBlock)
gh_pack_kernel(const uint8_t *__restrict__ src, uint32_t *__restrict__ plane, int64_t rows, int w, int wpr)
{
    const int64_t i = (int64_t)blockIdx.x * kThinBlock + threadIdx.x;
    if (i >= rows * wpr)
        return;
    const int64_t r = i / wpr;
    const int k = (int)(i - r * wpr), x0 = 32 * k;
    const uint8_t *q = src + r * w + x0;
    uint32_t bits = 0;
    if (FAST && x0 + 32 <= w) {
        const uint32_t *q4 = reinterpret_cast<const uint32_t *>(q);
#pragma unroll
        for (int g = 0; g < 8; g++) {
            const uint32_t v = q4[g];
            bits |= ((v & 0xffu) ? 1u : 0u) << (4 * g) | ((v & 0xff00u) ? 2u : 0u) << (4 * g) |
                    ((v & 0xff0000u) ? 4u : 0u) << (4 * g) | ((v & 0xff000000u) ? 8u : 0u) << (4 * g);
        }
    } else {
        const int cnt = w - x0 < 32 ? w - x0 : 32;
        for (int b = 0; b < cnt; b++)
            bits |= (q[b] ? 1u : 0u) << b;
    }
    plane[i] = bits;
}

// dst = src where the pixel's bit is set, else 0
template <bool FAST>
__global__ void __launch_bounds__(kThinBlock)
gh_unpack_kernel(const uint32_t *__restrict__ plane, const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                 int64_t rows, int w, int wpr)
{
    const int64_t i = (int64_t)blockIdx.x * kThinBlock + threadIdx.x;
    if (i >= rows * wpr)
        return;
    const int64_t r = i / wpr;
    const int k = (int)(i - r * wpr), x0 = 32 * k;
    const uint32_t bits = plane[i];
    const int64_t base = r * w + x0;
    if (FAST && x0 + 32 <= w) {
        const uint32_t *q4 = reinterpret_cast<const uint32_t *>(src + base);
        uint32_t *d4 = reinterpret_cast<uint32_t *>(dst + base);
#pragma unroll
        for (int g = 0; g < 8; g++) {
            const uint32_t nib = bits >> (4 * g);
            const uint32_t keep = ((nib & 1u) ? 0xffu : 0u) | ((nib & 2u) ? 0xff00u : 0u) |
                                  ((nib & 4u) ? 0xff0000u : 0u) | ((nib & 8u) ? 0xff000000u : 0u);
            d4[g] = q4[g] & keep;
        }
    } else {
        const int cnt = w - x0 < 32 ? w - x0 : 32;
        for (int b = 0; b < cnt; b++)
            dst[base + b] = (bits >> b) & 1u ? src[base + b] : (uint8_t)0;
    }
}

// K sub-iterations of one tile.  LDS word (lr, lk) is row ty*TH - K + lr, word tx*kTileOwnX - 1 + lk of the frame
// (0 outside it); the tile's own region is lr in [K, K + TH), lk in [1, kTileOwnX], TH = kTileRows - 2 K.  What the
// window lacks beyond its edge reaches one pixel further in per sub-iteration: after K of them rows K .. and the
// own words (32 >= K bits from the halo words' outer ends) are exact.
__global__ void __launch_bounds__(kThinBlock)
gh_tiled_kernel(const uint32_t *__restrict__ in, uint32_t *__restrict__ out, int n, int h, int w, int wpr, int K,
                uint32_t *__restrict__ flags)
{
    __shared__ uint32_t s_raw[kTileWords + 2];
    __shared__ uint32_t s_changed;
    uint32_t *s = s_raw + 1;
    const int tid = threadIdx.x, f = blockIdx.z;
    const int TH = kTileRows - 2 * K;
    const int row0 = (int)blockIdx.y * TH - K, word0 = (int)blockIdx.x * kTileOwnX - 1;
    const size_t frame = (size_t)f * h * wpr;
    int idx[kTilePer];
    uint32_t em[kTilePer], own[kTilePer];
    int64_t where[kTilePer];
#pragma unroll
    for (int j = 0; j < kTilePer; j++) {
        const int i = tid + j * kThinBlock, lr = i / kTileWordsX, lk = i % kTileWordsX;
        const int gy = row0 + lr, gk = word0 + lk;
        const bool inside = gy >= 0 && gy < h && gk >= 0 && gk < wpr;
        idx[j] = i;
        where[j] = inside ? (int64_t)gy * wpr + gk : -1;
        s[i] = inside ? in[frame + where[j]] : 0u;
        em[j] = inside && gy >= 1 && gy <= h - 2 && lr >= 1 && lr <= kTileRows - 2 ? gh_eligible(gk, w) : 0u;
        own[j] = lr >= K && lr < K + TH && lk >= 1 && lk <= kTileOwnX ? 0xffffffffu : 0u;
    }
    if (tid == 0)
        s[-1] = 0, s[kTileWords] = 0, s_changed = 0;
    __syncthreads();
    uint32_t changed = 0;                            // bit q: iteration q of this launch deleted an own pixel
    for (int k = 0; k < K; k++) {
        if (gh_sub_iteration<kTilePer>(s, idx, em, own, kTileWordsX, k & 1))
            changed |= 1u << (k >> 1);
        __syncthreads();
    }
    if (changed)
        atomicOr(&s_changed, changed);
    __syncthreads();
    if (tid < K / 2 && ((s_changed >> tid) & 1u))
        atomicOr(&flags[(size_t)tid * n + f], 1u);
#pragma unroll
    for (int j = 0; j < kTilePer; j++)
        if (own[j] && where[j] >= 0)
            out[frame + where[j]] = s[idx[j]];
}

// scratch of the tiled path: two stacks of bit planes and a flag per pair of sub-iterations, poll and frame
struct TiledLayout { size_t cur, nxt, flags, total; };
TiledLayout tiled_layout(int n, int h, int w)
{
    Carve c;
    const size_t plane_bytes = (size_t)n * h * words_per_row(w) * sizeof(uint32_t);
    return {c.take(plane_bytes), c.take(plane_bytes),
            c.take((size_t)kThinMaxPoll * (kThinMaxK / 2) * n * sizeof(uint32_t)), c.total};
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

int va_guo_hall_thinning_batch(const uint8_t *masks, const int32_t *shapes, const int64_t *offsets, int64_t total,
                               int m, int max_words, uint8_t *out, int32_t *iterations_out, int32_t *status,
                               void *stream)
{
    VA_ENTER();
    VA_REQUIRE(m >= 0 && total >= 0, "va_guo_hall_thinning_batch: negative count (m %d, total %lld)", m,
               (long long)total);
    VA_REQUIRE(max_words >= 0 && max_words <= kThinResidentMaxWords,
               "va_guo_hall_thinning_batch: max_words %d outside 0 .. %d", max_words, kThinResidentMaxWords);
    if (m == 0)
        return VA_OK;
    VA_REQUIRE(masks && shapes && offsets && out && iterations_out && status,
               "va_guo_hall_thinning_batch: NULL argument");
    hipStream_t st = as_stream(stream);
    const size_t lds = ((size_t)max_words + 2) * sizeof(uint32_t);
    const dim3 grid(m), block(kThinBlock);
    if (max_words <= 4 * kThinBlock)
        hipLaunchKernelGGL(gh_resident_kernel<4>, grid, block, lds, st, masks, shapes, offsets, total, max_words, out,
                           iterations_out, status);
    else if (max_words <= 16 * kThinBlock)
        hipLaunchKernelGGL(gh_resident_kernel<16>, grid, block, lds, st, masks, shapes, offsets, total, max_words, out,
                           iterations_out, status);
    else
        hipLaunchKernelGGL(gh_resident_kernel<kThinResidentMaxWords / kThinBlock>, grid, block, lds, st, masks, shapes,
                           offsets, total, max_words, out, iterations_out, status);
    VA_LAUNCH_CHECK("gh_resident_kernel");
    return VA_OK;
}

size_t va_guo_hall_thinning_scratch_bytes(int n, int h, int w)
{
    if (n <= 0 || h <= 0 || w <= 0 || n > 65535 || h > VA_THIN_MAX_ROWS || (size_t)h * (size_t)w >= kMaxFramePixels ||
        (size_t)n * h * words_per_row(w) >= ((size_t)1 << 31))
        return 0;
    return tiled_layout(n, h, w).total;
}

int va_guo_hall_thinning_u8(const uint8_t *src, void *scratch, size_t scratch_bytes, uint8_t *dst, int n, int h,
                            int w, int sub_iterations, int poll_period, int32_t *iterations_out,
                            int32_t *stats_out, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(n >= 0 && h > 0 && w > 0, "va_guo_hall_thinning_u8: bad shape (%d, %d, %d)", n, h, w);
    VA_REQUIRE(n <= kMaxGridYZ, "va_guo_hall_thinning_u8: %d frames, at most 65535 frames in one call are supported",
               n);
    VA_REQUIRE((size_t)h * (size_t)w < kMaxFramePixels,
               "va_guo_hall_thinning_u8: frames above 2^29 pixels are not supported");
    // grid.y = ceil(h / (64 - 2 K)) <= 65535 for every K, and the pack / unpack grids count words in 32 bits
    VA_REQUIRE(h <= VA_THIN_MAX_ROWS, "va_guo_hall_thinning_u8: %d rows, at most %d are supported", h,
               VA_THIN_MAX_ROWS);
    VA_REQUIRE((size_t)n * h * words_per_row(w) < ((size_t)1 << 31),
               "va_guo_hall_thinning_u8: a stack of 2^31 or more packed words is not supported");
    const int K = sub_iterations ? sub_iterations : 16, poll = poll_period ? poll_period : 2;
    VA_REQUIRE(K >= 2 && K <= kThinMaxK && K % 2 == 0,
               "va_guo_hall_thinning_u8: sub_iterations %d is not an even number in 2 .. %d", K, kThinMaxK);
    VA_REQUIRE(poll >= 1 && poll <= kThinMaxPoll, "va_guo_hall_thinning_u8: poll_period %d outside 1 .. %d", poll,
               kThinMaxPoll);
    if (stats_out)
        stats_out[0] = stats_out[1] = 0;
    if (n == 0)
        return VA_OK;
    VA_REQUIRE(src && scratch && dst, "va_guo_hall_thinning_u8: NULL argument");
    const TiledLayout L = tiled_layout(n, h, w);
    VA_REQUIRE(scratch_bytes >= L.total, "va_guo_hall_thinning_u8: scratch of %zu bytes, %zu needed", scratch_bytes,
               L.total);
    hipStream_t st = as_stream(stream);
    const int wpr = words_per_row(w), per_launch = K / 2, per_poll = poll * per_launch;
    const int64_t rows = (int64_t)n * h;
    uint32_t *cur = at<uint32_t>(scratch, L.cur), *nxt = at<uint32_t>(scratch, L.nxt);
    uint32_t *flags = at<uint32_t>(scratch, L.flags);
    const bool fast = (w & 3) == 0 && (((uintptr_t)src | (uintptr_t)dst) & 3) == 0;
    const dim3 words_grid((unsigned)cdiv(rows * wpr, kThinBlock)), block(kThinBlock);
    if (fast)
        hipLaunchKernelGGL(gh_pack_kernel<true>, words_grid, block, 0, st, src, cur, rows, w, wpr);
    else
        hipLaunchKernelGGL(gh_pack_kernel<false>, words_grid, block, 0, st, src, cur, rows, w, wpr);
    VA_LAUNCH_CHECK("gh_pack_kernel");
    const dim3 grid((unsigned)cdiv(wpr, kTileOwnX), (unsigned)cdiv(h, kTileRows - 2 * K), (unsigned)n);
    std::vector<uint32_t> host((size_t)per_poll * n);
    std::vector<int32_t> last(n, 0);                 // the last iteration of each frame that deleted a pixel
    int launches = 0, reads = 0;
    for (int64_t base = 0;; base += per_poll) {
        VA_HIP(hipMemsetAsync(flags, 0, host.size() * sizeof(uint32_t), st));
        for (int l = 0; l < poll; l++) {
            hipLaunchKernelGGL(gh_tiled_kernel, grid, block, 0, st, cur, nxt, n, h, w, wpr, K,
                               flags + (size_t)l * per_launch * n);
            VA_LAUNCH_CHECK("gh_tiled_kernel");
            uint32_t *t = cur;
            cur = nxt;
            nxt = t;
        }
        launches += poll;
        VA_HIP(hipMemcpyAsync(host.data(), flags, host.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        VA_HIP(hipStreamSynchronize(st));
        reads++;
        bool done = false;
        for (int q = 0; q < per_poll && !done; q++) {
            done = true;
            for (int f = 0; f < n; f++)
                if (host[(size_t)q * n + f]) {
                    last[f] = (int32_t)(base + q + 1);
                    done = false;
                }
        }
        if (done)
            break;
        if (base > (int64_t)h * w) {                 // every iteration before the last deletes a pixel
            set_error("guo-hall thinning: no fixed point after %lld iterations", (long long)base);
            return VA_ERR_HIP;
        }
    }
    if (fast)
        hipLaunchKernelGGL(gh_unpack_kernel<true>, words_grid, block, 0, st, cur, src, dst, rows, w, wpr);
    else
        hipLaunchKernelGGL(gh_unpack_kernel<false>, words_grid, block, 0, st, cur, src, dst, rows, w, wpr);
    VA_LAUNCH_CHECK("gh_unpack_kernel");
    if (iterations_out)
        for (int f = 0; f < n; f++)
            iterations_out[f] = last[f] + 1;         // the final, empty iteration counts
    if (stats_out)
        stats_out[0] = launches, stats_out[1] = reads;
    return VA_OK;
}

}  // extern "C"
