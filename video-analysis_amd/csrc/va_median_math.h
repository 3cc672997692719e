// va_median_math.h -- the packed-byte arithmetic of the temporal rank planes ("Temporal median") that
// the kernels of va_median.hip and the host test tests/median_shim.cpp share: everything one dword column does.  A
// dword column is four adjacent pixels of a plane, the bytes of one little-endian dword, over all t planes.  Its bytes
// are widened to two dwords of 16-bit halves (the even bytes 0 and 2, the odd bytes 1 and 3), so that a packed 16-bit
// minimum / maximum is a compare-exchange of two pixels, and 0xffff sorts behind every pixel value.
//   t <= 64   sort_pairs: Batcher's odd-even merge sort of N = 8, 16, 32 or 64 such dwords, the entries t .. N - 1
//             padded with 0xffff.  Every rank of the column is then one pick; the stack is read once.
//   t >= 65   ranks_counted: the rank-r value is the largest x with #{v < x} <= r, built bit by bit from the top;
//             each of the eight passes reads the column again and counts #{v >= trial} for up to K ranks at once in
//             bits 8 .. 15 of each half (t <= 255 makes a count fit).
// On the device the exchange is v_pk_min_u16 / v_pk_max_u16; on the host the same text runs serially.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VA_MEDIAN_HD __host__ __device__ __forceinline__
#else
#define VA_MEDIAN_HD inline
#endif

namespace va_median {

constexpr int kMaxPlanes = 255;              // a count of planes fits a byte
constexpr int kMaxRanks = 8;
constexpr int kSortMaxPlanes = 64;           // the deepest column the sorting path holds in registers
constexpr uint32_t kHalves = 0x00ff00ffu;    // the low byte of each 16-bit half
constexpr uint32_t kPad = 0xffffffffu;       // two halves above every pixel value
constexpr uint32_t kBias = 0x01000100u;      // bit 8 of each half: (v | bias) - trial keeps it where v >= trial

// the register columns of the sorting path for t planes: 8, 16, 32 or 64 (t <= kSortMaxPlanes)
VA_MEDIAN_HD int sort_class(int t) { return t <= 8 ? 8 : t <= 16 ? 16 : t <= 32 ? 32 : 64; }

// up to eight ranks in one 64-bit word, rank j in byte j
VA_MEDIAN_HD uint64_t pack_ranks(const int32_t *ranks, int k)
{
    uint64_t packed = 0;
    for (int j = 0; j < k; j++)
        packed |= (uint64_t)(uint32_t)ranks[j] << (8 * j);
    return packed;
}
VA_MEDIAN_HD int rank_of(uint64_t packed, int j) { return (int)((packed >> (8 * j)) & 0xffu); }

VA_MEDIAN_HD uint32_t even_bytes(uint32_t d) { return d & kHalves; }
VA_MEDIAN_HD uint32_t odd_bytes(uint32_t d) { return (d >> 8) & kHalves; }
VA_MEDIAN_HD uint32_t join_bytes(uint32_t even, uint32_t odd) { return even | (odd << 8); }

// bytes p .. p + 3 of a plane of px bytes as one dword.  kAligned: the plane starts on a dword and px is a multiple
// of four, so the dword lies inside it; otherwise byte by byte, and a byte at or beyond px reads as 0 (never loaded)
template <bool kAligned>
VA_MEDIAN_HD uint32_t load_column(const uint8_t *plane, size_t p, size_t px)
{
    uint32_t d = 0;
    if (kAligned) {
        __builtin_memcpy(&d, __builtin_assume_aligned(plane + p, 4), 4);
    } else {
        for (int b = 0; b < 4; b++)
            if (p + b < px)
                d |= (uint32_t)plane[p + b] << (8 * b);
    }
    return d;
}
template <bool kAligned>
VA_MEDIAN_HD void store_column(uint8_t *plane, size_t p, size_t px, uint32_t d)
{
    if (kAligned) {
        __builtin_memcpy(__builtin_assume_aligned(plane + p, 4), &d, 4);
    } else {
        for (int b = 0; b < 4; b++)
            if (p + b < px)
                plane[p + b] = (uint8_t)(d >> (8 * b));
    }
}

// compare-exchange of two pixels at once: lo gets the smaller of each 16-bit half, hi the larger
VA_MEDIAN_HD void exchange(uint32_t &lo, uint32_t &hi)
{
#if defined(__HIP_DEVICE_COMPILE__)
    typedef unsigned short halves_t __attribute__((ext_vector_type(2)));
    const halves_t a = __builtin_bit_cast(halves_t, lo), b = __builtin_bit_cast(halves_t, hi);
    lo = __builtin_bit_cast(uint32_t, __builtin_elementwise_min(a, b));
    hi = __builtin_bit_cast(uint32_t, __builtin_elementwise_max(a, b));
#else
    const uint32_t a0 = lo & 0xffffu, a1 = lo >> 16, b0 = hi & 0xffffu, b1 = hi >> 16;
    lo = (a0 < b0 ? a0 : b0) | ((a1 < b1 ? a1 : b1) << 16);
    hi = (a0 < b0 ? b0 : a0) | ((a1 < b1 ? b1 : a1) << 16);
#endif
}

// Batcher's odd-even merge sort on v[kLo .. kLo + kN), kN a power of two, as compile-time recursion: every index is
// a constant, so the array stays in registers.  merge<kLo, kN, kR> merges the two sorted halves of the elements
// kLo, kLo + kR, kLo + 2 kR, ... below kLo + kN.
template <int kLo, int kN, int kR, int kLen>
VA_MEDIAN_HD void merge_pairs(uint32_t (&v)[kLen])
{
    constexpr int kStep = kR * 2;
    if constexpr (kStep < kN) {
        merge_pairs<kLo, kN, kStep>(v);
        merge_pairs<kLo + kR, kN, kStep>(v);
#pragma unroll
        for (int i = kLo + kR; i + kR < kLo + kN; i += kStep)
            exchange(v[i], v[i + kR]);
    } else {
        exchange(v[kLo], v[kLo + kR]);
    }
}
template <int kLo, int kN, int kLen>
VA_MEDIAN_HD void sort_range(uint32_t (&v)[kLen])
{
    if constexpr (kN > 1) {
        sort_range<kLo, kN / 2>(v);
        sort_range<kLo + kN / 2, kN / 2>(v);
        merge_pairs<kLo, kN, 1>(v);
    }
}
template <int kN>
VA_MEDIAN_HD void sort_pairs(uint32_t (&v)[kN]) { sort_range<0, kN>(v); }

// v[rank] without an indexed register: one and-or per entry with a mask that is the same in every lane (a chain of
// selects on i == rank is folded back into an indexed load, which puts the column into scratch)
template <int kN>
VA_MEDIAN_HD uint32_t pick(const uint32_t (&v)[kN], int rank)
{
    uint32_t sel = 0;
#pragma unroll
    for (int i = 0; i < kN; i++)
        sel |= v[i] & (0u - (uint32_t)(i == rank));
    return sel;
}

// the compiler's scheduler does not move instructions across this line (device only): what is live on one side of it
// stays apart from what is live on the other
VA_MEDIAN_HD void schedule_fence()
{
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_sched_barrier(0);
#endif
}

// the even (kOdd = false) or odd bytes of the column dwords d[0 .. t) sorted, and the k ranks picked into res
template <int kN, bool kOdd>
VA_MEDIAN_HD void ranks_of_halves(const uint32_t (&d)[kN], int t, uint64_t ranks, int k, uint32_t (&res)[kMaxRanks])
{
    uint32_t v[kN];
#pragma unroll
    for (int i = 0; i < kN; i++)
        v[i] = i < t ? (kOdd ? odd_bytes(d[i]) : even_bytes(d[i])) : kPad;
    sort_pairs<kN>(v);
#pragma unroll
    for (int j = 0; j < kMaxRanks; j++) {
        res[j] = 0;
        if (j < k)
            res[j] = pick<kN>(v, rank_of(ranks, j));
    }
}

// The k rank planes of the dword column at byte p of a stack of t <= kN planes: out[j * px + p ..] = sorted[rank j].
// The two halves are sorted one after the other, so that the column's dwords and one sorted array are live at a time.
template <int kN, bool kAligned>
VA_MEDIAN_HD void ranks_sorted(const uint8_t *frames, int t, size_t px, size_t stride, uint64_t ranks, int k,
                               uint8_t *out, size_t p)
{
    uint32_t d[kN], even[kMaxRanks], odd[kMaxRanks];
#pragma unroll
    for (int i = 0; i < kN; i++) {
        d[i] = 0;
        if (i < t)
            d[i] = load_column<kAligned>(frames + (size_t)i * stride, p, px);
    }
    ranks_of_halves<kN, false>(d, t, ranks, k, even);
    schedule_fence();
    ranks_of_halves<kN, true>(d, t, ranks, k, odd);
    schedule_fence();
#pragma unroll
    for (int j = 0; j < kMaxRanks; j++)
        if (j < k)
            store_column<kAligned>(out + (size_t)j * px, p, px, join_bytes(even[j], odd[j]));
}

// one plane's halves (biased) into the count of a trial: bits 8 .. 15 of each half count the planes with v >= trial
VA_MEDIAN_HD uint32_t count_ge(uint32_t acc, uint32_t biased, uint32_t trial) { return acc + ((biased - trial) & kBias); }
// the trial bit stays in each half of `res` whose count of v >= trial reaches need = t - rank, i.e. #{v < trial} <= rank
VA_MEDIAN_HD uint32_t accept_bit(uint32_t res, uint32_t acc, uint32_t need, uint32_t bit)
{
    const uint32_t c0 = (acc >> 8) & 0xffu, c1 = acc >> 24;
    return res | (c0 >= need ? bit : 0u) | (c1 >= need ? bit << 16 : 0u);
}

// The same planes for a stack of any depth up to kMaxPlanes, kK ranks a pass (k <= kK; the spare slots repeat the
// last rank): eight passes over the column, one per bit of the value.
template <int kK, bool kAligned>
VA_MEDIAN_HD void ranks_counted(const uint8_t *frames, int t, size_t px, size_t stride, uint64_t ranks, int k,
                                uint8_t *out, size_t p)
{
    uint32_t res_even[kK], res_odd[kK], need[kK];
#pragma unroll
    for (int j = 0; j < kK; j++) {
        res_even[j] = res_odd[j] = 0;
        need[j] = (uint32_t)(t - rank_of(ranks, j < k ? j : k - 1));
    }
    for (uint32_t bit = 0x80u; bit; bit >>= 1) {
        uint32_t acc_even[kK], acc_odd[kK];
#pragma unroll
        for (int j = 0; j < kK; j++)
            acc_even[j] = acc_odd[j] = 0;
#pragma unroll 4
        for (int i = 0; i < t; i++) {
            const uint32_t d = load_column<kAligned>(frames + (size_t)i * stride, p, px);
            const uint32_t even = even_bytes(d) | kBias, odd = odd_bytes(d) | kBias;
#pragma unroll
            for (int j = 0; j < kK; j++) {
                acc_even[j] = count_ge(acc_even[j], even, res_even[j] | (bit * 0x00010001u));
                acc_odd[j] = count_ge(acc_odd[j], odd, res_odd[j] | (bit * 0x00010001u));
            }
        }
#pragma unroll
        for (int j = 0; j < kK; j++) {
            res_even[j] = accept_bit(res_even[j], acc_even[j], need[j], bit);
            res_odd[j] = accept_bit(res_odd[j], acc_odd[j], need[j], bit);
        }
    }
#pragma unroll
    for (int j = 0; j < kK; j++)
        if (j < k)
            store_column<kAligned>(out + (size_t)j * px, p, px, join_bytes(res_even[j], res_odd[j]));
}

}  // namespace va_median
