// va_intensity_math.h -- the arithmetic of the region intensity ("Region intensity"), written for host
// and device alike: the record layout and its empty values, the accumulation of a span of pixels into (label, partial
// record) runs, the merge of two partial records, the flush of a partial record into a record, and the percentile
// rule as an integer walk over 256 bins.  Today only the host test tests/region_intensity_shim.cpp compiles it, where
// it runs serially with plain stores; no kernel of the library includes it yet (DESIGN.md says why).  In device code
// the flush uses 64-bit integer add, min and max, which commute: a record does not depend on the order of arrival.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VA_INTENSITY_HD __host__ __device__ __forceinline__
#else
#define VA_INTENSITY_HD inline
#endif

namespace va_intensity {

// one record: kStride int64 per (frame, label, channel)
constexpr int kStride = 8;
enum { kSum = 0, kSumSq = 1, kSumX = 2, kSumY = 3, kMin = 4, kMax = 5, kCount = 6, kSpare = 7 };
constexpr int kEmptyMin = 256, kEmptyMax = -1;      // min and max of a region without pixels
constexpr int kBins = 256;                          // histogram bins of a (frame, label, channel)
constexpr int kSpan = 4;                            // consecutive pixels of one row that a lane covers

// the value of slot `slot` of a record no pixel has reached
VA_INTENSITY_HD int64_t empty_value(int slot) { return slot == kMin ? kEmptyMin : slot == kMax ? kEmptyMax : 0; }

// a label word names a region iff 1 <= l <= max_labels; 0, negative words and larger labels are ignored
VA_INTENSITY_HD bool is_region(int32_t l, int max_labels) { return l >= 1 && l <= max_labels; }

// The sums of at most 65536 pixels of one label (a wave's 256 in a kernel): Σv and Σv² fit 32 bits (65536 * 255²
// < 2^32), Σv·x and Σv·y are kept modulo 2^64 like the record's.
template <int C>
struct Partial {
    uint32_t count;
    uint32_t sum[C], sumsq[C];
    unsigned long long sumx[C], sumy[C];
    int32_t min[C], max[C];
};

template <int C>
VA_INTENSITY_HD void clear(Partial<C> &p)
{
    p.count = 0;
    for (int k = 0; k < C; k++) {
        p.sum[k] = p.sumsq[k] = 0;
        p.sumx[k] = p.sumy[k] = 0;
        p.min[k] = kEmptyMin;
        p.max[k] = kEmptyMax;
    }
}

// the pixel (x, y) with the samples v[0 .. C)
template <int C, class Sample>
VA_INTENSITY_HD void add_pixel(Partial<C> &p, const Sample *v, int x, int y)
{
    p.count++;
    for (int k = 0; k < C; k++) {
        const uint32_t s = (uint32_t)v[k];
        p.sum[k] += s;
        p.sumsq[k] += s * s;
        p.sumx[k] += (unsigned long long)s * (unsigned long long)x;
        p.sumy[k] += (unsigned long long)s * (unsigned long long)y;
        p.min[k] = (int32_t)s < p.min[k] ? (int32_t)s : p.min[k];
        p.max[k] = (int32_t)s > p.max[k] ? (int32_t)s : p.max[k];
    }
}

// a += b: two partial records of one label
template <int C>
VA_INTENSITY_HD void merge(Partial<C> &a, const Partial<C> &b)
{
    a.count += b.count;
    for (int k = 0; k < C; k++) {
        a.sum[k] += b.sum[k];
        a.sumsq[k] += b.sumsq[k];
        a.sumx[k] += b.sumx[k];
        a.sumy[k] += b.sumy[k];
        a.min[k] = b.min[k] < a.min[k] ? b.min[k] : a.min[k];
        a.max[k] = b.max[k] > a.max[k] ? b.max[k] : a.max[k];
    }
}

// The m <= kSpan pixels at columns x0 .. x0 + m - 1 of row y, labels l[0 .. m) and samples v[0 .. m * C), as runs of one
// region label: a run goes on over pixels of no region and ends where another region's label follows (the sums need
// no neighbourhood, and a region with holes then costs no more than a solid one).  Every run that ends inside the
// span goes to emit(label, partial); the last run stays in `tail`, and its label is returned (0: the span meets no
// region, and tail is empty).
template <int C, class Sample, class Emit>
VA_INTENSITY_HD int32_t accumulate_span(const int32_t *l, const Sample *v, int m, int x0, int y, int max_labels,
                                        Partial<C> &tail, Emit &&emit)
{
    int32_t cur = 0;
    clear(tail);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 0; j < kSpan; j++) {
        if (j >= m)
            continue;
        if (!is_region(l[j], max_labels))
            continue;
        if (cur && l[j] != cur) {
            emit(cur, tail);
            clear(tail);
        }
        cur = l[j];
        add_pixel<C>(tail, v + j * C, x0 + j, y);
    }
    return cur;
}

// a partial record into the C records of its (frame, label): rec[k * kStride + slot]
template <int C>
VA_INTENSITY_HD void flush(int64_t *rec, const Partial<C> &p)
{
    for (int k = 0; k < C; k++) {
        int64_t *r = rec + k * kStride;
#if defined(__HIP_DEVICE_COMPILE__)
        unsigned long long *u = reinterpret_cast<unsigned long long *>(r);
        long long *s = reinterpret_cast<long long *>(r);
        atomicAdd(u + kSum, (unsigned long long)p.sum[k]);
        atomicAdd(u + kSumSq, (unsigned long long)p.sumsq[k]);
        atomicAdd(u + kSumX, p.sumx[k]);
        atomicAdd(u + kSumY, p.sumy[k]);
        atomicMin(s + kMin, (long long)p.min[k]);
        atomicMax(s + kMax, (long long)p.max[k]);
        atomicAdd(u + kCount, (unsigned long long)p.count);
#else
        r[kSum] = (int64_t)((uint64_t)r[kSum] + p.sum[k]);
        r[kSumSq] = (int64_t)((uint64_t)r[kSumSq] + p.sumsq[k]);
        r[kSumX] = (int64_t)((uint64_t)r[kSumX] + p.sumx[k]);
        r[kSumY] = (int64_t)((uint64_t)r[kSumY] + p.sumy[k]);
        r[kMin] = p.min[k] < r[kMin] ? p.min[k] : r[kMin];
        r[kMax] = p.max[k] > r[kMax] ? p.max[k] : r[kMax];
        r[kCount] = (int64_t)((uint64_t)r[kCount] + p.count);
#endif
    }
}

// the nearest-rank rule: percentile q of n values is the value of rank max(1, ceil(q / 100 * n)), ranks from 1
inline uint64_t nearest_rank(double q, uint64_t n)
{
    const double r = ceil(q / 100.0 * (double)n);
    return r < 1.0 ? 1 : (uint64_t)r;
}

// the smallest value whose cumulative count reaches `rank` >= 1; -1 where the bins hold fewer than `rank` pixels
// (an empty region)
VA_INTENSITY_HD int percentile_walk(const uint32_t *bins, uint64_t rank)
{
    uint64_t cum = 0;
    for (int v = 0; v < kBins; v++) {
        cum += bins[v];
        if (cum >= rank)
            return v;
    }
    return -1;
}

}  // namespace va_intensity
