// A stand-alone host program around video-analysis_amd/csrc/va_intensity_math.h for tests/test_region_intensity_host.py:
// the region intensity of DESIGN.md §9, "Region intensity", computed serially with the header's record layout, span
// accumulation, merge, flush and percentile walk, compiled with the host C++ compiler under
// -fsanitize=address,undefined.  Spans are 4 pixels of one row, and the last runs of consecutive spans that carry one
// record are merged before they are flushed, in groups of 64 spans (the lanes of a wave, for a kernel on top of it).
// Every buffer here has exactly the size of what it holds, so an index beyond a plane or a table is reported.
// Input (stdin, binary): int32 n, h, w, c, max_labels; q float64 percentiles (q = 4); n * h * w int32 labels;
// n * h * w * c uint8 samples.
// Output (stdout, binary): the table, n * max_labels * c * 8 int64; the histograms, n * max_labels * c * 256 uint32;
// the percentiles, n * max_labels * c * q int32 (-1 for an empty region).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "va_intensity_math.h"

namespace vi = va_intensity;
constexpr int kQ = 4, kGroup = 64;

static bool read_all(void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, stdin) == bytes; }
static void write_all(const void *src, size_t bytes)
{
    if (bytes)
        fwrite(src, 1, bytes, stdout);
}

template <int C>
static int run(int n, int h, int w, int max_labels, const double *q)
{
    const size_t px = (size_t)h * w, entries = (size_t)n * max_labels * C;
    std::vector<int32_t> labels((size_t)n * px);
    std::vector<uint8_t> frames((size_t)n * px * C);
    if (!read_all(labels.data(), labels.size() * 4) || !read_all(frames.data(), frames.size()))
        return 2;
    std::vector<int64_t> table(entries * vi::kStride);
    for (size_t i = 0; i < table.size(); i++)
        table[i] = vi::empty_value((int)(i % vi::kStride));
    std::vector<uint32_t> hist(entries * vi::kBins, 0u);
    auto record = [&](int64_t key) { return table.data() + (size_t)key * C * vi::kStride; };
    const int w4 = (w + vi::kSpan - 1) / vi::kSpan;
    int64_t pending_key = -1;
    vi::Partial<C> pending;
    vi::clear(pending);
    size_t span = 0;
    for (int f = 0; f < n; f++)
        for (int y = 0; y < h; y++)
            for (int wi = 0; wi < w4; wi++, span++) {
                const int x0 = wi * vi::kSpan, m = w - x0 < vi::kSpan ? w - x0 : vi::kSpan;
                const size_t at = ((size_t)f * h + y) * w + x0;
                vi::Partial<C> tail;
                const int32_t lab = vi::accumulate_span<C>(
                    labels.data() + at, frames.data() + at * C, m, x0, y, max_labels, tail,
                    [&](int32_t a, const vi::Partial<C> &p) { vi::flush<C>(record((int64_t)f * max_labels + a - 1), p); });
                const int64_t key = lab ? (int64_t)f * max_labels + lab - 1 : -1;
                if (span % kGroup == 0 || key != pending_key) {         // a head: the segment in front is complete
                    if (pending_key >= 0)
                        vi::flush<C>(record(pending_key), pending);
                    pending_key = key;
                    pending = tail;
                } else {
                    vi::merge<C>(pending, tail);
                }
                for (int j = 0; j < m; j++)
                    if (vi::is_region(labels[at + j], max_labels))
                        for (int k = 0; k < C; k++)
                            hist[(((size_t)f * max_labels + labels[at + j] - 1) * C + k) * vi::kBins + frames[(at + j) * C + k]]++;
            }
    if (pending_key >= 0)
        vi::flush<C>(record(pending_key), pending);
    std::vector<int32_t> pct(entries * kQ);
    for (size_t e = 0; e < entries; e++) {
        const uint64_t count = (uint64_t)table[e * vi::kStride + vi::kCount];
        for (int i = 0; i < kQ; i++)
            pct[e * kQ + i] = vi::percentile_walk(hist.data() + e * vi::kBins, vi::nearest_rank(q[i], count));
    }
    write_all(table.data(), table.size() * 8);
    write_all(hist.data(), hist.size() * 4);
    write_all(pct.data(), pct.size() * 4);
    return 0;
}

int main()
{
    int32_t head[5];
    double q[kQ];
    if (!read_all(head, sizeof head) || !read_all(q, sizeof q))
        return 2;
    if (head[0] < 0 || head[1] < 1 || head[2] < 1 || head[4] < 1)
        return 3;
    if (head[3] == 1)
        return run<1>(head[0], head[1], head[2], head[4], q);
    if (head[3] == 3)
        return run<3>(head[0], head[1], head[2], head[4], q);
    return 3;
}
