// A stand-alone host program around video-analysis_amd/csrc/va_median_math.h for tests/test_temporal_median_host.py: the
// rank planes of DESIGN.md §9, "Temporal median", computed serially with the header's column logic, one dword column
// after the other, compiled with the host C++ compiler under -fsanitize=address,undefined.  The path of a call is
// chosen as va_temporal_ranks_u8 chooses it: the sorting network of the depth's class up to 64 planes, the counting
// passes (two or eight ranks a pass) above; dword accesses where px and the stride are multiples of four, byte accesses
// otherwise.  Every buffer here has exactly the size of what it holds -- (t - 1) * stride + px bytes of frames,
// k * px bytes of planes -- so a read beyond a plane's last byte or a write beyond the planes is reported.
// Input (stdin, binary), any number of calls: int64 t, px, stride, k; k int64 ranks; the frames.
// Output (stdout, binary): the k * px bytes of each call, one after the other.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "va_median_math.h"

static bool read_all(void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, stdin) == bytes; }

template <bool kAligned>
static void columns(const uint8_t *frames, int t, size_t px, size_t stride, uint64_t ranks, int k, uint8_t *out)
{
    for (size_t p = 0; p < px; p += 4) {
        if (t > va_median::kSortMaxPlanes) {
            if (k <= 2)
                va_median::ranks_counted<2, kAligned>(frames, t, px, stride, ranks, k, out, p);
            else
                va_median::ranks_counted<8, kAligned>(frames, t, px, stride, ranks, k, out, p);
            continue;
        }
        switch (va_median::sort_class(t)) {
        case 8: va_median::ranks_sorted<8, kAligned>(frames, t, px, stride, ranks, k, out, p); break;
        case 16: va_median::ranks_sorted<16, kAligned>(frames, t, px, stride, ranks, k, out, p); break;
        case 32: va_median::ranks_sorted<32, kAligned>(frames, t, px, stride, ranks, k, out, p); break;
        default: va_median::ranks_sorted<64, kAligned>(frames, t, px, stride, ranks, k, out, p); break;
        }
    }
}

int main()
{
    int64_t head[4];
    while (fread(head, 1, sizeof head, stdin) == sizeof head) {
        const int t = (int)head[0], k = (int)head[3];
        const size_t px = (size_t)head[1], stride = (size_t)head[2];
        if (t < 1 || t > va_median::kMaxPlanes || px < 1 || stride < px || k < 1 || k > va_median::kMaxRanks)
            return 2;
        int64_t wide[va_median::kMaxRanks];
        int32_t ranks[va_median::kMaxRanks];
        if (!read_all(wide, (size_t)k * sizeof wide[0]))
            return 2;
        for (int j = 0; j < k; j++) {
            if (wide[j] < 0 || wide[j] >= t)
                return 2;
            ranks[j] = (int32_t)wide[j];
        }
        std::vector<uint8_t> frames((size_t)(t - 1) * stride + px), out((size_t)k * px, 0xA5);
        if (!read_all(frames.data(), frames.size()))
            return 2;
        const uint64_t packed = va_median::pack_ranks(ranks, k);
        if (px % 4 == 0 && stride % 4 == 0)
            columns<true>(frames.data(), t, px, stride, packed, k, out.data());
        else
            columns<false>(frames.data(), t, px, stride, packed, k, out.data());
        fwrite(out.data(), 1, out.size(), stdout);
    }
    return 0;
}
