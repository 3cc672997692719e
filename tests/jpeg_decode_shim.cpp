// A stand-alone serial JPEG decoder made of va_jpeg_decode_math.h alone, for the host compiler and its sanitizers
// (tests/test_mjpeg_decode_host.py builds and runs it; nothing of it is loaded into Python).  It reads records from
// standard input until the end:
//   int32 h, w, c, ri, scan_begin, bytes | c * 64 bytes of quantisation tables | 2 * c HuffDecode tables | the file
// decodes each file from a heap buffer of exactly its size, and prints one line per record: the status word and the
// 64-bit FNV-1a hash of the pixels.  The segment splitter is the serial form of DESIGN.md §9, "Motion-JPEG
// decoding": the device's locate kernel finds the same ranges in parallel.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "va_jpeg_decode_math.h"

namespace {

bool read_exact(void *dst, size_t n) { return fread(dst, 1, n, stdin) == n; }

struct Range {
    int64_t begin, end;
};

// the nseg byte ranges (-1: missing) and the marker-sequence bit
int32_t split(const uint8_t *p, int64_t len, int64_t scan_begin, int64_t nseg, std::vector<Range> &out)
{
    out.assign((size_t)nseg, Range{-1, -1});
    int64_t begin = scan_begin < 0 ? 0 : scan_begin > len ? len : scan_begin, k = 0;
    int terminator = -1;
    bool stopped = false;
    for (int64_t i = begin; i + 1 < len; i++) {
        if (p[i] != 0xFF || p[i + 1] == 0 || p[i + 1] == 0xFF)
            continue;
        if (k < nseg)
            out[(size_t)k] = Range{begin, i};
        if (p[i + 1] != 0xD0 + (k & 7)) {
            terminator = p[i + 1];
            stopped = true;
            k++;
            break;
        }
        begin = i + 2;
        k++;
        i++;
    }
    if (!stopped) {
        if (k < nseg)
            out[(size_t)k] = Range{begin, len};
        k++;
    }
    return stopped && terminator == 0xD9 && k == nseg ? 0 : va_jpeg::kStatusMarker;
}

}  // namespace

int main()
{
    static_assert(sizeof(va_jpeg::HuffDecode) == 1416, "the table layout the host builds");
    int32_t head[6];
    while (read_exact(head, sizeof(head))) {
        const int h = head[0], w = head[1], c = head[2], ri = head[3];
        const int64_t scan_begin = head[4], len = head[5];
        if (h < 1 || w < 1 || (c != 1 && c != 3) || ri < 1 || len < 0)
            return 2;
        std::vector<uint8_t> qt((size_t)c * 64);
        std::vector<va_jpeg::HuffDecode> huff((size_t)2 * c);
        if (!read_exact(qt.data(), qt.size()) || !read_exact(huff.data(), huff.size() * sizeof(va_jpeg::HuffDecode)))
            return 3;
        uint8_t *file = new uint8_t[(size_t)len];        // exactly the file: a read behind it is an error
        if (!read_exact(file, (size_t)len))
            return 4;
        const int by = (h + 7) / 8, bx = (w + 7) / 8;
        const int64_t mcus = (int64_t)by * bx, nseg = (mcus + ri - 1) / ri;
        std::vector<Range> segs;
        int32_t status = split(file, len, scan_begin, nseg, segs);
        std::vector<int16_t> coef((size_t)c * mcus * 64, 0);
        for (int64_t j = 0; j < nseg; j++) {
            if (segs[(size_t)j].begin < 0)
                continue;
            va_jpeg::BitReader r = va_jpeg::open_bits(file, segs[(size_t)j].begin, segs[(size_t)j].end);
            int pred[3] = {0, 0, 0};
            bool dead = false;
            const int64_t m1 = (j + 1) * ri < mcus ? (j + 1) * ri : mcus;
            for (int64_t m = j * ri; m < m1 && !dead; m++)
                for (int ch = 0; ch < c && !dead; ch++) {
                    int16_t *blk = coef.data() + ((size_t)ch * mcus + m) * 64;
                    const int32_t e = va_jpeg::decode_block(r, huff[2 * ch], huff[2 * ch + 1], pred[ch],
                                                            [&](int i, int v) { blk[i] = (int16_t)v; });
                    if (e) {
                        status |= e;
                        dead = true;
                        memset(blk, 0, 64 * sizeof(int16_t));
                    }
                }
        }
        delete[] file;
        std::vector<uint8_t> pixels((size_t)h * w * c);
        for (int64_t m = 0; m < mcus; m++) {
            uint8_t smp[3][64];
            for (int ch = 0; ch < c; ch++)
                va_jpeg::inverse_block(coef.data() + ((size_t)ch * mcus + m) * 64, qt.data() + 64 * ch, smp[ch]);
            for (int y = 0; y < 8; y++)
                for (int x = 0; x < 8; x++) {
                    const int64_t gy = (m / bx) * 8 + y, gx = (m % bx) * 8 + x;
                    if (gy >= h || gx >= w)
                        continue;
                    uint8_t *dst = pixels.data() + (gy * w + gx) * c;
                    if (c == 1) {
                        dst[0] = smp[0][8 * y + x];
                    } else {
                        int rr, gg, bb;
                        va_jpeg::rgb_of(smp[0][8 * y + x], smp[1][8 * y + x], smp[2][8 * y + x], rr, gg, bb);
                        dst[0] = (uint8_t)rr, dst[1] = (uint8_t)gg, dst[2] = (uint8_t)bb;
                    }
                }
        }
        uint64_t hash = 1469598103934665603ull;
        for (uint8_t v : pixels)
            hash = (hash ^ v) * 1099511628211ull;
        printf("%d %llu\n", (int)status, (unsigned long long)hash);
    }
    return 0;
}
