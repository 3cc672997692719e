// A stand-alone serial JPEG decoder of every sampling layout, made of va_jpeg_decode_math.h alone, for the host
// compiler and its sanitizers (tests/test_mjpeg_decode_host.py and tests/test_mjpeg_subsampled_host.py build and run
// it; nothing of it is loaded into Python).  It reads records from standard input until the end:
//   int32 h, w, c, ri, scan_begin, bytes, luma_h, luma_v | c * 64 bytes of quantisation tables |
//   2 * c HuffDecode tables | the file
// decodes each file from a heap buffer of exactly its size, and prints one line per record: the status word and the
// 64-bit FNV-1a hash of the pixels.  The segment splitter is the serial form of DESIGN.md §9, "Motion-JPEG
// decoding": the device's locate kernel finds the same ranges in parallel.  The MCU walk, the clamps and the two
// upsampling formulas are the text the kernels call ("Subsampled Motion-JPEG decoding").
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
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

// the 64 samples of `blocks` blocks of rows of `across` blocks, as a plane of rows of across * 8 samples
void plane_of(const int16_t *coef, int64_t blocks, int64_t across, const uint8_t *q, std::vector<uint8_t> &plane)
{
    plane.resize((size_t)(blocks * 64));
    uint8_t smp[64];
    for (int64_t b = 0; b < blocks; b++) {
        va_jpeg::inverse_block(coef + b * 64, q, smp);
        for (int i = 0; i < 64; i++)
            plane[(size_t)(((b / across) * 8 + i / 8) * across * 8 + (b % across) * 8 + i % 8)] = smp[i];
    }
}

}  // namespace

int main()
{
    static_assert(sizeof(va_jpeg::HuffDecode) == 1416, "the table layout the host builds");
    int32_t head[8];
    while (read_exact(head, sizeof(head))) {
        const int h = head[0], w = head[1], c = head[2], ri = head[3], lh = head[6], lv = head[7];
        const int64_t scan_begin = head[4], len = head[5];
        const bool plain = lh == 1 && lv == 1, sampled = c == 3 && lh == 2 && (lv == 1 || lv == 2);
        if (h < 1 || w < 1 || (c != 1 && c != 3) || ri < 1 || len < 0 || !(plain || sampled))
            return 2;
        std::vector<uint8_t> qt((size_t)c * 64);
        std::vector<va_jpeg::HuffDecode> huff((size_t)2 * c);
        if (!read_exact(qt.data(), qt.size()) || !read_exact(huff.data(), huff.size() * sizeof(va_jpeg::HuffDecode)))
            return 3;
        uint8_t *file = new uint8_t[(size_t)len];        // exactly the file: a read behind it is an error
        if (!read_exact(file, (size_t)len))
            return 4;
        const int my = (h + 8 * lv - 1) / (8 * lv), mx = (w + 8 * lh - 1) / (8 * lh);
        const int64_t mcus = (int64_t)my * mx, nseg = (mcus + ri - 1) / ri;
        const int blocks = c == 1 ? 1 : va_jpeg::mcu_blocks(lh, lv);
        std::vector<Range> segs;
        int32_t status = split(file, len, scan_begin, nseg, segs);
        std::vector<int16_t> coef((size_t)blocks * mcus * 64, 0);
        for (int64_t j = 0; j < nseg; j++) {
            if (segs[(size_t)j].begin < 0)
                continue;
            va_jpeg::BitReader r = va_jpeg::open_bits(file, segs[(size_t)j].begin, segs[(size_t)j].end);
            int pred[3] = {0, 0, 0};
            bool dead = false;
            const int64_t m1 = (j + 1) * ri < mcus ? (j + 1) * ri : mcus;
            for (int64_t m = j * ri; m < m1 && !dead; m++)
                for (int k = 0; k < blocks && !dead; k++) {
                    int comp = 0;
                    int16_t *blk = coef.data() + va_jpeg::mcu_block_at(k, lh, lv, my, mx, m / mx, m % mx, comp) * 64;
                    const int32_t e = va_jpeg::decode_block(r, huff[2 * comp], huff[2 * comp + 1], pred[comp],
                                                            [&](int i, int v) { blk[i] = (int16_t)v; });
                    if (e) {
                        status |= e;
                        dead = true;
                        memset(blk, 0, 64 * sizeof(int16_t));
                    }
                }
        }
        delete[] file;
        // the planes: Y of my lv 8 x mx lh 8 samples, Cb and Cr of my 8 x mx 8
        const int64_t ys = (int64_t)mx * lh * 8, cs = (int64_t)mx * 8;
        std::vector<uint8_t> plane[3];
        plane_of(coef.data(), mcus * lh * lv, (int64_t)mx * lh, qt.data(), plane[0]);
        for (int comp = 1; comp < c; comp++)
            plane_of(coef.data() + (lh * lv + comp - 1) * mcus * 64, mcus, mx, qt.data() + 64 * comp, plane[comp]);
        const int cw = (w + lh - 1) / lh, ch = (h + lv - 1) / lv;
        uint8_t *pixels = new uint8_t[(size_t)h * w * c];
        for (int gy = 0; gy < h; gy++)
            for (int gx = 0; gx < w; gx++) {
                uint8_t *dst = pixels + ((size_t)gy * w + gx) * c;
                const int luma = plane[0][(size_t)(gy * ys + gx)];
                if (c == 1) {
                    dst[0] = (uint8_t)luma;
                    continue;
                }
                int chroma[2];
                for (int comp = 0; comp < 2; comp++)
                    chroma[comp] = plain ? plane[1 + comp][(size_t)(gy * cs + gx)] : va_jpeg::upsampled_at(
                        [&](int row, int col) {
                            if (row < 0 || row >= ch || col < 0 || col >= cw)
                                abort();                     // a padding sample, or none at all
                            return (int)plane[1 + comp][(size_t)(row * cs + col)];
                        },
                        gy, gx, lv, ch, cw);
                int rr, gg, bb;
                va_jpeg::rgb_of(luma, chroma[0], chroma[1], rr, gg, bb);
                dst[0] = (uint8_t)rr, dst[1] = (uint8_t)gg, dst[2] = (uint8_t)bb;
            }
        uint64_t hash = 1469598103934665603ull;
        for (size_t i = 0; i < (size_t)h * w * c; i++)
            hash = (hash ^ pixels[i]) * 1099511628211ull;
        delete[] pixels;
        printf("%d %llu\n", (int)status, (unsigned long long)hash);
    }
    return 0;
}
