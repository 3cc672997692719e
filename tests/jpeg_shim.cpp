// A stand-alone host program around video-analysis_amd/csrc/va_jpeg_math.h for tests/test_mjpeg_host.py: the header is
// compiled with the host C++ compiler (under -fsanitize=address,undefined there) into a serial encoder that walks
// the lanes of the device kernel one after the other.  Nothing here computes: colour conversion, transform,
// quantiser, Huffman strings, bit writer and stuffing all go to the header.
// Input (stdin, binary): int32 h, w, c; 128 bytes of quantisation tables (luma, chroma; natural order); h * w * c
// bytes of one frame.  Output (stdout, binary): the header's tables -- 64 int32 zigzag, 64 int32 DCT matrix, the
// HuffTables -- then per MCU row an int32 byte count and the stuffed bytes of its entropy segment.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "va_jpeg_math.h"

static void out32(int32_t v) { fwrite(&v, 4, 1, stdout); }

int main()
{
    int32_t dims[3];
    uint8_t qt[2][64];
    if (fread(dims, 4, 3, stdin) != 3 || fread(qt, 1, 128, stdin) != 128)
        return 2;
    const int h = dims[0], w = dims[1], c = dims[2];
    if (h < 1 || w < 1 || (c != 1 && c != 3))
        return 2;
    std::vector<uint8_t> frame((size_t)h * w * c);
    if (fread(frame.data(), 1, frame.size(), stdin) != frame.size())
        return 2;
    for (int k = 0; k < 64; k++)
        out32(va_jpeg::zigzag_at(k));
    for (int k = 0; k < 64; k++)
        out32(va_jpeg::dct_at(k / 8, k % 8));
    constexpr va_jpeg::HuffTables huff = va_jpeg::make_huff();
    fwrite(&huff, sizeof(huff), 1, stdout);

    const int mcus = (w + 7) / 8, nseg = (h + 7) / 8;
    for (int j = 0; j < nseg; j++) {
        // the segment's coefficients, block after block in coding order
        std::vector<std::vector<int16_t>> blocks;
        for (int m = 0; m < mcus; m++) {
            int x[3][64];
            for (int i = 0; i < 64; i++) {
                const int yy = 8 * j + i / 8 < h ? 8 * j + i / 8 : h - 1, xx = 8 * m + i % 8 < w ? 8 * m + i % 8 : w - 1;
                const uint8_t *p = &frame[((size_t)yy * w + xx) * c];
                if (c == 1) {
                    x[0][i] = p[0] - 128;
                } else {
                    int y, cb, cr;
                    va_jpeg::ycbcr(p[0], p[1], p[2], y, cb, cr);
                    x[0][i] = y - 128, x[1][i] = cb - 128, x[2][i] = cr - 128;
                }
            }
            for (int ch = 0; ch < c; ch++) {
                std::vector<int16_t> zz(64);
                va_jpeg::forward_block(x[ch], qt[ch ? 1 : 0], zz.data());
                blocks.push_back(zz);
            }
        }
        // the strings, one lane after the other: first their lengths, then the bits into a buffer of exactly that size
        std::vector<va_jpeg::Bits> strings;
        size_t total = 0;
        int pred[3] = {0, 0, 0};
        for (size_t q = 0; q < blocks.size(); q++) {
            const int ch = (int)(q % c), tab = ch ? 1 : 0;
            uint64_t nonzero = 0;
            for (int k = 0; k < 64; k++)
                nonzero |= (uint64_t)(blocks[q][k] != 0) << k;
            for (int k = 0; k < 64; k++) {
                strings.push_back(va_jpeg::coefficient_bits(huff.dc[tab], huff.ac[tab], k, blocks[q][k], pred[ch], nonzero));
                total += strings.back().len;
            }
            pred[ch] = blocks[q][0];
        }
        const int pad = (int)(-total & 7);
        strings.push_back(va_jpeg::Bits{(1ull << pad) - 1, pad});
        std::vector<uint32_t> words((total + pad + 31) / 32, 0u);
        uint32_t pos = 0;
        for (const va_jpeg::Bits &b : strings) {
            if (b.len < 0 || b.len > 59)
                return 3;
            va_jpeg::put_bits(pos, b, [&](uint32_t wi, uint32_t v) { words.at(wi) |= v; });
            pos += b.len;
        }
        const int nbytes = (int)((total + pad) / 8);
        std::vector<uint8_t> bytes;
        for (size_t wi = 0; wi < words.size(); wi++) {
            const int nvalid = nbytes - 4 * (int)wi < 4 ? nbytes - 4 * (int)wi : 4;
            uint8_t tmp[8];
            const int got = va_jpeg::put_stuffed(words[wi], nvalid, [&](int i, uint8_t v) { tmp[i] = v; });
            if (got != nvalid + va_jpeg::count_ff(words[wi], nvalid))
                return 4;
            bytes.insert(bytes.end(), tmp, tmp + got);
        }
        out32((int32_t)bytes.size());
        fwrite(bytes.data(), 1, bytes.size(), stdout);
    }
    return 0;
}
