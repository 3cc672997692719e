// A stand-alone host program around video-analysis_amd/csrc/va_jpeg_math.h for tests/test_mjpeg_encode_sampled_host.py:
// a serial encoder of the 4:2:2 and 4:2:0 streams of DESIGN.md §9, "Subsampled Motion-JPEG encoding", compiled with the
// host C++ compiler under -fsanitize=address,undefined.  The box average, the edge rule, the block-to-component map
// and the predictor map are the header's, as are colour conversion, transform, quantiser, Huffman strings, bit writer
// and stuffing; every buffer here has exactly the size of what it holds, so an index beyond a plane is reported.
// Input (stdin, binary): int32 h, w, H, V; 128 bytes of quantisation tables (luma, chroma; natural order); h * w * 3
// bytes of one RGB frame.  Output (stdout, binary): per MCU row an int32 byte count and the stuffed bytes of its
// entropy segment.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "va_jpeg_math.h"

static void out32(int32_t v) { fwrite(&v, 4, 1, stdout); }

int main()
{
    int32_t dims[4];
    uint8_t qt[2][64];
    if (fread(dims, 4, 4, stdin) != 4 || fread(qt, 1, 128, stdin) != 128)
        return 2;
    const int h = dims[0], w = dims[1], hs = dims[2], vs = dims[3];
    if (h < 1 || w < 1 || hs != 2 || (vs != 1 && vs != 2))
        return 2;
    std::vector<uint8_t> frame((size_t)h * w * 3);
    if (fread(frame.data(), 1, frame.size(), stdin) != frame.size())
        return 2;
    constexpr va_jpeg::HuffTables huff = va_jpeg::make_huff();
    const int hv = hs * vs, bpm = hv + 2;
    const int my = (h + 8 * vs - 1) / (8 * vs), mx = (w + 8 * hs - 1) / (8 * hs);
    const int ch = (h + vs - 1) / vs, cw = (w + hs - 1) / hs;          // the real samples of a chroma plane

    // Y per pixel; Cb and Cr averaged over the boxes, whose pixels beyond the frame repeat its edge
    std::vector<uint8_t> luma((size_t)h * w), chroma[2];
    chroma[0].resize((size_t)ch * cw), chroma[1].resize((size_t)ch * cw);
    for (int i = 0; i < ch; i++)
        for (int j = 0; j < cw; j++) {
            int sum[2] = {0, 0};
            for (int dy = 0; dy < vs; dy++)
                for (int dx = 0; dx < hs; dx++) {
                    const int yy = va_jpeg::edge_index(vs * i + dy, h), xx = va_jpeg::edge_index(hs * j + dx, w);
                    const uint8_t *p = &frame.at(((size_t)yy * w + xx) * 3);
                    int y, cb, cr;
                    va_jpeg::ycbcr(p[0], p[1], p[2], y, cb, cr);
                    luma.at((size_t)yy * w + xx) = (uint8_t)y;
                    sum[0] += cb, sum[1] += cr;
                }
            for (int k = 0; k < 2; k++)
                chroma[k].at((size_t)i * cw + j) = (uint8_t)va_jpeg::box_average(sum[k], hv);
        }

    for (int j = 0; j < my; j++) {
        // the segment's coefficients, block after block in coding order
        std::vector<std::vector<int16_t>> blocks;
        for (int m = 0; m < mx; m++)
            for (int k = 0; k < bpm; k++) {
                const int comp = va_jpeg::block_component(k, hv);
                int x[64];
                for (int i = 0; i < 64; i++) {
                    if (comp == 0) {
                        const int yy = va_jpeg::edge_index((j * vs + k / hs) * 8 + i / 8, h);
                        const int xx = va_jpeg::edge_index((m * hs + k % hs) * 8 + i % 8, w);
                        x[i] = luma.at((size_t)yy * w + xx) - 128;
                    } else {
                        const int yy = va_jpeg::edge_index(j * 8 + i / 8, ch), xx = va_jpeg::edge_index(m * 8 + i % 8, cw);
                        x[i] = chroma[comp - 1].at((size_t)yy * cw + xx) - 128;
                    }
                }
                std::vector<int16_t> zz(64);
                va_jpeg::forward_block(x, qt[comp ? 1 : 0], zz.data());
                blocks.push_back(zz);
            }
        // the strings, one lane after the other: first their lengths, then the bits into a buffer of exactly that size
        std::vector<va_jpeg::Bits> strings;
        size_t total = 0;
        for (size_t q = 0; q < blocks.size(); q++) {
            const int k = (int)(q % bpm), comp = va_jpeg::block_component(k, hv), tab = comp ? 1 : 0;
            const size_t back = (size_t)va_jpeg::predictor_back(k, hv, bpm);
            const int pred = q >= back ? blocks.at(q - back)[0] : 0;
            if (q >= back && va_jpeg::block_component((int)((q - back) % bpm), hv) != comp)
                return 5;
            uint64_t nonzero = 0;
            for (int i = 0; i < 64; i++)
                nonzero |= (uint64_t)(blocks[q][i] != 0) << i;
            for (int i = 0; i < 64; i++) {
                strings.push_back(va_jpeg::coefficient_bits(huff.dc[tab], huff.ac[tab], i, blocks[q][i], pred, nonzero));
                total += strings.back().len;
            }
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
