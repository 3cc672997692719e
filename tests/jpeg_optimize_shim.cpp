// A stand-alone host program around video-analysis_amd/csrc/va_jpeg_math.h for tests/test_mjpeg_optimize_host.py: the
// optimised Huffman tables of DESIGN.md §9, "Optimised Huffman tables", compiled with the host C++ compiler under
// -fsanitize=address,undefined.  The table construction (huff_code_sizes with one lane, huff_bits_vals), the symbols
// of a coefficient (coefficient_symbols) and the encoder's entries of a run-time table (huff_encoder_table) are the
// header's, as is everything the serial encoder around them does; every buffer has exactly the size of what it holds.
// Input (stdin, binary): int32 mode.
//   mode 0: int32 t, then t * 256 int64 counts.  Output: t tables of 16 + 256 bytes (BITS, HUFFVAL).
//   mode 1: int32 n, h, w, c, H, V; 128 bytes of quantisation tables (luma, chroma; natural order); n * h * w * c bytes
//           of frames.  Output: 4 * 256 int64 counts, 4 tables of 16 + 256 bytes (DC0, AC0, DC1, AC1), then per frame
//           and MCU row an int32 byte count and the stuffed bytes of its entropy segment under those tables, then an
//           int32: the most bits one coefficient added (with codes of up to 16 bits: at most 3 * 16 + 16 + 10 = 74,
//           which coefficient_bits_wide gives as two strings).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "va_jpeg_math.h"

static void out32(int32_t v) { fwrite(&v, 4, 1, stdout); }

static void table_of(const int64_t *freq, uint8_t *table)
{
    std::vector<int> codesize(va_jpeg::kHuffSymbols), count(va_jpeg::kHuffSymbols), start(va_jpeg::kHuffSymbols);
    va_jpeg::huff_code_sizes<1>(0, freq, [](va_jpeg::HuffPick p) { return p; }, codesize.data());
    va_jpeg::huff_bits_vals(codesize.data(), table, table + 16, count.data(), start.data());
}

int main()
{
    int32_t mode;
    if (fread(&mode, 4, 1, stdin) != 1)
        return 2;
    if (mode == 0) {
        int32_t t;
        if (fread(&t, 4, 1, stdin) != 1 || t < 0)
            return 2;
        for (int k = 0; k < t; k++) {
            std::vector<int64_t> freq(256);
            std::vector<uint8_t> table(16 + 256);
            if (fread(freq.data(), 8, 256, stdin) != 256)
                return 2;
            table_of(freq.data(), table.data());
            fwrite(table.data(), 1, table.size(), stdout);
        }
        return 0;
    }
    int32_t dims[6];
    uint8_t qt[2][64];
    if (fread(dims, 4, 6, stdin) != 6 || fread(qt, 1, 128, stdin) != 128)
        return 2;
    const int n = dims[0], h = dims[1], w = dims[2], c = dims[3], hs = dims[4], vs = dims[5];
    if (n < 1 || h < 1 || w < 1 || (c != 1 && c != 3) || hs < 1 || hs > 2 || vs < 1 || vs > hs || (c == 1 && hs * vs != 1))
        return 2;
    std::vector<uint8_t> frames((size_t)n * h * w * c);
    if (fread(frames.data(), 1, frames.size(), stdin) != frames.size())
        return 2;
    const int hv = hs * vs, bpm = c == 1 ? 1 : hv + 2;
    const int my = (h + 8 * vs - 1) / (8 * vs), mx = (w + 8 * hs - 1) / (8 * hs);
    const int ch = (h + vs - 1) / vs, cw = (w + hs - 1) / hs;          // the real samples of a chroma plane

    // the coefficients of every segment, block after block in coding order
    std::vector<std::vector<std::vector<int16_t>>> segments;
    for (int f = 0; f < n; f++) {
        const uint8_t *frame = &frames.at((size_t)f * h * w * c);
        std::vector<uint8_t> luma((size_t)h * w), chroma[2];
        if (c == 1) {
            luma.assign(frame, frame + (size_t)h * w);
        } else {
            chroma[0].resize((size_t)ch * cw), chroma[1].resize((size_t)ch * cw);
            for (int i = 0; i < ch; i++)
                for (int j = 0; j < cw; j++) {
                    int sum[2] = {0, 0};
                    for (int dy = 0; dy < vs; dy++)
                        for (int dx = 0; dx < hs; dx++) {
                            const int yy = va_jpeg::edge_index(vs * i + dy, h), xx = va_jpeg::edge_index(hs * j + dx, w);
                            const uint8_t *p = frame + ((size_t)yy * w + xx) * 3;
                            int y, cb, cr;
                            va_jpeg::ycbcr(p[0], p[1], p[2], y, cb, cr);
                            luma.at((size_t)yy * w + xx) = (uint8_t)y;
                            sum[0] += cb, sum[1] += cr;
                        }
                    for (int k = 0; k < 2; k++)
                        chroma[k].at((size_t)i * cw + j) = (uint8_t)va_jpeg::box_average(sum[k], hv);
                }
        }
        for (int j = 0; j < my; j++) {
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
            segments.push_back(blocks);
        }
    }

    // one walk of a segment's coefficients: visit(table class, coefficient index, value, predictor, non-zero mask)
    auto walk = [&](const std::vector<std::vector<int16_t>> &blocks, auto visit) {
        for (size_t q = 0; q < blocks.size(); q++) {
            const int k = (int)(q % bpm), comp = va_jpeg::block_component(k, hv);
            const size_t back = (size_t)va_jpeg::predictor_back(k, hv, bpm);
            const int pred = q >= back ? blocks.at(q - back)[0] : 0;
            uint64_t nonzero = 0;
            for (int i = 0; i < 64; i++)
                nonzero |= (uint64_t)(blocks[q][i] != 0) << i;
            for (int i = 0; i < 64; i++)
                visit(comp ? 1 : 0, i, blocks[q][i], pred, nonzero);
        }
    };

    std::vector<int64_t> freq(4 * 256, 0);
    for (const auto &blocks : segments)
        walk(blocks, [&](int tab, int i, int v, int pred, uint64_t nonzero) {
            va_jpeg::coefficient_symbols(i, v, pred, nonzero, [&](int ac, int symbol, int times) {
                freq.at((size_t)(2 * tab + ac) * 256 + symbol) += times;
            });
        });
    fwrite(freq.data(), 8, freq.size(), stdout);
    std::vector<uint8_t> tables(4 * (16 + 256), 0);
    std::vector<uint32_t> codes(4 * 256, 0);
    for (int t = 0; t < (c == 1 ? 2 : 4); t++) {
        table_of(&freq.at((size_t)t * 256), &tables.at((size_t)t * 272));
        va_jpeg::huff_encoder_table(&tables.at((size_t)t * 272), &tables.at((size_t)t * 272 + 16), &codes.at((size_t)t * 256));
    }
    fwrite(tables.data(), 1, tables.size(), stdout);

    int longest = 0;                 // the bits one coefficient adds, at most 74
    for (const auto &blocks : segments) {
        std::vector<va_jpeg::Bits> strings;
        size_t total = 0;
        walk(blocks, [&](int tab, int i, int v, int pred, uint64_t nonzero) {
            const va_jpeg::WideBits wide = va_jpeg::coefficient_bits_wide(
                &codes.at((size_t)(2 * tab) * 256), &codes.at((size_t)(2 * tab + 1) * 256), i, v, pred, nonzero);
            if (wide.zrl.len > 48 || wide.rest.len > 27)
                exit(3);
            longest = wide.zrl.len + wide.rest.len > longest ? wide.zrl.len + wide.rest.len : longest;
            strings.push_back(wide.zrl);
            strings.push_back(wide.rest);
            total += wide.zrl.len + wide.rest.len;
        });
        const int pad = (int)(-total & 7);
        strings.push_back(va_jpeg::Bits{(1ull << pad) - 1, pad});
        std::vector<uint32_t> words((total + pad + 31) / 32, 0u);
        uint32_t pos = 0;
        for (const va_jpeg::Bits &b : strings) {
            if (b.len < 0 || b.len > 48)
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
    out32(longest);
    return 0;
}
