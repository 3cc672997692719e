// A stand-alone serial run of the split decoder of DESIGN.md §9, "Split Motion-JPEG decoding", made of
// va_jpeg_decode_math.h alone, for the host compiler and its sanitizers (tests/test_mjpeg_split_host.py builds and
// runs it; nothing of it is loaded into Python).  It reads records from standard input until the end:
//   int32 h, w, c, sub, scan_begin, bytes, luma_h, luma_v, max_rounds | c * 64 bytes of quantisation tables |
//   2 * c HuffDecode tables | the file
// and does, lane by lane, what the device's launches do: the rounds of the scan with double-buffered exits, the
// check with its exclusive scans, the write pass into zeroed coefficients, the seal, and for a frame that did not
// converge the serial decode of the whole segment.  One line per record: the status word, the 64-bit FNV-1a hash of
// the pixels, and the rounds (-1: fell back).  The file lies in a heap buffer of exactly its size.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "va_jpeg_decode_math.h"

namespace {

bool read_exact(void *dst, size_t n) { return fread(dst, 1, n, stdin) == n; }

// the one segment [b, e) and the marker-sequence bit (the serial form of the locate kernel with nseg = 1)
int32_t locate(const uint8_t *p, int64_t len, int64_t scan_begin, int64_t &b, int64_t &e)
{
    b = scan_begin < 0 ? 0 : scan_begin > len ? len : scan_begin;
    e = len;
    int64_t k = 0;
    int terminator = -1;
    bool stopped = false;
    for (int64_t i = b; i + 1 < len; i++) {
        if (p[i] != 0xFF || p[i + 1] == 0 || p[i + 1] == 0xFF)
            continue;
        if (k == 0)
            e = i;
        if (p[i + 1] != 0xD0 + (k & 7)) {
            terminator = p[i + 1];
            stopped = true;
            k++;
            break;
        }
        k++;
        i++;
    }
    if (!stopped)
        k++;
    return stopped && terminator == 0xD9 && k == 1 ? 0 : va_jpeg::kStatusMarker;
}

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
    using namespace va_jpeg;
    static_assert(sizeof(HuffDecode) == 1416, "the table layout the host builds");
    static_assert(sizeof(ScanState) == 16, "a state is one 16-byte word");
    int32_t head[9];
    while (read_exact(head, sizeof(head))) {
        const int h = head[0], w = head[1], c = head[2], sub = head[3], lh = head[6], lv = head[7], max_rounds = head[8];
        const int64_t scan_begin = head[4], len = head[5];
        const bool plain = lh == 1 && lv == 1, sampled = c == 3 && lh == 2 && (lv == 1 || lv == 2);
        if (h < 1 || w < 1 || (c != 1 && c != 3) || sub < 16 || sub % 16 || len < 0 || max_rounds < 0 || !(plain || sampled))
            return 2;
        std::vector<uint8_t> qt((size_t)c * 64);
        std::vector<HuffDecode> huff((size_t)2 * c);
        if (!read_exact(qt.data(), qt.size()) || !read_exact(huff.data(), huff.size() * sizeof(HuffDecode)))
            return 3;
        uint8_t *file = new uint8_t[(size_t)len];        // exactly the file: a read behind it is an error
        if (!read_exact(file, (size_t)len))
            return 4;
        const int my = (h + 8 * lv - 1) / (8 * lv), mx = (w + 8 * lh - 1) / (8 * lh);
        const int64_t mcus = (int64_t)my * mx;
        const int blocks = c == 1 ? 1 : mcu_blocks(lh, lv), luma = lh * lv;
        const int64_t total = mcus * blocks;
        int64_t b = 0, e = 0;
        int32_t status = locate(file, len, scan_begin, b, e);
        const int64_t lanes = subsequences(e - b, sub);
        const auto stop_of = [&](int64_t i) { return i + 1 == lanes ? e : b + (i + 1) * sub; };

        // the scan: exits[round & 1] is written in `round`, from exits[(round - 1) & 1]
        std::vector<ScanState> entry((size_t)lanes), exits[2];
        exits[0].resize((size_t)lanes), exits[1].resize((size_t)lanes);
        std::vector<ScanLane> lane((size_t)lanes);
        std::vector<int> last((size_t)lanes, 0);
        for (int round = 1; round <= max_rounds; round++) {
            std::vector<ScanState> &now = exits[round & 1], &before = exits[(round - 1) & 1];
            for (int64_t i = 0; i < lanes; i++) {
                const ScanState in = i == 0 ? scan_state(b, 0, 0, 0) : round == 1 ? scan_guess(file, b, b + i * sub)
                                                                                 : before[(size_t)(i - 1)];
                if (round > 1 && same_state(in, entry[(size_t)i])) {
                    now[(size_t)i] = before[(size_t)i];
                    continue;
                }
                entry[(size_t)i] = in;
                lane[(size_t)i] = scan_lane(file, e, in, stop_of(i), huff.data(), blocks, luma);
                now[(size_t)i] = lane[(size_t)i].exit;
                last[(size_t)i] = round;
            }
        }
        // the check
        bool converged = max_rounds > 0;
        int rounds = 0;
        for (int64_t i = 0; i < lanes && max_rounds > 0; i++) {
            converged = converged && (i == 0 || same_state(entry[(size_t)i], exits[max_rounds & 1][(size_t)(i - 1)]));
            rounds = last[(size_t)i] > rounds ? last[(size_t)i] : rounds;
        }
        std::vector<int16_t> coef((size_t)total * 64, 0);
        if (converged) {
            uint64_t err = kNoError;
            int64_t begun = 0;
            uint32_t sums[3] = {0, 0, 0};
            for (int64_t i = 0; i < lanes; i++) {
                int64_t block = begun;
                uint32_t pred[3] = {sums[0], sums[1], sums[2]};
                const int32_t st = write_lane(file, e, entry[(size_t)i], stop_of(i), i + 1 == lanes, huff.data(), blocks, luma,
                                              total, block, pred, [&](int64_t cur, int idx, int v) {
                                                  if (cur < 0 || cur >= total || idx < 0 || idx > 63)
                                                      abort();
                                                  const int64_t m = cur / blocks;
                                                  int comp = 0;
                                                  coef[(size_t)(mcu_block_at((int)(cur % blocks), lh, lv, my, mx, m / mx,
                                                                             m % mx, comp) * 64 + idx)] = (int16_t)v;
                                              });
                if (st && error_word(block, st) < err)
                    err = error_word(block, st);
                begun += lane[(size_t)i].begun;
                for (int ch = 0; ch < 3; ch++)
                    sums[ch] += lane[(size_t)i].dc[ch];
            }
            if (err != kNoError) {                       // the seal
                status |= (int32_t)(err & 15u);
                for (int64_t cur = (int64_t)(err >> 4); cur < total; cur++) {
                    const int64_t m = cur / blocks;
                    int comp = 0;
                    memset(coef.data() + mcu_block_at((int)(cur % blocks), lh, lv, my, mx, m / mx, m % mx, comp) * 64, 0,
                           64 * sizeof(int16_t));
                }
            }
        } else {                                         // the fallback: the serial decoder
            BitReader r = open_bits(file, b, e);
            int pred[3] = {0, 0, 0};
            bool dead = false;
            for (int64_t m = 0; m < mcus && !dead; m++)
                for (int k = 0; k < blocks && !dead; k++) {
                    int comp = 0;
                    int16_t *blk = coef.data() + mcu_block_at(k, lh, lv, my, mx, m / mx, m % mx, comp) * 64;
                    const int32_t st = decode_block(r, huff[2 * comp], huff[2 * comp + 1], pred[comp],
                                                    [&](int i, int v) { blk[i] = (int16_t)v; });
                    if (st) {
                        status |= st;
                        dead = true;
                        memset(blk, 0, 64 * sizeof(int16_t));
                    }
                }
        }
        delete[] file;
        const int64_t ys = (int64_t)mx * lh * 8, cs = (int64_t)mx * 8;
        std::vector<uint8_t> plane[3];
        plane_of(coef.data(), mcus * lh * lv, (int64_t)mx * lh, qt.data(), plane[0]);
        for (int comp = 1; comp < c; comp++)
            plane_of(coef.data() + (lh * lv + comp - 1) * mcus * 64, mcus, mx, qt.data() + 64 * comp, plane[comp]);
        const int cw = (w + lh - 1) / lh, ch = (h + lv - 1) / lv;
        uint64_t hash = 1469598103934665603ull;
        for (int gy = 0; gy < h; gy++)
            for (int gx = 0; gx < w; gx++) {
                uint8_t px[3] = {plane[0][(size_t)(gy * ys + gx)], 0, 0};
                if (c == 3) {
                    int chroma[2];
                    for (int comp = 0; comp < 2; comp++)
                        chroma[comp] = plain ? plane[1 + comp][(size_t)(gy * cs + gx)] : upsampled_at(
                            [&](int row, int col) {
                                if (row < 0 || row >= ch || col < 0 || col >= cw)
                                    abort();
                                return (int)plane[1 + comp][(size_t)(row * cs + col)];
                            },
                            gy, gx, lv, ch, cw);
                    int rr, gg, bb;
                    rgb_of(px[0], chroma[0], chroma[1], rr, gg, bb);
                    px[0] = (uint8_t)rr, px[1] = (uint8_t)gg, px[2] = (uint8_t)bb;
                }
                for (int i = 0; i < c; i++)
                    hash = (hash ^ px[i]) * 1099511628211ull;
            }
        printf("%d %llu %d\n", (int)status, (unsigned long long)hash, converged ? rounds : -1);
    }
    return 0;
}
