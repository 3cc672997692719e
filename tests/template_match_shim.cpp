// A stand-alone host program around video-analysis_amd/csrc/va_template_match_math.h for
// tests/test_template_match_host.py: template matching of DESIGN.md §9, "Template matching", computed serially with
// the header's status checks, score function and combine rule, compiled with the host C++ compiler under
// -fsanitize=address,undefined.  The sums are plain loops over the window in uint32 accumulators, as the kernel's are.
// The best of a query is folded as the kernels fold it: one candidate per tile of kTileX x kTileY positions, then the
// tiles -- here from the last to the first, so that the answer shows the rule, not the order.  Every buffer has exactly
// the size of what it holds, so an access outside a frame or a template is reported.
// Input (stdin, binary), any number of runs: int64 method, n, h, w, stride, m, q; m x 2 int64 shapes; m + 1 int64
// offsets; q x 6 int64 queries; (n - 1) * stride + h * w bytes of frames (none for n = 0); offsets[m] bytes of templates.
// Output (stdout, binary) per run: q records (double score, int32 x, y, status, reserved), all zero but the status for
// a flagged query; then the (ny, nx) float64 maps of the queries with status 0, in order.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/videoanalysis_hip.h"
#include "va_template_match_math.h"

typedef va_match_best Best;
static_assert(sizeof(Best) == 24 && sizeof(va_match_query) == 24, "the records of the ABI");
// the header's constants are the ones the ABI states
static_assert(va_match::kTileX == VA_MATCH_TILE && va_match::kTileY == VA_MATCH_TILE, "VA_MATCH_TILE");
static_assert(va_match::kChunkRows == VA_MATCH_CHUNK_ROWS && va_match::kChunkCols == VA_MATCH_CHUNK_COLS, "VA_MATCH_CHUNK_*");
static_assert(va_match::kMaxTemplatePixels == VA_MATCH_MAX_TEMPLATE_PIXELS, "VA_MATCH_MAX_TEMPLATE_PIXELS");
static_assert(va_match::kSqdiff == VA_MATCH_SQDIFF && va_match::kSqdiffNormed == VA_MATCH_SQDIFF_NORMED &&
              va_match::kCcorr == VA_MATCH_CCORR && va_match::kCcorrNormed == VA_MATCH_CCORR_NORMED &&
              va_match::kCcoeff == VA_MATCH_CCOEFF && va_match::kCcoeffNormed == VA_MATCH_CCOEFF_NORMED, "VA_MATCH_*");
static_assert(va_match::kBadFrame == VA_MATCH_STATUS_FRAME && va_match::kBadTemplate == VA_MATCH_STATUS_TEMPLATE &&
              va_match::kEmptyWindow == VA_MATCH_STATUS_EMPTY && va_match::kOutside == VA_MATCH_STATUS_OUTSIDE &&
              va_match::kBadTemplateShape == VA_MATCH_STATUS_TEMPLATE_SHAPE &&
              va_match::kShortWorkspace == VA_MATCH_STATUS_WORKSPACE, "VA_MATCH_STATUS_*");

static bool read_all(void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, stdin) == bytes; }

int main()
{
    int64_t head[7];
    while (fread(head, 1, sizeof head, stdin) == sizeof head) {
        const int method = (int)head[0];
        const int64_t n = head[1], h = head[2], w = head[3], stride = head[4], m = head[5], nq = head[6];
        if (method < 0 || method >= va_match::kMethods || n < 0 || h < 1 || w < 1 || stride < h * w || m < 0 || nq < 0)
            return 2;
        std::vector<int64_t> shapes((size_t)m * 2), offsets((size_t)m + 1), queries((size_t)nq * 6);
        if (!read_all(shapes.data(), shapes.size() * 8) || !read_all(offsets.data(), offsets.size() * 8) ||
            !read_all(queries.data(), queries.size() * 8))
            return 2;
        std::vector<uint8_t> frames(n ? (size_t)((n - 1) * stride + h * w) : 0), templates((size_t)offsets[(size_t)m]);
        if (!read_all(frames.data(), frames.size()) || !read_all(templates.data(), templates.size()))
            return 2;
        std::vector<Best> bests((size_t)nq);
        std::vector<double> maps;
        for (int64_t k = 0; k < nq; k++) {
            const int64_t *q = &queries[(size_t)k * 6];
            const int32_t frame = (int32_t)q[0], templ = (int32_t)q[1], x0 = (int32_t)q[2], y0 = (int32_t)q[3];
            const int32_t nx = (int32_t)q[4], ny = (int32_t)q[5];
            int64_t th = 0, tw = 0, begin = 0;
            bool ok = false;
            if (templ >= 0 && templ < m) {
                th = shapes[(size_t)templ * 2];
                tw = shapes[(size_t)templ * 2 + 1];
                begin = offsets[(size_t)templ];
                ok = va_match::template_ok(th, tw, begin, offsets[(size_t)templ + 1]);
            }
            Best &out = bests[(size_t)k];
            memset(&out, 0, sizeof out);
            out.status = va_match::query_status(frame, templ, x0, y0, nx, ny, n, h, w, m, th, tw, ok);
            if (out.status)
                continue;
            const uint8_t *img = frames.data() + (size_t)frame * (size_t)stride, *tp = templates.data() + begin;
            uint32_t s_t = 0, s_tt = 0;
            for (int64_t i = 0; i < th * tw; i++) {
                s_t += tp[i];
                s_tt += (uint32_t)tp[i] * tp[i];
            }
            const size_t first = maps.size();
            maps.resize(first + (size_t)nx * (size_t)ny);
            const int tiles_x = (nx + va_match::kTileX - 1) / va_match::kTileX;
            const int64_t tiles = va_match::tiles_of(nx, ny);
            std::vector<va_match::Candidate> cands((size_t)tiles, va_match::Candidate{0.0, 0, 0, true});
            for (int j = 0; j < ny; j++) {
                for (int i = 0; i < nx; i++) {
                    uint32_t s_it = 0, s_i = 0, s_ii = 0;
                    for (int64_t r = 0; r < th; r++) {
                        const uint8_t *row = img + (size_t)(y0 + j + r) * (size_t)w + (size_t)(x0 + i);
                        for (int64_t c = 0; c < tw; c++) {
                            const uint32_t v = row[c];
                            s_it += v * tp[r * tw + c];
                            s_i += v;
                            s_ii += v * v;
                        }
                    }
                    const va_match::Candidate c = {va_match::score(method, th * tw, s_it, s_i, s_ii, s_t, s_tt), i, j, false};
                    maps[first + (size_t)j * (size_t)nx + (size_t)i] = c.score;
                    va_match::Candidate &slot = cands[(size_t)(j / va_match::kTileY) * (size_t)tiles_x + (size_t)(i / va_match::kTileX)];
                    if (va_match::better(method, c, slot))
                        slot = c;
                }
            }
            va_match::Candidate best = {0.0, 0, 0, true};
            for (int64_t t = tiles - 1; t >= 0; t--)
                if (va_match::better(method, cands[(size_t)t], best))
                    best = cands[(size_t)t];
            if (best.none)
                return 3;
            out.score = best.score;
            out.x = x0 + best.i;
            out.y = y0 + best.j;
        }
        fwrite(bests.data(), sizeof(Best), bests.size(), stdout);
        fwrite(maps.data(), sizeof(double), maps.size(), stdout);
    }
    return 0;
}
