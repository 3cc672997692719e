// va_template_match_math.h -- the scores, the rule that combines two candidate bests, the status checks and the tile
// constants of template matching ("Template matching") that the kernels of va_template_match.hip and
// the host test tests/template_match_shim.cpp share.
//
// Per position of a template of N = th * tw <= 65536 pixels the exact integers S_it = sum I T, S_i = sum I and
// S_ii = sum I I, per template S_t = sum T and S_tt = sum T T: each is at most 255 * 255 * 65536 < 2^32.  A score is
// float64, from these integers in one fixed order: the int64 numerators are exact, every conversion is of an integer
// below 2^53, and multiply, sqrt and divide round once each.  There is no float addition, so nothing can contract.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VA_MATCH_HD __host__ __device__ __forceinline__
#else
#define VA_MATCH_HD inline
#endif

namespace va_match {

constexpr int kSqdiff = 0, kSqdiffNormed = 1, kCcorr = 2, kCcorrNormed = 3, kCcoeff = 4, kCcoeffNormed = 5;
constexpr int kMethods = 6;
constexpr int kMaxTemplatePixels = 65536;       // 255 * 255 * 65536 = 4 261 478 400 < 2^32
// status bits of a query (VA_MATCH_STATUS_*)
constexpr int kBadFrame = 1, kBadTemplate = 2, kEmptyWindow = 4, kOutside = 8, kBadTemplateShape = 16, kShortWorkspace = 32;
// a workgroup's tile of positions, and the block of template rows and columns it has in LDS at a time
constexpr int kTileX = 32, kTileY = 32;
constexpr int kChunkRows = 16, kChunkCols = 64;

VA_MATCH_HD bool minimises(int method) { return method == kSqdiff || method == kSqdiffNormed; }

// the score of one position.  n: the template's pixels
VA_MATCH_HD double score(int method, int64_t n, int64_t s_it, int64_t s_i, int64_t s_ii, int64_t s_t, int64_t s_tt)
{
    switch (method) {
    case kSqdiff:
        return (double)(s_ii - 2 * s_it + s_tt);
    case kCcorr:
        return (double)s_it;
    case kCcoeff:
        return (double)(n * s_it - s_i * s_t) / (double)n;
    case kSqdiffNormed: {
        const double den = sqrt((double)s_ii * (double)s_tt);
        return den == 0.0 ? 1.0 : (double)(s_ii - 2 * s_it + s_tt) / den;
    }
    case kCcorrNormed: {
        const double den = sqrt((double)s_ii * (double)s_tt);
        return den == 0.0 ? 0.0 : (double)s_it / den;
    }
    default: {
        const int64_t a = n * s_ii - s_i * s_i, b = n * s_tt - s_t * s_t;
        const double den = sqrt((double)a * (double)b);
        return den == 0.0 ? 0.0 : (double)(n * s_it - s_i * s_t) / den;
    }
    }
}

// a candidate best: a score at the window position (i, j); none: no position yet
struct Candidate {
    double score;
    int32_t i, j;
    bool none;
};

// whether b replaces a as the best: the smaller score for the sqdiff methods, the larger one otherwise, and at equal
// scores the earlier position in raster order (j, then i).  The rule is a total order on candidates at different
// positions, so folding with it gives one answer whatever the grouping.
VA_MATCH_HD bool better(int method, const Candidate &b, const Candidate &a)
{
    if (b.none)
        return false;
    if (a.none)
        return true;
    if (b.score != a.score)
        return minimises(method) ? b.score < a.score : b.score > a.score;
    return b.j != a.j ? b.j < a.j : b.i < a.i;
}

// whether a template's shape and its place in the packed bytes are usable
VA_MATCH_HD bool template_ok(int64_t th, int64_t tw, int64_t begin, int64_t end)
{
    return th >= 1 && tw >= 1 && th * tw <= kMaxTemplatePixels && begin >= 0 && begin + th * tw <= end;
}

// the status of a query: 0, or the bits of what is wrong with it.  th, tw, tmpl_ok: of the query's template, read
// only when its index is in range (pass anything otherwise)
VA_MATCH_HD int query_status(int32_t frame, int32_t templ, int32_t x0, int32_t y0, int32_t nx, int32_t ny, int64_t n,
                             int64_t h, int64_t w, int64_t m, int64_t th, int64_t tw, bool tmpl_ok)
{
    int status = 0;
    if (frame < 0 || frame >= n)
        status |= kBadFrame;
    if (nx < 1 || ny < 1)
        status |= kEmptyWindow;
    if (templ < 0 || templ >= m)
        return status | kBadTemplate;
    if (!tmpl_ok)
        return status | kBadTemplateShape;
    if (!(status & kEmptyWindow) &&
        (x0 < 0 || y0 < 0 || (int64_t)x0 + nx - 1 + tw > w || (int64_t)y0 + ny - 1 + th > h))
        status |= kOutside;
    return status;
}

VA_MATCH_HD int64_t tiles_of(int32_t nx, int32_t ny)
{
    return (((int64_t)nx + kTileX - 1) / kTileX) * (((int64_t)ny + kTileY - 1) / kTileY);
}

// An upper bound of the tiles of queries with `positions` positions in all: a window of a x b = P positions has
// ceil(a / X) ceil(b / Y) <= 1 + (a - 1) / X + (b - 1) / Y + (a - 1)(b - 1) / (X Y) tiles, and (a - 1) + (b - 1) <= P - 1.
VA_MATCH_HD int64_t tiles_bound(int64_t queries, int64_t positions)
{
    constexpr int kSmaller = kTileX < kTileY ? kTileX : kTileY;
    return queries + positions / kSmaller + positions / (kTileX * kTileY) + 1;
}

}  // namespace va_match
