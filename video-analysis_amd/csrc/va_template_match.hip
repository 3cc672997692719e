// va_template_match.hip -- batched template matching on uint8 frames ("Template matching"): for every
// query (frame, template, x0, y0, nx, ny) the scores of the nx * ny window positions by one of cv2.matchTemplate's six
// methods, and the best of them as cv2.minMaxLoc picks it.  The scores, the rule that combines two bests and the status
// checks are va_template_match_math.h, the same text the host test compiles.
//
// Four launches a call, all on the caller's stream, none of which depends on the order in which workgroups run:
//   plan      one workgroup: the status of every query and the exclusive scan of the tiles of the valid ones, so
//             that tile t of the call belongs to the query q with tile_off[q] <= t < tile_off[q + 1]
//   templates one wave per template: S_t and S_tt
//   tiles     a fixed grid of workgroups walks the tiles.  A workgroup of four waves owns a tile of 32 x 32 positions,
//             a lane four positions side by side.  The template goes through LDS in blocks of up to 16 rows x 64
//             columns, zero-padded to whole dwords, next to the frame patch the block needs (tile + block extent - 1),
//             staged as bytes with two aligned dword loads and one v_alignbyte per patch dword where both dwords lie
//             inside the frame, byte loads otherwise.  Per template dword a lane reads one new patch dword, builds the
//             three other byte phases with v_alignbyte from the dword it already holds, and issues udot4 against the
//             template (S_it), against ones (S_i) and against itself (S_ii), the last two masked to the template's
//             columns.  Accumulators are uint32: exact, so the blocks may come in any order and size.  Scores are
//             computed once, in float64; a tile writes its scores where maps are asked for, and always its one
//             candidate best (wave reduction, then LDS) into the workspace.
//   bests     one wave per query folds the query's candidates; a flagged query writes its status and nothing else.
// The patch rows are 24 dwords apart, so the 4 rows x 8 dwords a half wave reads together fall on 32 different banks.
#include "va_common.h"
#include "va_scan.h"
#include "va_template_match_math.h"

namespace va {

namespace {

using va_match::Candidate;
using va_match::kChunkCols;
using va_match::kChunkRows;
using va_match::kTileX;
using va_match::kTileY;

constexpr int kMatchThreads = 256;                                   // four waves: 8 lanes x 32 rows of 4 positions
constexpr int kPatchStride = kTileX / 4 + kChunkCols / 4;            // 24 dwords: 8 (mod 16)
constexpr int kPatchRows = kTileY + kChunkRows - 1;
constexpr int kMatchGrid = 2048;                                     // workgroups that walk the tiles
constexpr int64_t kMaxTiles = ((int64_t)1 << 31) - 1;
static_assert(kTileX == 32 && kTileY * (kTileX / 4) == kMatchThreads, "a lane owns four positions of one row");
static_assert(kPatchStride % 16 == 8, "four rows of eight dwords on 32 banks");

struct MatchArgs {
    const uint8_t *frames;
    int64_t n, h, w, stride;
    const uint8_t *templates;
    const int32_t *shapes;
    const int64_t *toff;
    int64_t m;
    const int32_t *queries;             // six int32 a query
    int64_t nq;
    va_match_best *best;
    double *maps;
    const int64_t *map_off;
    uint32_t *tstats;                   // S_t, S_tt of every template
    int64_t *tile_off;                  // nq + 2: the scan, the total, and whether the total is beyond cand_cap
    va_match_best *cands;
    int64_t cand_cap;
    int method;
};

struct Query {
    int32_t frame, templ, x0, y0, nx, ny;
    int32_t th, tw;
    int64_t tbegin;
    int status;
};

__device__ __forceinline__ Query load_query(const MatchArgs &a, int64_t q)
{
    const int32_t *p = a.queries + 6 * q;
    Query r = {p[0], p[1], p[2], p[3], p[4], p[5], 0, 0, 0, 0};
    bool ok = false;
    if (r.templ >= 0 && r.templ < a.m) {
        r.th = a.shapes[2 * (int64_t)r.templ];
        r.tw = a.shapes[2 * (int64_t)r.templ + 1];
        r.tbegin = a.toff[r.templ];
        ok = va_match::template_ok(r.th, r.tw, r.tbegin, a.toff[r.templ + 1]);
    }
    r.status = va_match::query_status(r.frame, r.templ, r.x0, r.y0, r.nx, r.ny, a.n, a.h, a.w, a.m, r.th, r.tw, ok);
    return r;
}

__global__ void __launch_bounds__(1024)
match_plan_kernel(MatchArgs a)
{
    __shared__ int64_t part[16];
    int64_t carry = 0;
    for (int64_t base = 0; base < a.nq; base += 1024) {
        const int64_t q = base + threadIdx.x;
        int64_t tiles = 0;
        if (q < a.nq) {
            const Query r = load_query(a, q);
            if (r.status == 0)
                tiles = va_match::tiles_of(r.nx, r.ny);
        }
        int64_t total;
        const int64_t before = block_exclusive<16>(tiles, part, total);
        if (q < a.nq)
            a.tile_off[q] = carry + before;
        carry += total;
    }
    if (threadIdx.x == 0) {
        a.tile_off[a.nq] = carry;
        a.tile_off[a.nq + 1] = carry > a.cand_cap;
    }
}

__global__ void __launch_bounds__(kMatchThreads)
match_template_sums_kernel(MatchArgs a)
{
    const int lane = threadIdx.x % kWave;
    const int64_t t = (int64_t)blockIdx.x * (kMatchThreads / kWave) + threadIdx.x / kWave;
    if (t >= a.m)
        return;
    const int64_t th = a.shapes[2 * t], tw = a.shapes[2 * t + 1], begin = a.toff[t];
    uint32_t s = 0, ss = 0;
    if (va_match::template_ok(th, tw, begin, a.toff[t + 1])) {
        const uint8_t *tp = a.templates + begin;
        for (int k = lane; k < (int)(th * tw); k += kWave) {
            const uint32_t v = tp[k];
            s += v;
            ss += v * v;
        }
    }
    s = wave_sum(s);
    ss = wave_sum(ss);
    if (lane == 0) {
        a.tstats[2 * t] = s;
        a.tstats[2 * t + 1] = ss;
    }
}

// the four bytes at byte `p` of a frame of `bytes` bytes; a byte at or beyond `bytes` reads as 0
__device__ __forceinline__ uint32_t frame_dword(const uint8_t *frame, int64_t p, int64_t bytes)
{
    const uint8_t *g = frame + p;
    const uint32_t phase = (uint32_t)(reinterpret_cast<uintptr_t>(g) & 3u);
    const int64_t first = p - phase;
    if (first >= 0 && first + (phase ? 8 : 4) <= bytes) {
        const uint32_t *al = reinterpret_cast<const uint32_t *>(g - phase);
        const uint32_t lo = al[0], hi = phase ? al[1] : 0u;
        return __builtin_amdgcn_alignbyte(hi, lo, phase);
    }
    uint32_t v = 0;
#pragma unroll
    for (int b = 0; b < 4; b++)
        if (p + b < bytes)
            v |= (uint32_t)g[b] << (8 * b);
    return v;
}

__device__ __forceinline__ Candidate wave_best(int method, Candidate c)
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        Candidate o;
        o.score = __shfl_xor(c.score, d, kWave);
        o.i = __shfl_xor(c.i, d, kWave);
        o.j = __shfl_xor(c.j, d, kWave);
        o.none = __shfl_xor((int)c.none, d, kWave) != 0;
        if (va_match::better(method, o, c))
            c = o;
    }
    return c;
}

// one patch dword pair against one template dword: the four byte phases of the lane's four positions
__device__ __forceinline__ void accumulate(uint32_t d0, uint32_t d1, uint32_t t, uint32_t ones, uint32_t mask,
                                           uint32_t (&it)[4], uint32_t (&si)[4], uint32_t (&sii)[4])
{
    const uint32_t s[4] = {d0, __builtin_amdgcn_alignbyte(d1, d0, 1), __builtin_amdgcn_alignbyte(d1, d0, 2),
                           __builtin_amdgcn_alignbyte(d1, d0, 3)};
#pragma unroll
    for (int p = 0; p < 4; p++) {
        it[p] = __builtin_amdgcn_udot4(s[p], t, it[p], false);
        si[p] = __builtin_amdgcn_udot4(s[p], ones, si[p], false);
        sii[p] = __builtin_amdgcn_udot4(s[p] & mask, s[p], sii[p], false);
    }
}

__global__ void __launch_bounds__(kMatchThreads)
match_tiles_kernel(MatchArgs a)
{
    __shared__ uint32_t patch[kPatchRows * kPatchStride];
    __shared__ uint32_t tmpl[kChunkRows * (kChunkCols / 4)];
    __shared__ va_match_best wbest[kMatchThreads / kWave];
    const int64_t total = a.tile_off[a.nq];
    if (a.tile_off[a.nq + 1])
        return;
    const int tid = threadIdx.x, kx = tid & 7, ry = tid >> 3;
    for (int64_t tile = blockIdx.x; tile < total; tile += gridDim.x) {
        int64_t lo = 0, hi = a.nq;          // tile_off[lo] <= tile < tile_off[hi]
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (a.tile_off[mid] <= tile)
                lo = mid;
            else
                hi = mid;
        }
        const Query r = load_query(a, lo);
        const int tiles_x = (r.nx + kTileX - 1) / kTileX;
        const int local = (int)(tile - a.tile_off[lo]);
        const int ti = (local % tiles_x) * kTileX, tj = (local / tiles_x) * kTileY;      // the tile's first position
        const int vcols = min(kTileX, r.nx - ti), vrows = min(kTileY, r.ny - tj);
        const uint8_t *frame = a.frames + (int64_t)r.frame * a.stride;
        const uint8_t *tp = a.templates + r.tbegin;
        const int64_t frame_bytes = a.h * a.w;
        uint32_t it[4] = {0, 0, 0, 0}, si[4] = {0, 0, 0, 0}, sii[4] = {0, 0, 0, 0};
        for (int rb = 0; rb < r.th; rb += kChunkRows) {
            const int rows = min(kChunkRows, r.th - rb);
            for (int cb = 0; cb < r.tw; cb += kChunkCols) {
                const int cols = min(kChunkCols, r.tw - cb), ndw = (cols + 3) / 4;
                const int prow = vrows + rows - 1, pdw = (vcols + 3) / 4 + ndw;
                __syncthreads();                                // the reads of the block before
                for (int k = tid; k < prow * pdw; k += kMatchThreads) {
                    const int pr = k / pdw, pc = k % pdw;
                    const int64_t at = (int64_t)(r.y0 + tj + rb + pr) * a.w + (r.x0 + ti + cb + 4 * pc);
                    patch[pr * kPatchStride + pc] = frame_dword(frame, at, frame_bytes);
                }
                for (int k = tid; k < rows * ndw; k += kMatchThreads) {
                    const int tr = k / ndw, tc = k % ndw;
                    uint32_t v = 0;
#pragma unroll
                    for (int b = 0; b < 4; b++)
                        if (4 * tc + b < cols)
                            v |= (uint32_t)tp[(rb + tr) * r.tw + cb + 4 * tc + b] << (8 * b);
                    tmpl[tr * (kChunkCols / 4) + tc] = v;
                }
                __syncthreads();
                const int tail = cols - 4 * (ndw - 1);           // 1 .. 4 columns in the block's last dword
                const uint32_t tail_mask = tail == 4 ? 0xffffffffu : (1u << (8 * tail)) - 1u;
                for (int tr = 0; tr < rows; tr++) {
                    const uint32_t *row = patch + (ry + tr) * kPatchStride + kx;
                    const uint32_t *trow = tmpl + tr * (kChunkCols / 4);
                    uint32_t d0 = row[0];
                    for (int j = 0; j + 1 < ndw; j++) {
                        const uint32_t d1 = row[j + 1];
                        accumulate(d0, d1, trow[j], 0x01010101u, 0xffffffffu, it, si, sii);
                        d0 = d1;
                    }
                    accumulate(d0, row[ndw], trow[ndw - 1], 0x01010101u & tail_mask, tail_mask, it, si, sii);
                }
            }
        }
        const int64_t npix = (int64_t)r.th * r.tw;
        const int64_t s_t = a.tstats[2 * (int64_t)r.templ], s_tt = a.tstats[2 * (int64_t)r.templ + 1];
        const int j = tj + ry;
        Candidate best = {0.0, 0, 0, true};
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int i = ti + 4 * kx + p;
            if (i < r.nx && j < r.ny) {
                const Candidate c = {va_match::score(a.method, npix, it[p], si[p], sii[p], s_t, s_tt), i, j, false};
                if (a.maps)
                    a.maps[a.map_off[lo] + (int64_t)j * r.nx + i] = c.score;
                if (va_match::better(a.method, c, best))
                    best = c;
            }
        }
        best = wave_best(a.method, best);
        if (tid % kWave == 0)
            wbest[tid / kWave] = {best.score, best.i, best.j, best.none, 0};
        __syncthreads();
        if (tid == 0) {
            for (int k = 0; k < kMatchThreads / kWave; k++) {
                const Candidate c = {wbest[k].score, wbest[k].x, wbest[k].y, wbest[k].status != 0};
                if (va_match::better(a.method, c, best))
                    best = c;
            }
            a.cands[tile] = {best.score, r.x0 + best.i, r.y0 + best.j, 0, 0};
        }
    }
}

__global__ void __launch_bounds__(kMatchThreads)
match_bests_kernel(MatchArgs a)
{
    const int lane = threadIdx.x % kWave;
    const int64_t q = (int64_t)blockIdx.x * (kMatchThreads / kWave) + threadIdx.x / kWave;
    if (q >= a.nq)
        return;
    const Query r = load_query(a, q);
    const int status = r.status | (a.tile_off[a.nq + 1] ? va_match::kShortWorkspace : 0);
    if (status) {
        if (lane == 0)
            a.best[q].status = status;
        return;
    }
    Candidate best = {0.0, 0, 0, true};
    for (int64_t t = a.tile_off[q] + lane; t < a.tile_off[q + 1]; t += kWave) {
        const Candidate c = {a.cands[t].score, a.cands[t].x, a.cands[t].y, false};
        if (va_match::better(a.method, c, best))
            best = c;
    }
    best = wave_best(a.method, best);
    if (lane == 0)
        a.best[q] = {best.score, best.i, best.j, 0, 0};
}

struct MatchLayout {
    size_t tstats, tile_off, cands, total;
};

MatchLayout match_layout(int64_t nq, int64_t positions, int64_t m)
{
    Carve c;
    return {c.take((size_t)m * 2 * sizeof(uint32_t)), c.take((size_t)(nq + 2) * sizeof(int64_t)),
            c.take((size_t)va_match::tiles_bound(nq, positions) * sizeof(va_match_best)), c.total};
}

bool match_counts_ok(int64_t nq, int64_t positions, int64_t m)
{
    return nq >= 0 && positions >= 0 && m >= 0 && nq <= kMaxTiles && m <= kMaxTiles && positions <= ((int64_t)1 << 40) &&
           va_match::tiles_bound(nq, positions) <= kMaxTiles;
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

size_t va_template_match_workspace_bytes(int64_t n_queries, int64_t total_positions, int64_t n_templates)
{
    if (!match_counts_ok(n_queries, total_positions, n_templates))
        return 0;
    return match_layout(n_queries, total_positions, n_templates).total;
}

int va_template_match_u8(const va_match_args *args)
{
    const char *const fn = "va_template_match_u8";
    VA_REQUIRE(args, "%s: NULL argument", fn);
    VA_REQUIRE(args->struct_size == (int32_t)sizeof(va_match_args), "%s: struct_size %d, this library's va_match_args has %zu bytes",
               fn, args->struct_size, sizeof(va_match_args));
    VA_REQUIRE(args->method >= 0 && args->method < va_match::kMethods, "%s: unknown method %d (0 .. %d)", fn, args->method,
               va_match::kMethods - 1);
    const int64_t n = args->n, h = args->h, w = args->w, nq = args->n_queries, m = args->n_templates;
    VA_REQUIRE(h <= 0 || w <= 0 || (size_t)h * (size_t)w < kMaxFramePixels, "%s: frames above 2^29 pixels are not supported", fn);
    VA_REQUIRE(n >= 0 && h > 0 && w > 0, "%s: bad shape (%lld,%lld,%lld)", fn, (long long)n, (long long)h, (long long)w);
    VA_REQUIRE(args->frame_stride >= h * w, "%s: frame stride %lld below the frame size %lld", fn,
               (long long)args->frame_stride, (long long)(h * w));
    VA_REQUIRE(match_counts_ok(nq, args->total_positions, m),
               "%s: %lld queries of %lld positions and %lld templates: counts are 0 .. 2^31 - 1, and so is the bound of the "
               "tiles", fn, (long long)nq, (long long)args->total_positions, (long long)m);
    if (nq == 0)
        return VA_OK;
    VA_REQUIRE(args->queries_dev && (args->frames_dev || n == 0) && args->workspace_dev &&
               (m == 0 || (args->templates_dev && args->template_shapes_dev && args->template_offsets_dev)) &&
               (!args->maps_out_dev || args->map_offsets_dev), "%s: NULL argument", fn);
    VA_REQUIRE(aligned(args->queries_dev, 4) && aligned(args->template_shapes_dev, 4) &&
               aligned(args->template_offsets_dev, 8) && aligned(args->best_out_dev, 8) && aligned(args->maps_out_dev, 8) &&
               aligned(args->map_offsets_dev, 8) && aligned(args->workspace_dev, 8),
               "%s: queries and template shapes must be 4-byte aligned, offsets, bests, maps and the workspace 8-byte aligned", fn);
    const MatchLayout lay = match_layout(nq, args->total_positions, m);
    VA_REQUIRE(args->workspace_bytes >= lay.total, "%s: workspace of %zu bytes < required %zu", fn, args->workspace_bytes,
               lay.total);
    VA_ENTER();
    hipStream_t st = as_stream(args->stream);
    void *ws = args->workspace_dev;
    const int64_t cap = va_match::tiles_bound(nq, args->total_positions);
    const MatchArgs a = {args->frames_dev, n, h, w, args->frame_stride, args->templates_dev, args->template_shapes_dev,
                         args->template_offsets_dev, m, reinterpret_cast<const int32_t *>(args->queries_dev), nq,
                         args->best_out_dev, args->maps_out_dev, args->map_offsets_dev, at<uint32_t>(ws, lay.tstats),
                         at<int64_t>(ws, lay.tile_off), at<va_match_best>(ws, lay.cands), cap, args->method};
    hipLaunchKernelGGL(match_plan_kernel, dim3(1), dim3(1024), 0, st, a);
    VA_LAUNCH_CHECK("match_plan_kernel");
    if (m > 0) {
        hipLaunchKernelGGL(match_template_sums_kernel, dim3((unsigned)cdiv(m, kMatchThreads / kWave)), dim3(kMatchThreads), 0,
                           st, a);
        VA_LAUNCH_CHECK("match_template_sums_kernel");
    }
    hipLaunchKernelGGL(match_tiles_kernel, dim3((unsigned)(cap < kMatchGrid ? cap : kMatchGrid)), dim3(kMatchThreads), 0, st,
                       a);
    VA_LAUNCH_CHECK("match_tiles_kernel");
    if (args->best_out_dev) {
        hipLaunchKernelGGL(match_bests_kernel, dim3((unsigned)cdiv(nq, kMatchThreads / kWave)), dim3(kMatchThreads), 0, st, a);
        VA_LAUNCH_CHECK("match_bests_kernel");
    }
    return VA_OK;
}

}  // extern "C"
