// va_compose.hip -- the two passes behind video.io.composer.VideoComposer (video/io/composer.py); the definitions
// are pinned in DESIGN.md §9, "Composer".
//
// compose_layers : the pixel layers of every frame of a stack (highlight_mask :131-154, add_image :168-186,
//                  blend_image :190-210, and set_frame's copy of a monochrome frame into a colour video :103-105) in
//                  one pass.  A lane owns 16 consecutive pixels of a row, 16 bytes of a monochrome plane or 48 of an
//                  RGB one, and walks the frame's layers in order in registers: a frame is read once and written
//                  once however many layers it has, plus the layers' own images and masks.
// draw           : the thickness-1 LINE_8 primitives (cv2.polylines, drawContours, rectangle, circle), one workgroup
//                  per frame walking the frame's commands in order.  A run of commands of one colour is one phase,
//                  its commands dealt to the waves (to the whole workgroup when there are fewer than four) and the
//                  segments, or the steps of a circle's recurrence, to the lanes; between two phases the
//                  workgroup's stores are ordered by a fence and a barrier, so that the last command in list order
//                  that covers a pixel decides it.
// draw_contours  : a va_find_contours result as it lies in device memory, every contour a closed polyline in one
//                  colour (composer.py:228-237, findContours -> drawContours).  The batch's totals are known on the
//                  host, so the launch is chip-wide: one lane per slot checks the slot's table entries, one lane per
//                  point finds its slot by binary search in the offsets and draws the segment that starts at its
//                  point.  All stores carry one value, so no order between the lanes is needed: no LDS, no barrier.
#include "va_common.h"
#include "va_raster.h"

namespace va {

namespace {

constexpr int kComposeBlock = 256;
constexpr int kLanePixels = 16;
constexpr int kDrawBlock = 256;
constexpr int kDrawWaves = kDrawBlock / kWave;
constexpr int kContourBlock = 256;
constexpr int64_t kContourPieceLanes = (int64_t)1 << 30;     // lanes of one launch: 2^22 workgroups in grid x

typedef uint32_t u32x4 __attribute__((ext_vector_type(4), aligned(4)));

// NB bytes at p into NB / 4 words (little endian): 16-byte loads when p is 4-byte aligned and all NB bytes are
// there, else the first `valid` bytes one by one (the others read as 0)
template <int NB>
__device__ __forceinline__ void load_bytes(const uint8_t *p, int valid, uint32_t (&r)[NB / 4])
{
    if (valid == NB && ((uintptr_t)p & 3) == 0) {
#pragma unroll
        for (int i = 0; i < NB / 16; i++) {
            const u32x4 v = *reinterpret_cast<const u32x4 *>(p + 16 * i);
            r[4 * i] = v.x, r[4 * i + 1] = v.y, r[4 * i + 2] = v.z, r[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NB / 4; i++)
            r[i] = 0;
#pragma unroll
        for (int i = 0; i < NB; i++)
            if (i < valid)
                r[i / 4] |= (uint32_t)p[i] << (8 * (i % 4));
    }
}

template <int NB>
__device__ __forceinline__ void store_bytes(uint8_t *p, int valid, const uint32_t (&r)[NB / 4])
{
    if (valid == NB && ((uintptr_t)p & 3) == 0) {
#pragma unroll
        for (int i = 0; i < NB / 16; i++) {
            u32x4 v;
            v.x = r[4 * i], v.y = r[4 * i + 1], v.z = r[4 * i + 2], v.w = r[4 * i + 3];
            *reinterpret_cast<u32x4 *>(p + 16 * i) = v;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NB; i++)
            if (i < valid)
                p[i] = (uint8_t)(r[i / 4] >> (8 * (i % 4)));
    }
}

template <int NW>
__device__ __forceinline__ uint32_t get_byte(const uint32_t (&r)[NW], int i)        // i is a compile-time value
{
    return (r[i / 4] >> (8 * (i % 4))) & 255u;
}

template <int NW>
__device__ __forceinline__ void set_byte(uint32_t (&r)[NW], int i, uint32_t v)
{
    r[i / 4] = (r[i / 4] & ~(255u << (8 * (i % 4)))) | (v << (8 * (i % 4)));
}

struct ComposeArgs {
    const uint8_t *src;
    uint8_t *dst;
    int n, h, w, c_src;
    const va_compose_layer *layers;
    const int64_t *layer_off;
    int64_t nlayers;
    const uint8_t *images;
    int64_t images_bytes;
    const uint8_t *masks;
    int64_t masks_bytes;
    int chunks;                 // lanes of a row: ceil(w / 16)
    int64_t lanes;              // n * h * chunks
};

template <int C>
__global__ void __launch_bounds__(kComposeBlock) compose_layers_kernel(ComposeArgs a)
{
    const int64_t lane = (int64_t)blockIdx.x * kComposeBlock + threadIdx.x;
    if (lane >= a.lanes)
        return;
    const int k = (int)(lane % a.chunks);
    const int64_t row = lane / a.chunks;
    const int y = (int)(row % a.h);
    const int f = (int)(row / a.h);
    int64_t lo = a.layer_off[f], hi = a.layer_off[f + 1];
    if (!(lo >= 0 && lo <= hi && hi <= a.nlayers))        // a frame whose range leaves the table has no layers
        lo = hi = 0;
    const bool in_place = a.src == a.dst;
    if (lo == hi && in_place)
        return;
    const int x0 = k * kLanePixels;
    const int cnt = a.w - x0 < kLanePixels ? a.w - x0 : kLanePixels;
    const int64_t plane = (int64_t)a.h * a.w;
    const int64_t pix = (int64_t)f * plane + (int64_t)y * a.w + x0;          // first pixel of this lane
    const int64_t in_frame = (int64_t)y * a.w + x0;

    uint32_t px[C * 4];
    if (C == 3 && a.c_src == 1) {                   // set_frame: the value is copied into the three channels
        uint32_t g[4];
        load_bytes<16>(a.src + pix, cnt, g);
#pragma unroll
        for (int i = 0; i < C * 4; i++)
            px[i] = 0;
#pragma unroll
        for (int i = 0; i < kLanePixels * C; i++)
            px[i / 4] |= get_byte(g, i / C) << (8 * (i % 4));
    } else {
        load_bytes<16 * C>(a.src + pix * C, cnt * C, px);
    }

    for (int64_t l = lo; l < hi; l++) {
        const va_compose_layer L = a.layers[l];
        uint32_t m[4] = {0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u};
        if (L.mask_off >= 0) {
            if (L.mask_off > a.masks_bytes - plane)
                continue;                           // outside the masks: the layer is not applied
            load_bytes<16>(a.masks + L.mask_off + in_frame, cnt, m);
        }
        if (L.kind == VA_COMPOSE_HIGHLIGHT) {
            if (L.channel < -1 || L.channel >= C)
                continue;
            const double strength = (double)L.alpha, factor = L.factor;
#pragma unroll
            for (int p = 0; p < kLanePixels; p++) {
                if (!get_byte(m, p))
                    continue;
#pragma unroll
                for (int ch = 0; ch < C; ch++) {
                    if (C == 3 && L.channel >= 0 && L.channel != ch)
                        continue;
                    const double v = (double)get_byte(px, p * C + ch);
                    const double t = strength + factor * v;              // two roundings (-ffp-contract=off)
                    set_byte(px, p * C + ch, (uint32_t)(int)t & 255u);
                }
            }
        } else if (L.kind == VA_COMPOSE_ADD || L.kind == VA_COMPOSE_BLEND) {
            const int ic = L.image_channels;
            if (!(ic == 1 || (ic == 3 && C == 3)) || L.image_off < 0 || L.image_off > a.images_bytes - plane * ic)
                continue;
            uint32_t im[C * 4];
            const uint8_t *ip = a.images + L.image_off + in_frame * ic;
            if (C == 3 && ic == 1) {
                uint32_t g[4];
                load_bytes<16>(ip, cnt, g);
#pragma unroll
                for (int i = 0; i < C * 4; i++)
                    im[i] = 0;
#pragma unroll
                for (int i = 0; i < kLanePixels * C; i++)
                    im[i / 4] |= get_byte(g, i / C) << (8 * (i % 4));
            } else {
                load_bytes<16 * C>(ip, cnt * C, im);
            }
            const bool blend = L.kind == VA_COMPOSE_BLEND;
            const float alpha = L.alpha, beta = L.beta;
#pragma unroll
            for (int p = 0; p < kLanePixels; p++) {
                if (!get_byte(m, p))
                    continue;
#pragma unroll
                for (int ch = 0; ch < C; ch++) {
                    const uint32_t v = get_byte(px, p * C + ch), u = get_byte(im, p * C + ch);
                    uint32_t r;
                    if (blend) {
                        const float va_ = (float)v * alpha, ub = (float)u * beta;
                        float t = __builtin_rintf(va_ + ub);             // nearest, ties to even
                        t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
                        r = (uint32_t)t;
                    } else {
                        r = v + u > 255u ? 255u : v + u;
                    }
                    set_byte(px, p * C + ch, r);
                }
            }
        }
    }
    store_bytes<16 * C>(a.dst + pix * C, cnt * C, px);
}

// ------------------------------------------------------------------------------------------------ drawing
struct DrawArgs {
    uint8_t *frames;
    int n, h, w;
    const va_draw_cmd *cmds;
    const int64_t *cmd_off;
    int64_t ncmds;
    const int32_t *points;
    int64_t npoints;
    int32_t *status;
};

template <int C>
struct Plot {
    uint8_t *img;
    int w;
    uint32_t color;
    __device__ __forceinline__ void operator()(int64_t x, int64_t y) const
    {
        uint8_t *p = img + (y * w + x) * C;
        p[0] = (uint8_t)color;
        if (C == 3) {
            p[1] = (uint8_t)(color >> 8);
            p[2] = (uint8_t)(color >> 16);
        }
    }
};

__device__ __forceinline__ bool coord_ok(int64_t v) { return v >= -kPolyMaxCoord && v <= kPolyMaxCoord; }

// one command, shared by `team` lanes of which this is number `me`
template <int C>
__device__ void draw_cmd(const DrawArgs &a, const va_draw_cmd &cmd, uint8_t *img, int me, int team)
{
    const Plot<C> plot{img, a.w, cmd.color};
    if (cmd.kind == VA_DRAW_POLYLINE) {
        const int64_t k = cmd.count;
        const int32_t *v = a.points + 2 * cmd.first;
        const int64_t nseg = k == 0 ? 0 : k - 1 + ((cmd.flags & 1) ? 1 : 0);
        for (int64_t s = me; s < nseg; s += team) {
            const int64_t e = s + 1 == k ? 0 : s + 1;
            line8(a.w, a.h, v[2 * s], v[2 * s + 1], v[2 * e], v[2 * e + 1], plot);
        }
    } else {
        circle_steps(a.w, a.h, cmd.cx, cmd.cy, cmd.radius, (cmd.flags & 1) != 0, me, team, plot);
    }
}

template <int C>
__global__ void __launch_bounds__(kDrawBlock) draw_kernel(DrawArgs a)
{
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t lo = a.cmd_off[f], hi = a.cmd_off[f + 1];
    if (!(lo >= 0 && lo <= hi && hi <= a.ncmds)) {            // workgroup-uniform
        if (tid == 0)
            a.status[f] = VA_ERR_RANGE;
        return;
    }
    // every record and every point of the frame is checked before anything is drawn: a refused frame is untouched
    int bad = 0;
    for (int64_t i = lo + tid; i < hi; i += kDrawBlock) {
        const va_draw_cmd cmd = a.cmds[i];
        if (cmd.kind == VA_DRAW_POLYLINE)
            bad |= cmd.first < 0 || cmd.count < 0 || cmd.first > a.npoints || cmd.count > a.npoints - cmd.first;
        else if (cmd.kind == VA_DRAW_CIRCLE)
            bad |= !coord_ok(cmd.cx) || !coord_ok(cmd.cy) || cmd.radius > kPolyMaxCoord;
        else
            bad = 1;
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0)
            a.status[f] = VA_ERR_RANGE;
        return;
    }
    for (int64_t i = lo; i < hi; i++) {
        const va_draw_cmd cmd = a.cmds[i];
        if (cmd.kind != VA_DRAW_POLYLINE)
            continue;
        for (int64_t j = tid; j < 2 * (int64_t)cmd.count; j += kDrawBlock)
            bad |= !coord_ok(a.points[2 * cmd.first + j]);
    }
    if (__syncthreads_or(bad)) {
        if (tid == 0)
            a.status[f] = VA_ERR_RANGE;
        return;
    }
    uint8_t *img = a.frames + (int64_t)f * a.h * a.w * C;
    int64_t i = lo;
    while (i < hi) {
        // the phase: commands i .. j - 1 store one colour, so they commute
        const uint32_t color = a.cmds[i].color;
        int64_t j = i + 1;
        while (j < hi && a.cmds[j].color == color)
            j++;
        if (j - i >= kDrawWaves) {
            for (int64_t c = i + wave; c < j; c += kDrawWaves)
                draw_cmd<C>(a, a.cmds[c], img, lane, kWave);
        } else {
            for (int64_t c = i; c < j; c++)
                draw_cmd<C>(a, a.cmds[c], img, tid, kDrawBlock);
        }
        i = j;
        if (i < hi) {                       // the next phase overwrites: order this one's stores before it (only
            __threadfence_block();          // this workgroup ever touches the frame, so block scope is enough)
            __syncthreads();
        }
    }
    if (tid == 0)
        a.status[f] = VA_OK;
}


// ------------------------------------------------------------------------------------------------ contours
struct ContourDrawArgs {
    uint8_t *frames;
    int n_out, h, w;
    const va_contour_info *info;
    const int64_t *point_off;           // ncontours + 1 entries
    int64_t ncontours;
    const int32_t *points;
    int64_t npoints;
    const int32_t *frame_map;           // n_src entries, or NULL: the identity
    int n_src;
    uint32_t color;
    int32_t *status;
    int64_t first, lanes;               // this launch: lanes first .. lanes - 1 of ncontours + npoints
};

// the checks of slot s that need no point: its offsets, its frame and the frame's target.  false: none of its
// segments is drawn.  *target is -1 for a source frame the map leaves out (which is no error).
__device__ __forceinline__ bool contour_slot_ok(const ContourDrawArgs &a, int64_t s, int64_t lo, int64_t hi,
                                                int *target, bool *refused)
{
    *refused = true;
    if (!(lo >= 0 && lo <= hi && hi <= a.npoints))
        return false;
    const int f = a.info[s].frame;
    if (f < 0 || f >= a.n_src)
        return false;
    const int t = a.frame_map ? a.frame_map[f] : f;
    if (t < (a.frame_map ? -1 : 0) || t >= a.n_out)
        return false;
    *refused = false;
    *target = t;
    return t >= 0;
}

template <int C>
__global__ void __launch_bounds__(kContourBlock) draw_contours_kernel(ContourDrawArgs a)
{
    const int64_t lane = a.first + (int64_t)blockIdx.x * kContourBlock + threadIdx.x;
    if (lane >= a.lanes)
        return;
    int target;
    bool refused;
    if (lane < a.ncontours) {           // a slot lane: it reports what is wrong with the slot and draws nothing
        contour_slot_ok(a, lane, a.point_off[lane], a.point_off[lane + 1], &target, &refused);
        if (refused)
            a.status[0] = VA_ERR_RANGE;
        return;
    }
    // a point lane: the slot of point p is the last one that starts at or before p (the table is sorted when every
    // slot passes its check); only entries 1 .. ncontours - 1 are read here, s and s + 1 afterwards
    const int64_t p = lane - a.ncontours;
    int64_t s = 0, e = a.ncontours;
    if (e == 0)
        return;
    while (e - s > 1) {
        const int64_t mid = s + (e - s) / 2;
        if (a.point_off[mid] <= p)
            s = mid;
        else
            e = mid;
    }
    const int64_t lo = a.point_off[s], hi = a.point_off[s + 1];
    if (!contour_slot_ok(a, s, lo, hi, &target, &refused) || p < lo || p >= hi)
        return;                         // (the slot lane has reported a refused slot)
    const int64_t q = p + 1 == hi ? lo : p + 1;
    const int64_t x1 = a.points[2 * p], y1 = a.points[2 * p + 1], x2 = a.points[2 * q], y2 = a.points[2 * q + 1];
    if (!(coord_ok(x1) && coord_ok(y1) && coord_ok(x2) && coord_ok(y2))) {
        a.status[0] = VA_ERR_RANGE;
        return;
    }
    const Plot<C> plot{a.frames + (int64_t)target * a.h * a.w * C, a.w, a.color};
    line8(a.w, a.h, x1, y1, x2, y2, plot);
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

int va_compose_layers_u8(const uint8_t *src, int c_src, uint8_t *dst, int n, int h, int w, int c,
                         const va_compose_layer *layers, const int64_t *layer_off, int64_t nlayers,
                         const uint8_t *images, int64_t images_bytes, const uint8_t *masks, int64_t masks_bytes,
                         void *stream)
{
    VA_ENTER();
    VA_REQUIRE(n >= 0 && h >= 0 && w >= 0 && nlayers >= 0 && images_bytes >= 0 && masks_bytes >= 0,
               "va_compose_layers_u8: negative count (n %d, h %d, w %d, nlayers %lld, images %lld, masks %lld)", n, h,
               w, (long long)nlayers, (long long)images_bytes, (long long)masks_bytes);
    VA_REQUIRE((c_src == 1 || c_src == 3) && (c == 1 || c == 3) && c_src <= c,
               "va_compose_layers_u8: channels must be 1 or 3 with c_src <= c, got %d -> %d", c_src, c);
    VA_REQUIRE((size_t)h * w < kMaxFramePixels, "va_compose_layers_u8: frames above 2^29 pixels are not supported");
    VA_REQUIRE(src != dst || c_src == c || !src,
               "va_compose_layers_u8: src and dst must be distinct when c_src != c");
    if (n == 0 || h == 0 || w == 0 || (nlayers == 0 && src == dst && src))
        return VA_OK;
    VA_REQUIRE(src && dst && layer_off && (layers || nlayers == 0) && (images || images_bytes == 0) &&
                   (masks || masks_bytes == 0),
               "va_compose_layers_u8: NULL argument");
    VA_REQUIRE(aligned(layers, 8) && aligned(layer_off, 8),
               "va_compose_layers_u8: the layer tables must be 8-byte aligned");
    VA_REQUIRE(((int64_t)n * h * ((w + 15) / 16) + 255) / 256 < ((int64_t)1 << 31),
               "va_compose_layers_u8: the stack is too large for one launch");
    hipStream_t st = as_stream(stream);
    ComposeArgs a{src, dst, n, h, w, c_src, layers, layer_off, nlayers, images, images_bytes, masks, masks_bytes, 0, 0};
    a.chunks = (w + kLanePixels - 1) / kLanePixels;
    a.lanes = (int64_t)n * h * a.chunks;
    const int64_t blocks = (a.lanes + kComposeBlock - 1) / kComposeBlock;
    if (c == 1)
        hipLaunchKernelGGL(compose_layers_kernel<1>, dim3((unsigned)blocks), dim3(kComposeBlock), 0, st, a);
    else
        hipLaunchKernelGGL(compose_layers_kernel<3>, dim3((unsigned)blocks), dim3(kComposeBlock), 0, st, a);
    VA_LAUNCH_CHECK("compose_layers_kernel");
    return VA_OK;
}

int va_draw_u8(uint8_t *frames, int n, int h, int w, int c, const va_draw_cmd *cmds, const int64_t *cmd_off,
               int64_t ncmds, const int32_t *points, int64_t npoints, int32_t *status, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(n >= 0 && h >= 0 && w >= 0 && ncmds >= 0 && npoints >= 0,
               "va_draw_u8: negative count (n %d, h %d, w %d, ncmds %lld, npoints %lld)", n, h, w, (long long)ncmds,
               (long long)npoints);
    VA_REQUIRE(c == 1 || c == 3, "va_draw_u8: channels must be 1 or 3, got %d", c);
    VA_REQUIRE((size_t)h * w < kMaxFramePixels, "va_draw_u8: frames above 2^29 pixels are not supported");
    if (n == 0 || ncmds == 0)
        return VA_OK;
    VA_REQUIRE((frames || h == 0 || w == 0) && cmds && cmd_off && status && (points || npoints == 0),
               "va_draw_u8: NULL argument");
    VA_REQUIRE(aligned(cmds, 8) && aligned(cmd_off, 8) && aligned(points, 4) && aligned(status, 4),
               "va_draw_u8: the command tables must be 8-byte aligned, points and status 4-byte aligned");
    hipStream_t st = as_stream(stream);
    const DrawArgs a{frames, n, h, w, cmds, cmd_off, ncmds, points, npoints, status};
    if (c == 1)
        hipLaunchKernelGGL(draw_kernel<1>, dim3(n), dim3(kDrawBlock), 0, st, a);
    else
        hipLaunchKernelGGL(draw_kernel<3>, dim3(n), dim3(kDrawBlock), 0, st, a);
    VA_LAUNCH_CHECK("draw_kernel");
    return VA_OK;
}

int va_draw_contours_u8(uint8_t *frames, int n_out, int h, int w, int c, const va_contour_info *info,
                        const int64_t *point_off, int64_t ncontours, const int32_t *points, int64_t npoints,
                        const int32_t *frame_map, int n_src, uint32_t color, int32_t *status, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(n_out >= 0 && h >= 0 && w >= 0 && ncontours >= 0 && npoints >= 0 && n_src >= 0,
               "va_draw_contours_u8: negative count (n_out %d, h %d, w %d, ncontours %lld, npoints %lld, n_src %d)",
               n_out, h, w, (long long)ncontours, (long long)npoints, n_src);
    VA_REQUIRE(c == 1 || c == 3, "va_draw_contours_u8: channels must be 1 or 3, got %d", c);
    VA_REQUIRE((size_t)h * w < kMaxFramePixels,
               "va_draw_contours_u8: frames above 2^29 pixels are not supported");
    VA_REQUIRE(status && (frames || n_out == 0 || h == 0 || w == 0) && ((info && point_off) || ncontours == 0) &&
                   (points || npoints == 0),
               "va_draw_contours_u8: NULL argument");
    VA_REQUIRE(aligned(info, 8) && aligned(point_off, 8) && aligned(points, 4) && aligned(frame_map, 4) &&
                   aligned(status, 4),
               "va_draw_contours_u8: the records and offsets must be 8-byte aligned, points, map and status 4-byte "
               "aligned");
    hipStream_t st = as_stream(stream);
    VA_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), st));        // VA_OK, on every call
    if (ncontours == 0)
        return VA_OK;
    ContourDrawArgs a{frames, n_out, h, w, info, point_off, ncontours, points, npoints, frame_map, n_src, color,
                      status, 0, ncontours + npoints};
    for (a.first = 0; a.first < a.lanes; a.first += kContourPieceLanes) {
        const int64_t here = a.lanes - a.first < kContourPieceLanes ? a.lanes - a.first : kContourPieceLanes;
        const unsigned blocks = (unsigned)((here + kContourBlock - 1) / kContourBlock);
        if (c == 1)
            hipLaunchKernelGGL(draw_contours_kernel<1>, dim3(blocks), dim3(kContourBlock), 0, st, a);
        else
            hipLaunchKernelGGL(draw_contours_kernel<3>, dim3(blocks), dim3(kContourBlock), 0, st, a);
        VA_LAUNCH_CHECK("draw_contours_kernel");
    }
    return VA_OK;
}

}  // extern "C"
