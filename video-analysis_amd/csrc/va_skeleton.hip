// va_skeleton.hip -- skeleton graphs of the items of a ragged packed buffer (va_skeleton_graph; the definition is
// DESIGN.md §9, "Skeleton graphs").
//
// One thread per pixel of the packed buffer, one launch per step, every step chip-wide, so that 4096 worm boxes and
// a stack of 1080p frames are the same work: `total` pixels.  A pixel finds its item by a binary search of the
// offsets (12 steps for 4096 items); only the classify pass does that for every pixel, the later passes only for
// foreground, which is a per cent or so of a skeleton.
//   classify   adj[g]: the m-adjacency mask of pixel g (bit k = neighbour k in raster order NW N NE W E SW S SE),
//              from the item's own 3 x 3 neighbourhood: a neighbour beyond the item's border is background
//   union 1    union-find over the foreground, roots of smallest KEY, key = index | (d == 2) << 31: the root of a
//              component is its first node pixel if it has one, else (a pure ring) its first pixel, which so
//              becomes a node pixel
//   union 2    union-find over the node pixels, roots of smallest index: the node sets.  Lock-free atomicMin
//              linking as in va_ccl.hip; the forest after a launch does not depend on the order of the atomics
//   anchor     per root: atomicMax of d << 29 | (2^29 - 1 - local index), integer atomicAdd of pixels and edge ends
//   walk 1     one lane per node pixel, its edge ends one after the other: walk the chain to the far end, decide
//              ownership (the lexicographically smaller (index(a), index(c1))), count the owner's points
//   scan       block sums, one workgroup scans them, blocks apply them: node slots, edge slots and point offsets
//              in pixel order = the definition's order (items ascend with their offsets)
//   walk 2     the owners walk again and write records, lengths and points -- below the capacities only
// Every slot comes from these counts and scans; the atomics are integer min / max / add, whose results do not
// depend on their order, so two calls write identical bytes.
#include "va_common.h"
#include "va_scan.h"

namespace va {

namespace {

constexpr int kBlock = 256;
constexpr int kScanBlock = 1024;
constexpr int kScanWaves = kScanBlock / kWave;
constexpr uint32_t kBg = 0xFFFFFFFEu;      // forest word of a background pixel
constexpr uint32_t kChain = 0xFFFFFFFFu;   // forest word of a chain pixel (pass 2)
constexpr uint32_t kRingBit = 0x80000000u;
constexpr uint32_t kAnchorIdx = (1u << 29) - 1;
constexpr int64_t kMaxItemPixels = (int64_t)1 << 29;

struct Items {
    const int32_t *shapes;
    const int64_t *offsets;
    int64_t total;
    int m;
};

struct Where {
    int item, w, h, x, y;
    int64_t off;
};

// the item that holds packed element g: the last one whose offset is <= g (empty items share their offset with
// the next one and come before it).  false: g lies in no item (a gap, an item that would pass `total`, or one of
// 2^29 pixels or more, whose local indices the anchor key cannot hold: such an item is empty to every kernel)
__device__ __forceinline__ bool locate(const Items &it, int64_t g, Where *p)
{
    int lo = 0, hi = it.m;                 // first item with offset > g
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (it.offsets[mid] <= g)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo == 0)
        return false;
    const int i = lo - 1;
    const int h = it.shapes[2 * i], w = it.shapes[2 * i + 1];
    const int64_t off = it.offsets[i];
    if (h <= 0 || w <= 0 || off < 0 || (int64_t)h * w > it.total - off || (int64_t)h * w >= kMaxItemPixels)
        return false;
    const int64_t l = g - off;
    if (l >= (int64_t)h * w)
        return false;
    p->item = i;
    p->w = w;
    p->h = h;
    p->off = off;
    p->y = (int)(l / w);
    p->x = (int)(l - (int64_t)p->y * w);
    return true;
}

__device__ __forceinline__ int dir_dx(int k) { const int j = k < 4 ? k : k + 1; return j % 3 - 1; }
__device__ __forceinline__ int dir_dy(int k) { const int j = k < 4 ? k : k + 1; return j / 3 - 1; }

// ---- the forest (see va_ccl.hip: a stale parent is an older ancestor, the linking atomicMin tells the truth)
__device__ __forceinline__ uint32_t ld_forest(const uint32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void st_forest(uint32_t *p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ uint32_t idx_of(uint32_t key) { return key & ~kRingBit; }

__device__ uint32_t find_root(uint32_t *P, uint32_t a)
{
    for (;;) {
        const uint32_t p = ld_forest(P + idx_of(a));
        if (p == a)
            return a;
        const uint32_t gp = ld_forest(P + idx_of(p));
        if (gp == p)
            return p;
        st_forest(P + idx_of(a), gp);
        a = gp;
    }
}
__device__ uint32_t find_root_ro(const uint32_t *P, uint32_t a)
{
    for (;;) {
        const uint32_t p = ld_forest(P + idx_of(a));
        if (p == a)
            return a;
        a = p;
    }
}
__device__ void unite(uint32_t *P, uint32_t a, uint32_t b)
{
    for (;;) {
        a = find_root(P, a);
        b = find_root(P, b);
        if (a == b)
            return;
        if (a > b) {
            const uint32_t t = a;
            a = b;
            b = t;
        }
        const uint32_t old = atomicMin(P + idx_of(b), a);   // a < b
        if (old == b)
            return;
        b = old;
    }
}

// ---- classify: adjacency masks, and the forest of pass 1
__global__ void __launch_bounds__(kBlock) skel_classify(const uint8_t *img, Items it, uint8_t *adj, uint32_t *P)
{
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= it.total)
        return;
    Where p;
    uint32_t mask = 0, word = kBg;
    if (locate(it, g, &p) && img[g] != 0) {
        uint32_t fg = 0;                   // bit k: neighbour k is foreground (inside the item)
        for (int k = 0; k < 8; ++k) {
            const int x = p.x + dir_dx(k), y = p.y + dir_dy(k);
            if (x >= 0 && x < p.w && y >= 0 && y < p.h && img[p.off + (int64_t)y * p.w + x] != 0)
                fg |= 1u << k;
        }
        // N, W, E, S: bits 1, 3, 4, 6; a diagonal counts only between two background edge neighbours
        mask = fg & 0x5Au;
        if ((fg & 0x01u) && !(fg & 0x0Au)) mask |= 0x01u;   // NW: N and W
        if ((fg & 0x04u) && !(fg & 0x12u)) mask |= 0x04u;   // NE: N and E
        if ((fg & 0x20u) && !(fg & 0x48u)) mask |= 0x20u;   // SW: W and S
        if ((fg & 0x80u) && !(fg & 0x50u)) mask |= 0x80u;   // SE: E and S
        word = (uint32_t)g | (__popc(mask) == 2 ? kRingBit : 0u);
    }
    adj[g] = (uint8_t)mask;
    P[g] = word;
}

// ---- unions with the forward neighbours (E, SW, S, SE).  kRings: pass 1, every foreground pixel, keys carry the
// ring bit of their own degree; otherwise pass 2, node pixels only, keys are indices.  A key is never read from
// the forest, whose words other lanes are linking meanwhile
template <bool kRings>
__global__ void __launch_bounds__(kBlock) skel_union(const uint8_t *adj, Items it, uint32_t *P)
{
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= it.total)
        return;
    const uint32_t mask = adj[g], fwd = mask & 0xF0u;
    if (fwd == 0 || (!kRings && ld_forest(P + g) >= kBg))
        return;
    Where p;
    if (!locate(it, g, &p))
        return;
    const uint32_t mine = (uint32_t)g | (kRings && __popc(mask) == 2 ? kRingBit : 0u);
    for (int k = 4; k < 8; ++k) {
        if (!(fwd & (1u << k)))
            continue;
        const int64_t q = g + (int64_t)dir_dy(k) * p.w + dir_dx(k);
        if (!kRings && ld_forest(P + q) >= kBg)
            continue;                      // a chain pixel
        unite(P, mine, (uint32_t)q | (kRings && __popc((uint32_t)adj[q]) == 2 ? kRingBit : 0u));
    }
}

// ---- after pass 1: node pixels are d != 2 and the roots that are chain pixels; the forest of pass 2
__global__ void __launch_bounds__(kBlock) skel_nodes(const uint8_t *adj, int64_t total, uint32_t *P)
{
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= total)
        return;
    const uint32_t word = P[g];
    if (word == kBg)
        return;
    const bool chain = __popc((uint32_t)adj[g]) == 2;
    const bool node = !chain || word == ((uint32_t)g | kRingBit);
    P[g] = node ? (uint32_t)g : kChain;
}

__global__ void __launch_bounds__(kBlock) skel_flatten(int64_t total, uint32_t *P)
{
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= total)
        return;
    if (P[g] < kBg)
        P[g] = find_root_ro(P, (uint32_t)g);
}

// ---- per node: anchor key, pixels | edge ends << 32
__global__ void __launch_bounds__(kBlock) skel_anchor(const uint8_t *adj, Items it, const uint32_t *P,
                                                      uint32_t *anchor, unsigned long long *tally)
{
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= it.total)
        return;
    const uint32_t root = P[g];
    if (root >= kBg)
        return;
    Where p;
    if (!locate(it, g, &p))
        return;
    const uint32_t mask = adj[g];
    int ends = 0;
    for (int k = 0; k < 8; ++k)
        if ((mask & (1u << k)) && P[g + (int64_t)dir_dy(k) * p.w + dir_dx(k)] == kChain)
            ++ends;
    atomicMax(anchor + root, ((uint32_t)__popc(mask) << 29) | (kAnchorIdx - (uint32_t)(g - p.off)));
    atomicAdd(tally + root, 1ull | ((unsigned long long)ends << 32));
}

// the chain from node pixel a (at g) through its neighbour k, to the node pixel at the far end
struct Walk {
    int64_t b, ck;     // far node pixel, last chain pixel
    int k;             // chain pixels
};
// visit(x, y) sees every chain pixel in order
template <class Visit>
__device__ __forceinline__ Walk walk_chain(const uint8_t *adj, const uint32_t *P, const Where &p, int64_t g, int dir,
                                           Visit visit)
{
    Walk r;
    int x = p.x + dir_dx(dir), y = p.y + dir_dy(dir);
    int64_t cur = g + (int64_t)dir_dy(dir) * p.w + dir_dx(dir), prev = g;
    const int64_t limit = (int64_t)p.w * p.h;
    r.k = 0;
    while (P[cur] == kChain && r.k < limit) {
        visit(x, y);
        ++r.k;
        const uint32_t other = adj[cur] & ~(1u << (7 - dir));      // not the way back
        dir = __ffs(other) - 1;
        if (dir < 0)
            break;                         // cannot happen: a chain pixel has two neighbours
        prev = cur;
        x += dir_dx(dir);
        y += dir_dy(dir);
        cur += (int64_t)dir_dy(dir) * p.w + dir_dx(dir);
    }
    r.b = cur;
    r.ck = prev;
    return r;
}

__device__ __forceinline__ int64_t anchor_pixel(const uint32_t *anchor, uint32_t root, int64_t off)
{
    return off + (kAnchorIdx - (anchor[root] & kAnchorIdx));
}

// ---- walk 1: owned[g] = the directions whose edge this node pixel owns, npts[g] = the points of those edges
__global__ void __launch_bounds__(kBlock) skel_walk_count(const uint8_t *adj, Items it, const uint32_t *P,
                                                          const uint32_t *anchor, uint8_t *owned, int32_t *npts)
{
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= it.total)
        return;
    const uint32_t root = P[g];
    uint32_t own = 0;
    int points = 0;
    Where p;
    if (root < kBg && adj[g] != 0 && locate(it, g, &p)) {
        const uint32_t mask = adj[g];
        for (int k = 0; k < 8; ++k) {
            if (!(mask & (1u << k)))
                continue;
            const int64_t c1 = g + (int64_t)dir_dy(k) * p.w + dir_dx(k);
            if (P[c1] != kChain)
                continue;
            const Walk r = walk_chain(adj, P, p, g, k, [](int, int) {});
            if (P[r.b] >= kBg)
                continue;                  // cannot happen: the walk ran into its step limit
            if (g < r.b || (g == r.b && c1 < r.ck)) {
                own |= 1u << k;
                points += r.k + 2 + (anchor_pixel(anchor, root, p.off) != g) +
                          (anchor_pixel(anchor, P[r.b], p.off) != r.b);
            }
        }
    }
    owned[g] = (uint8_t)own;
    npts[g] = points;
}

// ---- scan: what pixel g adds to (nodes, edges, points)
__device__ __forceinline__ void pixel_counts(const uint32_t *P, const uint8_t *owned, const int32_t *npts, int64_t g,
                                             int64_t total, int *nodes, int *edges, int *points)
{
    *nodes = *edges = *points = 0;
    if (g < total) {
        *nodes = P[g] == (uint32_t)g;
        *edges = __popc((uint32_t)owned[g]);
        *points = npts[g];
    }
}

// what each workgroup of the scan adds to (nodes, edges, points), and the items' (nodes, edges).  A workgroup whose
// first and last pixel lie in one item -- every one in a frame stack -- adds its sums to that item's counters once;
// elsewhere each node pixel and owner adds its own.  Integer adds: the counters do not depend on their order
__global__ void __launch_bounds__(kScanBlock) skel_block_sums(const uint32_t *P, const uint8_t *owned,
                                                              const int32_t *npts, Items it, long long *sums,
                                                              int32_t *counts)
{
    __shared__ int one_item;
    __shared__ int wave_ne[kScanWaves];                    // nodes | edges << 16 (at most 1024 and 4096 a workgroup)
    __shared__ long long wave_pt[kScanWaves];
    const int64_t first = (int64_t)blockIdx.x * kScanBlock, g = first + threadIdx.x;
    if (threadIdx.x == 0) {
        const int64_t last = (first + kScanBlock < it.total ? first + kScanBlock : it.total) - 1;
        Where a, b;
        one_item = locate(it, first, &a) && locate(it, last, &b) && a.item == b.item ? a.item : -1;
    }
    int nodes, edges, points;
    pixel_counts(P, owned, npts, g, it.total, &nodes, &edges, &points);
    const int ne = wave_sum(nodes | (edges << 16));
    const long long pt = wave_sum((long long)points);
    if ((threadIdx.x & (kWave - 1)) == 0) {
        wave_ne[threadIdx.x / kWave] = ne;
        wave_pt[threadIdx.x / kWave] = pt;
    }
    __syncthreads();
    const int item = one_item;
    Where p;
    if (item < 0 && (nodes || edges) && locate(it, g, &p)) {
        if (nodes)
            atomicAdd(counts + 2 * p.item, 1);
        if (edges)
            atomicAdd(counts + 2 * p.item + 1, edges);
    }
    if (threadIdx.x == 0) {
        int sne = 0;
        long long sp = 0;
        for (int k = 0; k < kScanWaves; ++k) {
            sne += wave_ne[k];
            sp += wave_pt[k];
        }
        const int sn = sne & 0xFFFF, se = sne >> 16;
        sums[3 * (int64_t)blockIdx.x] = sn;
        sums[3 * (int64_t)blockIdx.x + 1] = se;
        sums[3 * (int64_t)blockIdx.x + 2] = sp;
        if (item >= 0 && sn)
            atomicAdd(counts + 2 * item, sn);
        if (item >= 0 && se)
            atomicAdd(counts + 2 * item + 1, se);
    }
}

// one workgroup: block sums -> exclusive (in place), the totals, the items' first node slots, point_off[0]
__global__ void __launch_bounds__(kScanBlock) skel_scan_sums(long long *sums, int64_t nblocks, const int32_t *counts,
                                                             int m, long long *first_node, int64_t *totals,
                                                             int64_t *point_off)
{
    __shared__ long long lds[kScanWaves];
    for (int c = 0; c < 3; ++c) {
        long long carry = 0;
        for (int64_t at = 0; at < nblocks; at += kScanBlock) {
            const int64_t i = at + threadIdx.x;
            const long long v = i < nblocks ? sums[3 * i + c] : 0;
            long long s;
            const long long e = block_exclusive<kScanWaves>(v, lds, s);
            if (i < nblocks)
                sums[3 * i + c] = carry + e;
            carry += s;
        }
        if (threadIdx.x == 0)
            totals[c] = carry;
    }
    long long carry = 0;
    for (int at = 0; at < m; at += kScanBlock) {
        const int i = at + threadIdx.x;
        const long long v = i < m ? counts[2 * i] : 0;
        long long s;
        const long long e = block_exclusive<kScanWaves>(v, lds, s);
        if (i < m)
            first_node[i] = carry + e;
        carry += s;
    }
    if (threadIdx.x == 0)
        point_off[0] = 0;
}

// ---- apply: node records and slots; edge and point bases of the owners
__global__ void __launch_bounds__(kScanBlock) skel_apply(const uint32_t *P, const uint8_t *owned, int32_t *npts,
                                                         Items it, const long long *sums, const uint32_t *anchor,
                                                         unsigned long long *tally, long long *point_base,
                                                         va_skeleton_node *nodes_out, int64_t cap_nodes)
{
    __shared__ long long lds[kScanWaves];
    const int64_t g = (int64_t)blockIdx.x * kScanBlock + threadIdx.x;
    int nodes, edges, points;
    pixel_counts(P, owned, npts, g, it.total, &nodes, &edges, &points);
    const long long *before = sums + 3 * (int64_t)blockIdx.x;          // what the workgroups in front add up to
    long long all;                                                      // (this workgroup's own sums: not needed here)
    const long long en = before[0] + block_exclusive<kScanWaves>((long long)nodes, lds, all);
    const long long ee = before[1] + block_exclusive<kScanWaves>((long long)edges, lds, all);
    const long long ep = before[2] + block_exclusive<kScanWaves>((long long)points, lds, all);
    Where p;
    if (nodes && locate(it, g, &p)) {
        const unsigned long long t = tally[g];
        if (en < cap_nodes) {
            const int64_t a = anchor_pixel(anchor, (uint32_t)g, p.off) - p.off;
            va_skeleton_node rec;
            rec.item = p.item;
            rec.x = (int32_t)(a % p.w);
            rec.y = (int32_t)(a / p.w);
            rec.degree = (int32_t)(t >> 32);
            rec.pixels = (int32_t)(t & 0xFFFFFFFFull);
            nodes_out[en] = rec;
        }
        tally[g] = (unsigned long long)en;     // from here on: the node's global slot
    }
    if (edges) {
        npts[g] = (int32_t)ee;                 // from here on: the first edge slot of this pixel's edges
        point_base[g] = ep;
    }
}

// ---- walk 2: the owners write their edges
__global__ void __launch_bounds__(kBlock) skel_walk_write(const uint8_t *adj, Items it, const uint32_t *P,
                                                          const uint32_t *anchor, const uint8_t *owned,
                                                          const int32_t *edge_base, const long long *point_base,
                                                          const unsigned long long *slot, const long long *first_node,
                                                          va_skeleton_edge *edges_out, int64_t *point_off,
                                                          int64_t cap_edges, int32_t *points_out, int64_t cap_points)
{
    const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (g >= it.total)
        return;
    const uint32_t own = owned[g];
    Where p;
    if (own == 0 || !locate(it, g, &p))
        return;
    int64_t e = edge_base[g];
    long long pt = point_base[g];
    const uint32_t root_a = P[g];
    const int64_t anc_a = anchor_pixel(anchor, root_a, p.off) - p.off;
    const int ax = (int)(anc_a % p.w), ay = (int)(anc_a / p.w);
    for (int k = 0; k < 8 && e < cap_edges; ++k) {
        if (!(own & (1u << k)))
            continue;
        // the curve: anchor(A), a unless it is the anchor, the chain, b unless it is the anchor, anchor(B)
        int32_t *out = nullptr;            // set below once the point count is known to fit
        int n = 0, px = ax, py = ay;
        double length = 0.0;
        auto emit = [&](int x, int y) {
            if (n > 0) {
                const float dx = (float)(x - px), dy = (float)(y - py);
                const float s = dx * dx + dy * dy;
                length += (double)(float)sqrt((double)s);   // the correctly rounded float32 root
            }
            if (out) {
                out[2 * n] = x;
                out[2 * n + 1] = y;
            }
            px = x;
            py = y;
            ++n;
        };
        // a first walk for the far end and the count, then the one that writes: the points may only be written
        // when all of them lie below cap_points
        const Walk r = walk_chain(adj, P, p, g, k, [](int, int) {});
        const uint32_t root_b = P[r.b];
        const int64_t anc_b = anchor_pixel(anchor, root_b, p.off) - p.off;
        const int bx = (int)((r.b - p.off) % p.w), by = (int)((r.b - p.off) / p.w);
        const int npoints = r.k + 2 + (anc_a != g - p.off) + (anc_b != r.b - p.off);
        if (pt + npoints <= cap_points)
            out = points_out + 2 * pt;
        emit(ax, ay);
        if (anc_a != g - p.off)
            emit(p.x, p.y);
        walk_chain(adj, P, p, g, k, emit);
        if (anc_b != r.b - p.off)
            emit(bx, by);
        emit((int)(anc_b % p.w), (int)(anc_b / p.w));
        va_skeleton_edge rec;
        rec.item = p.item;
        rec.node_a = (int32_t)((long long)slot[root_a] - first_node[p.item]);
        rec.node_b = (int32_t)((long long)slot[root_b] - first_node[p.item]);
        rec.npoints = npoints;
        rec.length = length;
        edges_out[e] = rec;
        point_off[e] = pt;
        point_off[e + 1] = pt + npoints;
        pt += npoints;
        ++e;
    }
}

// the workspace holds per pixel the forest, the anchor key and the tally of its node (zeroed per call), the adjacency
// and ownership masks, the point counts and the point offsets, then the scan's block sums
struct SkeletonLayout { size_t zeroed, anchor, tally, zeroed_bytes, forest, adj, owned, npts, point_base, sums,
                        first_node, total; };
SkeletonLayout skeleton_layout(int64_t total, int m)
{
    const size_t px = (size_t)(total > 0 ? total : 1);
    const size_t blocks = (px + kScanBlock - 1) / kScanBlock;
    Carve c;
    SkeletonLayout L;
    L.zeroed = c.take(0);
    L.anchor = c.take(px * 4);
    L.tally = c.take(px * 8);
    L.zeroed_bytes = c.total;
    L.forest = c.take(px * 4);
    L.adj = c.take(px);
    L.owned = c.take(px);
    L.npts = c.take(px * 4);
    L.point_base = c.take(px * 8);
    L.sums = c.take(blocks * 3 * 8);
    L.first_node = c.take((size_t)(m > 0 ? m : 1) * 8);
    L.total = c.total;
    return L;
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

size_t va_skeleton_graph_workspace_bytes(int64_t total, int m)
{
    if (total < 0 || m < 0)
        return 256;
    return skeleton_layout(total, m).total;
}

int va_skeleton_graph(const uint8_t *masks, const int32_t *shapes, const int64_t *offsets, int64_t total, int m,
                      int32_t *counts, int64_t *totals, va_skeleton_node *nodes, int64_t cap_nodes,
                      va_skeleton_edge *edges, int64_t *point_off, int64_t cap_edges, int32_t *points,
                      int64_t cap_points, void *workspace, size_t workspace_bytes, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(m >= 0 && total >= 0, "va_skeleton_graph: negative count (m %d, total %lld)", m, (long long)total);
    VA_REQUIRE(total < ((int64_t)1 << 31) - 2, "va_skeleton_graph: 2^31 - 2 or more packed elements are not supported");
    VA_REQUIRE(masks && shapes && offsets && counts && totals && nodes && edges && point_off && points && workspace,
               "va_skeleton_graph: NULL argument");
    VA_REQUIRE(cap_nodes >= 0 && cap_edges >= 0 && cap_points >= 0,
               "va_skeleton_graph: negative capacity (%lld nodes, %lld edges, %lld points)", (long long)cap_nodes,
               (long long)cap_edges, (long long)cap_points);
    VA_REQUIRE(aligned(points, 8) && aligned(nodes, 4) && aligned(edges, 8) && aligned(point_off, 8) &&
                   aligned(totals, 8) && aligned(counts, 4) && aligned(workspace, 8),
               "va_skeleton_graph: points, edge records, offsets, totals and workspace must be 8-byte aligned");
    VA_REQUIRE(workspace_bytes >= va_skeleton_graph_workspace_bytes(total, m),
               "va_skeleton_graph: workspace of %zu bytes < required %zu", workspace_bytes,
               va_skeleton_graph_workspace_bytes(total, m));
    hipStream_t st = as_stream(stream);
    const SkeletonLayout L = skeleton_layout(total, m);
    const Items it{shapes, offsets, total, m};
    uint32_t *P = at<uint32_t>(workspace, L.forest), *anchor = at<uint32_t>(workspace, L.anchor);
    unsigned long long *tally = at<unsigned long long>(workspace, L.tally);
    uint8_t *adj = at<uint8_t>(workspace, L.adj), *owned = at<uint8_t>(workspace, L.owned);
    int32_t *npts = at<int32_t>(workspace, L.npts);
    long long *point_base = at<long long>(workspace, L.point_base), *sums = at<long long>(workspace, L.sums);
    long long *first_node = at<long long>(workspace, L.first_node);

    if (m > 0)
        VA_HIP(hipMemsetAsync(counts, 0, (size_t)m * 2 * sizeof(int32_t), st));
    if (total == 0 || m == 0) {
        VA_HIP(hipMemsetAsync(totals, 0, 3 * sizeof(int64_t), st));
        VA_HIP(hipMemsetAsync(point_off, 0, sizeof(int64_t), st));
        return VA_OK;
    }
    VA_HIP(hipMemsetAsync(at(workspace, L.zeroed), 0, L.zeroed_bytes, st));
    const int grid = cdiv(total, kBlock), sgrid = cdiv(total, kScanBlock);
    skel_classify<<<grid, kBlock, 0, st>>>(masks, it, adj, P);
    VA_LAUNCH_CHECK("skel_classify");
    skel_union<true><<<grid, kBlock, 0, st>>>(adj, it, P);
    VA_LAUNCH_CHECK("skel_union");
    skel_nodes<<<grid, kBlock, 0, st>>>(adj, total, P);
    VA_LAUNCH_CHECK("skel_nodes");
    skel_union<false><<<grid, kBlock, 0, st>>>(adj, it, P);
    VA_LAUNCH_CHECK("skel_union");
    skel_flatten<<<grid, kBlock, 0, st>>>(total, P);
    VA_LAUNCH_CHECK("skel_flatten");
    skel_anchor<<<grid, kBlock, 0, st>>>(adj, it, P, anchor, tally);
    VA_LAUNCH_CHECK("skel_anchor");
    skel_walk_count<<<grid, kBlock, 0, st>>>(adj, it, P, anchor, owned, npts);
    VA_LAUNCH_CHECK("skel_walk_count");
    skel_block_sums<<<sgrid, kScanBlock, 0, st>>>(P, owned, npts, it, sums, counts);
    VA_LAUNCH_CHECK("skel_block_sums");
    skel_scan_sums<<<1, kScanBlock, 0, st>>>(sums, sgrid, counts, m, first_node, totals, point_off);
    VA_LAUNCH_CHECK("skel_scan_sums");
    skel_apply<<<sgrid, kScanBlock, 0, st>>>(P, owned, npts, it, sums, anchor, tally, point_base, nodes, cap_nodes);
    VA_LAUNCH_CHECK("skel_apply");
    skel_walk_write<<<grid, kBlock, 0, st>>>(adj, it, P, anchor, owned, npts, point_base, tally, first_node, edges,
                                             point_off, cap_edges, points, cap_points);
    VA_LAUNCH_CHECK("skel_walk_write");
    return VA_OK;
}

}  // extern "C"
