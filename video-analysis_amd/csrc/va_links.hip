// va_links.hip -- the overlap table between consecutive label planes of a stack ("Region links"):
// for pair t = (labels[t - 1] | prev, labels[t]) every (a, b, count) with a >= 1, b >= 1 and count pixels that hold a
// in the earlier plane and b in the later one, in the order of the first such pixel.  This replaces no call of the
// reference: it is what a tracker does first with the labels of video/analysis/regions.py:159-174 of consecutive
// frames, here without the label planes leaving the device.  The arithmetic is va_links_math.h, the same text the
// host test compiles.
//
// One lane per pixel, a workgroup per 256 consecutive pixels of one pair, the pairs in gridDim.y (pieces of 65535):
//   count       candidates (va_links_math.h) per pair, one add per wave; their sum over the batch is `need`
//   scan        exclusive scan of the pairs' table sizes (one workgroup), and two flags the kernels behind read:
//               `store` (need <= cap_links) and `tables` (the tables of all pairs fit the workspace together)
//   clear       the slots the tables of this call use
//   accumulate  a wave covers 64 consecutive pixels; the lane at the head of a run of one key inside them (a row
//               start is a head) inserts the run: compare-and-swap on the key, add on the count, min on the first
//               pixel.  Sum and min commute, so the entries do not depend on the order of arrival.  The runs of
//               the first four keys of a wave are summed in the wave first: one insert a key
//   own         a candidate that is its key's first pixel owns the link: owners per workgroup
//   scan        the workgroups of a pair (a workgroup per pair), then the pairs (one workgroup)
//   place       (store only) the owners again, ranked inside the workgroup by ballots: record at pair +
//               workgroup + rank
//   serial      (only where the tables do not fit together, which a capacity below need allows) the links per pair
//               with one table at a time: a workgroup owns a table region with room for any pair and walks its
//               pairs one after the other -- clear, accumulate, count the owners.  Slower, and exact
// Slots come from counts and scans alone: two calls write the same bytes, whatever the workspace held.  Every table
// slot and counter is written before it is read.  Nothing is written beyond cap_links records.
#include "va_common.h"
#include "va_links_math.h"
#include "va_scan.h"

namespace va {

namespace {

using va_links::Entry;

constexpr int kLinkBlock = 256;              // pixels of a workgroup: four waves
constexpr int kLinkWaves = kLinkBlock / kWave;
constexpr int kScanBlock = 1024;
constexpr int kMergedKeys = 4;               // keys of a wave whose runs are summed in the wave before they go in
constexpr int kClearMaxGrid = 4096;          // workgroups of the clear, which strides over the slots in use
constexpr int kSerialBlock = 1024;           // the serial pass: lanes of a workgroup, and its most workgroups
constexpr int kSerialMaxGrid = 256;
enum { kStore = 0, kTables = 1 };            // the flags in the workspace

struct LinksLayout { size_t ncand, tab_off, pair_off, go, block_cnt, table, total; };
inline int64_t links_blocks(int h, int w) { return ((int64_t)h * w + kLinkBlock - 1) / kLinkBlock; }
// the slots of a pair that has a candidate at every pixel: room for any pair
inline int64_t links_pair_slots(int h, int w) { return 2 * (int64_t)h * w + 1; }
// the tables of a call that stores its links hold at most 2 need + n slots, and need <= cap_links; no call needs
// more than one candidate per pixel.  Never less than room for one pair of any content: the serial pass
inline int64_t links_table_slots(int n, int h, int w, int64_t cap)
{
    const int64_t px = (int64_t)n * h * w, all = 2 * (cap < px ? cap : px) + n, one = links_pair_slots(h, w);
    return all > one ? all : one;
}
LinksLayout links_layout(int n, int h, int w, int64_t cap)
{
    Carve c;
    LinksLayout g;
    g.ncand = c.take((size_t)n * sizeof(int32_t));
    g.tab_off = c.take(((size_t)n + 1) * sizeof(int64_t));
    g.pair_off = c.take(((size_t)n + 1) * sizeof(int64_t));
    g.go = c.take(2 * sizeof(int32_t));
    g.block_cnt = c.take((size_t)n * links_blocks(h, w) * sizeof(int32_t));
    g.table = c.take((size_t)links_table_slots(n, h, w, cap) * sizeof(Entry));
    g.total = c.total;
    return g;
}

struct LinksArgs {
    const int32_t *prev, *labels;
    int n, h, w;
    int first_pair;         // the pair of blockIdx.y == 0 in this piece
};

// the planes of pair t; false for pair 0 of a call without `prev`
__device__ __forceinline__ bool pair_planes(const LinksArgs &a, int t, const int32_t *&E, const int32_t *&L)
{
    const size_t px = (size_t)a.h * a.w;
    L = a.labels + (size_t)t * px;
    E = t > 0 ? L - px : a.prev;
    return E != nullptr;
}

__global__ void __launch_bounds__(kLinkBlock)
links_count_kernel(LinksArgs a, int32_t *__restrict__ ncand)
{
    const int t = a.first_pair + blockIdx.y;
    const int32_t *E, *L;
    if (!pair_planes(a, t, E, L))
        return;
    const int px = a.h * a.w;
    const int p = blockIdx.x * kLinkBlock + threadIdx.x;
    bool cand = false;
    if (p < px)
        cand = va_links::is_candidate(E, L, a.w, p, p % a.w, va_links::key_at(E, L, p));
    const unsigned long long m = __ballot(cand);
    if (m && threadIdx.x % kWave == 0)
        atomicAdd(&ncand[t], __popcll(m));
}

// kNeed: in = candidates per pair; out = the exclusive scan of the table sizes, totals[1] = need and the flags
// go[kStore] = (need <= cap), go[kTables] = (the tables fit `slots` together).
// !kNeed: in = links per pair; out = their exclusive scan, totals[0] = the links of the batch.
template <bool kNeed>
__global__ void __launch_bounds__(kScanBlock)
links_scan_pairs_kernel(const int32_t *__restrict__ in, int n, int64_t cap, int64_t slots, int64_t *__restrict__ out,
                        int64_t *__restrict__ totals, int32_t *__restrict__ go)
{
    __shared__ int64_t wave_sums[kScanBlock / kWave];
    int64_t carry = 0, need = 0;
    for (int base = 0; base < n; base += kScanBlock) {
        const int t = base + threadIdx.x;
        const int64_t c = t < n ? in[t] : 0;
        int64_t sum, csum = 0;
        const int64_t excl = block_exclusive<0>(kNeed ? va_links::table_slots(c) : c, wave_sums, sum);
        if (kNeed)
            block_exclusive<0>(c, wave_sums, csum);
        if (t < n)
            out[t] = carry + excl;
        carry += sum;
        need += csum;
    }
    if (kNeed) {
        if (threadIdx.x == 0) {
            out[n] = carry;
            totals[1] = need;
            go[kStore] = need <= cap ? 1 : 0;
            go[kTables] = carry <= slots ? 1 : 0;
        }
    } else if (threadIdx.x == 0) {
        out[n] = carry;
        totals[0] = carry;
    }
}

__global__ void __launch_bounds__(kLinkBlock)
links_clear_kernel(Entry *__restrict__ table, const int64_t *__restrict__ tab_off, int n, const int32_t *__restrict__ go)
{
    if (!*go)
        return;
    Entry e;
    e.key = 0;
    e.count = 0;
    e.first = va_links::kNoPixel;
    const int64_t used = tab_off[n];
    for (int64_t s = (int64_t)blockIdx.x * kLinkBlock + threadIdx.x; s < used; s += (int64_t)gridDim.x * kLinkBlock)
        table[s] = e;
}

__global__ void __launch_bounds__(kLinkBlock)
links_accumulate_kernel(LinksArgs a, const int32_t *__restrict__ ncand, const int64_t *__restrict__ tab_off,
                        Entry *__restrict__ table, const int32_t *__restrict__ go)
{
    const int t = a.first_pair + blockIdx.y;
    const int32_t *E, *L;
    if (!*go || !pair_planes(a, t, E, L) || ncand[t] == 0)
        return;
    const int px = a.h * a.w;
    const int p = blockIdx.x * kLinkBlock + threadIdx.x;
    const int lane = threadIdx.x % kWave;
    const unsigned long long key = p < px ? va_links::key_at(E, L, p) : 0ull;
    // the lane in front holds the pixel to the left: its key, unless this lane starts a wave or a row
    const unsigned long long left = __shfl_up(key, 1, kWave);
    const bool head = key != 0 && (lane == 0 || p % a.w == 0 || left != key);
    // a run ends in front of the next head, the next pixel without a key, or the end of the wave
    const unsigned long long breaks = __ballot(head || key == 0);
    const unsigned long long above = lane == kWave - 1 ? 0ull : breaks >> (lane + 1);
    const int len = !head ? 0 : above ? __ffsll((long long)above) : kWave - lane;
    Entry *tab = table + tab_off[t];
    const uint32_t slots = (uint32_t)va_links::table_slots(ncand[t]);
    // The runs of a wave that share a key go in as one insert, for the first kMergedKeys keys of the wave: a large
    // region meets a large region in most waves it covers, and every insert of that key lands on one slot.  The
    // lowest lane of a key holds its first pixel.  (Whole waves get here: every return above is the workgroup's.)
    unsigned long long todo = __ballot(head);
    for (int round = 0; round < kMergedKeys && todo; round++) {
        const int leader = __ffsll((long long)todo) - 1;
        const bool mine = head && key == __shfl(key, leader, kWave);
        const int sum = wave_sum(mine ? len : 0);
        if (lane == leader)
            va_links::insert(tab, slots, key, sum, p);
        todo &= ~__ballot(mine);
    }
    if (head && ((todo >> lane) & 1))
        va_links::insert(tab, slots, key, len, p);
}

// the owner test of the lane's pixel: a candidate whose key has this pixel as its first; key and count come back
__device__ __forceinline__ bool links_owner(const LinksArgs &a, const int32_t *E, const int32_t *L, int p,
                                            const Entry *tab, uint32_t slots, unsigned long long &key, int32_t &count)
{
    if (p >= a.h * a.w)
        return false;
    key = va_links::key_at(E, L, p);
    if (!va_links::is_candidate(E, L, a.w, p, p % a.w, key))
        return false;
    const Entry *e = va_links::lookup(tab, slots, key);
    count = e->count;
    return e->first == p;
}

// kPlace = false: owners of the workgroup into block_cnt; true: block_cnt holds the exclusive scan inside the
// pair, pair_off the scan over the pairs, and every owner writes its record
template <bool kPlace>
__global__ void __launch_bounds__(kLinkBlock)
links_place_kernel(LinksArgs a, const int32_t *__restrict__ ncand, const int64_t *__restrict__ tab_off,
                   const Entry *__restrict__ table, const int32_t *__restrict__ go, int32_t *__restrict__ block_cnt,
                   const int64_t *__restrict__ pair_off, va_region_link *__restrict__ links, int64_t cap)
{
    __shared__ int wave_cnt[kLinkWaves];
    if (!*go)
        return;
    const int t = a.first_pair + blockIdx.y;
    const size_t cell = (size_t)t * gridDim.x + blockIdx.x;
    const int32_t *E, *L;
    const bool live = pair_planes(a, t, E, L) && ncand[t] != 0;       // (uniform over the workgroup)
    if (!live) {
        if (!kPlace && threadIdx.x == 0)
            block_cnt[cell] = 0;
        return;
    }
    const int p = blockIdx.x * kLinkBlock + threadIdx.x;
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    unsigned long long key = 0;
    int32_t count = 0;
    const bool own = links_owner(a, E, L, p, table + tab_off[t], (uint32_t)va_links::table_slots(ncand[t]), key, count);
    const unsigned long long m = __ballot(own);
    if (lane == 0)
        wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, all = 0;
    for (int k = 0; k < kLinkWaves; k++) {
        before += k < wave ? wave_cnt[k] : 0;
        all += wave_cnt[k];
    }
    if (!kPlace) {
        if (threadIdx.x == 0)
            block_cnt[cell] = all;
        return;
    }
    if (own) {
        const int64_t slot = pair_off[t] + block_cnt[cell] + before + __popcll(m & ((1ull << lane) - 1));
        if (slot < cap) {                       // (always: slot < total <= need <= cap)
            int4 rec;
            rec.x = t;
            rec.y = va_links::key_a(key);
            rec.z = va_links::key_b(key);
            rec.w = count;
            *reinterpret_cast<int4 *>(links + slot) = rec;
        }
    }
}

// the workgroup counts of one pair -> their exclusive scan, in place; nlinks[t] = their sum
__global__ void __launch_bounds__(kLinkBlock)
links_scan_blocks_kernel(int32_t *__restrict__ block_cnt, int blocks, int first_pair, const int32_t *__restrict__ go,
                         int32_t *__restrict__ nlinks)
{
    __shared__ int64_t wave_sums[kLinkWaves];
    if (!*go)
        return;
    const int t = first_pair + blockIdx.x;
    int32_t *cnt = block_cnt + (size_t)t * blocks;
    int64_t carry = 0;
    for (int base = 0; base < blocks; base += kLinkBlock) {
        const int k = base + threadIdx.x;
        int64_t sum;
        const int64_t excl = block_exclusive<0>(k < blocks ? (int64_t)cnt[k] : 0, wave_sums, sum);
        if (k < blocks)
            cnt[k] = (int32_t)(carry + excl);
        carry += sum;
    }
    if (threadIdx.x == 0)
        nlinks[t] = (int32_t)carry;
}

// the entry of a key read where the atomics of this launch wrote it: past the lane's first-level cache
__device__ __forceinline__ const Entry *lookup_written(Entry *tab, uint32_t slots, unsigned long long key)
{
    uint32_t s = va_links::first_slot(key, slots);
    while (__hip_atomic_load(&tab[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != key)
        s = va_links::next_slot(s, slots);
    return tab + s;
}

// The links per pair where the tables of all pairs do not fit the workspace together: workgroup g owns the region
// table + g * stride (stride: room for any pair) and walks the pairs g, g + gridDim.x, ...; per pair it clears the
// 2 c + 1 slots, inserts the runs as links_accumulate_kernel does, and counts the candidates that are their key's
// first pixel.  Barriers of the workgroup order the three steps; every branch around them is the workgroup's.
__global__ void __launch_bounds__(kSerialBlock)
links_count_serial_kernel(LinksArgs a, const int32_t *__restrict__ ncand, Entry *__restrict__ table, int64_t stride,
                          const int32_t *__restrict__ go, int32_t *__restrict__ nlinks)
{
    __shared__ int owners;
    if (go[kTables])
        return;
    const int px = a.h * a.w;
    const int tid = threadIdx.x, lane = tid % kWave;
    Entry *tab = table + (size_t)blockIdx.x * stride;
    for (int t = blockIdx.x; t < a.n; t += gridDim.x) {
        const int32_t *E, *L;
        const int c = ncand[t];
        if (!pair_planes(a, t, E, L) || c == 0) {
            if (tid == 0)
                nlinks[t] = 0;
            continue;
        }
        const uint32_t slots = (uint32_t)va_links::table_slots(c);
        Entry empty;
        empty.key = 0;
        empty.count = 0;
        empty.first = va_links::kNoPixel;
        for (uint32_t s = tid; s < slots; s += kSerialBlock)
            tab[s] = empty;
        if (tid == 0)
            owners = 0;
        __threadfence();
        __syncthreads();
        for (int base = 0; base < px; base += kSerialBlock) {
            const int p = base + tid;
            const unsigned long long key = p < px ? va_links::key_at(E, L, p) : 0ull;
            const unsigned long long left = __shfl_up(key, 1, kWave);
            const bool head = key != 0 && (lane == 0 || p % a.w == 0 || left != key);
            const unsigned long long breaks = __ballot(head || key == 0);
            if (head) {
                const unsigned long long above = lane == kWave - 1 ? 0ull : breaks >> (lane + 1);
                va_links::insert(tab, slots, key, above ? __ffsll((long long)above) : kWave - lane, p);
            }
        }
        __threadfence();
        __syncthreads();
        for (int base = 0; base < px; base += kSerialBlock) {
            const int p = base + tid;
            bool own = false;
            if (p < px) {
                const unsigned long long key = va_links::key_at(E, L, p);
                if (va_links::is_candidate(E, L, a.w, p, p % a.w, key)) {
                    Entry *e = const_cast<Entry *>(lookup_written(tab, slots, key));
                    own = __hip_atomic_load(&e->first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == p;
                }
            }
            const unsigned long long m = __ballot(own);
            if (m && lane == 0)
                atomicAdd(&owners, __popcll(m));
        }
        __syncthreads();
        if (tid == 0)
            nlinks[t] = owners;
        __syncthreads();                        // the next pair resets the counter and the region
    }
}

}  // namespace

}  // namespace va

using namespace va;

extern "C" {

size_t va_region_links_workspace_bytes(int n, int h, int w, int64_t cap_links)
{
    if (n <= 0 || h <= 0 || w <= 0 || cap_links < 0 || (size_t)h * (size_t)w >= kMaxFramePixels ||
        (int64_t)n * h * w >= ((int64_t)1 << 37))
        return 256;
    return links_layout(n, h, w, cap_links).total;
}

int va_region_links(const int32_t *prev, const int32_t *labels, int n, int h, int w, int32_t *nlinks, int64_t *totals,
                    va_region_link *links, int64_t cap_links, void *workspace, size_t workspace_bytes, void *stream)
{
    VA_ENTER();
    VA_REQUIRE(n >= 0 && h > 0 && w > 0, "va_region_links: bad shape (n %d, h %d, w %d)", n, h, w);
    VA_REQUIRE((size_t)h * (size_t)w < kMaxFramePixels, "va_region_links: frames above 2^29 pixels are not supported");
    VA_REQUIRE((int64_t)n * h * w < ((int64_t)1 << 37), "va_region_links: batches above 2^37 pixels are not supported");
    VA_REQUIRE(cap_links >= 0, "va_region_links: negative capacity (%lld links)", (long long)cap_links);
    VA_REQUIRE(totals && workspace && (n == 0 || (labels && nlinks)) && (cap_links == 0 || links),
               "va_region_links: NULL argument");
    VA_REQUIRE(aligned(totals, 8) && aligned(workspace, 16) && aligned(links, 16) && aligned(nlinks, 4) &&
                   aligned(labels, 4) && aligned(prev, 4),
               "va_region_links: records and workspace must be 16-byte aligned, totals 8-byte, labels 4-byte");
    VA_REQUIRE(workspace_bytes >= va_region_links_workspace_bytes(n, h, w, cap_links),
               "va_region_links: workspace of %zu bytes < required %zu", workspace_bytes,
               va_region_links_workspace_bytes(n, h, w, cap_links));
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        VA_HIP(hipMemsetAsync(totals, 0, 2 * sizeof(int64_t), st));
        return VA_OK;
    }
    const LinksLayout lay = links_layout(n, h, w, cap_links);
    int32_t *ncand = at<int32_t>(workspace, lay.ncand), *go = at<int32_t>(workspace, lay.go);
    int32_t *block_cnt = at<int32_t>(workspace, lay.block_cnt);
    int64_t *tab_off = at<int64_t>(workspace, lay.tab_off), *pair_off = at<int64_t>(workspace, lay.pair_off);
    Entry *table = at<Entry>(workspace, lay.table);
    const unsigned blocks = (unsigned)links_blocks(h, w);
    LinksArgs a = {prev, labels, n, h, w, 0};

    VA_HIP(hipMemsetAsync(ncand, 0, (size_t)n * sizeof(int32_t), st));
    for (a.first_pair = 0; a.first_pair < n; a.first_pair += kMaxGridYZ) {
        const unsigned pairs = (unsigned)(n - a.first_pair < kMaxGridYZ ? n - a.first_pair : kMaxGridYZ);
        hipLaunchKernelGGL(links_count_kernel, dim3(blocks, pairs), dim3(kLinkBlock), 0, st, a, ncand);
        VA_LAUNCH_CHECK("links_count_kernel");
    }
    // (a workspace with more room than asked for holds more tables side by side)
    const int64_t slots = (int64_t)((workspace_bytes - lay.table) / sizeof(Entry)), pair_slots = links_pair_slots(h, w);
    const int32_t *store = go + kStore, *tables = go + kTables;
    hipLaunchKernelGGL(links_scan_pairs_kernel<true>, dim3(1), dim3(kScanBlock), 0, st, ncand, n, cap_links, slots,
                       tab_off, totals, go);
    VA_LAUNCH_CHECK("links_scan_pairs_kernel");
    const int64_t clear_blocks = (slots + kLinkBlock - 1) / kLinkBlock;
    hipLaunchKernelGGL(links_clear_kernel, dim3((unsigned)(clear_blocks < kClearMaxGrid ? clear_blocks : kClearMaxGrid)),
                       dim3(kLinkBlock), 0, st, table, tab_off, n, tables);
    VA_LAUNCH_CHECK("links_clear_kernel");
    for (a.first_pair = 0; a.first_pair < n; a.first_pair += kMaxGridYZ) {
        const unsigned pairs = (unsigned)(n - a.first_pair < kMaxGridYZ ? n - a.first_pair : kMaxGridYZ);
        hipLaunchKernelGGL(links_accumulate_kernel, dim3(blocks, pairs), dim3(kLinkBlock), 0, st, a, ncand, tab_off,
                           table, tables);
        VA_LAUNCH_CHECK("links_accumulate_kernel");
    }
    for (a.first_pair = 0; a.first_pair < n; a.first_pair += kMaxGridYZ) {
        const unsigned pairs = (unsigned)(n - a.first_pair < kMaxGridYZ ? n - a.first_pair : kMaxGridYZ);
        hipLaunchKernelGGL(links_place_kernel<false>, dim3(blocks, pairs), dim3(kLinkBlock), 0, st, a, ncand, tab_off,
                           table, tables, block_cnt, pair_off, links, cap_links);
        VA_LAUNCH_CHECK("links_place_kernel<count>");
        hipLaunchKernelGGL(links_scan_blocks_kernel, dim3(pairs), dim3(kLinkBlock), 0, st, block_cnt, (int)blocks,
                           a.first_pair, tables, nlinks);
        VA_LAUNCH_CHECK("links_scan_blocks_kernel");
    }
    {   // (returns at once where the tables fit, as they do whenever need <= cap_links)
        const int64_t regions = slots / pair_slots;
        const int64_t grid = regions < n ? regions : n;
        a.first_pair = 0;
        hipLaunchKernelGGL(links_count_serial_kernel, dim3((unsigned)(grid < kSerialMaxGrid ? grid : kSerialMaxGrid)),
                           dim3(kSerialBlock), 0, st, a, ncand, table, pair_slots, go, nlinks);
        VA_LAUNCH_CHECK("links_count_serial_kernel");
    }
    hipLaunchKernelGGL(links_scan_pairs_kernel<false>, dim3(1), dim3(kScanBlock), 0, st, nlinks, n, cap_links, slots,
                       pair_off, totals, go);
    VA_LAUNCH_CHECK("links_scan_pairs_kernel");
    for (a.first_pair = 0; a.first_pair < n; a.first_pair += kMaxGridYZ) {
        const unsigned pairs = (unsigned)(n - a.first_pair < kMaxGridYZ ? n - a.first_pair : kMaxGridYZ);
        hipLaunchKernelGGL(links_place_kernel<true>, dim3(blocks, pairs), dim3(kLinkBlock), 0, st, a, ncand, tab_off,
                           table, store, block_cnt, pair_off, links, cap_links);
        VA_LAUNCH_CHECK("links_place_kernel<place>");
    }
    return VA_OK;
}

}  // extern "C"
