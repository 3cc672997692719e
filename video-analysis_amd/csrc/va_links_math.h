// va_links_math.h -- the arithmetic of the region links ("Region links") that the kernels of
// va_links.hip and the host test tests/region_links_shim.cpp share: the key of a pixel pair, the candidate rule,
// the size of a pair's table, the hash, the probe sequence, and insert / lookup on one table.  On the device insert
// claims a slot with a compare-and-swap and accumulates with integer add and min, which commute: the entry of a key
// does not depend on the order of arrival (its slot does, and no slot position is ever output).  On the host the
// same text runs serially with plain stores.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define VA_LINKS_HD __host__ __device__ __forceinline__
#else
#define VA_LINKS_HD inline
#endif

namespace va_links {

// one slot of a pair's open-addressing table; key 0 = empty (a valid key has a >= 1 in its high word)
struct Entry {
    unsigned long long key;
    int32_t count;      // pixels with this key
    int32_t first;      // smallest raster index among them
};
static_assert(sizeof(Entry) == 16, "a table slot is 16 bytes");
constexpr int32_t kNoPixel = 0x7fffffff;     // `first` of an empty slot: above every pixel index (< 2^29)

// the key of a pixel whose earlier plane holds a and whose later plane holds b; 0 where either is background (<= 0)
VA_LINKS_HD unsigned long long pack_key(int32_t a, int32_t b)
{
    return (a >= 1 && b >= 1) ? ((unsigned long long)(uint32_t)a << 32) | (uint32_t)b : 0ull;
}
VA_LINKS_HD int32_t key_a(unsigned long long key) { return (int32_t)(key >> 32); }
VA_LINKS_HD int32_t key_b(unsigned long long key) { return (int32_t)(key & 0xffffffffull); }

// the key at raster index p of a pair of h x w planes
VA_LINKS_HD unsigned long long key_at(const int32_t *E, const int32_t *L, int64_t p) { return pack_key(E[p], L[p]); }

// a candidate: a pixel with a key whose left and upper neighbours carry another key or do not exist.  The first
// raster pixel of every key is one (both neighbours come earlier in raster order), so the candidates of a pair
// bound its links from above.
VA_LINKS_HD bool is_candidate(const int32_t *E, const int32_t *L, int w, int64_t p, int x, unsigned long long key)
{
    if (key == 0)
        return false;
    if (x > 0 && key_at(E, L, p - 1) == key)
        return false;
    return !(p >= w && key_at(E, L, p - w) == key);
}

// slots of the table of a pair with c candidates: load factor below one half, so a probe always ends
VA_LINKS_HD int64_t table_slots(int64_t c) { return c > 0 ? 2 * c + 1 : 0; }

// 64 -> 32 bits (the finaliser of MurmurHash3): keys with equal low bits spread
VA_LINKS_HD uint32_t hash_key(unsigned long long k)
{
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return (uint32_t)(k >> 32);
}
// probe sequence: a multiply-high reduction of the hash to 0 .. slots - 1, then the next slot, wrapping
VA_LINKS_HD uint32_t first_slot(unsigned long long key, uint32_t slots)
{
    return (uint32_t)(((unsigned long long)hash_key(key) * slots) >> 32);
}
VA_LINKS_HD uint32_t next_slot(uint32_t slot, uint32_t slots) { return slot + 1 == slots ? 0 : slot + 1; }

// `len` pixels of `key`, the first of them at raster index `first`, into the table
VA_LINKS_HD void insert(Entry *tab, uint32_t slots, unsigned long long key, int32_t len, int32_t first)
{
    for (uint32_t s = first_slot(key, slots);; s = next_slot(s, slots)) {
#if defined(__HIP_DEVICE_COMPILE__)
        const unsigned long long old = atomicCAS(&tab[s].key, 0ull, key);
        if (old == 0ull || old == key) {
            atomicAdd(&tab[s].count, len);
            atomicMin(&tab[s].first, first);
            return;
        }
#else
        if (tab[s].key == 0ull || tab[s].key == key) {
            tab[s].key = key;
            tab[s].count += len;
            tab[s].first = first < tab[s].first ? first : tab[s].first;
            return;
        }
#endif
    }
}

// the entry of a key that has been inserted
VA_LINKS_HD const Entry *lookup(const Entry *tab, uint32_t slots, unsigned long long key)
{
    uint32_t s = first_slot(key, slots);
    while (tab[s].key != key)
        s = next_slot(s, slots);
    return tab + s;
}

}  // namespace va_links
