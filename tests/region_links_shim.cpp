// A stand-alone host program around video-analysis_amd/csrc/va_links_math.h for tests/test_region_links_host.py: the
// region links of DESIGN.md §9, "Region links", computed serially with the header's key, candidate rule, table size,
// hash, probe sequence, insert and lookup, compiled with the host C++ compiler under -fsanitize=address,undefined.
// Runs are cut where the kernel cuts them: at a row start and every 64 pixels of the frame.  Every buffer here has
// exactly the size of what it holds, so an index beyond a plane or a table is reported.
// Input (stdin, binary): int32 n, h, w, has_prev; the prev plane (h * w int32) where has_prev; n * h * w int32 labels.
// Output (stdout, binary): int64 total, need; n int32 links per pair; total records of 4 int32 (frame, a, b, count).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "va_links_math.h"

static bool read_all(void *dst, size_t bytes) { return bytes == 0 || fread(dst, 1, bytes, stdin) == bytes; }

int main()
{
    int32_t head[4];
    if (!read_all(head, sizeof head))
        return 2;
    const int n = head[0], h = head[1], w = head[2];
    const int64_t px = (int64_t)h * w;
    std::vector<int32_t> prev(head[3] ? px : 0), labels((size_t)n * px);
    if (!read_all(prev.data(), prev.size() * 4) || !read_all(labels.data(), labels.size() * 4))
        return 2;
    std::vector<int32_t> nlinks(n, 0), records;
    int64_t need = 0;
    for (int t = 0; t < n; t++) {
        const int32_t *L = labels.data() + (size_t)t * px;
        const int32_t *E = t ? L - px : (head[3] ? prev.data() : nullptr);
        if (!E)
            continue;
        int64_t cand = 0;
        for (int64_t p = 0; p < px; p++)
            cand += va_links::is_candidate(E, L, w, p, (int)(p % w), va_links::key_at(E, L, p));
        need += cand;
        const uint32_t slots = (uint32_t)va_links::table_slots(cand);
        std::vector<va_links::Entry> table(slots, va_links::Entry{0ull, 0, va_links::kNoPixel});
        for (int64_t p = 0; p < px;) {
            const unsigned long long key = va_links::key_at(E, L, p);
            int64_t q = p + 1;
            while (q < px && q % w != 0 && q % 64 != 0 && va_links::key_at(E, L, q) == key)
                q++;
            if (key)
                va_links::insert(table.data(), slots, key, (int32_t)(q - p), (int32_t)p);
            p = q;
        }
        for (int64_t p = 0; p < px; p++) {
            const unsigned long long key = va_links::key_at(E, L, p);
            if (!va_links::is_candidate(E, L, w, p, (int)(p % w), key))
                continue;
            const va_links::Entry *e = va_links::lookup(table.data(), slots, key);
            if (e->first == p) {
                const int32_t rec[4] = {t, va_links::key_a(key), va_links::key_b(key), e->count};
                records.insert(records.end(), rec, rec + 4);
                nlinks[t]++;
            }
        }
    }
    const int64_t totals[2] = {(int64_t)records.size() / 4, need};
    fwrite(totals, sizeof totals, 1, stdout);
    if (!nlinks.empty())
        fwrite(nlinks.data(), 4, nlinks.size(), stdout);
    if (!records.empty())
        fwrite(records.data(), 4, records.size(), stdout);
    return 0;
}
