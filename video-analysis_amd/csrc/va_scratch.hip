// va_scratch.hip -- device scratch of the stand-alone entry points: ScratchLease and its per-stream cache
//
// The contract:
//  * One lease per call, nothing shared between concurrent calls: the reference's concurrent callers
//    (VideoPreprocessor's worker threads, video/io/parallel.py:398-400) may use one stream each.
//  * A block is plain hipMalloc memory.  When the call returns, the block is cached under the call's stream,
//    and only a later call on that same stream may take it: the stream orders the kernels of the two calls,
//    and nothing else orders the reuse.  (Handing the block to hipFreeAsync instead made the next call of
//    the same size return a partly unwritten result)
//  * So a call touches a leased block in stream order only.  Before it writes one from the host -- a blocking
//    hipMemcpy runs on the null stream, which does not wait for a va_stream_create stream -- it synchronises
//    the stream: the previous call's kernels may still read the block (launch_resize's tables).
//  * Blocks are freed by va_trim; by va_stream_destroy for its stream, behind a synchronisation of it (a later
//    stream may get the same handle); and all of them, behind a device synchronisation, once more than
//    kScratchCacheCap bytes are cached or a hipMalloc fails.  Otherwise no lease synchronises anything.
//  * What a block holds when it is handed out is undefined.  Under va_test_hook_fill the whole block, fresh or
//    cached, is set to the fill byte on the lease's stream first (stream order: no synchronisation added).
#include <cstdlib>
#include <mutex>
#include <vector>

#include "va_common.h"

namespace va {
namespace {

int test_fill_from_env()                           // $VA_TEST_FILL: decimal 0..255, anything else is "off"
{
    const char *e = getenv("VA_TEST_FILL");
    if (!e || !*e)
        return -1;
    char *end = nullptr;
    long v = strtol(e, &end, 10);
    return (*end == 0 && v >= 0 && v <= 255) ? (int)v : -1;
}

}  // namespace

int g_test_fill = test_fill_from_env();

namespace {

struct ScratchBlock {
    void *ptr;
    size_t bytes;
    hipStream_t st;
};
std::mutex g_scratch_mu;
std::vector<ScratchBlock> g_scratch_free;
size_t g_scratch_cached = 0;
constexpr size_t kScratchCacheCap = 6ull << 30;

// frees the cached blocks of stream `only`, or all of them (only == nullptr); the caller holds the mutex
void release_locked(const hipStream_t *only = nullptr)
{
    size_t kept = 0;
    for (const ScratchBlock &b : g_scratch_free) {
        if (only && b.st != *only) {
            g_scratch_free[kept++] = b;
            continue;
        }
        (void)hipFree(b.ptr);
        g_scratch_cached -= b.bytes;
    }
    g_scratch_free.resize(kept);
}

}  // namespace

// the test fill of a block just handed out (the one branch the mode costs a lease when it is off)
static int fill_block(void *ptr, size_t bytes, hipStream_t st)
{
    if (g_test_fill < 0)
        return VA_OK;
    hipError_t e = hipMemsetAsync(ptr, g_test_fill, bytes, st);
    if (e != hipSuccess) {
        set_error("scratch: hipMemsetAsync(%zu) failed: %s", bytes, hipGetErrorString(e));
        return VA_ERR_HIP;
    }
    return VA_OK;
}

int ScratchLease::acquire(size_t need, hipStream_t stream)
{
    st = stream;
    need = need ? need : 256;
    {
        std::lock_guard<std::mutex> lock(g_scratch_mu);
        int best = -1;
        for (int i = 0; i < (int)g_scratch_free.size(); i++) {
            const ScratchBlock &b = g_scratch_free[i];
            if (b.st == st && b.bytes >= need && (best < 0 || b.bytes < g_scratch_free[best].bytes))
                best = i;
        }
        if (best >= 0 && g_scratch_free[best].bytes <= 2 * need + (1u << 20)) {
            ptr = g_scratch_free[best].ptr;
            bytes = g_scratch_free[best].bytes;
            g_scratch_cached -= bytes;
            g_scratch_free.erase(g_scratch_free.begin() + best);
            return fill_block(ptr, bytes, st);
        }
    }
    hipError_t e = hipMalloc(&ptr, need);
    if (e != hipSuccess) {                       // make room: drop what is cached, once
        (void)hipGetLastError();
        (void)hipDeviceSynchronize();
        scratch_release_cached(0);
        e = hipMalloc(&ptr, need);
    }
    if (e != hipSuccess) {
        ptr = nullptr;
        set_error("scratch: hipMalloc(%zu) failed: %s", need, hipGetErrorString(e));
        return VA_ERR_NOMEM;
    }
    bytes = need;
    return fill_block(ptr, bytes, st);
}

ScratchLease::~ScratchLease()
{
    if (!ptr)
        return;
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    if (g_scratch_cached + bytes > kScratchCacheCap) {
        (void)hipDeviceSynchronize();            // (nothing uses the blocks any more)
        release_locked();
    }
    g_scratch_free.push_back(ScratchBlock{ptr, bytes, st});
    g_scratch_cached += bytes;
}

void scratch_release_cached(size_t keep_bytes)     // (the caller has synchronised the device)
{
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    if (g_scratch_cached > keep_bytes)
        release_locked();
}

void scratch_purge_stream(hipStream_t st)          // (the caller has synchronised st)
{
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    release_locked(&st);
}

}  // namespace va
