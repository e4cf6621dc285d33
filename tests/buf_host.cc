// The owning buffer of the context (carparkingmaps_amd/csrc/cpm_buf.h) under a counting allocator that fails on request: a plain host
// program, built with the address and undefined-behaviour sanitizers by tests/test_buf_host.py.  Exit status 0: every check held.
#include <cstdio>
#include <cstdlib>

#include "cpm_buf.h"

namespace {

int g_allocs = 0, g_frees = 0, g_live = 0;
int g_fail_at = 0;  // the k-th call of alloc from now on fails (0: none)
size_t g_last_bytes = 0;

struct CountingAlloc {
    using error = int;
    static constexpr error ok = 0;
    static error alloc(void **p, size_t bytes)
    {
        ++g_allocs;
        if (g_fail_at > 0 && --g_fail_at == 0) return 2;  // (as hipErrorOutOfMemory: *p is left alone)
        *p = std::malloc(bytes);
        if (!*p) return 2;
        g_last_bytes = bytes;
        ++g_live;
        return ok;
    }
    static void free(void *p)
    {
        ++g_frees;
        --g_live;
        std::free(p);
    }
};
using Buf = cpm::Buf<double, CountingAlloc>;

int g_failed = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                     \
        }                                                                   \
    } while (0)

}  // namespace

int main()
{
    {
        Buf b;
        CHECK(b.p == nullptr && b.cap == 0 && b.get() == nullptr && !b.fits(0));
        CHECK(b.reserve(8) == 0 && b.p && b.cap == 8 && g_allocs == 1 && g_frees == 0 && g_last_bytes == 8 * sizeof(double));
        for (size_t i = 0; i < 8; ++i) b[i] = double(i);  // (every element is the buffer's: the sanitizer watches the ends)
        double *first = b;
        // a smaller or an equal size allocates nothing and keeps the pointer
        CHECK(b.reserve(8) == 0 && b.reserve(3) == 0 && b.reserve(0) == 0 && b.p == first && b.cap == 8 && g_allocs == 1 && g_frees == 0);
        // a grow frees exactly once and allocates exactly once
        CHECK(b.reserve(9) == 0 && b.cap == 9 && g_allocs == 2 && g_frees == 1 && g_live == 1);
        b[8] = 8.0;
        // a failed allocation leaves {nullptr, 0}; the next reserve succeeds
        g_fail_at = 1;
        CHECK(b.reserve(100) == 2 && b.p == nullptr && b.cap == 0 && g_allocs == 3 && g_frees == 2 && g_live == 0);
        CHECK(!b.fits(0));
        CHECK(b.reserve(4) == 0 && b.p && b.cap == 4 && g_allocs == 4 && g_frees == 2 && g_live == 1);
        // ... also when the failure meets an empty buffer
        Buf e;
        g_fail_at = 1;
        CHECK(e.reserve(1) == 2 && e.p == nullptr && e.cap == 0 && g_frees == 2);
        g_fail_at = 2;  // (the second call from here)
        CHECK(e.reserve(1) == 0 && e.cap == 1 && g_live == 2);
        CHECK(e.reserve(2) == 2 && e.p == nullptr && e.cap == 0 && g_live == 1);
    }
    CHECK(g_live == 0 && g_allocs == 7 && g_frees == 4);  // (b and nothing else was freed by a destructor: e was empty)
    {
        // reserve(0) yields a pointer that is not null, with room for one element
        Buf z;
        const int a0 = g_allocs;
        CHECK(z.reserve(0) == 0 && z.p != nullptr && z.cap == 1 && g_allocs == a0 + 1 && g_last_bytes == sizeof(double));
        z[0] = 1.0;
        CHECK(z.reserve(1) == 0 && g_allocs == a0 + 1);
    }
    {
        // destruction frees once; destruction after release() frees nothing
        const int f0 = g_frees;
        {
            Buf d;
            CHECK(d.reserve(5) == 0);
        }
        CHECK(g_frees == f0 + 1);
        {
            Buf r;
            CHECK(r.reserve(5) == 0);
            r.release();
            CHECK(g_frees == f0 + 2 && r.p == nullptr && r.cap == 0);
            r.release();  // (and a second release)
            CHECK(g_frees == f0 + 2);
        }
        CHECK(g_frees == f0 + 2);
    }
    {
        // swap trades the allocations: each is freed once, by its new owner
        const int f0 = g_frees;
        Buf x, y;
        CHECK(x.reserve(2) == 0 && y.reserve(7) == 0);
        double *px = x, *py = y;
        x.swap(y);
        CHECK(x.p == py && x.cap == 7 && y.p == px && y.cap == 2 && g_frees == f0);
        x[6] = 6.0;
        y.release();
        CHECK(g_frees == f0 + 1 && g_live == 1);
    }
    CHECK(g_live == 0 && g_allocs == g_frees + 3);  // (three allocations failed: nothing was handed out for them)
    if (g_failed) return 1;
    std::puts("buf_host: ok");
    return 0;
}
