// devbuf_check.cpp -- DevBuf<T> of csrc/device_mem.h on the CPU: a stand-alone program (its own main, no GPU, no HIP library).
// The buffer is instantiated with a counting allocator on malloc / free that can be told to fail its N-th request and records
// the live blocks; the two HIP calls the type makes besides allocating, and mmc_fail, are stubbed here.  Built with
// -fsanitize=address,undefined (tests/test_devbuf_host.py), so a double free or a use after free is fatal.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "../../mermaid_classifier_amd/csrc/device_mem.h"

static int g_fail_calls = 0, g_cleared = 0;
int mmc_fail(int code, const char*, ...) { ++g_fail_calls; return code; }
extern "C" hipError_t hipGetLastError(void) { ++g_cleared; return hipSuccess; }
extern "C" const char* hipGetErrorString(hipError_t) { return "stub"; }

struct CountingAlloc {
    static long requests, allocs, frees, live, max_live, fail_at;   // fail_at: the 1-based request that fails (0 = none)
    static size_t last_bytes;
    static hipError_t alloc(void** p, size_t bytes)
    {
        ++requests;
        last_bytes = bytes;
        if (requests == fail_at) { *p = nullptr; return hipErrorOutOfMemory; }
        *p = malloc(bytes);
        ++allocs; ++live;
        if (live > max_live) max_live = live;
        return hipSuccess;
    }
    static void release(void* p) { free(p); ++frees; --live; }
    static void fail_next() { fail_at = requests + 1; }
};
long CountingAlloc::requests = 0, CountingAlloc::allocs = 0, CountingAlloc::frees = 0, CountingAlloc::live = 0,
     CountingAlloc::max_live = 0, CountingAlloc::fail_at = 0;
size_t CountingAlloc::last_bytes = 0;

using A = CountingAlloc;
using Buf = DevBuf<float, A>;

static int g_checks = 0;
#define CHECK(cond)                                                          \
    do {                                                                     \
        ++g_checks;                                                          \
        if (!(cond)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static int reserve_keeps_and_grows_free_first()
{
    Buf b;
    CHECK(b.p == nullptr && b.cap == 0);
    CHECK(b.reserve(10) == 0);
    CHECK(b.p && b.cap == 10 && A::live == 1);
    CHECK(A::last_bytes == 10 * sizeof(float) + 256);   // the slack
    b.p[9] = 1.f;
    float* const p0 = b.p;
    const long req = A::requests;
    CHECK(b.reserve(10) == 0 && b.reserve(3) == 0 && b.reserve(0) == 0);
    CHECK(b.p == p0 && b.cap == 10 && A::requests == req);   // at or below cap: the pointer is kept, nothing is asked for
    A::max_live = A::live;
    CHECK(b.reserve(11) == 0);
    CHECK(b.cap == 11 && A::live == 1 && A::max_live == 1);   // never two live blocks for one buffer
    CHECK(A::last_bytes == 11 * sizeof(float) + 256);
    b.p[10] = 2.f;
    float* q = b;   // the implicit conversion readers use
    CHECK(q == b.p);
    Buf z;
    CHECK(z.alloc(0) && z.p && z.cap == 0 && A::last_bytes == 256);   // zero elements is never zero bytes
    return 0;
}

static int failure_leaves_it_empty()
{
    const long live0 = A::live;
    Buf b;
    CHECK(b.reserve(4) == 0);
    A::fail_next();
    const int fails = g_fail_calls;
    CHECK(b.reserve(8) == MMC_ERR_HIP && g_fail_calls == fails + 1);   // reported through HIP_TRY
    CHECK(b.p == nullptr && b.cap == 0 && A::live == live0);
    CHECK(b.reserve(8) == 0 && b.p && b.cap == 8);                     // and a later reserve succeeds
    b.p[7] = 3.f;
    A::fail_next();
    const int cleared = g_cleared;
    CHECK(!b.alloc(2) && g_fail_calls == fails + 1 && g_cleared == cleared + 1);   // alloc: not reported, sticky error cleared
    CHECK(b.p == nullptr && b.cap == 0 && A::live == live0);
    CHECK(b.alloc(2) && b.p && b.cap == 2 && A::live == live0 + 1);
    return 0;
}

// "build the new one, then replace", as the grow-and-move functions and the setters use it
static int replace(Buf& member, int64_t count, bool give_up, bool by_swap)
{
    Buf fresh;
    if (!fresh.alloc(count)) return MMC_ERR_NOMEM;
    fresh.p[count - 1] = 4.f;
    if (give_up) return MMC_ERR_HIP;   // (a copy into the new block failed)
    if (by_swap) member.swap(fresh);
    else member = std::move(fresh);
    return 0;
}

static int build_then_replace()
{
    const long live0 = A::live;
    Buf m;
    CHECK(m.reserve(5) == 0);
    m.p[4] = 5.f;
    float* const old = m.p;
    long frees = A::frees;
    CHECK(replace(m, 9, true, true) == MMC_ERR_HIP);
    CHECK(m.p == old && m.cap == 5 && m.p[4] == 5.f);           // abandoned: the old block is intact,
    CHECK(A::frees == frees + 1 && A::live == live0 + 1);       // the new one freed
    A::fail_next();
    CHECK(replace(m, 9, false, true) == MMC_ERR_NOMEM);
    CHECK(m.p == old && m.cap == 5 && A::frees == frees + 1 && A::live == live0 + 1);
    for (int by_swap = 0; by_swap < 2; ++by_swap) {
        frees = A::frees;
        CHECK(replace(m, 9 + by_swap, false, by_swap != 0) == 0);
        CHECK(m.cap == 9 + by_swap && m.p[m.cap - 1] == 4.f);
        CHECK(A::frees == frees + 1 && A::live == live0 + 1);   // completed: the old block freed exactly once
    }
    return 0;
}

static int moves_and_vectors()
{
    const long live0 = A::live, frees0 = A::frees;
    {
        Buf a;
        CHECK(a.reserve(3) == 0);
        float* const pa = a.p;
        Buf b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.p == pa && b.cap == 3 && A::live == live0 + 1);
        Buf c;
        CHECK(c.reserve(6) == 0 && A::live == live0 + 2);
        c = std::move(b);   // frees c's block, takes b's
        CHECK(c.p == pa && c.cap == 3 && b.p == nullptr && b.cap == 0 && A::live == live0 + 1);
        Buf& self = c;
        c = std::move(self);
        CHECK(c.p == pa && c.cap == 3 && A::live == live0 + 1);
    }
    CHECK(A::live == live0 && A::frees == frees0 + 2);
    {
        std::vector<Buf> v(3);
        for (int i = 0; i < 3; ++i) CHECK(v[i].reserve(i + 1) == 0);
        CHECK(A::live == live0 + 3);
        v.resize(40);   // reallocates the vector: the elements move
        CHECK(A::live == live0 + 3 && v[2].cap == 3 && v[39].p == nullptr);
        v[2].p[2] = 6.f;
        CHECK(v[39].reserve(2) == 0 && A::live == live0 + 4);
        v.resize(2);
        CHECK(A::live == live0 + 2);
        v.emplace_back();
        CHECK(v.back().alloc(7) && A::live == live0 + 3);
        v.clear();
        CHECK(A::live == live0);
        std::vector<Buf> w(2), x;
        CHECK(w[0].reserve(1) == 0 && w[1].reserve(1) == 0);
        x = std::move(w);
        CHECK(A::live == live0 + 2 && x.size() == 2);
    }
    CHECK(A::live == live0 && A::frees == frees0 + 2 + 5 + 2);
    return 0;
}

int main()
{
    if (reserve_keeps_and_grows_free_first() || failure_leaves_it_empty() || build_then_replace() || moves_and_vectors()) return 1;
    CHECK(A::live == 0 && A::allocs == A::frees && A::allocs > 0);
    printf("%d checks, %ld allocations, %ld frees\nall checks passed\n", g_checks, A::allocs, A::frees);
    return 0;
}
