// dev_buf_main.cpp - csrc/dev_buf.hpp (DevBuf / PinnedBuf, the owners of every device and pinned-host allocation) on the CPU:
// the four allocation calls are counting stand-ins over malloc / free, built with -fsanitize=address,undefined by
// tests/test_dev_buf_host.py (a double free, a leak or a use of a released block is the sanitizer's finding).  Checks:
//   * grow within the capacity allocates nothing; growth frees the old block BEFORE it allocates the new one;
//   * an allocation made to fail leaves an empty buffer of capacity 0, reports the error, and the next grow succeeds;
//   * a moved-from buffer frees nothing; a move assignment frees what the target held;
//   * every allocation is freed exactly once at scope exit, device and pinned calls never mixed.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <utility>
#include <vector>

enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
static std::vector<std::string> calls;   // "malloc" | "free" | "hostmalloc" | "hostfree", in order
static std::set<void*> live[2];          // device | pinned
static int fail_next = 0;                // the next n allocations fail
static int failures = 0;
#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            failures++;                                               \
            fprintf(stderr, "line %d: CHECK(%s)\n", __LINE__, #x);    \
        }                                                             \
    } while (0)
static hipError_t alloc_in(int kind, void** p, size_t n) {
    calls.push_back(kind ? "hostmalloc" : "malloc");
    if (fail_next > 0) {
        fail_next--;
        return hipErrorOutOfMemory;
    }
    *p = malloc(n ? n : 1);
    live[kind].insert(*p);
    return hipSuccess;
}
static hipError_t free_in(int kind, void* p) {
    calls.push_back(kind ? "hostfree" : "free");
    CHECK(live[kind].erase(p) == 1);  // allocated by the matching call, not freed before
    free(p);
    return hipSuccess;
}
static hipError_t hipMalloc(void** p, size_t n) { return alloc_in(0, p, n); }
static hipError_t hipFree(void* p) { return free_in(0, p); }
static hipError_t hipHostMalloc(void** p, size_t n) { return alloc_in(1, p, n); }
static hipError_t hipHostFree(void* p) { return free_in(1, p); }
#include "dev_buf.hpp"

static size_t count(const char* what) {
    size_t n = 0;
    for (auto& c : calls) n += c == what;
    return n;
}
struct Rec {
    unsigned w[12];
};
template <class BUF>
static void run(const char* m, const char* f) {
    calls.clear();
    {
        BUF a;
        CHECK(a.p == nullptr && a.cap == 0);
        CHECK(a.grow(0) == hipSuccess && calls.empty());  // nothing asked, nothing done
        CHECK(a.grow(100) == hipSuccess && a.p && a.cap == 100 && calls == std::vector<std::string>{m});
        a.p[99].w[11] = 7;  // the whole extent is there (sizeof(T) * n bytes)
        auto* p0 = a.p;
        CHECK(a.grow(100) == hipSuccess && a.grow(1) == hipSuccess && a.p == p0 && calls.size() == 1);  // within capacity: no call
        CHECK(a.grow(101) == hipSuccess && a.cap == 101);
        CHECK((calls == std::vector<std::string>{m, f, m}));  // growth: free first, then allocate
        fail_next = 1;
        CHECK(a.grow(500) == hipErrorOutOfMemory && a.p == nullptr && a.cap == 0);  // failed: empty, the old block is gone
        CHECK((calls == std::vector<std::string>{m, f, m, f, m}));
        CHECK(a.grow(5) == hipSuccess && a.cap == 5 && calls.size() == 6 && calls.back() == m);  // ... and usable again, nothing to free
        BUF b(std::move(a));
        CHECK(a.p == nullptr && a.cap == 0 && b.cap == 5 && calls.size() == 6);
        BUF c;
        CHECK(c.alloc(3) == hipSuccess && calls.size() == 7);
        c = std::move(b);  // frees c's block, takes b's
        CHECK(b.p == nullptr && c.cap == 5 && calls.size() == 8 && calls.back() == f);
        c.release();
        c.release();  // (idempotent)
        CHECK(c.p == nullptr && c.cap == 0 && calls.size() == 9);
        BUF d[2];
        for (auto& x : d) CHECK(x.alloc(8) == hipSuccess);
    }  // a, b, c are empty: only d's two blocks are freed here
    CHECK(calls.size() == 13 && count(m) == 7 && count(f) == 6 && fail_next == 0);  // seven requests, one of them refused: six blocks, six frees
    CHECK(live[0].empty() && live[1].empty());
}
int main() {
    run<DevBuf<Rec>>("malloc", "free");
    CHECK(count("hostmalloc") == 0 && count("hostfree") == 0);
    run<PinnedBuf<Rec>>("hostmalloc", "hostfree");
    CHECK(count("malloc") == 0 && count("free") == 0);
    printf("failures %d\n", failures);
    return failures != 0;
}
