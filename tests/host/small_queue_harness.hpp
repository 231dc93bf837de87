// small_queue_harness.hpp - what the stand-alone programs that drive csrc/small_queue.hpp on the CPU share (small_queue_main.cpp,
// small_queue_cells_main.cpp, small_queue_blob_cells_main.cpp, small_take_main.cpp): CHECK, the stall hook of small_submit_core, a
// watchdog, the bookkeeping of a stand-in launch (one launch per lane at a time, launches / requests carried / the largest), the
// PROOFS and BLOBS stand-ins, and the invariants of a queue that has gone idle.  Includes small_queue.hpp itself.
#pragma once
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <mutex>
#include <random>
#include <thread>
#include <vector>

// every fourth pass of a caller through the submit loop stalls hook_delay_us (when > 0) between reading its request's lane and
// reading the futex word it is about to sleep on - the window in which a leader can take the request
static std::atomic<long> hook_delay_us{0};
static std::atomic<unsigned> hook_calls{0};
static void hook_between_loads();
#define SMALL_QUEUE_TEST_HOOK_BETWEEN_LOADS() hook_between_loads()
#define KZG_HOST_FE_PER_BLOB 64  // small "blobs" (2 KiB): the hashing pool's code paths without 128 KiB per request
#include "small_queue.hpp"

static void hook_between_loads() {
    const long d = hook_delay_us.load(std::memory_order_relaxed);
    if (d > 0 && (hook_calls.fetch_add(1, std::memory_order_relaxed) & 3) == 0) std::this_thread::sleep_for(std::chrono::microseconds(d));
}
static std::atomic<int> failures{0};
#define CHECK(x)                                                      \
    do {                                                              \
        if (!(x)) {                                                   \
            failures++;                                               \
            fprintf(stderr, "CHECK failed: %s (line %d)\n", #x, __LINE__); \
        }                                                             \
    } while (0)

static void raise_to(std::atomic<uint64_t>& most, uint64_t v) {
    uint64_t seen = most.load();
    while (seen < v && !most.compare_exchange_weak(seen, v)) {
    }
}
// the callers meet here before every call: the queue goes IDLE after every burst of T calls
struct Barrier {
    const unsigned T;
    std::atomic<unsigned> count{0}, gen{0};
    void wait() {
        const unsigned g = gen.load(std::memory_order_acquire);
        if (count.fetch_add(1, std::memory_order_acq_rel) + 1 == T) {
            count.store(0, std::memory_order_relaxed);
            gen.fetch_add(1, std::memory_order_release);
        } else {
            while (gen.load(std::memory_order_acquire) == g) std::this_thread::yield();
        }
    }
};

struct Harness {
    const int lanes, fail_every, fail_at;  // launch number nth fails when nth % fail_every == fail_at
    std::atomic<int> in_launch[SMALL_LANES_MAX];
    std::atomic<uint64_t> launches{0}, carried{0}, largest{0}, failed_launches{0};
    std::atomic<bool> finished{false};
    std::thread watchdog;
    Harness(int lanes, int watchdog_s, int fail_every, int fail_at) : lanes(lanes), fail_every(fail_every), fail_at(fail_at) {
        for (auto& x : in_launch) x = 0;
        watchdog = std::thread([this, watchdog_s] {
            for (int i = 0; i < 10 * watchdog_s && !finished; i++) std::this_thread::sleep_for(std::chrono::milliseconds(100));
            if (!finished) {
                fprintf(stderr, "WATCHDOG: callers still waiting after %d s - a lost wake-up\n", watchdog_s);
                abort();
            }
        });
    }
    // a stand-in launch begins: on a lane of its own, one kind, nobody's request twice, m the items of its requests.
    // false: this launch is to fail (msg is set; every request of it then carries the error)
    bool enter(int li, const std::vector<SmallReq*>& batch, size_t m, SmallReq::Kind kind, std::string& msg) {
        CHECK(li >= 0 && li < lanes);
        CHECK(in_launch[li].fetch_add(1) == 0);  // one launch per lane at a time
        size_t items = 0;
        for (SmallReq* x : batch) {
            CHECK(x->kind == kind);  // never two kinds in one launch
            CHECK(!x->done.load());  // ... and nobody's request twice
            items += x->n;
        }
        CHECK(items == m && !batch.empty());
        const uint64_t nth = launches.fetch_add(1);
        carried += batch.size();
        raise_to(largest, batch.size());
        if ((int)(nth % (uint64_t)fail_every) != fail_at) return true;
        msg = "injected failure";
        failed_launches++;
        return false;
    }
    void leave(int li) { CHECK(in_launch[li].fetch_sub(1) == 1); }
    template <class Caller>
    void run_callers(int T, Caller&& caller) {
        std::vector<std::thread> ths;
        for (int t = 0; t < T; t++) ths.emplace_back(caller, t);
        for (auto& th : ths) th.join();
        finished = true;
        watchdog.join();
    }
    // the queue at the end of a run: empty, no lane busy, no more lanes than allowed, its totals what the stand-in saw
    void check_idle(const SmallQueue& Q, uint64_t queued_calls) {
        CHECK(Q.q.empty());
        CHECK(Q.n_lanes <= (size_t)lanes);
        for (size_t i = 0; i < Q.n_lanes; i++) CHECK(!Q.lanes[i]->busy);
        CHECK(carried.load() == queued_calls);  // every request was carried by exactly one launch
        CHECK(Q.launches == launches.load() && Q.requests == queued_calls);
    }
    int exit_code(SmallQueue& Q) {
        for (size_t i = 0; i < Q.n_lanes; i++) delete Q.lanes[i];
        return failures ? 1 : 0;
    }
};

// ---- the PROOFS and BLOBS stand-ins: results are functions of the request's OWN bytes
static void standin_proofs_or_blobs(SmallReq& x) {
    if (x.kind == SmallReq::PROOFS) {
        for (size_t i = 0; i < x.n; i++) {
            x.ok[i] = ((x.c[48 * i] + x.z[32 * i]) & 1) != 0;
            x.err[i] = x.p[48 * i] == 0xff;
            x.general[i] = x.y[32 * i] == 0x7e;
        }
    } else {
        hostpool::finish(*x.hash);  // the challenges this launch needs
        uint8_t acc = 0;
        for (size_t i = 0; i < x.n; i++) acc ^= x.hash->z_le[32 * i];
        x.ok[0] = (acc & 1) != 0;
        x.err[0] = x.blobs[0] == 0xee;
        x.general[0] = 0;
    }
}
// a PROOFS or BLOBS request over random bytes of its own, and the check of what came back
struct OldKindCall {
    enum : size_t { BLOB = (size_t)32 * KZG_HOST_FE_PER_BLOB };
    const bool blobs;
    const size_t n;
    std::vector<uint8_t> c, p, z, y, bl, zle, ok, err, gen;
    SmallReq r;
    OldKindCall(bool blobs, size_t n, std::mt19937_64& rng)
        : blobs(blobs), n(n), c(48 * n), p(48 * n), z(32 * n), y(32 * n), bl(blobs ? BLOB * n : 0), zle(32 * n), ok(n, 2), err(n, 2), gen(n, 2) {
        for (auto* v : {&c, &p, &z, &y, &bl})
            for (auto& b : *v) b = (uint8_t)rng();
        r.kind = blobs ? SmallReq::BLOBS : SmallReq::PROOFS;
        r.n = n;
        r.c = c.data();
        r.p = p.data();
        r.z = z.data();
        r.y = y.data();
        r.ok = reinterpret_cast<bool*>(ok.data());
        r.err = err.data();
        r.general = gen.data();
        if (blobs) {
            r.blobs = bl.data();
            r.hash = hostpool::make(zle.data(), bl.data(), c.data(), n);
            hostpool::post(r.hash, 4);
        }
    }
    void check() {  // (after a launch that did not fail)
        if (blobs) {
            uint8_t acc = 0;
            for (size_t i = 0; i < n; i++) {
                uint8_t want[32];
                host_blob_challenge(want, bl.data() + BLOB * i, c.data() + 48 * i);
                CHECK(memcmp(want, zle.data() + 32 * i, 32) == 0);
                acc ^= want[0];
            }
            CHECK(ok[0] == (acc & 1) && err[0] == (bl[0] == 0xee) && gen[0] == 0);
        } else {
            for (size_t i = 0; i < n; i++) {
                CHECK(ok[i] == ((c[48 * i] + z[32 * i]) & 1));
                CHECK(err[i] == (p[48 * i] == 0xff));
                CHECK(gen[i] == (y[32 * i] == 0x7e));
            }
        }
    }
};
