// small_queue_cells_main.cpp - the small-call queue's third request kind (csrc/small_queue.hpp SmallReq::CELLS: one call of the
// cell-proof verifier, coalesced into group launches) on the CPU with a stand-in launch, beside requests of the two older kinds;
// built with -fsanitize=thread (and once more with address,undefined) by tests/test_small_queue_cells_host.py.  Checks, under T
// concurrent callers of all three kinds:
//   * every request is completed exactly once, with the results of ITS OWN bytes - its verdict, its BadArgs flag with its own
//     message, its own batch challenge (computed by the owner while it waited, or by the leader, never twice) - or with the
//     error of the launch that carried it;
//   * a launch never mixes kinds;
//   * a CELLS launch never exceeds either limit (requests, cells in all), and a request larger than the cell limit still
//     leaves, alone;
//   * CELLS launches only run on the lanes that may carry them (argv[7] = the lane stride of a multi-device handle);
//   * the per-kind counters agree with what the stand-in saw;
//   * nothing hangs (a watchdog aborts: a lost wake-up would leave a caller asleep for ever) - with argv[6] = 1 the callers meet
//     at a barrier before every call, so the queue goes IDLE after every burst, and with argv[4] > 0 a caller stalls between
//     reading its request's lane and the futex word it will sleep on (SMALL_QUEUE_TEST_HOOK_BETWEEN_LOADS).
// usage: threads calls lanes [stall_us watchdog_s bursts lane_stride]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <atomic>
#include <random>
#include <thread>
#include <vector>

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

constexpr size_t CELL = 64;  // a small "cell": the code paths without 2 KiB per cell
// the stand-in for the transcript hash: a function of everything the request points at
static void cell_r(uint8_t out[32], const SmallReq& r) {
    uint64_t h = 1469598103934665603ull;
    auto eat = [&](const uint8_t* p, size_t n) {
        for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 1099511628211ull;
    };
    eat(r.c, 48 * r.n);
    eat(reinterpret_cast<const uint8_t*>(r.cell_indices), 8 * r.n);
    eat(r.cells, CELL * r.n);
    eat(r.p, 48 * r.n);
    for (int i = 0; i < 32; i++) out[i] = (uint8_t)(h >> (8 * (i & 7))) ^ (uint8_t)i;
}
static std::atomic<uint64_t> r_by_owner{0}, r_by_leader{0};
static bool cell_wait_work(SmallReq& r) {
    int idle = 0;
    if (!r.r_state.compare_exchange_strong(idle, 1, std::memory_order_acq_rel)) return false;
    cell_r(r.r_be, r);
    r.r_state.store(2, std::memory_order_release);
    r_by_owner++;
    return true;
}

int main(int argc, char** argv) {
    const int T = argc > 1 ? atoi(argv[1]) : 64, CALLS = argc > 2 ? atoi(argv[2]) : 100, LANES = argc > 3 ? atoi(argv[3]) : 2;
    hook_delay_us = argc > 4 ? atol(argv[4]) : 0;
    const int WATCHDOG_S = argc > 5 ? atoi(argv[5]) : 120;
    const bool BURSTS = argc > 6 && atoi(argv[6]) != 0;
    const int STRIDE = argc > 7 ? atoi(argv[7]) : 1;
    std::atomic<unsigned> bar_count{0}, bar_gen{0};
    auto barrier = [&] {
        const unsigned g = bar_gen.load(std::memory_order_acquire);
        if (bar_count.fetch_add(1, std::memory_order_acq_rel) + 1 == (unsigned)T) {
            bar_count.store(0, std::memory_order_relaxed);
            bar_gen.fetch_add(1, std::memory_order_release);
        } else {
            while (bar_gen.load(std::memory_order_acquire) == g) std::this_thread::yield();
        }
    };
    const size_t BLOB = (size_t)32 * KZG_HOST_FE_PER_BLOB;
    SmallQueue Q;
    Q.max_lanes = (size_t)LANES;
    Q.cap_proofs = 48;  // small capacities: launches fill up and leave requests behind
    Q.cap_blobs = 12;
    Q.cap_cell_requests = 5;
    Q.cap_cells = 30;
    Q.cell_lane_stride = (size_t)STRIDE;
    constexpr size_t CELLS_OVERSIZE = 41;  // > cap_cells: leaves alone
    std::atomic<int> in_launch[SMALL_LANES_MAX];
    for (auto& x : in_launch) x = 0;
    std::atomic<uint64_t> launches{0}, carried{0}, failed_launches{0}, cell_launches{0}, cell_carried{0}, cell_cells{0}, cell_largest{0}, oversize_alone{0};
    std::atomic<bool> finished{false};
    std::thread watchdog([&] {
        for (int i = 0; i < 10 * WATCHDOG_S && !finished; i++) std::this_thread::sleep_for(std::chrono::milliseconds(100));
        if (!finished) {
            fprintf(stderr, "WATCHDOG: callers still waiting after %d s - a lost wake-up\n", WATCHDOG_S);
            abort();
        }
    });
    // the stand-in launch: results are functions of the request's OWN bytes
    auto run = [&](int li, SmallLane& L, std::vector<SmallReq*>& batch, size_t m, SmallReq::Kind kind, std::string& msg) -> KzgRet {
        CHECK(li >= 0 && li < LANES);
        CHECK(in_launch[li].fetch_add(1) == 0);  // one launch per lane at a time
        (void)L;
        size_t items = 0;
        for (SmallReq* x : batch) {
            CHECK(x->kind == kind);  // never two kinds in one launch
            CHECK(!x->done.load());  // ... and nobody's request twice
            items += x->n;
        }
        CHECK(items == m && !batch.empty());
        if (kind == SmallReq::CELLS) {
            CHECK(li % STRIDE == 0);
            CHECK(batch.size() <= Q.cap_cell_requests);
            CHECK(m <= Q.cap_cells || batch.size() == 1);
            if (m > Q.cap_cells) oversize_alone++;
            cell_launches++;
            cell_carried += batch.size();
            cell_cells += m;
            uint64_t seen = cell_largest.load();
            while (seen < batch.size() && !cell_largest.compare_exchange_weak(seen, batch.size())) {
            }
        } else {
            CHECK(m <= (kind == SmallReq::PROOFS ? Q.cap_proofs : Q.cap_blobs));
        }
        const uint64_t nth = launches.fetch_add(1);
        carried += batch.size();
        std::this_thread::sleep_for(std::chrono::microseconds(150 + 2 * m));
        KzgRet rc = KZG_OK;
        if (nth % 97 == 13) {  // a launch that fails: every request of it carries the error
            rc = KZG_ERROR;
            msg = "injected failure";
            failed_launches++;
        } else {
            for (SmallReq* x : batch) {
                if (kind == SmallReq::PROOFS) {
                    for (size_t i = 0; i < x->n; i++) {
                        x->ok[i] = ((x->c[48 * i] + x->z[32 * i]) & 1) != 0;
                        x->err[i] = x->p[48 * i] == 0xff;
                        x->general[i] = x->y[32 * i] == 0x7e;
                    }
                } else if (kind == SmallReq::BLOBS) {
                    hostpool::finish(*x->hash);  // the challenges this launch needs
                    uint8_t acc = 0;
                    for (size_t i = 0; i < x->n; i++) acc ^= x->hash->z_le[32 * i];
                    x->ok[0] = (acc & 1) != 0;
                    x->err[0] = x->blobs[0] == 0xee;
                    x->general[0] = 0;
                } else {
                    // the leader collects the challenges: its own work for the requests nobody has started, a short wait for the
                    // ones whose owners are at it
                    int idle = 0;
                    if (x->r_state.compare_exchange_strong(idle, 1, std::memory_order_acq_rel)) {
                        cell_r(x->r_be, *x);
                        x->r_state.store(2, std::memory_order_release);
                        r_by_leader++;
                    } else {
                        while (x->r_state.load(std::memory_order_acquire) != 2) std::this_thread::yield();
                    }
                    x->err[0] = x->c[0] == 0xff;
                    x->ok[0] = !x->err[0] && ((x->r_be[0] ^ x->cells[0]) & 1) != 0;
                    if (x->err[0]) snprintf(x->msg, sizeof x->msg, "bad request %02x%02x", x->p[0], x->p[1]);
                }
            }
        }
        for (SmallReq* x : batch)
            if (x->hash) hostpool::finish(*x->hash);
        CHECK(in_launch[li].fetch_sub(1) == 1);
        return rc;
    };
    std::atomic<uint64_t> done_calls{0}, error_calls{0}, cell_calls{0}, oversize_calls{0};
    auto caller = [&](int t) {
        std::mt19937_64 rng(4321 + t);
        for (int k = 0; k < CALLS; k++) {
            if (BURSTS) barrier();
            const bool cells = t % 2 == 0, blobs = !cells && t % 8 == 1;
            size_t n = cells ? 1 + rng() % 12 : blobs ? 1 + rng() % 4 : 1 + rng() % 5;
            if (cells && rng() % 29 == 0) n = CELLS_OVERSIZE;
            std::vector<uint8_t> c(48 * n), p(48 * n), z(32 * n), y(32 * n), bl(blobs ? BLOB * n : 0), zle(32 * n), ce(cells ? CELL * n : 0);
            std::vector<uint64_t> ix(n);
            for (auto* v : {&c, &p, &z, &y, &bl, &ce})
                for (auto& b : *v) b = (uint8_t)rng();
            for (auto& v : ix) v = rng() % 128;
            if (cells && rng() % 7 == 0) c[0] = 0xff;  // a request the launch refuses (its neighbours keep their verdicts)
            std::vector<uint8_t> ok(n, 2), err(n, 2), gen(n, 2);
            SmallReq r;
            r.kind = cells ? SmallReq::CELLS : blobs ? SmallReq::BLOBS : SmallReq::PROOFS;
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
            if (cells) {
                r.cells = ce.data();
                r.cell_indices = ix.data();
                r.wait_work = cell_wait_work;
            }
            const KzgRet rc = small_submit_core(Q, r, run);
            CHECK(r.done.load());
            if (blobs) hostpool::finish(*r.hash);
            if (rc != KZG_OK) {
                CHECK(rc == KZG_ERROR && strcmp(r.msg, "injected failure") == 0);
                error_calls++;
            } else if (cells) {
                uint8_t want[32];
                cell_r(want, r);
                CHECK(r.r_state.load() == 2 && memcmp(want, r.r_be, 32) == 0);
                const bool bad = c[0] == 0xff;
                CHECK(err[0] == (bad ? 1 : 0));
                CHECK(ok[0] == ((!bad && ((want[0] ^ ce[0]) & 1)) ? 1 : 0));
                if (bad) {
                    char m[64];
                    snprintf(m, sizeof m, "bad request %02x%02x", p[0], p[1]);
                    CHECK(strcmp(r.msg, m) == 0);
                }
            } else if (blobs) {
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
            if (cells) cell_calls++;
            if (cells && n == CELLS_OVERSIZE) oversize_calls++;
            done_calls++;
            if (!BURSTS && (rng() & 7) == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 300));  // (not a pure closed loop)
        }
    };
    std::vector<std::thread> ths;
    for (int t = 0; t < T; t++) ths.emplace_back(caller, t);
    for (auto& th : ths) th.join();
    finished = true;
    watchdog.join();
    CHECK(done_calls.load() == (uint64_t)T * CALLS);
    CHECK(Q.q.empty());
    CHECK(Q.n_lanes >= 1 && Q.n_lanes <= (size_t)LANES);
    for (size_t i = 0; i < Q.n_lanes; i++) CHECK(!Q.lanes[i]->busy);
    CHECK(carried.load() == done_calls.load());  // every request was carried by exactly one launch
    CHECK(cell_carried.load() == cell_calls.load());
    CHECK(oversize_alone.load() == oversize_calls.load());
    if (T >= 8) CHECK(launches.load() < done_calls.load() && cell_launches.load() < cell_calls.load());  // ... and they travelled together
    CHECK(Q.launches == launches.load() && Q.requests == done_calls.load());
    CHECK(Q.cell_launches == cell_launches.load() && Q.cell_requests == cell_calls.load() && Q.cell_items == cell_cells.load() &&
          Q.cell_max_requests == cell_largest.load());
    CHECK(r_by_owner.load() + r_by_leader.load() <= cell_calls.load());  // no challenge computed twice (a failed launch may leave one uncomputed)
    CHECK(r_by_owner.load() + r_by_leader.load() + error_calls.load() >= cell_calls.load());
    printf("threads %d calls %llu launches %llu | cells: calls %llu launches %llu largest %llu requests, %llu oversize alone, r by owner %llu by leader %llu | "
           "failed launches %llu -> %llu calls saw the error; failures %d\n",
           T, (unsigned long long)done_calls.load(), (unsigned long long)launches.load(), (unsigned long long)cell_calls.load(),
           (unsigned long long)cell_launches.load(), (unsigned long long)cell_largest.load(), (unsigned long long)oversize_alone.load(),
           (unsigned long long)r_by_owner.load(), (unsigned long long)r_by_leader.load(), (unsigned long long)failed_launches.load(),
           (unsigned long long)error_calls.load(), failures.load());
    for (size_t i = 0; i < Q.n_lanes; i++) delete Q.lanes[i];
    return failures ? 1 : 0;
}
