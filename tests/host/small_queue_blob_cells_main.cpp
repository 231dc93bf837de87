// small_queue_blob_cells_main.cpp - the small-call queue's BLOB_CELLS requests (csrc/small_queue.hpp SmallReq::BLOB_CELLS: one call of
// kzg_verify_blob_cell_kzg_proofs, 1 to KZG_BLOB_CELL_COALESCE_MAX_BLOBS blobs, coalesced into blob-cell groups of up to 64 blobs) on
// the CPU with a stand-in launch; built with -fsanitize=thread and once more with address,undefined by
// tests/test_small_queue_blob_cells_host.py.  Every call has seeded per-blob expected answers (0 false | 1 true | 2 refused); the
// stand-in echoes each blob's expected answer from the request's OWN bytes and records what every launch carried.  Checks, under T
// concurrent callers:
//   * every request gets exactly its own answers, its own message and its own return code - or the error of the launch that
//     carried it;
//   * no launch exceeds 64 blobs;
//   * a call above 16 blobs is never enqueued (the entry point's routing predicate, small_blob_cells_queued, sends it to the
//     stand-in of the locked path) and a queue with the kind switched off enqueues nothing;
//   * a request is carried exactly once;
//   * the owners' and the leader's challenges: every blob hashed exactly once;
//   * with one thread, every launch carries one call;
//   * the kind's counters agree with what the stand-in saw; nothing hangs (a watchdog aborts).
// usage: threads calls lanes [watchdog_s lane_stride on]
#include "small_queue_harness.hpp"

constexpr size_t BLOB = 96, PROOFS = 128;  // a small "blob" and its "cell proofs": the code paths without 137 KB per blob
// the stand-in for the per-blob challenge: a function of everything blob b of the request points at
static void blob_r(uint8_t out[32], const SmallReq& r, size_t b) {
    uint64_t h = 1469598103934665603ull;
    auto eat = [&](const uint8_t* p, size_t n) {
        for (size_t i = 0; i < n; i++) h = (h ^ p[i]) * 1099511628211ull;
    };
    eat(r.c + 48 * b, 48);
    eat(r.blobs + BLOB * b, BLOB);
    eat(r.p + PROOFS * b, PROOFS);
    for (int i = 0; i < 32; i++) out[i] = (uint8_t)(h >> (8 * (i & 7))) ^ (uint8_t)i;
}
static std::atomic<uint64_t> r_by_owner{0}, r_by_leader{0};
static bool hash_one(SmallReq& r, size_t b, std::atomic<uint64_t>& who) {
    if (!small_claim(r, b, [&](uint8_t* out) { blob_r(out, r, b); })) return false;
    who++;
    return true;
}
static bool wait_work(SmallReq& r) {
    for (size_t b = 0; b < r.n_chal; b++)
        if (hash_one(r, b, r_by_owner)) return true;
    return false;
}
static const char* const WHY[3] = {"a blob holds a field element >= r", "invalid proof (not a G1 point)", "invalid commitment (not a G1 point)"};

int main(int argc, char** argv) {
    const int T = argc > 1 ? atoi(argv[1]) : 16, CALLS = argc > 2 ? atoi(argv[2]) : 200, LANES = argc > 3 ? atoi(argv[3]) : 2;
    const int WATCHDOG_S = argc > 4 ? atoi(argv[4]) : 120;
    const int STRIDE = argc > 5 ? atoi(argv[5]) : 1;
    const bool ON = argc > 6 ? atoi(argv[6]) != 0 : true;
    SmallQueue Q;
    Q.max_lanes = (size_t)LANES;
    Q.cell_lane_stride = (size_t)STRIDE;
    Q.rule[SmallReq::BLOB_CELLS].on = ON;
    CHECK(Q.rule[SmallReq::BLOB_CELLS].cap_items == 64 && KZG_BLOB_CELL_COALESCE_MAX_BLOBS == 16);
    Harness H(LANES, WATCHDOG_S, 89, 17);
    std::atomic<uint64_t> carried_blobs{0}, locked_calls{0};
    std::mutex comp_mu;
    std::vector<std::vector<size_t>> compositions;  // the sizes of the requests of every launch, in order
    // what a blob's bytes say about it: blobs[0] = the expected answer, blobs[1] = which reason a refused blob carries
    auto echo = [&](SmallReq& x, const char** first_why) {
        for (size_t b = 0; b < x.n; b++) {
            const uint8_t e = x.blobs[BLOB * b];
            x.err[b] = e == 2;
            x.ok[b] = e == 1;
            if (e == 2 && !*first_why) *first_why = WHY[x.blobs[BLOB * b + 1] % 3];
        }
    };
    auto run = [&](int li, SmallLane&, std::vector<SmallReq*>& batch, size_t m, SmallReq::Kind kind, std::string& msg) -> KzgRet {
        const bool works = H.enter(li, batch, m, kind, msg);
        CHECK(li % STRIDE == 0 && kind == SmallReq::BLOB_CELLS && m <= 64);
        std::vector<size_t> comp;
        for (SmallReq* x : batch) {
            CHECK(x->n >= 1 && x->n <= KZG_BLOB_CELL_COALESCE_MAX_BLOBS);  // nothing above 16 blobs was ever enqueued
            comp.push_back(x->n);
        }
        if (T == 1) CHECK(batch.size() == 1);
        {
            std::lock_guard<std::mutex> lk(comp_mu);
            compositions.push_back(comp);
        }
        carried_blobs += m;
        std::this_thread::sleep_for(std::chrono::microseconds(200 + 4 * m));
        for (SmallReq* x : batch) {
            if (!works) break;  // (every request of it carries the error)
            // the leader collects the challenges: its own work for the blobs nobody has started, a short wait for the others
            for (size_t b = 0; b < x->n; b++)
                if (!hash_one(*x, b, r_by_leader)) small_await(*x, b);
            const char* why = nullptr;
            echo(*x, &why);
            if (why) snprintf(x->msg, sizeof x->msg, "%s", why);
        }
        H.leave(li);
        return works ? KZG_OK : KZG_ERROR;
    };
    std::atomic<uint64_t> done_calls{0}, queued_calls{0}, error_calls{0}, queued_blobs{0}, hashed_ok_blobs{0};
    H.run_callers(T, [&](int t) {
        std::mt19937_64 rng(9001 + 131 * t);
        for (int k = 0; k < CALLS; k++) {
            size_t n = 1 + rng() % 16;          // 1 to 16 blobs
            if (rng() % 23 == 0) n = 17 + rng() % 8;  // ... and now and then a call above the threshold
            std::vector<uint8_t> c(48 * n), p(PROOFS * n), bl(BLOB * n), expect(n);
            for (auto* v : {&c, &p, &bl})
                for (auto& x : *v) x = (uint8_t)rng();
            for (size_t b = 0; b < n; b++) {
                expect[b] = rng() % 11 == 0 ? 2 : (uint8_t)(rng() & 1);
                bl[BLOB * b] = expect[b];
            }
            std::vector<uint8_t> ok(n, 7), err(n, 7), r_be(32 * n);
            std::vector<std::atomic<int>> state(n);
            for (auto& s : state) s.store(0);
            SmallReq r;
            r.kind = SmallReq::BLOB_CELLS;
            r.n = n;
            r.blobs = bl.data();
            r.c = c.data();
            r.p = p.data();
            r.ok = reinterpret_cast<bool*>(ok.data());
            r.err = err.data();
            r.chal = r_be.data(), r.chal_state = state.data(), r.n_chal = n;
            r.wait_work = wait_work;
            const char* want_why = nullptr;
            for (size_t b = 0; b < n && !want_why; b++)
                if (expect[b] == 2) want_why = WHY[bl[BLOB * b + 1] % 3];
            if (!small_blob_cells_queued(Q, n)) {  // the locked path's stand-in: the queue never sees the call
                CHECK(n > KZG_BLOB_CELL_COALESCE_MAX_BLOBS || !ON);
                const char* why = nullptr;
                echo(r, &why);
                locked_calls++;
            } else {
                const KzgRet rc = small_submit_core(Q, r, run);
                CHECK(r.done.load());
                queued_calls++;
                queued_blobs += n;
                if (rc != KZG_OK) {
                    CHECK(rc == KZG_ERROR && strcmp(r.msg, "injected failure") == 0);
                    error_calls++;
                    done_calls++;
                    continue;
                }
                for (size_t b = 0; b < n; b++) {  // its own challenges, each computed once
                    uint8_t want[32];
                    blob_r(want, r, b);
                    CHECK(state[b].load() == 2 && memcmp(want, r_be.data() + 32 * b, 32) == 0);
                }
                hashed_ok_blobs += n;
                // the return code the entry point makes of it: without err_out, a refused blob is the caller's own BadArgs
                CHECK((want_why != nullptr) == (r.msg[0] != 0));
                if (want_why) CHECK(strcmp(r.msg, want_why) == 0);
            }
            for (size_t b = 0; b < n; b++) {
                CHECK(err[b] == (expect[b] == 2 ? 1 : 0));
                CHECK(ok[b] == (expect[b] == 1 ? 1 : 0));
            }
            done_calls++;
            if ((rng() & 7) == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 300));  // (not a pure closed loop)
        }
    });
    std::atomic<uint64_t> &launches = H.launches, &largest = H.largest;
    CHECK(done_calls.load() == (uint64_t)T * CALLS && queued_calls.load() + locked_calls.load() == done_calls.load());
    H.check_idle(Q, queued_calls.load());
    CHECK(carried_blobs.load() == queued_blobs.load());
    if (!ON) CHECK(launches.load() == 0 && queued_calls.load() == 0);
    if (ON) CHECK(locked_calls.load() > 0 || T * CALLS < 100);  // (calls above the threshold did occur)
    if (T == 1) CHECK(launches.load() == queued_calls.load() && largest.load() <= 1);
    if (T >= 8 && ON) CHECK(launches.load() < queued_calls.load() && largest.load() >= 2);  // ... and they travelled together
    for (const auto& comp : compositions) {
        size_t m = 0;
        for (size_t n : comp) m += n;
        CHECK(m <= 64);
    }
    CHECK(compositions.size() == launches.load());
    const SmallKindStats& st = Q.stats[SmallReq::BLOB_CELLS];
    CHECK(st.launches == launches.load() && st.requests == queued_calls.load() && st.items == queued_blobs.load() && st.max_requests == largest.load());
    CHECK(Q.stats[SmallReq::CELLS].launches == 0 && Q.stats[SmallReq::CELLS].requests == 0);
    // no challenge computed twice (a failed launch may leave some uncomputed)
    CHECK(r_by_owner.load() + r_by_leader.load() <= queued_blobs.load() && r_by_owner.load() + r_by_leader.load() >= hashed_ok_blobs.load());
    printf("threads %d calls %llu (%llu locked) launches %llu largest %llu requests, blobs %llu, r by owner %llu by leader %llu | "
           "failed launches %llu -> %llu calls saw the error; failures %d\n",
           T, (unsigned long long)done_calls.load(), (unsigned long long)locked_calls.load(), (unsigned long long)launches.load(),
           (unsigned long long)largest.load(), (unsigned long long)queued_blobs.load(), (unsigned long long)r_by_owner.load(),
           (unsigned long long)r_by_leader.load(), (unsigned long long)H.failed_launches.load(), (unsigned long long)error_calls.load(), failures.load());
    return H.exit_code(Q);
}
