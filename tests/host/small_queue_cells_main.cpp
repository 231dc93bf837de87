// small_queue_cells_main.cpp - the small-call queue's CELLS requests (csrc/small_queue.hpp SmallReq::CELLS: one call of the
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
#include "small_queue_harness.hpp"

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
static bool cell_hash(SmallReq& r, std::atomic<uint64_t>& who) {
    if (!small_claim(r, 0, [&](uint8_t* out) { cell_r(out, r); })) return false;
    who++;
    return true;
}
static bool cell_wait_work(SmallReq& r) { return cell_hash(r, r_by_owner); }

int main(int argc, char** argv) {
    const int T = argc > 1 ? atoi(argv[1]) : 64, CALLS = argc > 2 ? atoi(argv[2]) : 100, LANES = argc > 3 ? atoi(argv[3]) : 2;
    hook_delay_us = argc > 4 ? atol(argv[4]) : 0;
    const int WATCHDOG_S = argc > 5 ? atoi(argv[5]) : 120;
    const bool BURSTS = argc > 6 && atoi(argv[6]) != 0;
    const int STRIDE = argc > 7 ? atoi(argv[7]) : 1;
    Barrier barrier{(unsigned)T};
    SmallQueue Q;
    Q.max_lanes = (size_t)LANES;
    Q.rule[SmallReq::PROOFS].cap_items = 48;  // small capacities: launches fill up and leave requests behind
    Q.rule[SmallReq::BLOBS].cap_items = 12;
    Q.rule[SmallReq::CELLS].cap_requests = 5;
    Q.rule[SmallReq::CELLS].cap_items = 30;
    const SmallKindRule& cell_rule = Q.rule[SmallReq::CELLS];
    Q.cell_lane_stride = (size_t)STRIDE;
    constexpr size_t CELLS_OVERSIZE = 41;  // > the CELLS cap_items: leaves alone
    Harness H(LANES, WATCHDOG_S, 97, 13);
    std::atomic<uint64_t> cell_launches{0}, cell_carried{0}, cell_cells{0}, cell_largest{0}, oversize_alone{0};
    // the stand-in launch: results are functions of the request's OWN bytes
    auto run = [&](int li, SmallLane&, std::vector<SmallReq*>& batch, size_t m, SmallReq::Kind kind, std::string& msg) -> KzgRet {
        const bool works = H.enter(li, batch, m, kind, msg);
        if (kind == SmallReq::CELLS) {
            CHECK(li % STRIDE == 0);
            CHECK(batch.size() <= cell_rule.cap_requests);
            CHECK(m <= cell_rule.cap_items || batch.size() == 1);
            if (m > cell_rule.cap_items) oversize_alone++;
            cell_launches++;
            cell_carried += batch.size();
            cell_cells += m;
            raise_to(cell_largest, batch.size());
        } else {
            CHECK((kind == SmallReq::PROOFS || kind == SmallReq::BLOBS) && m <= Q.rule[kind].cap_items);
        }
        std::this_thread::sleep_for(std::chrono::microseconds(150 + 2 * m));
        for (SmallReq* x : batch) {
            if (works && kind != SmallReq::CELLS) standin_proofs_or_blobs(*x);
            else if (works) {
                // the leader collects the challenges: its own work for the requests nobody has started, a short wait for the
                // ones whose owners are at it
                if (!cell_hash(*x, r_by_leader)) small_await(*x, 0);
                x->err[0] = x->c[0] == 0xff;
                x->ok[0] = !x->err[0] && ((x->chal[0] ^ x->cells[0]) & 1) != 0;
                if (x->err[0]) snprintf(x->msg, sizeof x->msg, "bad request %02x%02x", x->p[0], x->p[1]);
            }
            if (x->hash) hostpool::finish(*x->hash);
        }
        H.leave(li);
        return works ? KZG_OK : KZG_ERROR;
    };
    std::atomic<uint64_t> done_calls{0}, error_calls{0}, cell_calls{0}, oversize_calls{0};
    H.run_callers(T, [&](int t) {
        std::mt19937_64 rng(4321 + t);
        for (int k = 0; k < CALLS; k++) {
            if (BURSTS) barrier.wait();
            const bool cells = t % 2 == 0, blobs = !cells && t % 8 == 1;
            size_t n = cells ? 1 + rng() % 12 : blobs ? 1 + rng() % 4 : 1 + rng() % 5;
            if (cells && rng() % 29 == 0) n = CELLS_OVERSIZE;
            OldKindCall call(blobs, n, rng);  // (a CELLS request: c, p and the result buffers of a PROOFS one)
            SmallReq& r = call.r;
            std::vector<uint8_t> ce(cells ? CELL * n : 0);
            std::vector<uint64_t> ix(n);
            for (auto& b : ce) b = (uint8_t)rng();
            for (auto& v : ix) v = rng() % 128;
            if (cells && rng() % 7 == 0) call.c[0] = 0xff;  // a request the launch refuses (its neighbours keep their verdicts)
            uint8_t r_be[32];
            std::atomic<int> r_state{0};
            if (cells) {
                r.kind = SmallReq::CELLS;
                r.cells = ce.data();
                r.cell_indices = ix.data();
                r.chal = r_be, r.chal_state = &r_state, r.n_chal = 1;
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
                CHECK(r_state.load() == 2 && memcmp(want, r_be, 32) == 0);
                const bool bad = call.c[0] == 0xff;
                CHECK(call.err[0] == (bad ? 1 : 0));
                CHECK(call.ok[0] == ((!bad && ((want[0] ^ ce[0]) & 1)) ? 1 : 0));
                if (bad) {
                    char m[64];
                    snprintf(m, sizeof m, "bad request %02x%02x", call.p[0], call.p[1]);
                    CHECK(strcmp(r.msg, m) == 0);
                }
            } else call.check();
            if (cells) cell_calls++;
            if (cells && n == CELLS_OVERSIZE) oversize_calls++;
            done_calls++;
            if (!BURSTS && (rng() & 7) == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 300));  // (not a pure closed loop)
        }
    });
    CHECK(done_calls.load() == (uint64_t)T * CALLS);
    H.check_idle(Q, done_calls.load());
    CHECK(Q.n_lanes >= 1);
    CHECK(cell_carried.load() == cell_calls.load());
    CHECK(oversize_alone.load() == oversize_calls.load());
    if (T >= 8) CHECK(H.launches.load() < done_calls.load() && cell_launches.load() < cell_calls.load());  // ... and they travelled together
    const SmallKindStats& st = Q.stats[SmallReq::CELLS];
    CHECK(st.launches == cell_launches.load() && st.requests == cell_calls.load() && st.items == cell_cells.load() && st.max_requests == cell_largest.load());
    CHECK(r_by_owner.load() + r_by_leader.load() <= cell_calls.load());  // no challenge computed twice (a failed launch may leave one uncomputed)
    CHECK(r_by_owner.load() + r_by_leader.load() + error_calls.load() >= cell_calls.load());
    printf("threads %d calls %llu launches %llu | cells: calls %llu launches %llu largest %llu requests, %llu oversize alone, r by owner %llu by leader %llu | "
           "failed launches %llu -> %llu calls saw the error; failures %d\n",
           T, (unsigned long long)done_calls.load(), (unsigned long long)H.launches.load(), (unsigned long long)cell_calls.load(),
           (unsigned long long)cell_launches.load(), (unsigned long long)cell_largest.load(), (unsigned long long)oversize_alone.load(),
           (unsigned long long)r_by_owner.load(), (unsigned long long)r_by_leader.load(), (unsigned long long)H.failed_launches.load(),
           (unsigned long long)error_calls.load(), failures.load());
    return H.exit_code(Q);
}
