// small_queue_main.cpp - the small-call queue's submit loop (csrc/small_queue.hpp small_submit_core: leader / follower coalescing,
// futex words, requeue, linger) on the CPU with a stand-in for the GPU launch, built with -fsanitize=thread (and once more with
// address,undefined) by tests/test_small_queue_host.py.  Checks, under T concurrent callers of mixed kinds:
//   * every caller gets exactly the results of ITS OWN request (computed from its own bytes), or - for a launch that failed -
//     the launch's error code and message; nobody else's;
//   * nothing hangs (a watchdog aborts after 120 s: a lost wake-up would leave a caller asleep for ever);
//   * requests really travel together (fewer launches than requests), never beyond a launch's capacity, never two launches on
//     one lane at a time, never more lanes than allowed;
//   * the blob callers' challenge hashes (the persistent pool of host_only.hpp) are complete when the launch reads them.
// argv[4] > 0: every fourth pass of a caller through the submit loop stalls that many microseconds between reading its request's
// lane and reading the futex word it is about to sleep on (SMALL_QUEUE_TEST_HOOK_BETWEEN_LOADS) - the window in which a leader can
// take the request and move the queue's sleepers; a caller that then slept on the queue's word would never be woken once traffic
// stops (round-5 advisor finding).  argv[5]: watchdog seconds.  argv[6] = 1: the callers meet at a barrier before every call,
// so the queue goes IDLE after every burst of T calls and a caller left asleep on the wrong word stays asleep (continuous
// traffic would wake it by accident).  Without the re-read of r.lane in small_submit_core this mode hangs within a few bursts.
#include "small_queue_harness.hpp"

int main(int argc, char** argv) {
    const int T = argc > 1 ? atoi(argv[1]) : 64, CALLS = argc > 2 ? atoi(argv[2]) : 200, LANES = argc > 3 ? atoi(argv[3]) : 2;
    hook_delay_us = argc > 4 ? atol(argv[4]) : 0;
    const int WATCHDOG_S = argc > 5 ? atoi(argv[5]) : 120;
    const bool BURSTS = argc > 6 && atoi(argv[6]) != 0;
    Barrier barrier{(unsigned)T};
    SmallQueue Q;
    Q.max_lanes = (size_t)LANES;
    Q.rule[SmallReq::PROOFS].cap_items = 48;  // small capacities: launches fill up and leave requests behind (the `more` path)
    Q.rule[SmallReq::BLOBS].cap_items = 12;
    Harness H(LANES, WATCHDOG_S, 97, 13);
    // the stand-in launch: results are functions of the request's OWN bytes
    auto run = [&](int li, SmallLane&, std::vector<SmallReq*>& batch, size_t m, SmallReq::Kind kind, std::string& msg) -> KzgRet {
        const bool works = H.enter(li, batch, m, kind, msg);
        CHECK((kind == SmallReq::PROOFS || kind == SmallReq::BLOBS) && m <= Q.rule[kind].cap_items);
        std::this_thread::sleep_for(std::chrono::microseconds(150 + 2 * m));  // "1.7 ms whether it carries 1 or 200"
        for (SmallReq* x : batch) {
            if (works) standin_proofs_or_blobs(*x);
            if (x->hash) hostpool::finish(*x->hash);
        }
        H.leave(li);
        return works ? KZG_OK : KZG_ERROR;
    };
    std::atomic<uint64_t> done_calls{0}, error_calls{0};
    H.run_callers(T, [&](int t) {
        std::mt19937_64 rng(1234 + t);
        for (int k = 0; k < CALLS; k++) {
            if (BURSTS) barrier.wait();
            const bool blobs = t % 8 == 0;
            OldKindCall call(blobs, blobs ? 1 + rng() % 4 : 1 + rng() % 5, rng);
            const KzgRet rc = small_submit_core(Q, call.r, run);
            if (blobs) hostpool::finish(*call.r.hash);
            if (rc != KZG_OK) {
                CHECK(rc == KZG_ERROR && strcmp(call.r.msg, "injected failure") == 0);
                error_calls++;
            } else call.check();
            done_calls++;
            if (!BURSTS && (rng() & 7) == 0) std::this_thread::sleep_for(std::chrono::microseconds(rng() % 300));  // (not a pure closed loop)
        }
    });
    CHECK(done_calls.load() == (uint64_t)T * CALLS);
    H.check_idle(Q, done_calls.load());
    CHECK(Q.n_lanes >= 1);
    if (T >= 8) CHECK(H.launches.load() < done_calls.load());  // ... and they travelled together
    printf("threads %d calls %llu launches %llu (%.1f requests per launch, largest %llu items) failed launches %llu -> %llu calls saw the error; failures %d\n", T,
           (unsigned long long)done_calls.load(), (unsigned long long)H.launches.load(), (double)H.carried.load() / (double)H.launches.load(),
           (unsigned long long)Q.max_items, (unsigned long long)H.failed_launches.load(), (unsigned long long)error_calls.load(), failures.load());
    return H.exit_code(Q);
}
