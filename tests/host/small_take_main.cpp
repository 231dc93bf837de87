// small_take_main.cpp - the taking of a launch's requests off the small-call queue (csrc/small_queue.hpp small_take: one loop, the
// kinds' differences in SmallQueue::rule), case by case on hand-built queues: single-threaded and deterministic, built with
// -fsanitize=address,undefined by tests/test_small_take_host.py.  Per case: which requests leave (taken, with the lane set) and how
// many items, which stay - untouched and in their order - and the kind's counters.
#include "small_queue_harness.hpp"

#include <deque>
#include <initializer_list>
#include <utility>

using Kind = SmallReq::Kind;
struct Case {
    SmallQueue Q;
    std::deque<SmallReq> reqs;  // (a deque: the requests do not move)
    Case(std::initializer_list<std::pair<Kind, size_t>> queue) {
        for (const auto& kn : queue) {
            reqs.emplace_back();
            reqs.back().kind = kn.first;
            reqs.back().n = kn.second;
            Q.q.push_back(&reqs.back());
        }
    }
    // small_take(kind) on lane li takes exactly the requests at `want` (positions in the queue as built, oldest first)
    void take(int li, Kind kind, std::initializer_list<size_t> want, uint64_t launches_so_far = 0) {
        std::vector<SmallReq*> batch, expect, rest;
        batch.reserve(Q.q.size());
        size_t items = 0;
        for (size_t i = 0; i < reqs.size(); i++) {
            bool in = false;
            for (size_t w : want) in |= w == i;
            if (in) expect.push_back(&reqs[i]), items += reqs[i].n;
            else if (!reqs[i].taken.load()) rest.push_back(&reqs[i]);
        }
        const SmallKindStats before = Q.stats[kind];
        CHECK(before.launches == launches_so_far);
        const size_t m = small_take(Q, li, kind, batch);
        CHECK(m == items);
        CHECK(batch == expect);  // (the same requests, oldest first)
        for (SmallReq* x : expect) CHECK(x->kind == kind && x->taken.load() && x->lane.load() == li && !x->done.load());
        CHECK(std::vector<SmallReq*>(Q.q.begin(), Q.q.end()) == rest);  // the others keep their place and their order ...
        for (SmallReq* x : rest) CHECK(!x->taken.load() && x->lane.load() == -1 && !x->done.load());  // ... untouched
        const SmallKindStats& st = Q.stats[kind];
        CHECK(st.launches == before.launches + 1 && st.items == before.items + items);
        CHECK(st.max_requests == std::max<uint64_t>(before.max_requests, expect.size()));
        for (int k = 0; k < SmallReq::KINDS; k++)
            if (k != kind) CHECK(Q.stats[k].launches == 0 && Q.stats[k].items == 0 && Q.stats[k].max_requests == 0);
    }
};

int main() {
    const Kind PROOFS = SmallReq::PROOFS, BLOBS = SmallReq::BLOBS, CELLS = SmallReq::CELLS, BLOB_CELLS = SmallReq::BLOB_CELLS;
    {  // the defaults of the table
        SmallQueue Q;
        CHECK(Q.rule[PROOFS].cap_items == 1024 && Q.rule[PROOFS].cap_requests == SIZE_MAX && !Q.rule[PROOFS].in_order && !Q.rule[PROOFS].cell_lanes);
        CHECK(Q.rule[BLOBS].cap_items == 256 && Q.rule[BLOBS].cap_requests == SIZE_MAX && !Q.rule[BLOBS].in_order && !Q.rule[BLOBS].cell_lanes);
        CHECK(Q.rule[CELLS].cap_items == 128 * 256 && Q.rule[CELLS].cap_requests == 128 && Q.rule[CELLS].in_order && Q.rule[CELLS].cell_lanes);
        CHECK(Q.rule[BLOB_CELLS].cap_items == 64 && Q.rule[BLOB_CELLS].cap_requests == SIZE_MAX && Q.rule[BLOB_CELLS].in_order && Q.rule[BLOB_CELLS].cell_lanes);
        for (int k = 0; k < SmallReq::KINDS; k++) CHECK(Q.rule[k].on);
    }
    {  // PROOFS pack: the 500 does not fit and is passed over; the scan stops at m == cap
        Case c({{PROOFS, 600}, {PROOFS, 500}, {PROOFS, 400}, {PROOFS, 24}});
        c.take(1, PROOFS, {0, 2, 3});
        CHECK(c.Q.q.size() == 1 && c.Q.q.front()->n == 500);
        c.take(0, PROOFS, {1}, 1);  // ... and leaves with the next launch
        CHECK(c.Q.q.empty() && c.Q.stats[PROOFS].max_requests == 3);
    }
    {  // kinds interleaved: only PROOFS leaves, the others keep their relative order
        Case c({{BLOBS, 3}, {PROOFS, 1}, {CELLS, 7}, {PROOFS, 2}, {BLOBS, 1}, {CELLS, 2}, {PROOFS, 5}});
        c.take(0, PROOFS, {1, 3, 6});
        CHECK(c.Q.q.size() == 4 && c.Q.q[0] == &c.reqs[0] && c.Q.q[1] == &c.reqs[2] && c.Q.q[2] == &c.reqs[4] && c.Q.q[3] == &c.reqs[5]);
    }
    {  // BLOBS pack: 200 + 56 = the cap, where the scan stops (the 1 behind it stays)
        Case c({{BLOBS, 200}, {BLOBS, 100}, {BLOBS, 56}, {BLOBS, 1}});
        c.take(0, BLOBS, {0, 2});
        CHECK(c.Q.q.size() == 2 && c.Q.q[0]->n == 100 && c.Q.q[1]->n == 1);
    }
    {  // CELLS in order: the first misfit ends the launch, the 50 behind it stays although it would fit
        Case c({{CELLS, 200}, {CELLS, 150}, {CELLS, 50}});
        c.Q.rule[CELLS].cap_items = 300;
        c.take(0, CELLS, {0});
        CHECK(c.Q.q.size() == 2 && c.Q.q[0]->n == 150 && c.Q.q[1]->n == 50);
    }
    {  // CELLS: an oversize first request leaves, alone
        Case c({{CELLS, 200}, {CELLS, 50}});
        c.Q.rule[CELLS].cap_items = 100;
        c.take(2, CELLS, {0});
        CHECK(c.Q.q.size() == 1 && c.Q.q[0]->n == 50);
    }
    {  // CELLS: the limit in requests
        Case c({{CELLS, 1}, {CELLS, 1}, {CELLS, 1}});
        c.Q.rule[CELLS].cap_requests = 2;
        c.take(0, CELLS, {0, 1});
        CHECK(c.Q.q.size() == 1 && c.Q.stats[CELLS].max_requests == 2);
    }
    {  // BLOB_CELLS in order: 63 blobs, the 2 ends the launch and the 1 behind it stays
        Case c({{BLOB_CELLS, 16}, {BLOB_CELLS, 16}, {BLOB_CELLS, 16}, {BLOB_CELLS, 15}, {BLOB_CELLS, 2}, {BLOB_CELLS, 1}});
        c.take(0, BLOB_CELLS, {0, 1, 2, 3});
        CHECK(c.Q.stats[BLOB_CELLS].items == 63 && c.Q.q.size() == 2 && c.Q.q[0]->n == 2 && c.Q.q[1]->n == 1);
    }
    {  // the lanes of the cell kinds
        SmallQueue Q;
        Q.cell_lane_stride = 2;
        for (Kind k : {PROOFS, BLOBS, CELLS, BLOB_CELLS}) CHECK(small_lane_carries(Q, 0, k) && small_lane_carries(Q, 2, k));
        CHECK(small_lane_carries(Q, 1, PROOFS) && small_lane_carries(Q, 1, BLOBS));
        CHECK(!small_lane_carries(Q, 1, CELLS) && !small_lane_carries(Q, 1, BLOB_CELLS));
        Q.cell_lane_stride = 1;
        for (Kind k : {PROOFS, BLOBS, CELLS, BLOB_CELLS}) CHECK(small_lane_carries(Q, 1, k));
    }
    printf("small_take cases done; failures %d\n", failures.load());
    return failures ? 1 : 0;
}
