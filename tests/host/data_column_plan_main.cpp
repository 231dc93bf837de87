// Stand-alone check of kzg_rs_amd/csrc/data_column_plan.hpp (tests/test_data_columns_cpu.py builds it with g++ and
// -fsanitize=address,undefined and runs it): the plan of the uniform group and every term of both outputs against a brute-force
// restatement made from the layout alone, for small (S, m, m') with m' < m among them.
#include <cstdio>
#include <cstring>
#include <vector>

#include "data_column_plan.hpp"
using namespace kzg;

static int failures = 0;
#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            if (failures++ < 20) printf("FAIL line %d: %s\n", __LINE__, #c); \
        }                                                                 \
    } while (0)

// commitment of blob k = 48 bytes holding tag[k]: equal tags are equal commitments
static void one_case(const std::vector<uint32_t>& tag, const std::vector<uint64_t>& cols, const std::vector<uint32_t>& dead) {
    const uint32_t m = (uint32_t)tag.size();
    std::vector<uint8_t> cm(48 * (size_t)m);
    for (uint32_t k = 0; k < m; k++) memset(cm.data() + 48 * (size_t)k, (int)(tag[k] + 1), 48);
    CellGroupPlan P;
    data_column_plan(P, cm.data(), m, cols.data(), cols.size());
    // brute force: distinct tags in first-seen order, the slots = sidecars with a column below 128
    std::vector<uint32_t> uniq, ci(m), slots;
    for (uint32_t k = 0; k < m; k++) {
        uint32_t i = 0;
        while (i < uniq.size() && tag[uniq[i]] != tag[k]) i++;
        if (i == uniq.size()) uniq.push_back(k);
        ci[k] = i;
    }
    for (size_t j = 0; j < cols.size(); j++) {
        CHECK(P.kind[j] == (cols[j] >= 128 ? CELL_GROUP_BAD_INDEX : CELL_GROUP_GROUP));
        CHECK(P.off[j] == j * (size_t)m);
        if (cols[j] < 128) slots.push_back((uint32_t)j);
    }
    const uint32_t S = (uint32_t)slots.size(), mp = (uint32_t)uniq.size(), nG = S * m;
    CHECK(P.G == S && P.nG == nG && P.mtot == mp && P.max_ll == m && P.max_rl == m + mp + 64);
    CHECK(P.slot_batch == slots && P.uniq_entry == uniq && P.ci == ci);
    const uint32_t NP = data_column_points(S, m, mp), SKIP = data_column_skip_point(S, m, mp), NS = data_column_scalars(S, m, mp);
    CHECK(NP == S * m + mp + 65 && SKIP == NP - 1);
    CHECK(NP == cell_group_points(nG, mp) && SKIP == cell_group_skip_point(nG, mp));  // (the launch code sizes its buffers by these)
    CHECK(NS == 2 * S * m + S * mp + 64 * S);
    CHECK(P.idx.size() >= P.o_wstart + mp + 1 && P.idx.size() >= P.o_col_id + S && P.idx.size() >= P.o_wlist + m && P.idx.size() >= P.o_cstart + S + 1);
    if (failures) return;
    for (uint32_t g = 0; g <= S; g++) CHECK(P.idx[P.o_cstart + g] == g * m);
    for (uint32_t g = 0; g < S; g++) CHECK(P.idx[P.o_col_id + g] == cols[slots[g]]);
    // wlist: the cells of commitment i in ascending k, commitment after commitment
    uint32_t at = 0;
    for (uint32_t i = 0; i < mp; i++) {
        CHECK(P.idx[P.o_wstart + i] == at);
        for (uint32_t k = 0; k < m; k++)
            if (ci[k] == i) CHECK(P.idx[P.o_wlist + at++] == k);
    }
    CHECK(at == m && P.idx[P.o_wstart + mp] == m);
    // every term of both outputs, padding included
    const uint32_t max_terms = P.max_rl + 3;
    for (uint32_t g = 0; g < S; g++) {
        bool live = true;
        for (uint32_t d : dead) live = live && d != g;
        for (uint32_t o = 0; o < 2; o++)
            for (uint32_t t = 0; t < max_terms; t++) {
                const CellGroupTerm tm = data_column_term(o, t, g, S, m, mp, live);
                uint32_t point = SKIP, scalar = 0;
                if (live && t < m) point = g * m + t, scalar = o * nG + g * m + t;                            // proof t of the slot: r^t | r^t g_c
                else if (live && o && t < m + mp) point = nG + (t - m), scalar = 2 * nG + g * mp + (t - m);   // the SHARED row, the slot's weight
                else if (live && o && t < m + mp + 64) point = nG + mp + (t - m - mp), scalar = 2 * nG + S * mp + 64 * g + (t - m - mp);
                CHECK(tm.point == point && tm.scalar == scalar);
                CHECK(tm.point < NP && tm.scalar < NS);
                const bool pad = !live || (o == 0 ? t >= m : t >= m + mp + 64);
                CHECK(!pad || (tm.point == SKIP && tm.scalar == 0));
                CHECK(pad || tm.point != SKIP);
            }
    }
    // the uniform group is the general plan's lists for the expansion, with the commitment rows of slot 0 standing for every slot's
    std::vector<uint8_t> ecm;
    std::vector<uint64_t> eix;
    std::vector<size_t> sizes(cols.size(), m);
    for (size_t j = 0; j < cols.size(); j++) {
        ecm.insert(ecm.end(), cm.begin(), cm.end());
        eix.insert(eix.end(), m, cols[j]);
    }
    CellGroupPlan Q;
    cell_group_plan(Q, ecm.data(), eix.data(), sizes.data(), cols.size(), CELL_GROUP_MAX_CELLS);
    CHECK(Q.G == S && Q.nG == nG && Q.mtot == S * mp && Q.slot_batch == P.slot_batch);
    CHECK(S == 0 || (Q.max_rl == P.max_rl && Q.max_ll == P.max_ll));  // (without a slot nothing is launched and the general plan has no longest list)
    for (uint32_t g = 0; g < S && !failures; g++)
        for (uint32_t o = 0; o < 2; o++)
            for (uint32_t t = 0; t < Q.max_rl; t++) {
                const CellGroupTerm a = data_column_term(o, t, g, S, m, mp, true);
                const CellGroupTerm b = cell_group_term(o, t, g, Q.idx[Q.o_cstart + g], m, Q.idx[Q.o_ustart + g], mp, nG, Q.mtot, true);
                if (t < m) CHECK(a.point == b.point && a.scalar == b.scalar);                          // the proofs: the same rows
                else if (o && t < m + mp) CHECK(a.point + g * mp == b.point && a.scalar - 2 * nG == b.scalar - 2 * nG);  // row i of slot 0 for row g m' + i
                else if (o && t < m + mp + 64) CHECK(a.point - (nG + mp) == b.point - (nG + Q.mtot));  // the same monomial point
                for (uint32_t k = 0; k < m; k++) CHECK(Q.ci[g * m + k] == P.ci[k]);
            }
}

int main() {
    one_case({0}, {5}, {});                                  // S = 1, m = 1
    one_case({0, 1, 2}, {0, 64, 127}, {});                   // m' = m
    one_case({0, 1, 0, 2, 1, 0}, {3, 3, 77, 1, 9}, {2});     // m' = 3 < m = 6, a column twice, a slot masked out
    one_case({7, 7, 7, 7}, {127, 0}, {0, 1});                // m' = 1, every slot masked out
    one_case({0, 1, 2, 1, 3, 4}, {0, 200, 3, 128, 64}, {});  // two sidecars out of range: S = 3 of 5
    one_case({4, 4}, {500}, {});                             // no slot at all
    std::vector<uint32_t> big(256);
    for (uint32_t k = 0; k < 256; k++) big[k] = k % 200;     // m = 256 (the group's limit), m' = 200
    one_case(big, {1, 2}, {});
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("data_column_plan: ok\n");
    return 0;
}
