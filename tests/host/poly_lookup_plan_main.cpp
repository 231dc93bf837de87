// Host program over kzg_rs_amd/csrc/poly_lookup_plan.hpp (tests/test_poly_lookup_plan_cpu.py): the limits, the words, the plan of a call
// given by its shapes, and `run`: the three kernels of poly_lookup_kernels.hpp on the CPU exactly as they compose the bodies - lm_insert
// per table row, lm_probe and lm_count_found per (lookup, row) with the addition to the found row's counter, lm_store per row - over a
// workspace of evaluations the test writes, with the lanes of every launch taken in a given order (forward, reverse, a fixed shuffle):
// the result must not depend on it.  `full`: the walks over a slot array this program fills itself, which no call can produce.
// The outputs are compared with tests/poly_lookup_model.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "poly_lookup_plan.hpp"

using namespace kzg;

static bool read_element(FILE* f, LmQuad* two) {  // 64 hex digits -> the 32 bytes as they lie in the workspace
    char buf[80];
    if (fscanf(f, "%79s", buf) != 1 || strlen(buf) != 64) return false;
    uint8_t b[32];
    for (int i = 0; i < 32; i++) {
        unsigned v = 0;
        if (sscanf(buf + 2 * i, "%2x", &v) != 1) return false;
        b[i] = (uint8_t)v;
    }
    memcpy(two, b, 32);
    return true;
}

// the lanes 0 .. count - 1 of a launch in the order `order`: 0 forward, 1 reverse, 2 a fixed shuffle (an LCG's Fisher-Yates)
static std::vector<uint32_t> lanes(size_t count, int order) {
    std::vector<uint32_t> v(count);
    for (size_t k = 0; k < count; k++) v[k] = (uint32_t)(order == 1 ? count - 1 - k : k);
    if (order == 2) {
        uint64_t x = 0x2545F4914F6CDD1Dull;
        for (size_t k = count; k > 1; k--) {
            x = x * 6364136223846793005ull + 1442695040888963407ull;
            const size_t j = (size_t)((x >> 33) % k);
            const uint32_t t = v[k - 1];
            v[k - 1] = v[j], v[j] = t;
        }
    }
    return v;
}

struct Call {
    LmPlan pl;
    std::vector<LmQuad> ws;  // [U][n] elements of two quads
    size_t n_polys;
};

// "n width n_lookups n_polys", the table's and the lookups' polynomial indices (all of set 0), then n_polys rows of n evaluations
static int read_call(const char* path, Call& c, bool& refused) {
    FILE* f = fopen(path, "r");
    if (!f) return printf("no input\n"), 1;
    size_t n = 0, width = 0, n_lookups = 0;
    if (fscanf(f, "%zu %zu %zu %zu", &n, &width, &n_lookups, &c.n_polys) != 4) return printf("bad head\n"), 1;
    std::vector<uint32_t> names(2 * width * (1 + n_lookups) + 2, 0);
    for (size_t k = 0; k < width * (1 + n_lookups); k++)
        if (fscanf(f, "%u", &names[2 * k + 1]) != 1) return printf("bad column\n"), 1;
    const size_t set_coeffs[1] = {n}, set_polys[1] = {c.n_polys};
    const LmRefusal bad = lm_plan(c.pl, set_coeffs, set_polys, 1, names.data(), names.data() + 2 * width, width, n_lookups, n);
    refused = bad != LM_OK;
    if (refused) return printf("refused %d\n", (int)bad), fclose(f), 0;
    std::vector<LmQuad> all(2 * c.n_polys * n);
    for (size_t k = 0; k < c.n_polys * n; k++)
        if (!read_element(f, &all[2 * k])) return printf("bad evaluation\n"), 1;
    fclose(f);
    c.ws.assign(2 * c.pl.U * n, LmQuad{{0, 0, 0, 0}});  // the deduplicated rows, as the pad and the transforms leave them
    for (size_t u = 0; u < c.pl.U; u++) memcpy(&c.ws[2 * u * n], &all[2 * (size_t)c.pl.ref[u].poly * n], 32 * n);
    return 0;
}

// run FILE hash_bits order
static int run(const char* path, long hash_bits, int order) {
    Call c;
    bool refused = false;
    if (int rc = read_call(path, c, refused)) return rc;
    if (refused) return 0;
    const LmPlan& pl = c.pl;
    const uint32_t n = (uint32_t)pl.n, C = (uint32_t)pl.C, mask = lm_hash_mask(hash_bits);
    // the workspace behind the rows, by the plan's layout, and the memsets
    if (lm_ws_slots_at(pl) != 32 * pl.U * pl.n || lm_ws_counters_at(pl) != lm_ws_slots_at(pl) + 4 * pl.C || lm_ws_miss_at(pl) != lm_ws_counters_at(pl) + 4 * pl.n ||
        lm_workspace_bytes(pl) != lm_ws_miss_at(pl) + 4)
        return printf("the workspace layout\n"), 1;
    std::vector<uint32_t> slots(C, LM_EMPTY), counters(n, 0u);
    uint32_t first_miss = LM_EMPTY, flag = 0;
    // k_lm_insert
    const PqGrid gr = lm_grid_rows(pl), gc = lm_grid_count(pl);
    std::vector<int> ran(n, 0);
    for (uint32_t lane : lanes((size_t)gr.x * LM_THREADS, order)) {
        if (lane >= n) continue;
        flag |= lm_insert(c.ws.data(), pl.table, slots.data(), n, C, mask, lane);
        ran[lane]++;
    }
    for (int r : ran)
        if (r != 1) return printf("a table row is not inserted exactly once\n"), 1;
    size_t taken = 0;
    for (uint32_t v : slots) taken += v != LM_EMPTY;
    // k_lm_count: grid (x, lookups)
    for (uint32_t lane : lanes((size_t)gc.x * LM_THREADS * gc.y, order)) {
        const uint32_t l = lane / (gc.x * (uint32_t)LM_THREADS), i = lane % (gc.x * (uint32_t)LM_THREADS);
        if (i >= n) continue;
        const uint32_t row = lm_probe(c.ws.data(), pl.table, slots.data(), n, C, mask, l, i);
        if (lm_count_found(row, &first_miss, &flag, n, l, i)) LmAtomics::add(&counters.at(row), 1u);
    }
    // k_lm_store
    std::vector<LmQuad> out(2 * (size_t)n);
    for (uint32_t lane : lanes((size_t)gr.x * LM_THREADS, order))
        if (lane < n) lm_store(out.data(), lane, counters[lane]);
    printf("flag %u miss %u taken %zu starts", flag, first_miss, taken);
    for (uint32_t j = 0; j < n; j++) printf(" %u", lm_start_slot(lm_hash(c.ws.data(), n, pl.table.trow, pl.table.width, j), mask, C));
    printf("\n");
    for (uint32_t j = 0; j < n; j++) {
        uint8_t b[32];
        memcpy(b, &out[2 * (size_t)j], 32);
        for (int k = 0; k < 32; k++) printf("%02x", b[k]);
        printf("\n");
    }
    return 0;
}

// full FILE: every slot taken by table row 0 before the launches - the insert of a row with another tuple and the probe of a tuple that is
// not row 0's must end at the walk bound with LM_WALK_BIT, and a slot that holds neither LM_EMPTY nor a row must end a walk at once
static int full(const char* path) {
    Call c;
    bool refused = false;
    if (int rc = read_call(path, c, refused)) return rc;
    if (refused) return 0;
    const LmPlan& pl = c.pl;
    const uint32_t n = (uint32_t)pl.n, C = (uint32_t)pl.C, mask = lm_hash_mask(32);
    std::vector<uint32_t> slots(C, 0u);
    uint32_t first_miss = LM_EMPTY;
    for (uint32_t j = 0; j < n; j++) printf("%u ", lm_insert(c.ws.data(), pl.table, slots.data(), n, C, mask, j));
    printf("\n");
    for (uint32_t v : slots)
        if (v != 0u) return printf("a full slot array was written\n"), 1;
    for (uint32_t i = 0; pl.lookups && i < n; i++) {
        uint32_t flag = 0;
        const uint32_t row = lm_probe(c.ws.data(), pl.table, slots.data(), n, C, mask, 0, i);
        const bool found = lm_count_found(row, &first_miss, &flag, n, 0, i);
        printf("%s%u:%u ", found ? "row" : row == LM_WALKED ? "walked" : "miss", found ? row : 0u, flag);
    }
    printf("\nmiss %u\n", first_miss);
    std::fill(slots.begin(), slots.end(), n);  // no row
    printf("%u %u\n", lm_insert(c.ws.data(), pl.table, slots.data(), n, C, mask, n - 1),
           pl.lookups ? (unsigned)(lm_probe(c.ws.data(), pl.table, slots.data(), n, C, mask, 0, 0) == LM_WALKED) : 1u);
    return 0;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "limits") {
        printf("%zu %zu %zu %zu %zu %u %u %zu %zu\n", LM_MAX_WIDTH, LM_MAX_LOOKUPS, LM_MAX_SETS, LM_MAX_REFS, LM_THREADS, LM_EMPTY, LM_WALK_BIT, PA_MAX_SCALARS, FRNTT_MAX);
        return 0;
    }
    if (cmd == "words") {
        for (int r = LM_OK; r <= LM_MISSING; r++) printf("%d %s\n", r, lm_refusal_words((LmRefusal)r));
        return 0;
    }
    if (cmd == "gpwords") {  // the grand product's, which the rule for the sets' lengths reuses
        for (int r = GP_OK; r <= GP_DEN_VANISHES; r++) printf("%d %s\n", r, gp_refusal_words((GpRefusal)r));
        return 0;
    }
    if (cmd == "mask" && argc == 3) {
        printf("%u\n", lm_hash_mask(atol(argv[2])));
        return 0;
    }
    // plan n_sets width n_lookups domain_n null_mask check_polys, then per set "n_coeffs n_polys", then the (set, poly) pairs of the
    // table and the lookups.  null_mask: 1 set_coeffs, 2 table, 4 lookups are passed as null pointers
    if (cmd == "plan" && argc >= 8) {
        size_t a[4];
        for (int i = 0; i < 4; i++) a[i] = strtoull(argv[2 + i], nullptr, 10);
        const int null_mask = atoi(argv[6]), check_polys = atoi(argv[7]);
        const size_t n_sets = a[0], width = a[1], n_lookups = a[2];
        int at = 8;
        std::vector<size_t> set_coeffs(n_sets + 1, 0), set_polys(n_sets + 1, 0);
        for (size_t k = 0; k < n_sets; k++) {
            if (at + 1 >= argc) return 2;
            set_coeffs[k] = strtoull(argv[at++], nullptr, 10), set_polys[k] = strtoull(argv[at++], nullptr, 10);
        }
        std::vector<uint32_t> names;
        while (at < argc) names.push_back((uint32_t)strtoul(argv[at++], nullptr, 10));
        const size_t tw = 2 * (width <= LM_MAX_WIDTH ? width : 0);
        names.resize(tw + 2 * (width <= LM_MAX_WIDTH && n_lookups <= LM_MAX_LOOKUPS ? width * n_lookups : 0) + 2, 0);
        std::unique_ptr<LmPlan> pl(new LmPlan());
        const LmRefusal bad = lm_plan(*pl, null_mask & 1 ? nullptr : set_coeffs.data(), check_polys ? set_polys.data() : nullptr, n_sets, null_mask & 2 ? nullptr : names.data(),
                                      null_mask & 4 ? nullptr : names.data() + tw, width, n_lookups, a[3]);
        printf("%d\n", (int)bad);
        if (bad == LM_OK) {
            printf("%zu %zu %zu %zu %u %u %u %u %u %zu %zu %zu %d\n", pl->U, pl->workspace, pl->C, lm_workspace_bytes(*pl), lm_grid_rows(*pl).x, lm_grid_count(*pl).x,
                   lm_grid_count(*pl).y, lm_grid_pad(*pl).x, lm_grid_pad(*pl).y, lm_ntt_chunk(*pl, pl->U), lm_ntt_chunks(*pl, pl->U), lm_args_bytes(*pl), pl->logn);
            for (size_t u = 0; u < pl->U; u++) printf("%u:%u ", pl->ref[u].set, pl->ref[u].poly);
            printf("\n");
            for (size_t k = 0; k < width; k++) printf("%u ", pl->table.trow[k]);
            for (size_t l = 0; l < n_lookups; l++)
                for (size_t k = 0; k < width; k++) printf("%u ", pl->table.lrow[l][k]);
            printf("\n");
        }
        return 0;
    }
    if (cmd == "run" && argc == 5) return run(argv[2], atol(argv[3]), atoi(argv[4]));
    if (cmd == "full" && argc == 3) return full(argv[2]);
    fprintf(stderr, "usage: limits | words | gpwords | mask k | plan ... | run FILE hash_bits order | full FILE\n");
    return 2;
}
