// Host program over kzg_rs_amd/csrc/poly_blind_plan.hpp (tests/test_poly_blind_plan_cpu.py): the limits, the words, the plan of a call
// given by its shapes, the root, and `run`: the table of prepared blinders and every row of the new set on the CPU exactly as the kernels
// of poly_blind_kernels.hpp compose them - pb_beta per table entry, then per workgroup, lane and round the element pb_elem names, moved
// where pb_patched says it lies outside the row's patch and made by pb_element where it lies inside - on the inputs of a file the test
// writes, whose outputs the test compares with tests/poly_blind_model.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "poly_blind_plan.hpp"

using namespace kzg;

static void print_fr(const Fr& a) {  // plain value, big-endian hex
    uint8_t b[32];
    FrF::to_be_bytes(b, a);
    for (int i = 0; i < 32; i++) printf("%02x", b[i]);
    printf("\n");
}
static bool read_fr(FILE* f, Fr& out) {  // 64 hex digits
    char buf[80];
    if (fscanf(f, "%79s", buf) != 1 || strlen(buf) != 64) return false;
    uint8_t b[32];
    for (int i = 0; i < 32; i++) {
        unsigned v = 0;
        if (sscanf(buf + 2 * i, "%2x", &v) != 1) return false;
        b[i] = (uint8_t)v;
    }
    out = FrF::from_be_bytes(b);
    return true;
}

// run FILE: "pieces n c count k has_rotate" (n: any length, see below), count rotate bytes when has_rotate, the blinders, then count rows of c coefficients
static int run(const char* path) {
    FILE* f = fopen(path, "r");
    if (!f) return printf("no input\n"), 1;
    int pieces = 0, has_rotate = 0;
    size_t n = 0, c = 0, count = 0, k = 0;
    if (fscanf(f, "%d %zu %zu %zu %zu %d", &pieces, &n, &c, &count, &k, &has_rotate) != 6) return printf("bad head\n"), 1;
    PbPlan pl{};
    // a domain that is no power of two is planned as the next one and moved: the bodies take any n (no rotation then: no root)
    const bool free_n = n && frntt_log2(n) < 0;
    if (free_n && has_rotate) return printf("a rotation needs a power of two\n"), 1;
    const PbRefusal bad = pb_plan(pl, c, count, 0, count, free_n ? pa_pow2_at_least(n) : n, k, pieces != 0);
    if (bad == PB_OK && free_n) pl.n = n, pl.out_coeffs = c > n + pl.k ? c : n + pl.k;
    if (bad != PB_OK) {
        printf("refused %d\n", (int)bad);
        fclose(f);
        return 0;
    }
    std::vector<uint8_t> rotate(count, 0);
    for (size_t j = 0; has_rotate && j < count; j++) {
        unsigned v = 0;
        if (fscanf(f, "%u", &v) != 1) return printf("bad rotate\n"), 1;
        rotate[j] = (uint8_t)v;
    }
    std::vector<Fr> blinders(pb_blinders(pl));
    for (Fr& b : blinders)
        if (!read_fr(f, b)) return printf("bad blinder\n"), 1;
    std::vector<std::vector<Fr>> src(count, std::vector<Fr>(c));
    for (auto& row : src)
        for (Fr& x : row)
            if (!read_fr(f, x)) return printf("bad coefficient\n"), 1;
    fclose(f);
    // k_blind_prepare: a lane per entry
    uint32_t flag = 0;
    std::vector<Fr> beta(pl.table);
    const PqGrid gp = pb_grid_prepare(pl);
    std::vector<int> made(pl.table, 0);
    for (size_t w = 0; w < gp.x; w++)
        for (size_t t = 0; t < PB_PREPARE_THREADS; t++) {
            const size_t e = w * PB_PREPARE_THREADS + t;
            if (e >= pl.table) continue;
            beta[e] = pb_beta([&](size_t q) { return blinders.at(q); }, has_rotate ? rotate.data() : nullptr, count, pl.k, pl.logn, pl.pieces, e, flag);
            made[e]++;
        }
    for (int m : made)
        if (m != 1) return printf("a table entry is not made exactly once\n"), 1;
    // k_poly_blind: every workgroup of the grid
    const PqGrid g = pb_grid(pl);
    std::vector<std::vector<Fr>> out(count, std::vector<Fr>(pl.out_coeffs));
    std::vector<std::vector<int>> written(count, std::vector<int>(pl.out_coeffs, 0));
    for (size_t j = 0; j < g.y; j++) {
        const PbPatch patch = pb_patch(pl.pieces, pl.k, j);
        if ((size_t)patch.lo + patch.k > pl.table || (size_t)patch.hi + patch.k > pl.table) return printf("a patch runs past the table\n"), 1;
        for (size_t w = 0; w < g.x; w++)
            for (size_t t = 0; t < PB_THREADS; t++)
                for (size_t u = 0; u < PB_PER_LANE; u++) {
                    const size_t i = pb_elem(w, t, u);
                    if (i >= pl.out_coeffs) continue;
                    if (pb_patched(patch.k, pl.n, i))
                        out[j][i] = pb_element([&](size_t at) { return src[j].at(at); }, beta.data(), patch, pl.c, pl.n, i);
                    else
                        out[j][i] = i < pl.c ? src[j][i] : FrF::zero();
                    written[j][i]++;
                }
    }
    printf("flag %u out_coeffs %zu\n", flag, pl.out_coeffs);
    for (size_t j = 0; j < count; j++)
        for (size_t i = 0; i < pl.out_coeffs; i++) {
            if (written[j][i] != 1) return printf("an element is not written exactly once\n"), 1;
            if (!(flag & PB_BAD_BLINDER) && FrF::geq_mod(out[j][i])) return printf("not canonical\n"), 1;
            print_fr(out[j][i]);
        }
    return 0;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "limits") {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %u\n", PB_MAX_BLINDERS, PB_THREADS, PB_PER_LANE, PB_TILE, PB_PREPARE_THREADS, PA_MAX_COEFFS, PA_MAX_SCALARS, FRNTT_MAX,
               PB_BAD_BLINDER);
        return 0;
    }
    if (cmd == "words") {
        for (int r = PB_OK; r <= PB_BLINDER_RANGE; r++) printf("%d %s\n", r, pb_refusal_words((PbRefusal)r));
        return 0;
    }
    if (cmd == "omega" && argc == 3) {
        print_fr(FrF::from_mont(pb_omega(atoi(argv[2]))));
        return 0;
    }
    if (cmd == "plan" && argc == 9) {  // plan n_coeffs n_polys first count domain_n n_blinders pieces
        size_t a[6];
        for (int i = 0; i < 6; i++) a[i] = strtoull(argv[2 + i], nullptr, 10);
        PbPlan pl{};
        const PbRefusal bad = pb_plan(pl, a[0], a[1], a[2], a[3], a[4], a[5], atoi(argv[8]) != 0);
        printf("%d\n", (int)bad);
        if (bad == PB_OK) {
            printf("%zu %u %u %zu %u %zu %zu %zu %zu %d\n", pl.out_coeffs, pb_grid(pl).x, pb_grid(pl).y, pl.table, pb_grid_prepare(pl).x, pl.k, pb_blinders(pl), pb_args_rotate_at(pl),
                   pb_args_bytes(pl), pl.logn);
            const PbPatch first = pb_patch(pl.pieces, pl.k, 0), last = pb_patch(pl.pieces, pl.k, pl.count - 1);
            printf("%u %u %u %u %u %u\n", first.lo, first.hi, first.k, last.lo, last.hi, last.k);
        }
        return 0;
    }
    if (cmd == "run" && argc == 3) return run(argv[2]);
    fprintf(stderr, "usage: limits | words | omega logn | plan n_coeffs n_polys first count domain_n n_blinders pieces | run FILE\n");
    return 2;
}
