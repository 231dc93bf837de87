// Stand-alone driver of kzg_rs_amd/csrc/poly_arith_plan.hpp (tests/test_poly_arith_plan_cpu.py builds it with g++, once plain and once
// with -fsanitize=address,undefined): it plans a call the way the host code does, from arrays of exactly the sizes the contract names
// (the sanitizers watch them), and prints what the header computes; the test compares with its own arithmetic.
//   limits                          -> "max_sets max_terms max_factors max_chain max_polys max_coeffs max_scalars ntt_max sop_tile threads max_refs not_divisible_bit"
//   words                           -> per refusal code "code words"
//   plan v piece nulls set_coeffs set_polys term ...
//        set_coeffs, set_polys: comma lists ("-": none; set_polys "-": indices unchecked); nulls: a bit mask of pointers passed as NULL
//        (1 set_coeffs, 2 term_sizes, 4 factors); term: "set.poly,set.poly,..." or "_" for a term without factors
//     -> "code" of pa_plan, and on 0:
//        "L0 N L pieces out_coeffs U workspace chain logN" | the distinct polynomials "set.poly ..." | per term "size slot ..."
//        | the grids "pad.x pad.y sop.x sop.last_elem div.x coeffs.x" | "chunk chunks chunk_polys(N)" | "workspace_bytes out_scalars sources_at coeffs_at prepared_at
//        args_bytes sizeof_table sizeof_source"
//   coeffs hex ...                  -> "code" of pa_check_coeffs
//   lincomb n_coeffs count n_out null hex ...  -> "code" of pa_lincomb_check (null = 1: the factors passed as NULL)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "poly_arith_plan.hpp"
using namespace kzg;

static bool hex32(const char* s, uint8_t* out) {
    if (strlen(s) != 64) return false;
    for (int i = 0; i < 32; i++) {
        unsigned v = 0;
        if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}
static std::vector<size_t> list_of(const char* s) {
    std::vector<size_t> out;
    if (!strcmp(s, "-")) return out;
    for (const char* p = s; *p;) {
        char* end = nullptr;
        out.push_back(strtoull(p, &end, 10));
        p = *end == ',' ? end + 1 : end;
    }
    return out;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "limits")) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u\n", PA_MAX_SETS, PA_MAX_TERMS, PA_MAX_FACTORS, PA_MAX_CHAIN, PA_MAX_POLYS, PA_MAX_COEFFS, PA_MAX_SCALARS, FRNTT_MAX,
               PF_TILE, PA_THREADS, PA_MAX_REFS, PA_NOT_DIVISIBLE_BIT);
        return 0;
    }
    if (!strcmp(argv[1], "words")) {
        for (int r = PA_OK; r <= PA_LC_FACTOR; r++) printf("%d %s\n", r, pa_refusal_words((PaRefusal)r));
        return 0;
    }
    if (!strcmp(argv[1], "coeffs")) {
        std::vector<uint8_t> c(32 * (size_t)(argc - 2));
        for (int a = 2; a < argc; a++)
            if (!hex32(argv[a], c.data() + 32 * (a - 2))) return 2;
        if (c.empty()) c.reserve(1);
        printf("%d\n", (int)pa_check_coeffs(c.data(), (size_t)(argc - 2)));
        return 0;
    }
    if (!strcmp(argv[1], "lincomb") && argc >= 6) {
        const size_t n = strtoull(argv[2], nullptr, 10), count = strtoull(argv[3], nullptr, 10), n_out = strtoull(argv[4], nullptr, 10);
        const bool null = atoi(argv[5]) != 0;
        std::vector<uint8_t> c(32 * (size_t)(argc - 6));
        for (int a = 6; a < argc; a++)
            if (!hex32(argv[a], c.data() + 32 * (a - 6))) return 2;
        if (c.empty()) c.reserve(1);
        printf("%d\n", (int)pa_lincomb_check(n, count, n_out, null ? nullptr : c.data()));
        return 0;
    }
    if (!strcmp(argv[1], "plan") && argc >= 7) {
        const size_t v = strtoull(argv[2], nullptr, 10), piece = strtoull(argv[3], nullptr, 10);
        const unsigned nulls = (unsigned)strtoul(argv[4], nullptr, 10);
        // exactly the elements the contract names, on the heap: an index past them is a sanitizer report
        std::vector<size_t> set_coeffs = list_of(argv[5]), set_polys = list_of(argv[6]), term_sizes;
        const bool with_polys = strcmp(argv[6], "-") != 0;
        std::vector<uint32_t> factors;
        for (int a = 7; a < argc; a++) {
            size_t k = 0;
            if (strcmp(argv[a], "_") != 0) {
                for (const char* p = argv[a]; *p;) {
                    char* end = nullptr;
                    factors.push_back((uint32_t)strtoul(p, &end, 10));
                    if (*end != '.') return 2;
                    factors.push_back((uint32_t)strtoul(end + 1, &end, 10));
                    p = *end == ',' ? end + 1 : end;
                    k++;
                }
            }
            term_sizes.push_back(k);
        }
        const size_t n_sets = set_coeffs.size(), n_terms = term_sizes.size();
        if (with_polys && set_polys.size() != n_sets) return 2;
        if (set_coeffs.empty()) set_coeffs.reserve(1);
        if (term_sizes.empty()) term_sizes.reserve(1);
        if (factors.empty()) factors.reserve(1);
        std::unique_ptr<PaPlan> plan(new PaPlan());
        const PaPlan& pl = *plan;
        const PaRefusal rc = pa_plan(*plan, nulls & 1 ? nullptr : set_coeffs.data(), with_polys ? set_polys.data() : nullptr, n_sets, nulls & 2 ? nullptr : term_sizes.data(),
                                     nulls & 4 ? nullptr : factors.data(), n_terms, v, piece);
        printf("%d\n", (int)rc);
        if (rc != PA_OK) return 0;
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %d\n", pl.L0, pl.N, pl.L, pl.pieces, pl.out_coeffs, pl.U, pl.workspace, pl.chain, pl.logN);
        for (size_t u = 0; u < pl.U; u++) printf("%u.%u ", pl.ref[u].set, pl.ref[u].poly);
        printf("\n");
        for (size_t t = 0; t < n_terms; t++) {
            printf("%u", pl.table.size[t]);
            for (uint32_t j = 0; j < pl.table.size[t]; j++) printf(" %u", (unsigned)pl.table.slot[t][j]);
            printf("\n");
        }
        const PqGrid gp = pa_grid_pad(pl), gs = pa_grid_sop(pl), gd = pa_grid_div(pl), gc = pa_grid_coeffs(n_terms);
        printf("%u %u %u %zu %u %u\n", gp.x, gp.y, gs.x, pf_elem(gs.x - 1, PF_THREADS - 1, PF_PER_LANE - 1), gd.x, gc.x);
        printf("%zu %zu %zu\n", pa_ntt_chunk(pl), pa_ntt_chunks(pl), frntt_chunk_polys(pl.N));
        printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", pa_workspace_bytes(pl), pa_out_scalars(pl), pa_args_sources_at(), pa_args_coeffs_at(pl), pa_args_prepared_at(pl), pa_args_bytes(pl),
               sizeof(PaTable), sizeof(PaSource));
        // the transform chunks cover every row exactly once
        std::vector<int> seen(pl.U, 0);
        for (size_t c = 0; c < pa_ntt_chunks(pl); c++)
            for (size_t k = 0; k < frntt_chunk_size(pl.U, c, pa_ntt_chunk(pl)); k++) seen[frntt_chunk_lo(c, pa_ntt_chunk(pl)) + k]++;
        for (size_t u = 0; u < pl.U; u++)
            if (seen[u] != 1) return 3;
        return 0;
    }
    return 2;
}
