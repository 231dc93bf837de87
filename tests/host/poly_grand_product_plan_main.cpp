// Stand-alone driver of kzg_rs_amd/csrc/poly_grand_product_plan.hpp (tests/test_poly_grand_product_plan_cpu.py builds it with g++, once
// plain and once with -fsanitize=address,undefined): it plans a call the way the host code does, from arrays of exactly the sizes the
// contract names (the sanitizers watch them), and prints what the header computes; the test compares with its own arithmetic.
//   limits   -> "max_products max_factors max_sets max_refs threads per_lane tile waves max_polys max_scalars ntt_max den_vanishes_bit"
//   words    -> per refusal code "code words"
//   rpow     -> GP_RPOW, a line of 64 hex digits per row (the value, most significant digit first)
//   sizes    -> per power of two n = 1 .. 2^20, for one product of one factor each side: "n tiles run last_lane_lo pad.x chunk_polys"
//   plan domain_n with_shift nulls set_coeffs set_polys product ...
//        set_coeffs, set_polys: comma lists ("-": none; set_polys "-": indices unchecked); nulls: a bit mask of pointers passed as NULL
//        (1 set_coeffs, 2 num_sizes, 4 den_sizes, 8 factors); product: "num/den", a side "set.poly,set.poly,..." or "_" for none
//     -> "code" of gp_plan, and on 0:
//        "n logn U workspace tiles run products out_polys" | the distinct polynomials "set.poly ..." | per product two lines "size slot ..."
//        (numerator, denominator) | the grids "pad.x pad.y tiles.x tiles.y carries.x carries.y" | "fwd_chunk fwd_chunks out_chunk out_chunks
//        reserve chunk_polys(n)" | "workspace_bytes out_scalars sources_at upload_bytes tiles_at carries_at totals_at args_bytes sizeof_table"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/kzg_rs_amd.h"
#include "poly_grand_product_plan.hpp"
using namespace kzg;

static_assert(KZG_POLYS_GP_MAX_PRODUCTS == GP_MAX_PRODUCTS && KZG_POLYS_GP_MAX_FACTORS == GP_MAX_FACTORS && KZG_POLYS_SOP_MAX_SETS == GP_MAX_SETS &&
                  KZG_POLYS_MAX_POLYS == PA_MAX_POLYS && KZG_POLYS_MAX_SCALARS == PA_MAX_SCALARS && KZG_FR_NTT_MAX == FRNTT_MAX,
              "the plan's limits are the header's");
static_assert(sizeof(GpTable) % 32 == 0 && GP_TILE == 1024 && GP_MAX_REFS == 256, "the table is cut into 32-byte pieces; 256 references fit the 16-bit slots");

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
// "set.poly,set.poly" or "_" -> the count, the pairs appended
static bool side_of(const std::string& s, std::vector<uint32_t>& factors, size_t& k) {
    k = 0;
    if (s == "_") return true;
    for (const char* p = s.c_str(); *p;) {
        char* end = nullptr;
        factors.push_back((uint32_t)strtoul(p, &end, 10));
        if (*end != '.') return false;
        factors.push_back((uint32_t)strtoul(end + 1, &end, 10));
        p = *end == ',' ? end + 1 : end;
        k++;
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "limits")) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u\n", GP_MAX_PRODUCTS, GP_MAX_FACTORS, GP_MAX_SETS, GP_MAX_REFS, GP_THREADS, GP_PER_LANE, GP_TILE, GP_WAVES, PA_MAX_POLYS,
               PA_MAX_SCALARS, FRNTT_MAX, GP_DEN_VANISHES_BIT);
        return 0;
    }
    if (!strcmp(argv[1], "words")) {
        for (int r = GP_OK; r <= GP_DEN_VANISHES; r++) printf("%d %s\n", r, gp_refusal_words((GpRefusal)r));
        return 0;
    }
    if (!strcmp(argv[1], "rpow")) {
        for (size_t k = 0; k <= GP_MAX_FACTORS; k++) {
            for (int i = 7; i >= 0; i--) printf("%08x", GP_RPOW[k][i]);
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "sizes")) {
        std::unique_ptr<GpPlan> plan(new GpPlan());
        for (size_t n = 1; n <= FRNTT_MAX; n <<= 1) {
            const std::vector<size_t> set_coeffs{n}, one{1};
            const std::vector<uint32_t> factors{0, 0, 0, 1};
            if (gp_plan(*plan, set_coeffs.data(), nullptr, 1, one.data(), one.data(), factors.data(), 1, n, 1) != GP_OK) return 3;
            printf("%zu %zu %zu %zu %u %zu\n", plan->n, plan->tiles, plan->run, gp_lane_lo(plan->tiles - 1, GP_THREADS - 1), gp_grid_pad(*plan).x, frntt_chunk_polys(n));
        }
        return 0;
    }
    if (!strcmp(argv[1], "plan") && argc >= 7) {
        const size_t domain_n = strtoull(argv[2], nullptr, 10);
        const int with_shift = atoi(argv[3]);
        const unsigned nulls = (unsigned)strtoul(argv[4], nullptr, 10);
        // exactly the elements the contract names, on the heap: an index past them is a sanitizer report
        std::vector<size_t> set_coeffs = list_of(argv[5]), set_polys = list_of(argv[6]), num_sizes, den_sizes;
        const bool with_polys = strcmp(argv[6], "-") != 0;
        std::vector<uint32_t> factors;
        for (int a = 7; a < argc; a++) {
            const std::string p = argv[a];
            const size_t cut = p.find('/');
            if (cut == std::string::npos) return 2;
            size_t kn = 0, kd = 0;
            if (!side_of(p.substr(0, cut), factors, kn) || !side_of(p.substr(cut + 1), factors, kd)) return 2;
            num_sizes.push_back(kn), den_sizes.push_back(kd);
        }
        const size_t n_sets = set_coeffs.size(), n_products = num_sizes.size();
        if (with_polys && set_polys.size() != n_sets) return 2;
        if (set_coeffs.empty()) set_coeffs.reserve(1);
        if (num_sizes.empty()) num_sizes.reserve(1), den_sizes.reserve(1);
        if (factors.empty()) factors.reserve(1);
        std::unique_ptr<GpPlan> plan(new GpPlan());
        const GpPlan& pl = *plan;
        const GpRefusal rc = gp_plan(*plan, nulls & 1 ? nullptr : set_coeffs.data(), with_polys ? set_polys.data() : nullptr, n_sets, nulls & 2 ? nullptr : num_sizes.data(),
                                     nulls & 4 ? nullptr : den_sizes.data(), nulls & 8 ? nullptr : factors.data(), n_products, domain_n, with_shift);
        printf("%d\n", (int)rc);
        if (rc != GP_OK) return 0;
        printf("%zu %d %zu %zu %zu %zu %zu %zu\n", pl.n, pl.logn, pl.U, pl.workspace, pl.tiles, pl.run, pl.products, pl.out_polys);
        for (size_t u = 0; u < pl.U; u++) printf("%u.%u ", pl.ref[u].set, pl.ref[u].poly);
        printf("\n");
        for (size_t g = 0; g < n_products; g++)
            for (int side = 0; side < 2; side++) {
                printf("%u", pl.table.size[g][side]);
                for (uint32_t j = 0; j < pl.table.size[g][side]; j++) printf(" %u", (unsigned)pl.table.slot[g][side][j]);
                if (memcmp(pl.table.start[g][side], GP_RPOW[pl.table.size[g][side]], 32) != 0) return 3;
                printf("\n");
            }
        const PqGrid gp = gp_grid_pad(pl), gt = gp_grid_tiles(pl), gc = gp_grid_carries(pl);
        printf("%u %u %u %u %u %u\n", gp.x, gp.y, gt.x, gt.y, gc.x, gc.y);
        printf("%zu %zu %zu %zu %zu %zu\n", gp_ntt_chunk(pl, pl.U), gp_ntt_chunks(pl, pl.U), gp_ntt_chunk(pl, pl.out_polys), gp_ntt_chunks(pl, pl.out_polys), gp_ntt_reserve(pl),
               frntt_chunk_polys(pl.n));
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", gp_workspace_bytes(pl), gp_out_scalars(pl), gp_args_sources_at(), gp_args_upload_bytes(pl), gp_args_tiles_at(pl),
               gp_args_carries_at(pl), gp_args_totals_at(pl), gp_args_bytes(pl), sizeof(GpTable));
        // the transform chunks cover every row exactly once, forward and back
        for (size_t rows : {pl.U, pl.out_polys}) {
            std::vector<int> seen(rows, 0);
            const size_t cp = gp_ntt_chunk(pl, rows);
            for (size_t c = 0; c < (rows ? gp_ntt_chunks(pl, rows) : 0); c++)
                for (size_t k = 0; k < frntt_chunk_size(rows, c, cp); k++) seen[frntt_chunk_lo(c, cp) + k]++;
            for (size_t u = 0; u < rows; u++)
                if (seen[u] != 1) return 3;
        }
        // every tile lies in exactly one lane's run of the carry kernel
        std::vector<int> owned(pl.tiles, 0);
        for (size_t lane = 0; lane < GP_THREADS; lane++)
            for (size_t u = 0; u < pl.run; u++)
                if (lane * pl.run + u < pl.tiles) owned[lane * pl.run + u]++;
        for (size_t t = 0; t < pl.tiles; t++)
            if (owned[t] != 1) return 3;
        return 0;
    }
    return 2;
}
