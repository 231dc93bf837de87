// Stand-alone driver of kzg_rs_amd/csrc/poly_fraction_sum_plan.hpp (tests/test_poly_fraction_sum_plan_cpu.py builds it with g++, once
// plain and once with -fsanitize=address,undefined): it plans a call the way the host code does, from arrays of exactly the sizes the
// contract names (the sanitizers watch them), and prints what the header computes; the test compares with its own arithmetic.
//   limits   -> "max_sums max_fractions max_factors max_sets max_fracs max_refs threads per_lane tile waves max_scalars ntt_max
//                with_shift with_steps bad_coeff_bit den_vanishes_bit"
//   words    -> per refusal code "code words"
//   tiles n ... -> per n (any size, not only a domain's) "n tiles run": gp_tiles and gp_carry_run, the geometry of all five launches
//   rows     -> per flags value 0 .. 3, for sums 0 and 5: "flags rows phi shift steps park phi5 shift5 steps5 park5" (a row that the
//               flags do not ask for prints as -1)
//   plan domain_n flags nulls set_coeffs set_polys sum ...
//        set_coeffs, set_polys: comma lists ("-": none; set_polys "-": indices unchecked); nulls: a bit mask of pointers passed as NULL
//        (1 set_coeffs, 2 frac_counts, 4 coeffs, 8 num_sizes, 16 den_sizes, 32 factors); sum: its fractions "num/den" joined by "+", a
//        side "set.poly,set.poly,..." or "_" for none; "0" for a sum of no fractions.  Fraction k of the call gets the coefficient
//        whose 32 bytes are all 0x10 + k.
//     -> "code" of fs_plan, and on 0:
//        "n logn U workspace tiles run sums fractions rows out_polys" | the distinct polynomials "set.poly ..." | per sum "first count" |
//        per fraction two lines "size slot ..." (numerator, denominator) | the grids "pad.x pad.y tiles.x tiles.y carries.x carries.y" |
//        "fwd_chunk fwd_chunks out_chunk out_chunks reserve chunk_polys(n)" | "workspace_bytes out_scalars sources_at upload_bytes
//        tiles_at carries_at sums_at totals_at args_bytes sizeof_table"
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/kzg_rs_amd.h"
#include "poly_fraction_sum_plan.hpp"
using namespace kzg;

static_assert(KZG_POLYS_FS_MAX_SUMS == FS_MAX_SUMS && KZG_POLYS_FS_MAX_FRACTIONS == FS_MAX_FRACTIONS && KZG_POLYS_FS_MAX_FACTORS == FS_MAX_FACTORS &&
                  KZG_POLYS_SOP_MAX_SETS == FS_MAX_SETS && KZG_POLYS_MAX_SCALARS == PA_MAX_SCALARS && KZG_FR_NTT_MAX == FRNTT_MAX &&
                  KZG_POLYS_FS_WITH_SHIFT == FS_WITH_SHIFT && KZG_POLYS_FS_WITH_STEPS == FS_WITH_STEPS,
              "the plan's limits are the header's");
static_assert(sizeof(FsTable) % 32 == 0 && offsetof(FsTable, coeff) % 16 == 0 && FS_MAX_REFS == 1024 && FS_MAX_SUMS * 3 <= PA_MAX_POLYS,
              "the table is cut into 32-byte pieces and its c_k are read 16 bytes at a time; 1024 references fit the 16-bit slots");

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
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %u %u %u %u\n", FS_MAX_SUMS, FS_MAX_FRACTIONS, FS_MAX_FACTORS, FS_MAX_SETS, FS_MAX_FRACS, FS_MAX_REFS, GP_THREADS,
               GP_PER_LANE, GP_TILE, GP_WAVES, PA_MAX_SCALARS, FRNTT_MAX, FS_WITH_SHIFT, FS_WITH_STEPS, FS_BAD_COEFF_BIT, GP_DEN_VANISHES_BIT);
        return 0;
    }
    if (!strcmp(argv[1], "words")) {
        for (int r = FS_OK; r <= FS_DEN_VANISHES; r++) printf("%d %s\n", r, fs_refusal_words((FsRefusal)r));
        return 0;
    }
    if (!strcmp(argv[1], "tiles")) {
        for (int a = 2; a < argc; a++) {
            const size_t n = strtoull(argv[a], nullptr, 10);
            printf("%zu %zu %zu\n", n, gp_tiles(n), gp_carry_run(gp_tiles(n)));
        }
        return 0;
    }
    if (!strcmp(argv[1], "rows")) {
        for (unsigned flags = 0; flags < 4; flags++) {
            printf("%u %zu", flags, fs_rows(flags));
            for (size_t g : {(size_t)0, (size_t)5})
                printf(" %zu %ld %ld %zu", fs_row_phi(g, flags), flags & FS_WITH_SHIFT ? (long)fs_row_shift(g, flags) : -1L, flags & FS_WITH_STEPS ? (long)fs_row_steps(g, flags) : -1L,
                       fs_row_park(g, flags));
            printf("\n");
        }
        return 0;
    }
    if (!strcmp(argv[1], "plan") && argc >= 7) {
        const size_t domain_n = strtoull(argv[2], nullptr, 10);
        const unsigned flags = (unsigned)strtoul(argv[3], nullptr, 10);
        const unsigned nulls = (unsigned)strtoul(argv[4], nullptr, 10);
        // exactly the elements the contract names, on the heap: an index past them is a sanitizer report
        std::vector<size_t> set_coeffs = list_of(argv[5]), set_polys = list_of(argv[6]), frac_counts, num_sizes, den_sizes;
        const bool with_polys = strcmp(argv[6], "-") != 0;
        std::vector<uint32_t> factors;
        for (int a = 7; a < argc; a++) {
            std::string rest = argv[a];
            size_t count = 0;
            while (rest != "0" && !rest.empty()) {
                const size_t plus = rest.find('+');
                const std::string p = rest.substr(0, plus);
                rest = plus == std::string::npos ? "" : rest.substr(plus + 1);
                const size_t cut = p.find('/');
                if (cut == std::string::npos) return 2;
                size_t kn = 0, kd = 0;
                if (!side_of(p.substr(0, cut), factors, kn) || !side_of(p.substr(cut + 1), factors, kd)) return 2;
                num_sizes.push_back(kn), den_sizes.push_back(kd), count++;
            }
            frac_counts.push_back(count);
        }
        const size_t n_sets = set_coeffs.size(), n_sums = frac_counts.size();
        std::vector<uint8_t> coeffs(32 * num_sizes.size());
        for (size_t k = 0; k < num_sizes.size(); k++) memset(coeffs.data() + 32 * k, (int)(0x10 + k), 32);
        if (with_polys && set_polys.size() != n_sets) return 2;
        if (set_coeffs.empty()) set_coeffs.reserve(1);
        if (frac_counts.empty()) frac_counts.reserve(1);
        if (num_sizes.empty()) num_sizes.reserve(1), den_sizes.reserve(1), coeffs.reserve(1);
        if (factors.empty()) factors.reserve(1);
        std::unique_ptr<FsPlan> plan(new FsPlan());
        const FsPlan& pl = *plan;
        const FsRefusal rc = fs_plan(*plan, nulls & 1 ? nullptr : set_coeffs.data(), with_polys ? set_polys.data() : nullptr, n_sets, nulls & 2 ? nullptr : frac_counts.data(), n_sums,
                                     nulls & 4 ? nullptr : coeffs.data(), nulls & 8 ? nullptr : num_sizes.data(), nulls & 16 ? nullptr : den_sizes.data(),
                                     nulls & 32 ? nullptr : factors.data(), domain_n, flags, false);
        printf("%d\n", (int)rc);
        if (rc != FS_OK) return 0;
        printf("%zu %d %zu %zu %zu %zu %zu %zu %zu %zu\n", pl.n, pl.logn, pl.U, pl.workspace, pl.tiles, pl.run, pl.sums, pl.fractions, pl.rows, pl.out_polys);
        for (size_t u = 0; u < pl.U; u++) printf("%u.%u ", pl.ref[u].set, pl.ref[u].poly);
        printf("\n");
        if (memcmp(pl.table.rpow, GP_RPOW, sizeof(GP_RPOW)) != 0 || pl.table.n_sums != n_sums || pl.table.flags != flags || pl.table.rows != pl.rows) return 3;
        for (size_t g = 0; g < n_sums; g++) printf("%u %u\n", pl.table.first[g], pl.table.count[g]);
        for (size_t k = 0; k < pl.fractions; k++) {
            for (size_t b = 0; b < 32; b++)
                if (pl.table.coeff[k][b] != (uint8_t)(0x10 + k)) return 3;
            for (int side = 0; side < 2; side++) {
                printf("%u", (unsigned)pl.table.size[k][side]);
                for (uint32_t j = 0; j < pl.table.size[k][side]; j++) printf(" %u", (unsigned)pl.table.slot[k][side][j]);
                printf("\n");
            }
        }
        const PqGrid gp = fs_grid_pad(pl), gt = fs_grid_tiles(pl), gc = fs_grid_carries(pl);
        printf("%u %u %u %u %u %u\n", gp.x, gp.y, gt.x, gt.y, gc.x, gc.y);
        printf("%zu %zu %zu %zu %zu %zu\n", fs_ntt_chunk(pl, pl.U), fs_ntt_chunks(pl, pl.U), fs_ntt_chunk(pl, pl.out_polys), fs_ntt_chunks(pl, pl.out_polys), fs_ntt_reserve(pl),
               frntt_chunk_polys(pl.n));
        printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", fs_workspace_bytes(pl), fs_out_scalars(pl), fs_args_sources_at(), fs_args_upload_bytes(pl), fs_args_tiles_at(pl),
               fs_args_carries_at(pl), fs_args_sums_at(pl), fs_args_totals_at(pl), fs_args_bytes(pl), sizeof(FsTable));
        // the transform chunks cover every row exactly once, forward and back
        for (size_t rows : {pl.U, pl.out_polys}) {
            std::vector<int> seen(rows, 0);
            const size_t cp = fs_ntt_chunk(pl, rows);
            for (size_t c = 0; c < (rows ? fs_ntt_chunks(pl, rows) : 0); c++)
                for (size_t k = 0; k < frntt_chunk_size(rows, c, cp); k++) seen[frntt_chunk_lo(c, cp) + k]++;
            for (size_t u = 0; u < rows; u++)
                if (seen[u] != 1) return 3;
        }
        // every tile lies in exactly one lane's run of the carry kernels, and every index in exactly one lane of one tile
        std::vector<int> owned(pl.tiles, 0);
        for (size_t lane = 0; lane < GP_THREADS; lane++)
            for (size_t u = 0; u < pl.run; u++)
                if (lane * pl.run + u < pl.tiles) owned[lane * pl.run + u]++;
        for (size_t t = 0; t < pl.tiles; t++)
            if (owned[t] != 1) return 3;
        if (gp_lane_lo(pl.tiles - 1, GP_THREADS - 1) + GP_PER_LANE < pl.n || (pl.tiles > 1 && gp_lane_lo(pl.tiles - 1, 0) >= pl.n)) return 3;
        return 0;
    }
    return 2;
}
