// Stand-alone driver of kzg_rs_amd/csrc/poly_multiopen_plan.hpp (tests/test_poly_multiopen_plan_cpu.py builds it with g++, once plain
// and once with -fsanitize=address,undefined): it validates a call the way the host code does, from arrays of exactly the sizes the
// contract names (the sanitizers watch them), and prints what the header computes; the test compares with its own arithmetic.
//   limits                                   -> "max_groups max_set_points max_points scalar_threads max_openings max_coeffs chunk_scalars lincomb_tile"
//   words                                    -> per refusal code "code words"
//   validate n_coeffs count gamma z nulls group ...
//        count: a number, or "groups" for the verifier's form; gamma, z: 64 hex digits (z "-": no second step); nulls: a bit mask of
//        pointers passed as NULL (1 group_sizes, 2 set_sizes, 4 points, 8 gamma); group: "m:hex,hex,..." (m polynomials at those points)
//     -> "code" of mo_validate, and on 0:
//        "n_groups count n_points n_values n_union max_pts max_pairs" | per group "poly0 polys pt0 pts val0" | t_index | t_first (n_union entries)
//        | per polynomial its group | per (group, T_u) 0 or 1 in one line per group | "code" of mo_check_z (0 without z)
//        | "h_scalars fold_bytes quotient_scalars tile_scalars carry_scalars zs_bytes ys_bytes factor_scalars"
//        | "points_at gamma_at gpow_at w_at args_bytes sizeof_shape" | the lincomb grid "x y last_elem INT_MAX"
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "poly_multiopen_plan.hpp"
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

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "limits")) {
        printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", MO_MAX_GROUPS, MO_MAX_SET_POINTS, MO_MAX_POINTS, MO_SCALAR_THREADS, PQ_MAX_OPENINGS, PQ_MAX_COEFFS, PQ_CHUNK_SCALARS, PF_TILE);
        return 0;
    }
    if (!strcmp(argv[1], "words")) {
        for (int r = MO_OK; r <= MO_Z_IN_T; r++) printf("%d %s\n", r, mo_refusal_words((MoRefusal)r));
        return 0;
    }
    if (!strcmp(argv[1], "validate") && argc >= 7) {
        const size_t n = strtoull(argv[2], nullptr, 10);
        const size_t count = !strcmp(argv[3], "groups") ? MO_COUNT_FROM_GROUPS : strtoull(argv[3], nullptr, 10);
        std::vector<uint8_t> gamma(32), z(32);
        if (!hex32(argv[4], gamma.data())) return 2;
        const bool with_z = strcmp(argv[5], "-") != 0;
        if (with_z && !hex32(argv[5], z.data())) return 2;
        const unsigned nulls = (unsigned)strtoul(argv[6], nullptr, 10);
        std::vector<size_t> group_sizes, set_sizes;
        std::vector<uint8_t> points;
        for (int a = 7; a < argc; a++) {
            char* end = nullptr;
            group_sizes.push_back(strtoull(argv[a], &end, 10));
            if (*end != ':') return 2;
            size_t t = 0;
            for (const char* p = end + 1; *p;) {
                std::string tok(p, strcspn(p, ","));
                uint8_t v[32];
                if (!hex32(tok.c_str(), v)) return 2;
                points.insert(points.end(), v, v + 32);
                t++;
                p += tok.size();
                if (*p == ',') p++;
            }
            set_sizes.push_back(t);
        }
        // exactly the bytes the contract names, on the heap: an index past them is a sanitizer report
        std::vector<size_t> gs(group_sizes), ss(set_sizes);
        std::vector<uint8_t> pts(points);
        if (gs.empty()) gs.reserve(1), ss.reserve(1);
        if (pts.empty()) pts.reserve(1);
        MoShape sh;
        const MoRefusal rc = mo_validate(sh, nulls & 1 ? nullptr : gs.data(), nulls & 2 ? nullptr : ss.data(), gs.size(), count, nulls & 4 ? nullptr : pts.data(), nulls & 8 ? nullptr : gamma.data());
        printf("%d\n", (int)rc);
        if (rc != MO_OK) return 0;
        printf("%u %u %u %u %u %u %u\n", sh.n_groups, sh.count, sh.n_points, sh.n_values, sh.n_union, sh.max_pts, sh.max_pairs);
        for (uint32_t g = 0; g < sh.n_groups; g++) printf("%u %u %u %u %u\n", sh.g[g].poly0, sh.g[g].polys, sh.g[g].pt0, sh.g[g].pts, sh.g[g].val0);
        for (uint32_t j = 0; j < sh.n_points; j++) printf("%u ", sh.t_index[j]);
        printf("\n");
        for (uint32_t u = 0; u < sh.n_union; u++) printf("%u ", sh.t_first[u]);
        printf("\n");
        for (uint32_t i = 0; i < sh.count; i++) printf("%u ", mo_group_of(sh, i));
        printf("\n");
        for (uint32_t g = 0; g < sh.n_groups; g++) {
            for (uint32_t u = 0; u < sh.n_union; u++) printf("%d ", (int)mo_in_group(sh, g, u));
            printf("\n");
        }
        printf("%d\n", with_z ? (int)mo_check_z(sh, pts.data(), z.data()) : 0);
        printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", mo_h_scalars(n), mo_fold_bytes(n), mo_quotient_scalars(sh, n), mo_tile_scalars(sh, n), mo_carry_scalars(sh, n), mo_zs_bytes(sh),
               mo_ys_bytes(sh), mo_factor_scalars(sh));
        printf("%zu %zu %zu %zu %zu %zu\n", mo_args_points_at(), mo_args_gamma_at(sh), mo_args_gpow_at(sh), mo_args_w_at(sh), mo_args_bytes(sh), sizeof(MoShape));
        const PqGrid gl = mo_grid_lincomb(n);
        printf("%u %u %zu %d\n", gl.x, gl.y, pf_elem(gl.x ? gl.x - 1 : 0, PF_THREADS - 1, PF_PER_LANE - 1), INT_MAX);
        // the zrep layout of the first step: every value slot is written exactly once
        std::vector<uint8_t> slots(sh.n_values, 0);
        for (uint32_t g = 0; g < sh.n_groups; g++)
            for (uint32_t k = 0; k < sh.g[g].polys; k++)
                for (uint32_t a = 0; a < sh.g[g].pts; a++) slots[sh.g[g].val0 + k * sh.g[g].pts + a]++;
        for (uint32_t v = 0; v < sh.n_values; v++)
            if (slots[v] != 1) return 3;
        return 0;
    }
    return 2;
}
