// Stand-alone driver of kzg_rs_amd/csrc/poly_fold_plan.hpp (tests/test_poly_fold_plan_cpu.py builds it with g++, once plain and once
// with -fsanitize=address,undefined): it walks the plan the way the host code and the fold kernel do, into arrays the sanitizers watch,
// and prints what the header computes; the test compares with its own arithmetic.
//   geometry                  -> "threads per_lane tile eval_threads chunk_scalars max_coeffs max_openings"
//   cover lo hi               -> per n in [lo, hi]: "n tiles covered once" - covered = elements below n some lane of the fold owns,
//                                once = 1 if each was owned exactly once
//   chunks n_coeffs n_polys   -> "cp chunks" then per VISIT "chunk first end staged_scalars stage_bytes"
//   sizes n_coeffs n_polys n_points -> "cp gp groups" | the fold's grid "x y" | "stage_bytes fold_bytes quotient_scalars tile_scalars zs_bytes"
//                                | per group "first size" | "n last_elem pairs_of_a_chunk INT_MAX"
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "poly_fold_plan.hpp"
using namespace kzg;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "geometry")) {
        printf("%zu %zu %zu %zu %zu %zu %zu\n", PF_THREADS, PF_PER_LANE, PF_TILE, PF_EVAL_THREADS, PQ_CHUNK_SCALARS, PQ_MAX_COEFFS, PQ_MAX_OPENINGS);
        return 0;
    }
    if (!strcmp(argv[1], "cover") && argc == 4) {
        const size_t lo = strtoull(argv[2], nullptr, 10), hi = strtoull(argv[3], nullptr, 10);
        for (size_t n = lo; n <= hi; n++) {
            std::vector<uint8_t> owned(n, 0);  // (exactly n: an index at n or above is a sanitizer report)
            size_t covered = 0;
            for (size_t t = 0; t < pf_tiles(n); t++)
                for (size_t th = 0; th < PF_THREADS; th++)
                    for (size_t u = 0; u < PF_PER_LANE; u++) {
                        const size_t i = pf_elem(t, th, u);
                        if (i < n) owned[i]++, covered++;  // the kernel's own bound check
                    }
            bool once = true;
            for (size_t i = 0; i < n; i++) once = once && owned[i] == 1;
            printf("%zu %zu %zu %d\n", n, pf_tiles(n), covered, (int)once);
        }
        return 0;
    }
    if (!strcmp(argv[1], "chunks") && argc == 4) {
        const size_t n = strtoull(argv[2], nullptr, 10), n_polys = strtoull(argv[3], nullptr, 10);
        const size_t cp = pf_chunk_polys(n), chunks = pf_chunks(n_polys, cp);
        printf("%zu %zu\n", cp, chunks);
        std::vector<uint8_t> seen(n_polys, 0);
        for (size_t v = 0; v < chunks; v++) {
            const size_t c = pf_visit(chunks, v), k0 = pf_chunk_first(c, cp), k1 = pf_chunk_end(n_polys, c, cp);
            for (size_t k = k0; k < k1; k++) seen[k]++;
            printf("%zu %zu %zu %zu %zu\n", c, k0, k1, (k1 - k0) * n, pf_stage_bytes(n, k1 - k0));
        }
        for (size_t k = 0; k < n_polys; k++)
            if (seen[k] != 1) return 3;
        return 0;
    }
    if (!strcmp(argv[1], "sizes") && argc == 5) {
        const size_t n = strtoull(argv[2], nullptr, 10), n_polys = strtoull(argv[3], nullptr, 10), n_points = strtoull(argv[4], nullptr, 10);
        const size_t cp = pf_chunk_polys(n) < n_polys ? pf_chunk_polys(n) : n_polys, gp = pf_group_points(n) < n_points ? pf_group_points(n) : n_points;
        const size_t groups = pf_groups(n_points, gp);
        printf("%zu %zu %zu\n", cp, gp, groups);
        const PqGrid f = pf_grid_fold(n, gp);
        printf("%u %u\n", f.x, f.y);
        printf("%zu %zu %zu %zu %zu\n", pf_stage_bytes(n, cp), pf_fold_bytes(n, gp), pf_quotient_scalars(n, gp), pf_tile_scalars(n, cp, gp), 32 * pf_pairs(cp, gp));
        for (size_t g = 0; g <= groups; g++) printf("%zu %zu\n", pf_group_first(g, gp), pf_group_size(n_points, g, gp));  // (one behind the last: size 0)
        printf("%zu %zu %zu %d\n", n, pf_elem(pf_tiles(n) ? pf_tiles(n) - 1 : 0, PF_THREADS - 1, PF_PER_LANE - 1), pf_pairs(cp, gp), INT_MAX);
        return 0;
    }
    return 2;
}
