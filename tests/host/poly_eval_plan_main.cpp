// Stand-alone driver of kzg_rs_amd/csrc/poly_eval_plan.hpp (tests/test_poly_eval_plan_cpu.py builds it with g++, once plain and once
// with -fsanitize=address,undefined): it walks the grid of k_poly_tile_sums_points the way the kernel does, into arrays the sanitizers
// watch, and prints what the header computes; the test compares with its own arithmetic.
//   geometry                    -> "points threads lane tile waves"
//   cover polys n_points        -> "blocks grid_y pairs hit once tail_size" - hit = (workgroup row, slot) places that map to a pair below
//                                  polys x n_points, once = 1 if every pair was hit exactly once and every slot of every block maps
//                                  below that bound; exit 3 if a slot maps outside
//   grid n_coeffs polys n_points -> "x y tile_sums last_index" - the grid, the tile sums the launch writes, the largest index it writes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "poly_eval_plan.hpp"
using namespace kzg;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "geometry")) {
        printf("%zu %zu %zu %zu %zu\n", PE_POINTS, PE_THREADS, PQ_LANE, PQ_TILE, PQ_WAVES);
        return 0;
    }
    if (!strcmp(argv[1], "cover") && argc == 4) {
        const size_t polys = strtoull(argv[2], nullptr, 10), n_points = strtoull(argv[3], nullptr, 10), pairs = polys * n_points;
        const PqGrid g = pe_grid(1, polys, n_points);
        std::vector<uint8_t> seen(pairs, 0);  // (exactly the pairs: an index at or above is a sanitizer report)
        size_t hit = 0;
        for (size_t y = 0; y < g.y; y++) {
            const size_t k = pe_poly_of(y, n_points), b = pe_block_of(y, n_points), cnt = pe_block_size(n_points, b);
            if (k >= polys || b >= pe_blocks(n_points) || cnt == 0 || cnt > PE_POINTS) return 3;
            for (size_t u = 0; u < cnt; u++) {  // the kernel's own loop bound
                const size_t q = pe_pair(k, n_points, b, u);
                if (q >= pairs || pe_block_lo(b) + u >= n_points) return 3;
                seen[q]++, hit++;
            }
        }
        bool once = true;
        for (size_t q = 0; q < pairs; q++) once = once && seen[q] == 1;
        const size_t blocks = pe_blocks(n_points);
        printf("%zu %u %zu %zu %d %zu\n", blocks, g.y, pairs, hit, (int)once, blocks ? pe_block_size(n_points, blocks - 1) : 0);
        return pe_block_size(n_points, blocks) == 0 ? 0 : 3;  // nothing behind the last block
    }
    if (!strcmp(argv[1], "grid") && argc == 5) {
        const size_t n = strtoull(argv[2], nullptr, 10), polys = strtoull(argv[3], nullptr, 10), n_points = strtoull(argv[4], nullptr, 10);
        const PqGrid g = pe_grid(n, polys, n_points);
        const size_t scalars = pq_tile_scalars(n, polys * n_points);
        std::vector<uint8_t> written(scalars, 0);
        size_t last = 0;
        for (size_t y = 0; y < g.y; y++)
            for (size_t t = 0; t < g.x; t++)
                for (size_t u = 0; u < pe_block_size(n_points, pe_block_of(y, n_points)); u++) {
                    const size_t at = pq_tile_index(g.x, pe_pair(pe_poly_of(y, n_points), n_points, pe_block_of(y, n_points), u), t);
                    if (at >= scalars) return 3;
                    written[at]++;
                    last = at > last ? at : last;
                }
        for (size_t i = 0; i < scalars; i++)
            if (written[i] != 1) return 3;
        printf("%u %u %zu %zu\n", g.x, g.y, scalars, last);
        return 0;
    }
    return 2;
}
