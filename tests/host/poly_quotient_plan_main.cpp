// Stand-alone driver of kzg_rs_amd/csrc/poly_quotient_plan.hpp (tests/test_poly_quotient_plan_cpu.py builds it with g++ and
// -fsanitize=address,undefined): it walks the geometry the way the kernels do, into arrays the sanitizers watch, and prints what the
// header computes; the test compares with its own arithmetic.
//   geometry               -> "lane wave tile threads chunk_scalars max_coeffs max_openings"
//   cover lo hi            -> per n in [lo, hi]: "n tiles run covered once chain threads" - covered = coefficients some lane owns below n,
//                             once = 1 if each was owned exactly once, chain = tiles the carry chain visits from tile 0 to the last,
//                             threads = carry-launch threads that own a tile
//   chunks n_coeffs n_points n_polys -> "chunk n_chunks" then per chunk "lo m poly_first poly_end quotient_scalars stage_bytes tile_scalars"
//   sizes n_coeffs pairs   -> the grids "x y" of tile sums, carries, decode, and the largest int a kernel takes ("n tiles pair0 poly0")
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "poly_quotient_plan.hpp"
using namespace kzg;

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "geometry")) {
        printf("%zu %zu %zu %zu %zu %zu %zu\n", PQ_LANE, PQ_WAVE, PQ_TILE, PQ_THREADS, PQ_CHUNK_SCALARS, PQ_MAX_COEFFS, PQ_MAX_OPENINGS);
        return 0;
    }
    if (!strcmp(argv[1], "cover") && argc == 4) {
        const size_t lo = strtoull(argv[2], nullptr, 10), hi = strtoull(argv[3], nullptr, 10);
        for (size_t n = lo; n <= hi; n++) {
            const size_t tiles = pq_tiles(n), run = pq_carry_run(tiles);
            std::vector<uint8_t> owned(n, 0);  // (exactly n: an index at n or above is a sanitizer report)
            size_t covered = 0, tile_total = 0;
            for (size_t t = 0; t < tiles; t++) {
                tile_total += pq_tile_size(n, t);
                for (size_t th = 0; th < PQ_THREADS; th++)
                    for (size_t j = 0; j < PQ_LANE; j++) {
                        const size_t i = pq_lane_lo(t, th) + j;
                        if (i < n) owned[i]++, covered++;  // the kernels' own bound check
                    }
            }
            bool once = tile_total == n;
            for (size_t i = 0; i < n; i++) once = once && owned[i] == 1;
            // the carry into tile t comes from tile t + 1: from tile 0 the chain visits every tile and ends at the last
            size_t chain = 0;
            for (size_t t = tiles ? 0 : PQ_NO_TILE; t != PQ_NO_TILE; t = pq_carry_from(tiles, t)) {
                if (t != chain) return 3;
                chain++;
            }
            // the carry launch: thread k owns tiles [k run, (k + 1) run)
            std::vector<uint8_t> scanned(tiles, 0);
            size_t threads = 0;
            for (size_t k = 0; k < PQ_THREADS; k++) {
                bool any = false;
                for (size_t u = 0; u < run; u++)
                    if (k * run + u < tiles) scanned[k * run + u]++, any = true;
                threads += any;
            }
            for (size_t t = 0; t < tiles; t++) once = once && scanned[t] == 1;
            printf("%zu %zu %zu %zu %d %zu %zu\n", n, tiles, run, covered, (int)once, chain, threads);
        }
        return 0;
    }
    if (!strcmp(argv[1], "chunks") && argc == 5) {
        const size_t n = strtoull(argv[2], nullptr, 10), n_points = strtoull(argv[3], nullptr, 10), n_polys = strtoull(argv[4], nullptr, 10);
        const size_t pairs = n_points * n_polys, chunk = pq_chunk_pairs(n, n_points);
        printf("%zu %zu\n", chunk, pq_chunks(pairs, chunk));
        for (size_t k = 0; k <= pq_chunks(pairs, chunk); k++) {  // (one behind the last: size 0)
            const size_t lo = pq_chunk_lo(k, chunk), m = pq_chunk_size(pairs, k, chunk);
            if (!m) {
                printf("%zu 0 0 0 0 0 0\n", lo);
                continue;
            }
            const size_t k0 = pq_poly_first(lo, n_points), k1 = pq_poly_end(lo, m, n_points);
            printf("%zu %zu %zu %zu %zu %zu %zu\n", lo, m, k0, k1, pq_quotient_scalars(n, m), pq_stage_bytes(n, k1 - k0), pq_tile_scalars(n, m));
        }
        return 0;
    }
    if (!strcmp(argv[1], "sizes") && argc == 4) {
        const size_t n = strtoull(argv[2], nullptr, 10), pairs = strtoull(argv[3], nullptr, 10);
        const PqGrid a = pq_grid_tiles(n, pairs), b = pq_grid_carries(pairs), c = pq_grid_decode(n, pairs);
        printf("%u %u\n%u %u\n%u %u\n", a.x, a.y, b.x, b.y, c.x, c.y);
        // what the kernels take as int: n, the tile count, a chunk's first pair and polynomial, and the largest coefficient index a lane forms
        const size_t last_index = pq_lane_lo(pq_tiles(n) ? pq_tiles(n) - 1 : 0, PQ_THREADS - 1) + PQ_LANE - 1;
        printf("%zu %zu %zu %zu %d\n", n, pq_tiles(n), pairs, last_index, INT_MAX);
        return 0;
    }
    return 2;
}
