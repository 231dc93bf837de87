// poly_fold_plan.hpp - host planning of the batched openings (capi_poly_batch.hpp) and the geometry of their fold
// (poly_fold_kernels.hpp): which element a lane of the fold owns, how the polynomials of a call are cut into chunks, in which order the
// chunks are visited, how the points are cut into groups, and the sizes of the buffers.
// Plain C++, no HIP: tests/host/poly_fold_plan_main.cpp builds it with g++ (tests/test_poly_fold_plan_cpu.py).  Everything is
// constexpr, so the kernels read the same functions.
//
// f_j = sum_k gamma_j^k p_k is a Horner recurrence in gamma_j over the POLYNOMIALS: acc = p_k + gamma_j acc for k from the last
// polynomial down to 0, coefficient by coefficient.  The staged coefficients are cut into chunks of whole polynomials of at most
// PQ_CHUNK_SCALARS scalars; chunk c holds polynomials [c cp, min(m, (c + 1) cp)) and the chunks are visited from the LAST to the first,
// so the recurrence carries across them in the fold buffer [point][n_coeffs].  The fold is element-wise: lane t of workgroup w owns
// the PF_PER_LANE elements w PF_TILE + u PF_THREADS + t - consecutive lanes read consecutive 32-byte elements.
// The points of a call are cut into groups that keep the fold buffer (and the quotients behind it) within PQ_CHUNK_SCALARS; every
// group runs the whole chain over all polynomials.  One group is the rule: 8 points at 2^20 coefficients, 4096 up to 2^11.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "poly_quotient_plan.hpp"

namespace kzg {

constexpr size_t PF_THREADS = 256;                     // lanes of a fold workgroup
constexpr size_t PF_PER_LANE = 2;                      // elements per lane, PF_THREADS apart
constexpr size_t PF_TILE = PF_THREADS * PF_PER_LANE;   // elements per workgroup
constexpr size_t PF_EVAL_THREADS = 64;                 // k_poly_eval_tiles: one wavefront per (polynomial, point) pair

// the fold's element map and grid: x = tiles of n elements, y = the points of the group
constexpr size_t pf_tiles(size_t n) { return (n + PF_TILE - 1) / PF_TILE; }
constexpr size_t pf_elem(size_t tile, size_t thread, size_t u) { return tile * PF_TILE + u * PF_THREADS + thread; }
constexpr PqGrid pf_grid_fold(size_t n, size_t points) { return PqGrid{(unsigned)pf_tiles(n), (unsigned)points}; }

// polynomials per chunk: as many as keep the staged scalars within PQ_CHUNK_SCALARS, at least one, at most what a call may hold
constexpr size_t pf_chunk_polys(size_t n_coeffs) {
    size_t m = n_coeffs ? PQ_CHUNK_SCALARS / n_coeffs : PQ_MAX_OPENINGS;
    if (m > PQ_MAX_OPENINGS) m = PQ_MAX_OPENINGS;
    return m < 1 ? 1 : m;
}
constexpr size_t pf_chunks(size_t n_polys, size_t cp) { return (n_polys + cp - 1) / cp; }
// the v-th chunk VISITED (v = 0 first) is chunk pf_visit(chunks, v): the last one first
constexpr size_t pf_visit(size_t chunks, size_t v) { return chunks - 1 - v; }
constexpr size_t pf_chunk_first(size_t c, size_t cp) { return c * cp; }
constexpr size_t pf_chunk_end(size_t n_polys, size_t c, size_t cp) { return (c + 1) * cp < n_polys ? (c + 1) * cp : n_polys; }

// points per group: the fold buffer and the quotients of a group stay within PQ_CHUNK_SCALARS scalars each
constexpr size_t pf_group_points(size_t n_coeffs) { return pf_chunk_polys(n_coeffs); }
constexpr size_t pf_groups(size_t n_points, size_t gp) { return (n_points + gp - 1) / gp; }
constexpr size_t pf_group_first(size_t g, size_t gp) { return g * gp; }
constexpr size_t pf_group_size(size_t n_points, size_t g, size_t gp) { return g * gp >= n_points ? 0 : (n_points - g * gp < gp ? n_points - g * gp : gp); }

// the finishing launch of the individual values: thread k of the pair's wavefront owns the consecutive tiles [k run, (k + 1) run)
constexpr size_t pf_eval_run(size_t tiles) { return tiles ? (tiles + PF_EVAL_THREADS - 1) / PF_EVAL_THREADS : 1; }

// buffer sizes of a call whose chunks hold `polys` polynomials and whose groups hold `points` points
constexpr size_t pf_stage_bytes(size_t n_coeffs, size_t polys) { return pq_stage_bytes(n_coeffs, polys); }       // the coefficients as given
constexpr size_t pf_fold_bytes(size_t n_coeffs, size_t points) { return 32 * n_coeffs * points; }                // f[point][n_coeffs], big-endian
constexpr size_t pf_quotient_scalars(size_t n_coeffs, size_t points) { return pq_quotient_scalars(n_coeffs, points); }
constexpr size_t pf_pairs(size_t polys, size_t points) { return polys * points; }                                // (polynomial, point) pairs of a chunk
constexpr size_t pf_tile_scalars(size_t n_coeffs, size_t polys, size_t points) {                                 // tile sums: the chunk's pairs, then the fold's
    return pq_tile_scalars(n_coeffs, pf_pairs(polys, points) > points ? pf_pairs(polys, points) : points);
}

}  // namespace kzg
