// poly_eval_plan.hpp - geometry of the many-points tile sums (poly_eval_kernels.hpp: k_poly_tile_sums_points), which serve
// kzg_polys_evaluate and the individual values of the resident batched opening (capi_polys.hpp): how the points of a call fall into
// blocks, the grid, and which (polynomial, point) pair slot u of block b is.
// Plain C++, no HIP: tests/host/poly_eval_plan_main.cpp builds it with g++ (tests/test_poly_eval_plan_cpu.py).  Everything is
// constexpr, so the kernel reads the same functions.
//
// The lane / wavefront / tile geometry is poly_quotient_plan.hpp's (PQ_LANE coefficients per lane, PQ_TILE per workgroup).  Where
// k_poly_tile_sums spends one workgroup per (tile, pair), this launch spends one per (tile, polynomial, BLOCK of points): the lane's
// coefficients are loaded, range-checked and kept in registers once, and the suffix Horner recurrence runs for the block's points one
// after the other.  The n_points points of a call are shared by its polynomials; block b holds points [b PE_POINTS, min(n_points,
// (b + 1) PE_POINTS)), the last block is the tail.  Pairs are numbered as everywhere else: pair = polynomial x n_points + point.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "poly_quotient_plan.hpp"

namespace kzg {

constexpr size_t PE_POINTS = 8;            // points per block: 1 KB of LDS for the wavefronts' sums (PQ_WAVES x 32 B per point)
constexpr size_t PE_THREADS = PQ_THREADS;  // lanes of a workgroup: the tile of the quotient scan
static_assert(PE_POINTS <= PE_THREADS, "thread u of a workgroup finishes point u of its block");

// blocks of n_points points, block b's first point and size (0 beyond the last block)
constexpr size_t pe_blocks(size_t n_points) { return (n_points + PE_POINTS - 1) / PE_POINTS; }
constexpr size_t pe_block_lo(size_t b) { return b * PE_POINTS; }
constexpr size_t pe_block_size(size_t n_points, size_t b) {
    return pe_block_lo(b) >= n_points ? 0 : (n_points - pe_block_lo(b) < PE_POINTS ? n_points - pe_block_lo(b) : PE_POINTS);
}
// grid: x = tiles of n coefficients, y = (polynomial, block) in this order; PE_THREADS lanes each
constexpr PqGrid pe_grid(size_t n, size_t polys, size_t n_points) { return PqGrid{(unsigned)pq_tiles(n), (unsigned)(polys * pe_blocks(n_points))}; }
constexpr size_t pe_poly_of(size_t y, size_t n_points) { return y / pe_blocks(n_points); }
constexpr size_t pe_block_of(size_t y, size_t n_points) { return y % pe_blocks(n_points); }
// the pair of slot u (u < pe_block_size) of block b of polynomial `poly` (counted within the launch)
constexpr size_t pe_pair(size_t poly, size_t n_points, size_t b, size_t u) { return poly * n_points + pe_block_lo(b) + u; }

}  // namespace kzg
