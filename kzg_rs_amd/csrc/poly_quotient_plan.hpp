// poly_quotient_plan.hpp - host planning of the coefficient-form openings (capi_poly.hpp) and the geometry of their device stage
// (poly_quotient_kernels.hpp): how the n coefficients of a polynomial fall into lanes, wavefronts and workgroup tiles, the grid of
// each of the three launches, how the (polynomial, point) pairs of a call are cut into chunks, and the sizes of the buffers.
// Plain C++, no HIP: tests/host/poly_quotient_plan_main.cpp builds it with g++ (tests/test_poly_quotient_plan_cpu.py).  Everything
// is constexpr, so the kernels read the same functions.
//
// p(X) = sum_(i<n) a_i X^i at z: the suffix Horner values H_i = a_i + z H_(i+1), H_n = 0, give y = H_0 and the quotient's
// coefficients q_i = H_(i+1).  A lane owns PQ_LANE consecutive coefficients, a wavefront 64 lanes' worth, a workgroup tile
// PQ_THREADS lanes' worth; tile t covers [t PQ_TILE, min(n, (t + 1) PQ_TILE)).  The carry INTO tile t is H at the first index
// behind it, i.e. what tile t + 1 and everything above it sum to: the carries chain from the last tile (carry 0) down to tile 0.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace kzg {

constexpr size_t PQ_LANE = 8;                        // coefficients per lane: 256 contiguous bytes
constexpr size_t PQ_WAVE = 64 * PQ_LANE;             // ... per wavefront
constexpr size_t PQ_THREADS = 256;                   // lanes of a workgroup, of all three launches
constexpr size_t PQ_WAVES = PQ_THREADS / 64;
constexpr size_t PQ_TILE = PQ_THREADS * PQ_LANE;     // ... per workgroup tile
constexpr int PQ_LANE_LOG2 = 3, PQ_TILE_LOG2 = 11;   // z^PQ_LANE and z^PQ_TILE by squarings
static_assert((size_t)1 << PQ_LANE_LOG2 == PQ_LANE && (size_t)1 << PQ_TILE_LOG2 == PQ_TILE, "the powers of z are made by squarings");
constexpr size_t PQ_MAX_COEFFS = (size_t)1 << 20;    // = the largest prepared point set
constexpr size_t PQ_MAX_OPENINGS = 4096;             // (polynomial, point) pairs of one call
constexpr size_t PQ_CHUNK_SCALARS = (size_t)1 << 23; // quotient scalars in flight: 256 MB of limbs
constexpr size_t PQ_NO_TILE = ~(size_t)0;

// tiles of n coefficients, and tile t's range
constexpr size_t pq_tiles(size_t n) { return (n + PQ_TILE - 1) / PQ_TILE; }
constexpr size_t pq_tile_lo(size_t t) { return t * PQ_TILE; }
constexpr size_t pq_tile_size(size_t n, size_t t) { return pq_tile_lo(t) >= n ? 0 : (n - pq_tile_lo(t) < PQ_TILE ? n - pq_tile_lo(t) : PQ_TILE); }
// the first coefficient of thread `thread` of tile t (it owns PQ_LANE from there; those at n and above read as 0)
constexpr size_t pq_lane_lo(size_t t, size_t thread) { return pq_tile_lo(t) + thread * PQ_LANE; }
// the tile whose sum enters tile t's carry first (PQ_NO_TILE: t is the last tile, its carry is 0)
constexpr size_t pq_carry_from(size_t tiles, size_t t) { return t + 1 < tiles ? t + 1 : PQ_NO_TILE; }
// the carry launch: ONE workgroup per pair, thread k scans the consecutive tiles [k run, (k + 1) run)
constexpr size_t pq_carry_run(size_t tiles) { return tiles ? (tiles + PQ_THREADS - 1) / PQ_THREADS : 1; }
// where pair q's tile t lies in the tile-sum and carry arrays of a chunk
constexpr size_t pq_tile_index(size_t tiles, size_t q, size_t t) { return q * tiles + t; }

// grids: x = tiles (tile sums, apply) or 1 (carries), y = the pairs of the chunk; PQ_THREADS lanes each
struct PqGrid {
    unsigned x, y;
};
constexpr PqGrid pq_grid_tiles(size_t n, size_t pairs) { return PqGrid{(unsigned)pq_tiles(n), (unsigned)pairs}; }
constexpr PqGrid pq_grid_carries(size_t pairs) { return PqGrid{1u, (unsigned)pairs}; }
// the commit's decode: one lane per coefficient, y = polynomials
constexpr PqGrid pq_grid_decode(size_t n, size_t polys) { return PqGrid{(unsigned)((n + PQ_THREADS - 1) / PQ_THREADS), (unsigned)polys}; }

// Pairs per chunk: as many as keep pairs x n_coeffs quotient scalars within PQ_CHUNK_SCALARS (at least one: n_coeffs <= PQ_MAX_COEFFS
// is below the cap), whole polynomials when the n_points pairs of one fit, so that a polynomial is uploaded once.
constexpr size_t pq_chunk_pairs(size_t n_coeffs, size_t n_points) {
    size_t m = n_coeffs ? PQ_CHUNK_SCALARS / n_coeffs : PQ_MAX_OPENINGS;
    if (m > PQ_MAX_OPENINGS) m = PQ_MAX_OPENINGS;
    if (m < 1) m = 1;
    if (n_points && m >= n_points) m -= m % n_points;
    return m;
}
constexpr size_t pq_chunks(size_t pairs, size_t chunk) { return (pairs + chunk - 1) / chunk; }
constexpr size_t pq_chunk_lo(size_t k, size_t chunk) { return k * chunk; }
constexpr size_t pq_chunk_size(size_t pairs, size_t k, size_t chunk) { return k * chunk >= pairs ? 0 : (pairs - k * chunk < chunk ? pairs - k * chunk : chunk); }
// the polynomials pairs [lo, lo + m) name: [first, last)
constexpr size_t pq_poly_first(size_t lo, size_t n_points) { return lo / n_points; }
constexpr size_t pq_poly_end(size_t lo, size_t m, size_t n_points) { return (lo + m - 1) / n_points + 1; }

// buffer sizes of a chunk of `pairs` pairs over `polys` polynomials
constexpr size_t pq_stage_bytes(size_t n_coeffs, size_t polys) { return 32 * n_coeffs * polys; }   // the coefficients as given
constexpr size_t pq_quotient_scalars(size_t n_coeffs, size_t pairs) { return n_coeffs * pairs; }   // q[pair][n_coeffs], the last one 0
constexpr size_t pq_tile_scalars(size_t n_coeffs, size_t pairs) { return pq_tiles(n_coeffs) * pairs; }  // tile sums; as many carries

}  // namespace kzg
