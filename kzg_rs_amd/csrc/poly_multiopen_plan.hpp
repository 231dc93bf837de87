// poly_multiopen_plan.hpp - host planning of the multi-point opening of resident polynomials at per-group point sets
// (capi_polys_multiopen.hpp, kernels: poly_multiopen_kernels.hpp): the limits, the argument validation, how the groups' polynomials,
// points and values are laid out, the union T of the groups' point sets, and the sizes of the buffers.
// Plain C++, no HIP: tests/host/poly_multiopen_plan_main.cpp builds it with g++ (tests/test_poly_multiopen_plan_cpu.py).  Everything
// is constexpr, so the kernels read the same functions and the same MoShape.
//
// The call covers `count` polynomials cut into n_groups consecutive groups; group g holds m_g polynomials [poly0, poly0 + m_g) and
// t_g points [pt0, pt0 + t_g) of the flat point list, and its values lie at ys[val0 + k t_g + a] for its polynomial k and point a.
// Per group the device runs t_g single-point scans of ONE folded polynomial F_g - the (F_g, s) pairs of the group, pair a at the
// group's point a - so a group takes t_g n_coeffs quotient scalars, within PQ_CHUNK_SCALARS whatever the group.
// T is the union of the groups' points AS FIELD VALUES: equality is decided on the canonical bytes (memcmp after the check against
// r), never by arithmetic.  t_index[j] = the index in T of flat point j; t_first[u] = the first flat point that holds T_u.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "poly_fold_plan.hpp"

namespace kzg {

constexpr size_t MO_MAX_GROUPS = 16;                                  // = KZG_MULTIOPEN_MAX_GROUPS
constexpr size_t MO_MAX_SET_POINTS = 8;                               // = KZG_MULTIOPEN_MAX_SET_POINTS
constexpr size_t MO_MAX_POINTS = MO_MAX_GROUPS * MO_MAX_SET_POINTS;   // of the flat point list, and of T
constexpr size_t MO_SCALAR_THREADS = 256;                             // lanes of the one workgroup of a scalar kernel
static_assert(MO_MAX_SET_POINTS * PQ_MAX_COEFFS <= PQ_CHUNK_SCALARS, "a group's scans stay within one chunk of quotient scalars");
static_assert(MO_MAX_POINTS + MO_MAX_GROUPS + 1 <= MO_SCALAR_THREADS, "a lane per point, per group and one for Z_T in the scalar kernels");

enum MoRefusal : int {
    MO_OK = 0,
    MO_NULL,          // a null pointer
    MO_GROUPS,        // n_groups == 0 or above MO_MAX_GROUPS
    MO_EMPTY_GROUP,   // an m_g of 0
    MO_EMPTY_SET,     // a t_g of 0
    MO_SET_POINTS,    // a t_g above MO_MAX_SET_POINTS
    MO_COUNT,         // sum m_g != count
    MO_OPENINGS,      // sum m_g t_g above PQ_MAX_OPENINGS
    MO_POINT_RANGE,   // a point >= r
    MO_GAMMA_RANGE,   // gamma >= r
    MO_EQUAL_POINTS,  // two equal points inside one group
    MO_Z_RANGE,       // z >= r
    MO_Z_IN_T,        // z is one of the points
};
constexpr const char* mo_refusal_words(MoRefusal r) {
    return r == MO_NULL            ? "null argument"
           : r == MO_GROUPS        ? "n_groups must be 1 .. 16"
           : r == MO_EMPTY_GROUP   ? "a group holds no polynomial"
           : r == MO_EMPTY_SET     ? "a group holds no point"
           : r == MO_SET_POINTS    ? "a group holds more than 8 points"
           : r == MO_COUNT         ? "the group sizes do not add up to count"
           : r == MO_OPENINGS      ? "more than 4096 openings"
           : r == MO_POINT_RANGE   ? "an evaluation point is not below r"
           : r == MO_GAMMA_RANGE   ? "a batching factor is not below r"
           : r == MO_EQUAL_POINTS  ? "two equal points in one group"
           : r == MO_Z_RANGE       ? "an evaluation point is not below r"
           : r == MO_Z_IN_T        ? "z is one of the opening points"
                                   : "";
}

struct MoGroup {
    uint32_t poly0, polys, pt0, pts, val0;  // the group's polynomials | its points in the flat list | its first value in ys
};
// what both scalar kernels read from device memory, and the host's view of a validated call
struct MoShape {
    uint32_t n_groups, count, n_points, n_values, n_union, max_pts, max_pairs, pad;  // sum t_g | sum m_g t_g | |T| | max t_g | max m_g t_g
    MoGroup g[MO_MAX_GROUPS];
    uint32_t t_index[MO_MAX_POINTS];
    uint32_t t_first[MO_MAX_POINTS];
};

// r, big-endian
constexpr uint8_t MO_R_BE[32] = {0x73, 0xED, 0xA7, 0x53, 0x29, 0x9D, 0x7D, 0x48, 0x33, 0x39, 0xD8, 0x08, 0x09, 0xA1, 0xD8, 0x05,
                                 0x53, 0xBD, 0xA4, 0x02, 0xFF, 0xFE, 0x5B, 0xFE, 0xFF, 0xFF, 0xFF, 0xFF, 0x00, 0x00, 0x00, 0x01};
constexpr int mo_cmp32(const uint8_t* a, const uint8_t* b) {
    for (int i = 0; i < 32; i++)
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    return 0;
}
constexpr bool mo_below_r(const uint8_t* be) { return mo_cmp32(be, MO_R_BE) < 0; }

// the group of polynomial i of the call (i < count)
constexpr uint32_t mo_group_of(const MoShape& sh, uint32_t i) {
    uint32_t g = 0;
    while (g + 1 < sh.n_groups && i >= sh.g[g].poly0 + sh.g[g].polys) g++;
    return g;
}
// is T_u one of group g's points?
constexpr bool mo_in_group(const MoShape& sh, uint32_t g, uint32_t u) {
    for (uint32_t a = 0; a < sh.g[g].pts; a++)
        if (sh.t_index[sh.g[g].pt0 + a] == u) return true;
    return false;
}

// The arguments of kzg_polys_multiopen_begin / kzg_verify_kzg_multiopen behind the null checks -> the shape, or the first refusal in
// the order of the list above.  points: sum t_g x 32 bytes, gamma: 32 bytes, big-endian.  count: the polynomials of the prover's
// range, or MO_COUNT_FROM_GROUPS for the verifier, whose commitments are as many as the groups say.
constexpr size_t MO_COUNT_FROM_GROUPS = ~(size_t)0;
constexpr MoRefusal mo_validate(MoShape& sh, const size_t* group_sizes, const size_t* set_sizes, size_t n_groups, size_t count, const uint8_t* points, const uint8_t* gamma) {
    if (!group_sizes || !set_sizes || !points || !gamma) return MO_NULL;
    if (n_groups == 0 || n_groups > MO_MAX_GROUPS) return MO_GROUPS;
    sh = MoShape{};
    for (size_t g = 0; g < n_groups; g++) {
        if (group_sizes[g] == 0) return MO_EMPTY_GROUP;
        if (set_sizes[g] == 0) return MO_EMPTY_SET;
        if (set_sizes[g] > MO_MAX_SET_POINTS) return MO_SET_POINTS;
    }
    size_t polys = 0, pts = 0, vals = 0;
    for (size_t g = 0; g < n_groups; g++) {
        if (group_sizes[g] > ~(size_t)0 - polys) return count == MO_COUNT_FROM_GROUPS ? MO_OPENINGS : MO_COUNT;  // (a sum that wraps is not count)
        polys += group_sizes[g];
    }
    if (count != MO_COUNT_FROM_GROUPS && polys != count) return MO_COUNT;
    if (polys > PQ_MAX_OPENINGS) return MO_OPENINGS;  // (t_g >= 1: at least as many openings; below, nothing can wrap)
    count = polys, polys = 0;
    for (size_t g = 0; g < n_groups; g++) {
        const size_t m = group_sizes[g], t = set_sizes[g];
        sh.g[g] = MoGroup{(uint32_t)polys, (uint32_t)m, (uint32_t)pts, (uint32_t)t, (uint32_t)vals};
        if (t > sh.max_pts) sh.max_pts = (uint32_t)t;
        if (m * t > sh.max_pairs) sh.max_pairs = (uint32_t)(m * t);
        polys += m, pts += t, vals += m * t;
    }
    if (vals > PQ_MAX_OPENINGS) return MO_OPENINGS;
    sh.n_groups = (uint32_t)n_groups, sh.count = (uint32_t)count, sh.n_points = (uint32_t)pts, sh.n_values = (uint32_t)vals;
    for (size_t j = 0; j < pts; j++)
        if (!mo_below_r(points + 32 * j)) return MO_POINT_RANGE;
    if (!mo_below_r(gamma)) return MO_GAMMA_RANGE;
    for (size_t g = 0; g < n_groups; g++)
        for (size_t a = 0; a < sh.g[g].pts; a++)
            for (size_t b = 0; b < a; b++)
                if (mo_cmp32(points + 32 * (sh.g[g].pt0 + a), points + 32 * (sh.g[g].pt0 + b)) == 0) return MO_EQUAL_POINTS;
    for (size_t j = 0; j < pts; j++) {  // the union, in the order of first appearance
        uint32_t u = 0;
        while (u < sh.n_union && mo_cmp32(points + 32 * j, points + 32 * sh.t_first[u]) != 0) u++;
        if (u == sh.n_union) sh.t_first[sh.n_union++] = (uint32_t)j;
        sh.t_index[j] = u;
    }
    return MO_OK;
}
// z of the second step (and of the verifier) against the shape's points
constexpr MoRefusal mo_check_z(const MoShape& sh, const uint8_t* points, const uint8_t* z) {
    if (!points || !z) return MO_NULL;
    if (!mo_below_r(z)) return MO_Z_RANGE;
    for (uint32_t u = 0; u < sh.n_union; u++)
        if (mo_cmp32(z, points + 32 * sh.t_first[u]) == 0) return MO_Z_IN_T;
    return MO_OK;
}

// grids: the linear combination is element-wise with the fold's lane map (pf_elem), x = its tiles; the scalar kernels are one workgroup
constexpr PqGrid mo_grid_lincomb(size_t n) { return PqGrid{(unsigned)pf_tiles(n), 1u}; }

// buffer sizes
constexpr size_t mo_h_scalars(size_t n_coeffs) { return n_coeffs ? n_coeffs : 1; }                                  // h, limbs (kept by the state)
constexpr size_t mo_fold_bytes(size_t n_coeffs) { return pf_fold_bytes(n_coeffs, 1); }                              // F_g, then M: big-endian, ONE polynomial
constexpr size_t mo_quotient_scalars(const MoShape& sh, size_t n_coeffs) { return pq_quotient_scalars(n_coeffs, sh.max_pts); }   // a group's t_g scans
constexpr size_t mo_tile_scalars(const MoShape& sh, size_t n_coeffs) { return pq_tile_scalars(n_coeffs, sh.max_pairs); }       // the values' pairs (>= t_g)
constexpr size_t mo_carry_scalars(const MoShape& sh, size_t n_coeffs) { return pq_tile_scalars(n_coeffs, sh.max_pts); }
constexpr size_t mo_zs_bytes(const MoShape& sh) { return 32 * (size_t)sh.n_values; }        // per group its points, once per polynomial (k_poly_eval_tiles reads pair q's z at zs[q])
constexpr size_t mo_ys_bytes(const MoShape& sh) { return 32 * (size_t)sh.n_values; }
constexpr size_t mo_factor_scalars(const MoShape& sh) { return (size_t)sh.count + 1; }      // c_i, then -Z_T(z)
// the state's small arguments on the device, 32-byte aligned pieces: the shape | the points | gamma | gamma^i (Montgomery) | w (Montgomery)
constexpr size_t mo_align32(size_t x) { return (x + 31) / 32 * 32; }
constexpr size_t mo_args_points_at() { return mo_align32(sizeof(MoShape)); }
constexpr size_t mo_args_gamma_at(const MoShape& sh) { return mo_args_points_at() + 32 * (size_t)sh.n_points; }
constexpr size_t mo_args_gpow_at(const MoShape& sh) { return mo_args_gamma_at(sh) + 32; }
constexpr size_t mo_args_w_at(const MoShape& sh) { return mo_args_gpow_at(sh) + 32 * (size_t)sh.count; }
constexpr size_t mo_args_bytes(const MoShape& sh) { return mo_args_w_at(sh) + 32 * (size_t)sh.n_points; }

}  // namespace kzg
