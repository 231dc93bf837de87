// data_column_plan.hpp - host planning of kzg_verify_data_column_sidecars (capi_data_columns.hpp): the column sidecars of ONE block
// as a uniform group.  Every sidecar brings one column index, m cells and m proofs against the block's m commitments, which are
// given once; the distinct ones among them - m', compared as bytes, first-seen order - are decoded once and their table rows are
// shared by every slot of the group.  Plain C++ without HIP calls, so that tests/host/data_column_plan_host.cpp builds it with g++;
// data_column_term below is also what the term-table kernel runs.
//
// Sidecar j is what cell_group_plan.hpp makes of a batch of m cells with the cell index column_indices[j] repeated:
//   BAD_INDEX  its column index is >= 128: the single call's KZG_BADARGS, nothing to launch
//   GROUP      everything else: slot g of the group, slots numbered in sidecar order (S of them)
// (m == 0 and m above the group's threshold never reach this plan: the entry point answers them itself.)  The shape is uniform:
// slot g holds dense cells [g m, (g + 1) m), touches one column, and cell k of EVERY slot belongs to distinct commitment ci[k].
// So the (slot, column) and (slot, commitment) counting sorts of the general plan shrink to one list shared by all slots: wlist,
// the cells 0 .. m - 1 sorted by commitment, stable - every weight is summed in ascending k.
#pragma once
#include "cell_group_plan.hpp"

namespace kzg {

// Layout of the group's decoded points and of its scalars, for S slots of m cells over m' distinct commitments:
//   points   [proofs S m | the block's m' distinct commitments | [tau^i]G1 64 | SKIP]
//   scalars  [r^k S m | r^k g_c S m | commitment weights m' PER SLOT | -I_i 64 per slot], g_c = h_c^64 of the slot's column
KZG_CG_HD inline uint32_t data_column_points(uint32_t S, uint32_t m, uint32_t mp) { return S * m + mp + CELL_GROUP_FE + 1; }
KZG_CG_HD inline uint32_t data_column_skip_point(uint32_t S, uint32_t m, uint32_t mp) { return S * m + mp + CELL_GROUP_FE; }
KZG_CG_HD inline uint32_t data_column_scalars(uint32_t S, uint32_t m, uint32_t mp) { return 2 * S * m + S * mp + CELL_GROUP_FE * S; }
// Term t of output o of slot g: output 0 = its m proofs with r^k; output 1 = the proofs with r^k g_c, the m' commitment rows -
// the SAME rows for every slot - with the slot's own weights, the 64 monomial points with -I_i; every entry beyond and every entry
// of a slot that is not live points at SKIP.  The lists are cell_group_term's for (n, m) = (m, m'), commitments at u0 = 0.
KZG_CG_HD inline CellGroupTerm data_column_term(uint32_t o, uint32_t t, uint32_t g, uint32_t S, uint32_t m, uint32_t mp, bool live) {
    const uint32_t nG = S * m;
    CellGroupTerm r;
    r.point = data_column_skip_point(S, m, mp);
    r.scalar = 0;
    if (!live) return r;
    if (t < m) {
        r.point = g * m + t;
        r.scalar = (o ? nG : 0u) + g * m + t;
    } else if (o && t < m + mp) {
        r.point = nG + (t - m);
        r.scalar = 2 * nG + g * mp + (t - m);
    } else if (o && t < m + mp + CELL_GROUP_FE) {
        r.point = nG + mp + (t - m - mp);
        r.scalar = 2 * nG + S * mp + CELL_GROUP_FE * g + (t - m - mp);
    }
    return r;
}

// The uniform group in the form the shared launch code reads (CellGroupPlan): "batch" j = sidecar j with m entries, so entry
// off[j] + k is cell k of sidecar j; uniq_entry[i] = the blob whose commitment is distinct commitment i; ci [m] = the transcript's
// commitment index of cell k, the same for every slot.  Of the device words only these are laid out (the others stay empty):
//   cstart [S + 1]   g m                    col_id [S]        the column index of slot g
//   wlist [m]        cells 0 .. m - 1 by commitment, stable   wstart [m' + 1]   range of `wlist` per distinct commitment
// (ustart is never read for this shape: every slot's commitments are dense commitments 0 .. m' - 1.)
inline void data_column_plan(CellGroupPlan& P, const uint8_t* commitments, size_t n_blobs, const uint64_t* column_indices, size_t n_sidecars) {
    P = CellGroupPlan();
    const uint32_t m = (uint32_t)n_blobs;
    P.kind.assign(n_sidecars, CELL_GROUP_EMPTY);
    P.off.assign(n_sidecars + 1, 0);
    for (size_t j = 0; j < n_sidecars; j++) {
        P.off[j + 1] = P.off[j] + n_blobs;
        P.kind[j] = column_indices[j] >= (uint64_t)CELL_GROUP_COLUMNS ? CELL_GROUP_BAD_INDEX : CELL_GROUP_GROUP;
        if (P.kind[j] == CELL_GROUP_GROUP) P.slot_batch.push_back((uint32_t)j);
    }
    const uint32_t S = P.G = (uint32_t)P.slot_batch.size();
    P.nG = S * m;
    P.ci.resize(m);
    cell_dedup(commitments, m, P.ci.data(), P.uniq_entry);
    const uint32_t mp = P.mtot = (uint32_t)P.uniq_entry.size();
    P.Utot = S;
    P.max_ll = m, P.max_rl = m + mp + CELL_GROUP_FE;
    P.o_cstart = 0, P.o_col_id = S + 1, P.o_wlist = P.o_col_id + S, P.o_wstart = P.o_wlist + m;
    P.o_ustart = P.o_colstart = P.o_cell_slot = P.o_cidx = P.o_order = P.o_col_start = P.o_wstart + mp + 1;
    P.idx.assign(P.o_wstart + mp + 1, 0u);
    uint32_t* const w = P.idx.data();
    for (uint32_t g = 0; g <= S; g++) w[P.o_cstart + g] = g * m;
    for (uint32_t g = 0; g < S; g++) w[P.o_col_id + g] = (uint32_t)column_indices[P.slot_batch[g]];
    std::vector<uint32_t> pos(mp + 1, 0u);
    for (uint32_t k = 0; k < m; k++) pos[P.ci[k] + 1]++;
    for (uint32_t i = 0; i < mp; i++) pos[i + 1] += pos[i];
    for (uint32_t i = 0; i <= mp; i++) w[P.o_wstart + i] = pos[i];
    for (uint32_t k = 0; k < m; k++) w[P.o_wlist + pos[P.ci[k]]++] = k;
}

}  // namespace kzg
