// Host build of kzg_rs_amd/csrc/cell_group_plan.hpp for tests/test_cell_groups_cpu.py: the plan of both cell verifiers as the
// library makes it, and the term tables as the group call's kernel fills them (cell_group_term).
#include "cell_group_plan.hpp"
using namespace kzg;
extern "C" {
void* h_cg_plan(const uint8_t* commitments, const uint64_t* cell_indices, const size_t* batch_sizes, size_t n_batches, size_t threshold) {
    CellGroupPlan* p = new CellGroupPlan();
    cell_group_plan(*p, commitments, cell_indices, batch_sizes, n_batches, threshold);
    return p;
}
void h_cg_free(void* p) { delete static_cast<CellGroupPlan*>(p); }
// 0 G, 1 nG, 2 mtot, 3 Utot, 4 max_ll, 5 max_rl, 6 words of idx, 7.. the offsets of its arrays in declaration order, 17 the
// library's threshold, 18 the batches a call takes
size_t h_cg_number(const void* p_, int which) {
    const CellGroupPlan& p = *static_cast<const CellGroupPlan*>(p_);
    const size_t v[] = {p.G, p.nG, p.mtot, p.Utot, p.max_ll, p.max_rl, p.idx.size(), p.o_cstart, p.o_ustart, p.o_colstart, p.o_cell_slot, p.o_cidx,
                        p.o_order, p.o_col_start, p.o_col_id, p.o_wlist, p.o_wstart, CELL_GROUP_MAX_CELLS, CELL_GROUP_MAX_BATCHES};
    return v[which];
}
// 0 kind [n_batches], 1 slot_batch [G], 2 uniq_entry [mtot], 3 idx, 4 ci [nG]
void h_cg_array(const void* p_, int which, uint32_t* out) {
    const CellGroupPlan& p = *static_cast<const CellGroupPlan*>(p_);
    if (which == 0)
        for (size_t i = 0; i < p.kind.size(); i++) out[i] = p.kind[i];
    const std::vector<uint32_t>* v = which == 1 ? &p.slot_batch : which == 2 ? &p.uniq_entry : which == 3 ? &p.idx : which == 4 ? &p.ci : nullptr;
    if (v)
        for (size_t i = 0; i < v->size(); i++) out[i] = (*v)[i];
}
// the term tables [2 G][max_rl] as k_cell_terms writes them
void h_cg_terms(const void* p_, const uint32_t* live, uint32_t* term_point, uint32_t* term_scalar) {
    const CellGroupPlan& p = *static_cast<const CellGroupPlan*>(p_);
    const uint32_t* cstart = p.idx.data() + p.o_cstart;
    const uint32_t* ustart = p.idx.data() + p.o_ustart;
    for (uint32_t bo = 0; bo < 2 * p.G; bo++)
        for (uint32_t t = 0; t < p.max_rl; t++) {
            const uint32_t g = bo >> 1;
            const CellGroupTerm tm =
                cell_group_term(bo & 1, t, g, cstart[g], cstart[g + 1] - cstart[g], ustart[g], ustart[g + 1] - ustart[g], p.nG, p.mtot, live[g] != 0);
            term_point[(size_t)bo * p.max_rl + t] = tm.point;
            term_scalar[(size_t)bo * p.max_rl + t] = tm.scalar;
        }
}
uint32_t h_cg_skip_point(uint32_t nG, uint32_t mtot) { return cell_group_skip_point(nG, mtot); }
uint32_t h_cg_points(uint32_t nG, uint32_t mtot) { return cell_group_points(nG, mtot); }
uint32_t h_cg_scalars(uint32_t nG, uint32_t mtot, uint32_t G) { return cell_group_scalars(nG, mtot, G); }
}
