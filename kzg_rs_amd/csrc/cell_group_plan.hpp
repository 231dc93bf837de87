// cell_group_plan.hpp - host planning of the cell verifiers: which batches of kzg_verify_cell_kzg_proof_batches
// (capi_cell_groups.hpp) ride in the group launch, and the index words the r -> scalars kernels (cell_kernels.hpp) read.
// kzg_verify_cell_kzg_proof_batch (capi_cells.hpp) plans its one batch here too, with a threshold no batch exceeds: G = 1.
// Plain C++ without HIP calls, so that tests/host/cell_group_plan_host.cpp builds it with g++; cell_group_term below is also what
// the term-table kernel runs.
//
// A call brings n_batches independent batches; batch b is entries [off[b], off[b + 1]) of the caller's arrays.  A batch is
//   EMPTY      no cells: true, nothing to launch
//   BAD_INDEX  a cell index >= 128: the single call's KZG_BADARGS, nothing to launch
//   LARGE      more than `threshold` cells: run through the single-batch path (its term list would not fit the window kernel's LDS list)
//   GROUP      everything else: slot g of the group launch, slots numbered in batch order
// The cells of the GROUP batches are numbered densely, slot after slot ("dense cell" q); the distinct commitments of a slot - compared
// as bytes, first-seen order, nothing shared between slots - likewise ("dense commitment" i), and its touched columns in ascending
// cell index ("dense column" u).  Every list below is a STABLE counting sort, so every device sum runs in ascending k within its
// batch, whichever entry point the batch came through.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#if defined(__HIPCC__)
#define KZG_CG_HD __host__ __device__
#else
#define KZG_CG_HD
#endif

namespace kzg {

// T: the largest batch that rides in the group launch.  Output 1 of a slot has at most 2 T + 64 = 576 terms, four chunk entries
// each: 2 308 words of the window kernel's 10 752-word LDS list, and the padding of every slot's tables to the longest stays small.
constexpr size_t CELL_GROUP_MAX_CELLS = 256;
constexpr size_t CELL_GROUP_MAX_BATCHES = 4096;  // batches per call
constexpr uint32_t CELL_GROUP_COLUMNS = 128, CELL_GROUP_FE = 64;

enum : uint8_t { CELL_GROUP_EMPTY = 0, CELL_GROUP_GROUP = 1, CELL_GROUP_LARGE = 2, CELL_GROUP_BAD_INDEX = 3 };

struct CellGroupTerm {
    uint32_t point, scalar;
};
// Layout of the group's decoded points and of its scalars, for nG dense cells, mtot dense commitments and G slots:
//   points   [proofs nG | distinct commitments mtot | [tau^i]G1 64 | SKIP], SKIP = the identity: its flag is set, so the window
//            kernel gives every term on it the digit 0
//   scalars  [r^k nG | r^k h^64 nG | commitment weights mtot | -I_i 64 per slot]
KZG_CG_HD inline uint32_t cell_group_points(uint32_t nG, uint32_t mtot) { return nG + mtot + CELL_GROUP_FE + 1; }
KZG_CG_HD inline uint32_t cell_group_skip_point(uint32_t nG, uint32_t mtot) { return nG + mtot + CELL_GROUP_FE; }
KZG_CG_HD inline uint32_t cell_group_scalars(uint32_t nG, uint32_t mtot, uint32_t G) { return 2 * nG + mtot + CELL_GROUP_FE * G; }
// Term t of output o of slot g (cells [c0, c0 + n), commitments [u0, u0 + m)): output 0 = the n proofs with r^k; output 1 = the
// proofs with r^k h^64, the m commitments with their weights, the 64 monomial points - shared by every slot - with -I_i; every
// entry beyond (the tables are padded to the group's longest list) and every entry of a slot that is not live points at SKIP.
KZG_CG_HD inline CellGroupTerm cell_group_term(uint32_t o, uint32_t t, uint32_t g, uint32_t c0, uint32_t n, uint32_t u0, uint32_t m, uint32_t nG,
                                               uint32_t mtot, bool live) {
    CellGroupTerm r;
    r.point = cell_group_skip_point(nG, mtot);
    r.scalar = 0;
    if (!live) return r;
    if (t < n) {
        r.point = c0 + t;
        r.scalar = (o ? nG : 0u) + c0 + t;
    } else if (o && t < n + m) {
        r.point = nG + u0 + (t - n);
        r.scalar = 2 * nG + u0 + (t - n);
    } else if (o && t < n + m + CELL_GROUP_FE) {
        r.point = nG + mtot + (t - n - m);
        r.scalar = 2 * nG + mtot + CELL_GROUP_FE * g + (t - n - m);
    }
    return r;
}

// ci[k] = index of commitment k among the distinct ones of the n given (compared as bytes), numbered in first-seen order;
// uniq gains base + the first k that holds distinct commitment i, for every i
inline void cell_dedup(const uint8_t* commitments, size_t n, uint32_t* ci, std::vector<uint32_t>& uniq, size_t base = 0) {
    std::unordered_map<std::string, uint32_t> seen;
    seen.reserve(n);
    for (size_t k = 0; k < n; k++) {
        auto it = seen.emplace(std::string(reinterpret_cast<const char*>(commitments + 48 * k), 48), (uint32_t)seen.size());
        if (it.second) uniq.push_back((uint32_t)(base + k));
        ci[k] = it.first->second;
    }
}

struct CellGroupPlan {
    std::vector<uint8_t> kind;     // [n_batches]
    std::vector<size_t> off;       // [n_batches + 1] prefix sums of batch_sizes
    std::vector<uint32_t> slot_batch;  // [G] batch of slot g
    std::vector<uint32_t> uniq_entry;  // [mtot] entry of the caller's arrays that holds dense commitment i (its first cell)
    std::vector<uint32_t> ci;          // [nG] commitment of dense cell q among its slot's distinct ones (the transcript's index)
    uint32_t G = 0, nG = 0, mtot = 0, Utot = 0;
    uint32_t max_ll = 0, max_rl = 0;   // the longest output 0 / output 1 list: max n, max (n + m + 64)
    // the device words, one upload: every array at its offset
    //   cstart [G + 1]   dense cell range of slot g          ustart [G + 1]    dense commitment range
    //   colstart [G + 1] dense column range                  cell_slot [nG]    slot of dense cell q
    //   cidx [nG]        cell index of dense cell q          order [nG]        dense cells by (slot, column), stable
    //   col_start [Utot + 1] range of `order` per dense column   col_id [Utot] its cell index
    //   wlist [nG]       dense cells by (slot, commitment), stable   wstart [mtot + 1] range of `wlist` per dense commitment
    std::vector<uint32_t> idx;
    size_t o_cstart = 0, o_ustart = 0, o_colstart = 0, o_cell_slot = 0, o_cidx = 0, o_order = 0, o_col_start = 0, o_col_id = 0, o_wlist = 0, o_wstart = 0;
};

// The batches given one by one: commitments[b] / cell_indices[b] = the batch_sizes[b] entries of batch b, wherever they lie (the
// requests of concurrent callers, capi_coalesce.hpp).  "Entry" e of the plan = off[b] + k, cell k of batch b, as if the arrays were one.
inline void cell_group_plan(CellGroupPlan& P, const uint8_t* const* commitments, const uint64_t* const* cell_indices, const size_t* batch_sizes,
                            size_t n_batches, size_t threshold) {
    P = CellGroupPlan();
    P.kind.assign(n_batches, CELL_GROUP_EMPTY);
    P.off.assign(n_batches + 1, 0);
    for (size_t b = 0; b < n_batches; b++) P.off[b + 1] = P.off[b] + batch_sizes[b];
    for (size_t b = 0; b < n_batches; b++) {
        const size_t n = batch_sizes[b];
        if (n == 0) continue;
        bool bad = false;
        for (size_t k = 0; k < n && !bad; k++) bad = cell_indices[b][k] >= (uint64_t)CELL_GROUP_COLUMNS;
        P.kind[b] = bad ? CELL_GROUP_BAD_INDEX : n > threshold ? CELL_GROUP_LARGE : CELL_GROUP_GROUP;
        if (P.kind[b] == CELL_GROUP_GROUP) {
            P.slot_batch.push_back((uint32_t)b);
            P.nG += (uint32_t)n;
        }
    }
    P.G = (uint32_t)P.slot_batch.size();
    const uint32_t G = P.G, nG = P.nG;
    // first pass: the distinct commitments and the touched columns of every slot
    std::vector<uint32_t> cstart(G + 1, 0), ustart(G + 1, 0), colstart(G + 1, 0), col_id;
    P.ci.resize(nG);
    const std::vector<uint32_t>& ci = P.ci;
    for (uint32_t g = 0; g < G; g++) {
        const size_t b = P.slot_batch[g], e0 = P.off[b], n = batch_sizes[b];
        cell_dedup(commitments[b], n, P.ci.data() + cstart[g], P.uniq_entry, e0);
        bool touched[CELL_GROUP_COLUMNS] = {};
        for (size_t k = 0; k < n; k++) touched[cell_indices[b][k]] = true;
        for (uint32_t c = 0; c < CELL_GROUP_COLUMNS; c++)
            if (touched[c]) col_id.push_back(c);
        cstart[g + 1] = cstart[g] + (uint32_t)n;
        ustart[g + 1] = (uint32_t)P.uniq_entry.size();
        colstart[g + 1] = (uint32_t)col_id.size();
        const uint32_t m = ustart[g + 1] - ustart[g];
        if ((uint32_t)n > P.max_ll) P.max_ll = (uint32_t)n;
        if ((uint32_t)n + m + CELL_GROUP_FE > P.max_rl) P.max_rl = (uint32_t)n + m + CELL_GROUP_FE;
    }
    P.mtot = (uint32_t)P.uniq_entry.size();
    P.Utot = (uint32_t)col_id.size();
    const uint32_t mtot = P.mtot, Utot = P.Utot;
    size_t o = 0;
    auto take = [&](size_t words) {
        const size_t at = o;
        o += words;
        return at;
    };
    P.o_cstart = take(G + 1), P.o_ustart = take(G + 1), P.o_colstart = take(G + 1), P.o_cell_slot = take(nG), P.o_cidx = take(nG), P.o_order = take(nG),
    P.o_col_start = take(Utot + 1), P.o_col_id = take(Utot), P.o_wlist = take(nG), P.o_wstart = take(mtot + 1);
    P.idx.assign(o + 1, 0u);
    uint32_t* const w = P.idx.data();
    for (uint32_t g = 0; g <= G; g++) w[P.o_cstart + g] = cstart[g], w[P.o_ustart + g] = ustart[g], w[P.o_colstart + g] = colstart[g];
    for (uint32_t u = 0; u < Utot; u++) w[P.o_col_id + u] = col_id[u];
    // second pass: the two counting sorts of every slot
    for (uint32_t g = 0; g < G; g++) {
        const uint64_t* const cix = cell_indices[P.slot_batch[g]];
        const uint32_t c0 = cstart[g], n = cstart[g + 1] - c0, u0 = ustart[g], m = ustart[g + 1] - u0, k0 = colstart[g], U = colstart[g + 1] - k0;
        uint32_t cnt[CELL_GROUP_COLUMNS + 1] = {};
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t c = (uint32_t)cix[k];
            w[P.o_cell_slot + c0 + k] = g;
            w[P.o_cidx + c0 + k] = c;
            cnt[c + 1]++;
        }
        for (uint32_t c = 0; c < CELL_GROUP_COLUMNS; c++) cnt[c + 1] += cnt[c];
        for (uint32_t u = 0; u < U; u++) w[P.o_col_start + k0 + u] = c0 + cnt[col_id[k0 + u]];
        for (uint32_t k = 0; k < n; k++) w[P.o_order + c0 + cnt[w[P.o_cidx + c0 + k]]++] = c0 + k;
        std::vector<uint32_t> pos(m + 1, 0u);
        for (uint32_t k = 0; k < n; k++) pos[ci[c0 + k] + 1]++;
        for (uint32_t i = 0; i < m; i++) pos[i + 1] += pos[i];
        for (uint32_t i = 0; i < m; i++) w[P.o_wstart + u0 + i] = c0 + pos[i];
        for (uint32_t k = 0; k < n; k++) w[P.o_wlist + c0 + pos[ci[c0 + k]]++] = c0 + k;
    }
    w[P.o_col_start + Utot] = nG;
    w[P.o_wstart + mtot] = nG;
}
// ... and given as one array each, batch after batch (kzg_verify_cell_kzg_proof_batches' arguments)
inline void cell_group_plan(CellGroupPlan& P, const uint8_t* commitments, const uint64_t* cell_indices, const size_t* batch_sizes, size_t n_batches,
                            size_t threshold) {
    std::vector<const uint8_t*> c(n_batches);
    std::vector<const uint64_t*> ix(n_batches);
    size_t off = 0;
    for (size_t b = 0; b < n_batches; b++) {
        c[b] = commitments + 48 * off;
        ix[b] = cell_indices + off;
        off += batch_sizes[b];
    }
    cell_group_plan(P, c.data(), ix.data(), batch_sizes, n_batches, threshold);
}

}  // namespace kzg
