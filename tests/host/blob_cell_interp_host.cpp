// Host build of kzg_rs_amd/csrc/blob_cell_interp.hpp for tests/test_blob_cells_cpu.py (no GPU needed: the header is plain C++): the
// five phases of k_blob_cell_scalars (blob_cell_kernels.hpp), lane after lane instead of side by side, a loop end where the kernel
// has a barrier.  Field elements cross as 8 little-endian 32-bit words (canonical residues); W is the table of w8192^e R', 9 limbs
// each.
#include <vector>

#include "blob_cell_interp.hpp"
using namespace kzg;
static void put(uint32_t* p, const uint32_t (&w)[8]) {
    for (int i = 0; i < 8; i++) p[i] = w[i];
}
extern "C" {
// coef: the 4 096 coefficients; r: the challenge.  r_pow, r_pow_g [128]: r^c and r^c g_c; w: the commitment's weight as lane 0
// writes it; s [64]: s_j; neg_i [64]: -I_i
void h_blob_cell_scalars(uint32_t* r_pow, uint32_t* r_pow_g, uint32_t* w, uint32_t* s, uint32_t* neg_i, const uint32_t* coef, const uint32_t* r,
                         const uint32_t* W) {
    std::vector<Fr29> rpow(BLOB_CELL_CELLS), part(BLOB_CELL_LANES), sent(BLOB_CELL_FE);
    auto load_w = [&](uint32_t e) {
        Fr29 x;
        for (int i = 0; i < 9; i++) x.l[i] = W[9 * e + i];
        return x;
    };
    auto load_a = [&](uint32_t k) {
        uint32_t t[8];
        for (int i = 0; i < 8; i++) t[i] = coef[8 * k + i];
        return fr29_from_words(t);
    };
    uint32_t rw[8];
    for (int i = 0; i < 8; i++) rw[i] = r[i];
    for (int t = 0; t < BLOB_CELL_CELLS; t++) {
        uint32_t a[8], b[8];
        blob_cell_phase_powers(t, rw, load_w, rpow.data(), a, b);
        put(r_pow + 8 * t, a);
        put(r_pow_g + 8 * t, b);
    }
    for (int t = 0; t < BLOB_CELL_LANES; t++) blob_cell_phase_s_part(t, load_w, rpow.data(), part.data());
    for (int t = 0; t < BLOB_CELL_FE; t++) {
        uint32_t s0[8];
        blob_cell_phase_s_fold(t, part.data(), sent.data(), s0);
        if (t == 0) put(w, s0);
        // (the kernel keeps s_j as an entry and writes s_0 alone; here every s_j comes back: the entry times 1 is the plain residue)
        uint32_t o[8];
        cell_fr_canonical(o, fr29_mul(sent[t], fr29_small(1u)));
        put(s + 8 * t, o);
    }
    for (int t = 0; t < BLOB_CELL_LANES; t++) blob_cell_phase_i_part(t, load_a, sent.data(), part.data());
    for (int t = 0; t < BLOB_CELL_FE; t++) {
        uint32_t o[8];
        blob_cell_phase_i_fold(t, part.data(), o);
        put(neg_i + 8 * t, o);
    }
}
}
