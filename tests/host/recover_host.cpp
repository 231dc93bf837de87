// Host build of kzg_rs_amd/csrc/recover_ntt.hpp (over cell_ntt.hpp) for tests/test_cell_recover_cpu.py: the steps of the kernels
// of recover_kernels.hpp, element by element instead of lane by lane.  Field elements cross as 8 little-endian 32-bit words
// (canonical residues); W is the table of w8192^e R', 9 limbs each.
#include <vector>

#include "recover_ntt.hpp"
using namespace kzg;
static Fr29 ldw(const uint32_t* p) {
    uint32_t t[8];
    for (int i = 0; i < 8; i++) t[i] = p[i];
    return fr29_from_words(t);
}
static Fr29 ldt(const uint32_t* W, uint32_t e) {
    Fr29 r;
    for (int i = 0; i < 9; i++) r.l[i] = W[9 * e + i];
    return r;
}
static void stw(uint32_t* p, const Fr29& a) {
    uint32_t t[8];
    cell_fr_canonical(t, a);
    for (int i = 0; i < 8; i++) p[i] = t[i];
}
static int brp(int x, int bits) {
    int r = 0;
    for (int i = 0; i < bits; i++) r |= ((x >> i) & 1) << (bits - 1 - i);
    return r;
}
// in place, bit-reversed order in, natural order out
static void stages(std::vector<Fr29>& a, bool inverse, const uint32_t* W) {
    const int n = (int)a.size();
    for (int half = 1; half < n; half <<= 1)
        for (int j = 0; j < n / 2; j++) {
            const NttBfly b = cell_ntt_bfly(j, half, inverse);
            cell_ntt_apply(a[b.i0], a[b.i1], ldt(W, b.e));
        }
}
static void dump(uint32_t* trace, int step, const std::vector<Fr29>& a) {
    if (trace)
        for (int k = 0; k < RECOVER_N; k++) stw(trace + (step * RECOVER_N + k) * 8, a[k]);
}
extern "C" {
// k_recover_cell_idft: u[i] = 64 P_i(y_c) from the 64 entries of cell c
void h_recover_cell_u(uint32_t* u, const uint32_t* cell, int c, const uint32_t* W) {
    std::vector<Fr29> a(64);
    for (int j = 0; j < 64; j++) a[j] = ldw(cell + 8 * j);
    stages(a, true, W);
    for (int i = 0; i < 64; i++) stw(u + 8 * i, recover_mul(a[i], ldt(W, recover_pow_index((uint32_t)brp(c, 7), (uint32_t)i, true))));
}
// k_recover_vanishing, the build: z's 128 coefficients; miss[k] = cell brp7(k) is missing
void h_recover_vanish(uint32_t* z_out, const uint8_t* miss, const uint32_t* W) {
    std::vector<Fr29> z(RECOVER_N, fr29_small(0u));
    z[0] = fr29_small(1u);
    for (int k = 0; k < RECOVER_N; k++) {
        if (!miss[k]) continue;
        std::vector<Fr29> nz(RECOVER_N);
        for (int j = 0; j < RECOVER_N; j++) nz[j] = recover_vanish_step(j ? z[j - 1] : fr29_small(0u), z[j], ldt(W, 64u * k));
        z = nz;
    }
    for (int j = 0; j < RECOVER_N; j++) stw(z_out + 8 * j, z[j]);
}
// k_recover_vanishing, the tables: zev[c] = z(y_c) (by cell index) and zcos[k] = z(s w128^k), both canonical
void h_recover_tables(uint32_t* zev, uint32_t* zcos, const uint32_t* z, const uint32_t* W) {
    std::vector<Fr29> a(RECOVER_N), b(RECOVER_N);
    for (int j = 0; j < RECOVER_N; j++) {
        a[brp(j, 7)] = ldw(z + 8 * j);
        b[brp(j, 7)] = recover_mul(ldw(z + 8 * j), ldt(W, (uint32_t)j));
    }
    stages(a, false, W);
    stages(b, false, W);
    for (int k = 0; k < RECOVER_N; k++) {
        stw(zev + 8 * brp(k, 7), a[k]);
        stw(zcos + 8 * k, b[k]);
    }
}
// k_recover_poly for one i: u[c] = 64 P_i(y_c) (read where given[c]), zev[c], invz[k] = 1 / z(s w128^k) (canonical; the 2^-20 is
// applied here as in the kernel) -> p[k] = the 128 coefficients the kernel tests and stores, ev[c] = P_i(y_c) h_c^i; trace: the
// vectors after each of the seven steps in natural order (7 x 128 elements), with the scaling the kernel holds them in
void h_recover_poly(uint32_t* p, uint32_t* ev, uint32_t* trace, const uint32_t* u, const uint8_t* given, const uint32_t* zev, const uint32_t* invz, int i,
                    const uint32_t* W) {
    std::vector<Fr29> a(RECOVER_N), t(RECOVER_N), nat(RECOVER_N);
    for (int c = 0; c < RECOVER_N; c++) a[c] = given[c] ? recover_mul(ldw(u + 8 * c), recover_to_entry(ldw(zev + 8 * c))) : fr29_small(0u);
    for (int k = 0; k < RECOVER_N; k++) nat[k] = a[brp(k, 7)];
    dump(trace, 0, nat);
    stages(a, true, W);
    dump(trace, 1, a);
    for (int k = 0; k < RECOVER_N; k++) nat[k] = t[brp(k, 7)] = recover_mul(a[k], ldt(W, (uint32_t)k));
    dump(trace, 2, nat);
    a = t;
    stages(a, false, W);
    dump(trace, 3, a);
    for (int k = 0; k < RECOVER_N; k++) {
        uint32_t w[8];
        for (int l = 0; l < 8; l++) w[l] = invz[8 * k + l];
        nat[k] = t[brp(k, 7)] = recover_mul(a[k], recover_invz_entry(w));
    }
    dump(trace, 4, nat);
    a = t;
    stages(a, true, W);
    dump(trace, 5, a);
    for (int k = 0; k < RECOVER_N; k++) nat[k] = recover_mul(a[k], ldt(W, recover_pow_index(1u, (uint32_t)k, true)));
    dump(trace, 6, nat);
    for (int k = 0; k < RECOVER_N; k++) stw(p + 8 * k, nat[k]);
    for (int k = 0; k < RECOVER_N; k++) a[brp(k, 7)] = k < 64 ? nat[k] : fr29_small(0u);
    stages(a, false, W);
    for (int k = 0; k < RECOVER_N; k++) stw(ev + 8 * brp(k, 7), recover_mul(a[k], ldt(W, recover_pow_index((uint32_t)k, (uint32_t)i, false))));
}
// k_recover_cells: the 64 entries of a cell from ev[i] = P_i(y_c) h_c^i
void h_recover_cell_out(uint32_t* cell, const uint32_t* ev, const uint32_t* W) {
    std::vector<Fr29> a(64);
    for (int i = 0; i < 64; i++) a[brp(i, 6)] = ldw(ev + 8 * i);
    stages(a, false, W);
    for (int j = 0; j < 64; j++) stw(cell + 8 * j, a[brp(j, 6)]);
}
int h_recover_is_zero(const uint32_t* w) {
    uint32_t t[8];
    for (int i = 0; i < 8; i++) t[i] = w[i];
    return recover_is_zero(t) ? 1 : 0;
}
}
