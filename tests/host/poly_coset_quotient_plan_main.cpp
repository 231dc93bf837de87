// Host program over kzg_rs_amd/csrc/poly_coset_quotient_plan.hpp (tests/test_poly_coset_quotient_plan_cpu.py): the limits, the words,
// the plan of a call given by its shapes, the root, and `run`: the load, the recombination and the check on the CPU exactly as the
// kernels of poly_coset_quotient_kernels.hpp compose them - cq_coset_constants, cq_call_constant, cq_batch_inverse, cq_load_index and
// cq_pieces_index with the lane's powers made as the lanes make them (cq_pow of the first index, then the step constant) - around a
// naive n-point transform, against schoolbook long division by X^n - 1.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "poly_coset_quotient_plan.hpp"

using namespace kzg;

static std::vector<size_t> csv(const char* s) {
    std::vector<size_t> v;
    if (!strcmp(s, "-")) return v;
    for (const char* p = s; *p;) {
        v.push_back(strtoull(p, (char**)&p, 10));
        if (*p == ',') p++;
    }
    return v;
}
static void print_fr(const Fr& a) {  // plain value, big-endian hex
    uint8_t b[32];
    FrF::to_be_bytes(b, a);
    for (int i = 0; i < 32; i++) printf("%02x", b[i]);
    printf("\n");
}
static Fr inv_pow(const Fr& a) {  // a^(r - 2), Montgomery form
    uint32_t e[8];
    for (int i = 0; i < 8; i++) e[i] = consts::FR_MOD[i];
    e[0] -= 2u, e[1] -= 1u;  // (the lowest word of r is 1: the borrow)
    return pow_limbs<Fr, 8>(a, e, FrF::one(), [](const Fr& x, const Fr& y) { return FrF::mul(x, y); });
}
static uint64_t rng_state;
static uint32_t rnd32() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 32);
}
static Fr rnd_mont() {  // a random residue, Montgomery form (any 256-bit value is reduced by the product with R^2)
    Fr a;
    for (int i = 0; i < 8; i++) a.l[i] = rnd32();
    a.l[7] &= 0x3fffffffu;
    return FrF::to_mont(a);
}
typedef std::vector<Fr> Poly;  // Montgomery form, lowest degree first
static Poly pmul(const Poly& a, const Poly& b) {
    Poly out(a.size() + b.size() - 1, FrF::zero());
    for (size_t i = 0; i < a.size(); i++)
        for (size_t j = 0; j < b.size(); j++) out[i + j] = FrF::add(out[i + j], FrF::mul(a[i], b[j]));
    return out;
}
// naive transform of plain values with the Montgomery root w: out[i] = sum_t in[t] w^(i t); inverse: w^-1 and 1 / n
static std::vector<Fr> dft(const std::vector<Fr>& in, const Fr& wM, bool inverse) {
    const size_t n = in.size();
    const Fr w = inverse ? inv_pow(wM) : wM;
    Fr scale = FrF::one();
    if (inverse) {
        Fr nM = FrF::one();
        for (size_t k = 1; k < n; k <<= 1) nM = FrF::dbl(nM);
        scale = inv_pow(nM);
    }
    std::vector<Fr> out(n);
    Fr wi = FrF::one();
    for (size_t i = 0; i < n; i++) {
        Fr acc = FrF::zero(), p = FrF::one();
        for (size_t t = 0; t < n; t++) {
            acc = FrF::add(acc, FrF::mul(p, in[t]));
            p = FrF::mul(p, wi);
        }
        out[i] = FrF::mul(scale, acc);
        wi = FrF::mul(wi, w);
    }
    return out;
}

template <int LOGD>
static bool pieces_all(const std::vector<std::vector<Fr>>& rows, std::vector<std::vector<Fr>>& T, const Fr* c, size_t n, uint32_t pieces) {
    bool rem = false;
    for (size_t tile = 0; tile < cq_tiles(n); tile++)
        for (size_t t = 0; t < CQ_THREADS; t++) {
            const uint32_t i0 = (uint32_t)cq_elem(tile, t, 0);
            Fr zM = cq_pow(c[cq_const_call() + CQ_K_ZETA_INV], i0), sM = cq_pow(c[cq_const_call() + CQ_K_G_INV], i0);
            for (size_t k = 0; k < CQ_PER_LANE; k++) {
                const size_t i = cq_elem(tile, t, k);
                if (i >= n) break;
                rem |= cq_pieces_index<LOGD>([&](int j) { return rows[j][i]; }, [&](int m, const Fr& v) { T[m][i] = v; }, c, zM, sM, pieces);
                zM = FrF::mul(zM, c[cq_const_call() + CQ_K_ZETA_INV_STEP]);
                sM = FrF::mul(sM, c[cq_const_call() + CQ_K_G_INV_STEP]);
            }
        }
    return rem;
}

// run n F len seed rem_k: F factors of `len` coefficients, the term prod p - (prod p mod X^n - 1); rem_k >= 0 adds c X^rem_k
static int run(size_t n, size_t F, size_t len, uint64_t seed, long rem_k) {
    rng_state = seed * 2654435761u + 12345;
    std::vector<Poly> polys(F);
    for (auto& p : polys) {
        p.resize(len);
        for (auto& x : p) x = rnd_mont();
    }
    Poly prod(1, FrF::one());
    for (auto& p : polys) prod = pmul(prod, p);
    Poly red(n, FrF::zero());
    for (size_t i = 0; i < prod.size(); i++) red[i % n] = FrF::add(red[i % n], prod[i]);
    Poly mono;
    if (rem_k >= 0) {
        mono.assign((size_t)rem_k + 1, FrF::zero());
        mono[(size_t)rem_k] = rnd_mont();
    }
    // sets: 0 = the factors (len), 1 = red (n), 2 = the monomial
    const size_t set_coeffs[3] = {len, n, mono.size()};
    std::vector<size_t> term_sizes = {F, 1};
    std::vector<uint32_t> factors;
    for (size_t k = 0; k < F; k++) factors.push_back(0), factors.push_back((uint32_t)k);
    factors.push_back(1), factors.push_back(0);
    if (rem_k >= 0) term_sizes.push_back(1), factors.push_back(2), factors.push_back(0);
    std::unique_ptr<CqPlan> plan(new CqPlan());
    const CqRefusal bad = cq_plan(*plan, set_coeffs, nullptr, rem_k >= 0 ? 3 : 2, term_sizes.data(), factors.data(), term_sizes.size(), n);
    if (bad != CQ_OK) {
        printf("refused %d\n", (int)bad);
        return 0;
    }
    const CqPlan& pl = *plan;
    const size_t D = pl.D, U = pl.pa.U;
    // the term coefficients: 1, -1, 1 (Montgomery form) - the sum is prod - red (+ mono)
    const Fr coef[3] = {FrF::one(), FrF::neg(FrF::one()), FrF::one()};
    // schoolbook: P, then long division from the top
    Poly P = prod;
    for (size_t i = 0; i < n; i++) P[i] = FrF::sub(P[i], red[i]);
    for (size_t i = 0; i < mono.size(); i++) P[i] = FrF::add(P[i], mono[i]);
    if (P.size() != pl.pa.L0) return printf("L0 mismatch\n"), 1;
    Poly q(pl.L, FrF::zero()), rest = P;
    for (size_t i = P.size() - 1; i >= n; i--) {
        q[i - n] = rest[i];
        rest[i - n] = FrF::add(rest[i - n], rest[i]);
    }
    bool want_rem = false;
    for (size_t i = 0; i < n; i++) want_rem |= !FrF::is_zero(rest[i]);
    // the sources as the device sees them: plain canonical
    std::vector<std::vector<Fr>> src(U);
    for (size_t u = 0; u < U; u++) {
        const Poly& p = pl.pa.ref[u].set == 0 ? polys[pl.pa.ref[u].poly] : pl.pa.ref[u].set == 1 ? red : mono;
        for (const Fr& x : p) src[u].push_back(FrF::from_mont(x));
    }
    // k_cq_constants
    std::vector<Fr> c(cq_const_count(), FrF::zero());
    Fr e[CQ_MAX_COSETS], pre[CQ_MAX_COSETS];
    for (uint32_t j = 0; j < D; j++) e[j] = cq_coset_constants(c.data(), pl.logn, pl.logD, j);
    for (uint32_t k = 0; k < CQ_CALL_CONSTS; k++) c[cq_const_call() + k] = cq_call_constant(pl.logn, pl.logD, k);
    cq_batch_inverse(c.data(), e, pre, (int)D, inv_pow);
    const Fr wn = cq_pow(cq_g(1 + pl.logn + pl.logD), (uint32_t)(2 * D));  // zeta^D = w_n
    std::vector<std::vector<Fr>> rows(D);
    for (uint32_t j = 0; j < D; j++) {
        const Fr cM = c[CQ_COSET_CONSTS * j + CQ_K_C], step = c[CQ_COSET_CONSTS * j + CQ_K_SIGMA_STEP];
        std::vector<std::vector<Fr>> ws(U, std::vector<Fr>(n));
        for (size_t tile = 0; tile < cq_tiles(n); tile++)
            for (size_t t = 0; t < CQ_THREADS; t++) {  // k_cq_load's lane
                Fr pw[CQ_PER_LANE];
                pw[0] = cq_pow(c[CQ_COSET_CONSTS * j + CQ_K_SIGMA], (uint32_t)cq_elem(tile, t, 0));
                for (size_t k = 1; k < CQ_PER_LANE; k++) pw[k] = FrF::mul(pw[k - 1], step);
                for (size_t u = 0; u < U; u++)
                    for (size_t k = 0; k < CQ_PER_LANE; k++) {
                        const size_t i = cq_elem(tile, t, k);
                        if (i >= n) continue;
                        ws[u][i] = cq_load_index([&](size_t at) { return src[u][at]; }, src[u].size(), n, i, cM, pw[k]);
                        if (FrF::geq_mod(ws[u][i])) return printf("load not canonical\n"), 1;
                    }
            }
        for (size_t u = 0; u < U; u++) ws[u] = dft(ws[u], wn, false);
        std::vector<Fr> sum(n, FrF::zero());  // k_poly_sop: the term's coefficient, then its factors' evaluations
        for (size_t t = 0; t < pl.pa.table.n_terms; t++)
            for (size_t i = 0; i < n; i++) {
                Fr p = coef[t];
                for (size_t f = 0; f < pl.pa.table.size[t]; f++) p = FrF::mul(p, FrF::to_mont(ws[pl.pa.table.slot[t][f]][i]));
                sum[i] = FrF::add(sum[i], FrF::from_mont(p));
            }
        rows[j] = dft(sum, wn, true);
    }
    std::vector<std::vector<Fr>> T(D, std::vector<Fr>(n, FrF::zero()));
    const bool rem = pl.logD == 1   ? pieces_all<1>(rows, T, c.data(), n, (uint32_t)pl.pieces)
                     : pl.logD == 2 ? pieces_all<2>(rows, T, c.data(), n, (uint32_t)pl.pieces)
                     : pl.logD == 3 ? pieces_all<3>(rows, T, c.data(), n, (uint32_t)pl.pieces)
                                    : pieces_all<4>(rows, T, c.data(), n, (uint32_t)pl.pieces);
    size_t wrong = 0;
    if (!want_rem)
        for (size_t m = 0; m < pl.pieces; m++)
            for (size_t i = 0; i < n; i++) {
                const Fr want = m * n + i < pl.L ? FrF::from_mont(q[m * n + i]) : FrF::zero();
                wrong += !FrF::eq(want, T[m][i]) || FrF::geq_mod(T[m][i]);
            }
    printf("D %zu pieces %zu U %zu flag %d want_flag %d wrong %zu\n", D, pl.pieces, U, (int)rem, (int)want_rem, wrong);
    return 0;
}

int main(int argc, char** argv) {
    const std::string cmd = argc > 1 ? argv[1] : "";
    if (cmd == "limits") {
        printf("%zu %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %u\n", CQ_MAX_COSETS, CQ_ROOT_LOG2, CQ_THREADS, CQ_PER_LANE, CQ_TILE, PA_MAX_SETS, PA_MAX_TERMS, PA_MAX_FACTORS,
               PA_MAX_SCALARS, FRNTT_MAX, cq_const_count(), CQ_NOT_DIVISIBLE_BIT);
        return 0;
    }
    if (cmd == "words") {
        for (int r = CQ_OK; r <= CQ_NOT_DIVISIBLE; r++) printf("%d %s\n", r, cq_refusal_words((CqRefusal)r));
        return 0;
    }
    if (cmd == "root") {
        Fr g = cq_root();
        print_fr(FrF::from_mont(g));
        for (int k = 0; k < CQ_ROOT_LOG2 - 1; k++) g = FrF::sqr(g);
        print_fr(FrF::from_mont(g));  // r - 1
        print_fr(FrF::from_mont(cq_g(20)));
        return 0;
    }
    if (cmd == "plan" && argc >= 6) {  // plan domain_n nulls set_coeffs set_polys term ...; a term: s.p,s.p,... or _
        const size_t n = strtoull(argv[2], nullptr, 10);
        const int nulls = atoi(argv[3]);
        std::vector<size_t> sc = csv(argv[4]), sp = csv(argv[5]), sizes;
        std::vector<uint32_t> fac;
        for (int a = 6; a < argc; a++) {
            size_t k = 0;
            if (strcmp(argv[a], "_"))
                for (const char* p = argv[a]; *p; k++) {
                    fac.push_back((uint32_t)strtoul(p, (char**)&p, 10));
                    p++;  // '.'
                    fac.push_back((uint32_t)strtoul(p, (char**)&p, 10));
                    if (*p == ',') p++;
                }
            sizes.push_back(k);
        }
        std::unique_ptr<CqPlan> plan(new CqPlan());
        const CqRefusal bad = cq_plan(*plan, nulls & 1 ? nullptr : sc.data(), strcmp(argv[5], "-") ? sp.data() : nullptr, sc.size(), nulls & 2 ? nullptr : sizes.data(),
                                      nulls & 4 ? nullptr : fac.data(), sizes.size(), n);
        printf("%d\n", (int)bad);
        if (bad == CQ_OK) {
            const CqPlan& pl = *plan;
            printf("%zu %zu %zu %zu %zu %zu %zu %d %d\n", pl.pa.L0, pl.D, pl.L, pl.pieces, pl.pa.U, pl.workspace, pl.M, pl.logn, pl.logD);
            printf("%u %u %u %u %zu %zu %zu\n", cq_grid_load(pl).x, cq_grid_load(pl).y, cq_grid_pieces(pl).x, cq_grid_sop(pl).x, cq_ntt_chunk(pl, pl.pa.U),
                   cq_ntt_chunks(pl, pl.pa.U), cq_ntt_reserve(pl));
            printf("%zu %zu %zu\n", cq_args_upload_bytes(pl), cq_args_consts_at(pl), cq_args_bytes(pl));
        }
        return 0;
    }
    if (cmd == "run" && argc == 7) return run(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), strtoull(argv[4], nullptr, 10), strtoull(argv[5], nullptr, 10), atol(argv[6]));
    fprintf(stderr, "usage: limits | words | root | plan ... | run n F len seed rem_k\n");
    return 2;
}
