// The statements of the GLV split (glv_split.hpp), for a scope that holds the canonical scalar `k` (Fr, plain limbs): they leave
// `Fr out` = k1 (limbs 0..3) | k2 (limbs 4..7).  Barrett with M = floor(2^383 / x^2): the quotient estimate is low by at most 1
// for k < 2^255.
    uint32_t prod[16];
#pragma unroll
    for (int j = 0; j < 16; j++) prod[j] = 0;
#pragma unroll
    for (int a = 0; a < 8; a++) {
        uint64_t c = 0;
#pragma unroll
        for (int b = 0; b < 8; b++) {
            uint64_t t = (uint64_t)k.l[a] * consts::GLV_M[b] + prod[a + b] + c;
            prod[a + b] = (uint32_t)t;
            c = t >> 32;
        }
        prod[a + 8] = (uint32_t)c;
    }
    uint32_t q[4];
#pragma unroll
    for (int j = 0; j < 4; j++) q[j] = (prod[11 + j] >> 31) | (prod[12 + j] << 1);
    // rem = k - q * L  (fits in 160 bits: rem < 2 L)
    uint32_t ql[8];
#pragma unroll
    for (int j = 0; j < 8; j++) ql[j] = 0;
#pragma unroll
    for (int a = 0; a < 4; a++) {
        uint64_t c = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            uint64_t t = (uint64_t)q[a] * consts::GLV_L[b] + ql[a + b] + c;
            ql[a + b] = (uint32_t)t;
            c = t >> 32;
        }
        ql[a + 4] = (uint32_t)c;
    }
    uint32_t rem[5], borrow = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) rem[j] = subb(k.l[j], ql[j], borrow);
    // if rem >= L: rem -= L, q += 1
    uint32_t d[5], bo = 0;
#pragma unroll
    for (int j = 0; j < 5; j++) d[j] = subb(rem[j], j < 4 ? consts::GLV_L[j] : 0u, bo);
    const bool ge = bo == 0;
    uint32_t carry = ge ? 1u : 0u;
    Fr out;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        out.l[j] = ge ? d[j] : rem[j];
        out.l[4 + j] = addc(q[j], 0u, carry);
    }
