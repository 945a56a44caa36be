// sp1_amd/csrc/bn254.hpp — arithmetic in the BN254 scalar field for gfx950 device code (and the same code on the host).
//
// p = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001 < 2^254. An element is 8 little-endian u32 words
// in Montgomery form, R = 2^256 (the byte layout of halo2's Fr and of the C ABI); every function below takes and returns
// CANONICAL words (< p) unless its name says lazy.
//
// Multiplication: coarsely integrated operand scanning (CIOS) with 32-bit limbs, in the "no final carry" form: p's top limb
// is below 2^31 - 2, so the running sum t of each outer step fits in 8 limbs + the carry of the two inner chains and the
// 9th and 10th limbs of textbook CIOS never exist (the result is < 2p; one conditional subtraction makes it canonical).
// Each of the 8 outer steps is 8 multiply-accumulates of a_j b_i, one m = t_0 (-p^-1) mod 2^32 and 8 of m p_j.
// Two ways to issue a multiply-accumulate (DESIGN.md §Outer commitments records the measured choice):
//   MulForm::Mad   one v_mad_u64_u32 (32 x 32 + 64-bit addend) and a 64-bit add of the carry;
//   MulForm::LoHi  v_mul_lo_u32 + v_mul_hi_u32 and add-with-carry chains (the two multiplies issue at ~2x the rate of
//                  v_mad_u64_u32 on this chip, profiles/r01_ubench_int.txt, but the carries cost more adds).
// The linear layers of the permutation add lazily: 4p < 5p < 2^256, so a sum of three lanes plus a lane (or twice a lane)
// is exact in 256 bits and is brought back below p with conditional subtractions of 4p, 2p, p.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "outer_poseidon2_rc.inc"

#define BN_HD __host__ __device__ __forceinline__

namespace bn254 {

struct Fr { uint32_t w[8]; };

enum class MulForm { Mad, LoHi };

constexpr uint32_t NP = OUTER_NP;                  // -p^-1 mod 2^32
static_assert(NP == 0xefffffffu, "Montgomery constant of the BN254 scalar field");

BN_HD Fr P() { return Fr{OUTER_P_WORDS}; }
BN_HD Fr R1() { return Fr{OUTER_R_WORDS}; }        // Montgomery(1)
BN_HD Fr R2() { return Fr{OUTER_R2_WORDS}; }
BN_HD Fr zero() { return Fr{{0, 0, 0, 0, 0, 0, 0, 0}}; }
// k p for k = 1, 2, 4 (all < 2^256)
template <int K> BN_HD Fr p_times() {
    const uint32_t p[8] = OUTER_P_WORDS;
    Fr r;
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) { c += (uint64_t)p[i] * K; r.w[i] = (uint32_t)c; c >>= 32; }
    return r;
}

// r = a + b over 256 bits (the caller guarantees no overflow)
BN_HD Fr add_lazy(const Fr& a, const Fr& b) {
    Fr r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t s = (uint64_t)a.w[i] + b.w[i] + c;
        r.w[i] = (uint32_t)s;
        c = (uint32_t)(s >> 32);
    }
    return r;
}
// x >= m ? x - m : x
BN_HD Fr cond_sub(const Fr& x, const Fr& m) {
    Fr d;
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t s = (uint64_t)x.w[i] - m.w[i] - borrow;
        d.w[i] = (uint32_t)s;
        borrow = (uint32_t)(s >> 32) & 1u;
    }
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.w[i] = borrow ? x.w[i] : d.w[i];
    return r;
}
BN_HD Fr reduce_2p(const Fr& x) { return cond_sub(x, p_times<1>()); }                          // [0, 2p) -> [0, p)
BN_HD Fr reduce_4p(const Fr& x) { return reduce_2p(cond_sub(x, p_times<2>())); }               // [0, 4p) -> [0, p)
BN_HD Fr reduce_5p(const Fr& x) { return reduce_4p(cond_sub(x, p_times<4>())); }               // [0, 5p) -> [0, p)

BN_HD Fr add(const Fr& a, const Fr& b) { return reduce_2p(add_lazy(a, b)); }
BN_HD Fr dbl(const Fr& a) { return add(a, a); }
BN_HD Fr sub(const Fr& a, const Fr& b) {
    Fr d;
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const uint64_t s = (uint64_t)a.w[i] - b.w[i] - borrow;
        d.w[i] = (uint32_t)s;
        borrow = (uint32_t)(s >> 32) & 1u;
    }
    const Fr p = P();
    Fr r;
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {              // + p when a < b (wraps back into [0, p))
        const uint64_t s = (uint64_t)d.w[i] + (borrow ? p.w[i] : 0u) + c;
        r.w[i] = (uint32_t)s;
        c = (uint32_t)(s >> 32);
    }
    return r;
}

// canonical compare: -1, 0, 1
BN_HD int cmp(const Fr& a, const Fr& b) {
    int r = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) r = a.w[i] > b.w[i] ? 1 : (a.w[i] < b.w[i] ? -1 : r);
    return r;
}
BN_HD bool is_canonical(const Fr& a) { return cmp(a, P()) < 0; }
BN_HD bool eq(const Fr& a, const Fr& b) { return cmp(a, b) == 0; }

// lo(a b + t + c) -> returned, hi -> c
template <MulForm F> BN_HD uint32_t mac(uint32_t a, uint32_t b, uint32_t t, uint32_t& c) {
#if defined(__HIP_DEVICE_COMPILE__)
    if (F == MulForm::LoHi) {
        const uint32_t lo = a * b;
        uint32_t hi = __umulhi(a, b);
        const uint32_t s = lo + t;
        hi += s < t;
        const uint32_t r = s + c;
        hi += r < c;
        c = hi;
        return r;
    }
#endif
    const uint64_t r = (uint64_t)a * b + t + c;
    c = (uint32_t)(r >> 32);
    return (uint32_t)r;
}

// a b R^-1 mod p for a, b < p; result canonical
template <MulForm F = MulForm::Mad> BN_HD Fr mul(const Fr& a, const Fr& b) {
    const Fr p = P();
    uint32_t t[8];
#pragma unroll
    for (int j = 0; j < 8; j++) t[j] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint32_t A = 0, C = 0;
        t[0] = mac<F>(a.w[0], b.w[i], t[0], A);
        const uint32_t m = t[0] * NP;
        (void)mac<F>(m, p.w[0], t[0], C);      // low word is 0 by construction of m
#pragma unroll
        for (int j = 1; j < 8; j++) {
            t[j] = mac<F>(a.w[j], b.w[i], t[j], A);
            t[j - 1] = mac<F>(m, p.w[j], t[j], C);
        }
        t[7] = C + A;
    }
    Fr r;
#pragma unroll
    for (int j = 0; j < 8; j++) r.w[j] = t[j];
    return reduce_2p(r);
}
template <MulForm F = MulForm::Mad> BN_HD Fr sqr(const Fr& a) { return mul<F>(a, a); }
template <MulForm F = MulForm::Mad> BN_HD Fr to_monty(const Fr& canonical) { return mul<F>(canonical, R2()); }
template <MulForm F = MulForm::Mad> BN_HD Fr from_monty(const Fr& m) {
    Fr one = zero();
    one.w[0] = 1;
    return mul<F>(m, one);
}

// reduce_31: sum canonical(v_i) 2^(31 i), i < n <= 8 (v_i < 2^31: the sum is < 2^248 < p, canonical as an integer)
BN_HD Fr pack31(const uint32_t (&v)[8]) {
    Fr r = zero();
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int bit = 31 * i, k = bit >> 5, sh = bit & 31;
        r.w[k] |= v[i] << sh;
        if (sh > 1) r.w[k + 1] |= v[i] >> (32 - sh);
    }
    return r;
}

}  // namespace bn254
