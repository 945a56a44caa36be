// sp1_amd/csrc/bb31.hpp — BabyBear (p = 2^31 - 2^27 + 1) arithmetic and the Poseidon2 permutation of the BabyBear commit path
// (babybear.hip), for gfx950 device code and for the host. Words are Montgomery form, R = 2^32. The parameters and what pins
// them are stated in babybear.hip and oracle/bb_commit.hpp; tests/native/bb31_ops.hip includes this file unchanged and
// tests/test_bb31_arith.py checks every operation against Python integers.
//
// Range arguments (restated as arithmetic by test_bb31_arith.py::test_documented_bounds):
//   monty_reduce  x < 2^32 p: u = (x p^-1 mod 2^32) p < 2^32 p is congruent to x mod 2^32, so (x - u) / 2^32 is an integer in
//                 (-p, p) and one conditional addition of p brings it into [0, p).
//   add / sub     reduced words in, a reduced word out: a + b <= 2p - 2 < 2^32, a + p - b < 2p < 2^32.
//   internal_linear  the largest argument it passes to monty_reduce is 16 (p - 1) + (p - 1) 2^15 < 2^47, far inside 2^32 p.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define BB_HD __host__ __device__ __forceinline__

namespace sp1hip {
namespace bb {

constexpr uint32_t P = 0x78000001u;
constexpr uint32_t MU = 0x88000001u;             // p^-1 mod 2^32  (p MU = 1 mod 2^32)
constexpr int TWO_ADICITY = 27;
static_assert((uint32_t)(P * MU) == 1u, "Montgomery constant");

BB_HD uint32_t monty_reduce(uint64_t x) {       // x < 2^32 p  ->  x 2^-32 mod p
    const uint32_t t = (uint32_t)x * MU;
    const uint64_t u = (uint64_t)t * P;
    const uint32_t hi = (uint32_t)((x - u) >> 32);
    return x < u ? hi + P : hi;
}
BB_HD uint32_t add(uint32_t a, uint32_t b) { const uint32_t s = a + b; return s >= P ? s - P : s; }
BB_HD uint32_t sub(uint32_t a, uint32_t b) { return a >= b ? a - b : a + P - b; }
BB_HD uint32_t mul(uint32_t a, uint32_t b) { return monty_reduce((uint64_t)a * b); }
inline uint32_t to_monty(uint32_t c) {
    const uint64_t r = ((uint64_t)1 << 32) % P;
    return monty_reduce((uint64_t)(c % P) * (uint32_t)((r * r) % P));
}
inline uint32_t pow(uint32_t b, uint64_t e) { uint32_t r = to_monty(1); while (e) { if (e & 1) r = mul(r, b); b = mul(b, b); e >>= 1; } return r; }
inline uint32_t two_adic_generator(int bits) {
    uint32_t g = pow(to_monty(31), (P - 1) >> TWO_ADICITY);
    for (int i = bits; i < TWO_ADICITY; i++) g = mul(g, g);
    return g;
}

struct RoundConstants { uint32_t ext[8][16], internal[13]; };
static const uint32_t RC_CANONICAL[30][16] = {
#include "bb_poseidon2_rc.inc"
};
inline RoundConstants make_round_constants() {
    RoundConstants rc;
    for (int r = 0; r < 4; r++)
        for (int i = 0; i < 16; i++) { rc.ext[r][i] = to_monty(RC_CANONICAL[r][i]); rc.ext[4 + r][i] = to_monty(RC_CANONICAL[17 + r][i]); }
    for (int r = 0; r < 13; r++) rc.internal[r] = to_monty(RC_CANONICAL[4 + r][0]);
    return rc;
}

BB_HD void external_linear(uint32_t* s) {
#pragma unroll
    for (int j = 0; j < 16; j += 4) {
        const uint32_t x0 = s[j], x1 = s[j + 1], x2 = s[j + 2], x3 = s[j + 3];
        const uint32_t t01 = add(x0, x1), t23 = add(x2, x3), t0123 = add(t01, t23);
        const uint32_t t01123 = add(t0123, x1), t01233 = add(t0123, x3);
        s[j] = add(t01123, t01);
        s[j + 1] = add(t01123, add(x2, x2));
        s[j + 2] = add(t01233, t23);
        s[j + 3] = add(t01233, add(x0, x0));
    }
    uint32_t sums[4];
#pragma unroll
    for (int k = 0; k < 4; k++) sums[k] = add(add(s[k], s[k + 4]), add(s[k + 8], s[k + 12]));
#pragma unroll
    for (int j = 0; j < 16; j++) s[j] = add(s[j], sums[j & 3]);
}
// s_i <- (sum + d_i s_i) 2^-32, d = [-2, 1, 2, 4, ..., 2^13, 2^15]: one 64-bit sum, one shift-add and one reduction per lane
BB_HD void internal_linear(uint32_t* s) {
    uint64_t sum = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) sum += s[i];
    const uint64_t v0 = s[0], neg0 = v0 ? P - v0 : 0;
    const uint32_t n0 = monty_reduce(sum - v0 + neg0);
#pragma unroll
    for (int i = 1; i < 16; i++) s[i] = monty_reduce(sum + ((uint64_t)s[i] << (i == 15 ? 15 : i - 1)));
    s[0] = n0;
}
BB_HD uint32_t sbox(uint32_t x) {
    const uint32_t x2 = mul(x, x), x3 = mul(x2, x), x4 = mul(x2, x2);
    return mul(x4, x3);
}
BB_HD void permute(uint32_t* s, const RoundConstants* __restrict__ rc) {
    external_linear(s);
#pragma unroll 1
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int i = 0; i < 16; i++) s[i] = sbox(add(s[i], rc->ext[r][i]));
        external_linear(s);
    }
#pragma unroll 1
    for (int r = 0; r < 13; r++) {
        s[0] = sbox(add(s[0], rc->internal[r]));
        internal_linear(s);
    }
#pragma unroll 1
    for (int r = 4; r < 8; r++) {
#pragma unroll
        for (int i = 0; i < 16; i++) s[i] = sbox(add(s[i], rc->ext[r][i]));
        external_linear(s);
    }
}

}  // namespace bb
}  // namespace sp1hip
