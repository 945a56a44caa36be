// sp1_amd/csrc/fp256.hpp — arithmetic modulo an odd modulus of N 32-bit limbs (N = 8: the 256-bit base fields of the curve
// precompiles), for host and device code alike. The modulus is DATA: a Modulus<N> holds its limbs and the three numbers derived
// from them, so nothing here knows secp256k1's special form and the same code serves every 256-bit field (and, with N = 12,
// bls12-381's). csrc/rv64_bigmod.hpp is the host precedent: generic Montgomery CIOS and Fermat inversion.
//
// Values are canonical (not Montgomery) integers in [0, p), little-endian limbs: that is what the trace's byte columns hold.
//   add / sub / mul / inv        the field operations; mul is two CIOS passes (a b R^-1, then times R^2 R^-1), inv is a^(p-2)
//   mul_quotient                 the integer (a b - r) / p for r = a b mod p: what FieldOpCols calls `carry`. It is below 2^(32N), and
//                                division by the odd p is exact, so it equals the low N limbs of (a b - r) times p^-1 mod 2^(32N):
//                                two low-half products, no long division
// Every loop is over a constant bound and fully unrolled and every limb array is indexed by constants only, so on the device the
// limbs live in registers (a run-time index would send the array to scratch). inv's 32N-step loop stays rolled: it shifts the
// exponent instead of indexing it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define FP_HD __host__ __device__ __forceinline__

namespace sp1hip {
namespace fp256 {

template <int N> struct U {
    uint32_t w[N];
};

// p (odd), -p^-1 mod 2^32, R^2 mod p with R = 2^(32N), p^-1 mod R
template <int N> struct Modulus {
    uint32_t p[N];
    uint32_t r2[N];
    uint32_t pinv[N];
    uint32_t n0;
};

template <int N> FP_HD U<N> small(uint32_t v) {
    U<N> r;
#pragma unroll
    for (int i = 0; i < N; i++) r.w[i] = i == 0 ? v : 0u;
    return r;
}
template <int N> FP_HD U<N> from_limbs(const uint32_t (&v)[N]) {
    U<N> r;
#pragma unroll
    for (int i = 0; i < N; i++) r.w[i] = v[i];
    return r;
}
template <int N> FP_HD bool equal(const U<N>& a, const U<N>& b) {
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < N; i++) d |= a.w[i] ^ b.w[i];
    return d == 0;
}
template <int N> FP_HD U<N> select(bool c, const U<N>& x, const U<N>& y) {
    U<N> r;
#pragma unroll
    for (int i = 0; i < N; i++) r.w[i] = c ? x.w[i] : y.w[i];
    return r;
}
// r = a + b mod 2^(32N); returns the carry out
template <int N> FP_HD uint32_t add_carry(U<N>& r, const U<N>& a, const U<N>& b) {
    uint64_t c = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        c += (uint64_t)a.w[i] + b.w[i];
        r.w[i] = (uint32_t)c;
        c >>= 32;
    }
    return (uint32_t)c;
}
// r = a - b mod 2^(32N); returns the borrow out
template <int N> FP_HD uint32_t sub_borrow(U<N>& r, const U<N>& a, const U<N>& b) {
    uint32_t br = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        const uint64_t d = (uint64_t)a.w[i] - b.w[i] - br;
        r.w[i] = (uint32_t)d;
        br = (uint32_t)(d >> 32) & 1u;
    }
    return br;
}
// the low N limbs of a * b
template <int N> FP_HD U<N> mul_lo(const U<N>& a, const U<N>& b) {
    U<N> r = small<N>(0);
#pragma unroll
    for (int i = 0; i < N; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < N - i; j++) {
            const uint64_t s = (uint64_t)a.w[j] * b.w[i] + r.w[i + j] + c;
            r.w[i + j] = (uint32_t)s;
            c = s >> 32;
        }
    }
    return r;
}

// a b R^-1 mod p (CIOS: Koc, Acar, Kaliski 1996), for a b < p R; the result is reduced
template <int N> FP_HD U<N> mont_mul(const U<N>& a, const U<N>& b, const Modulus<N>& m) {
    uint32_t t[N + 2];
#pragma unroll
    for (int i = 0; i < N + 2; i++) t[i] = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < N; j++) {
            const uint64_t s = (uint64_t)a.w[j] * b.w[i] + t[j] + c;
            t[j] = (uint32_t)s;
            c = s >> 32;
        }
        uint64_t s = (uint64_t)t[N] + c;
        t[N] = (uint32_t)s;
        t[N + 1] = (uint32_t)(s >> 32);
        const uint32_t q = t[0] * m.n0;
        c = ((uint64_t)q * m.p[0] + t[0]) >> 32;
#pragma unroll
        for (int j = 1; j < N; j++) {
            const uint64_t s2 = (uint64_t)q * m.p[j] + t[j] + c;
            t[j - 1] = (uint32_t)s2;
            c = s2 >> 32;
        }
        s = (uint64_t)t[N] + c;
        t[N - 1] = (uint32_t)s;
        t[N] = t[N + 1] + (uint32_t)(s >> 32);
    }
    U<N> r, d;
#pragma unroll
    for (int i = 0; i < N; i++) r.w[i] = t[i];
    const uint32_t br = sub_borrow(d, r, from_limbs(m.p));
    return select(t[N] != 0 || br == 0, d, r);                   // t in [0, 2p): one subtraction
}

// (a + b) mod p for a, b < p; *quotient = (a + b - result) / p, 0 or 1
template <int N> FP_HD U<N> add(const U<N>& a, const U<N>& b, const Modulus<N>& m, uint32_t* quotient = nullptr) {
    U<N> s, d;
    const uint32_t cy = add_carry(s, a, b), br = sub_borrow(d, s, from_limbs(m.p));
    const bool ge = cy != 0 || br == 0;
    if (quotient) *quotient = ge ? 1u : 0u;
    return select(ge, d, s);
}
// (a - b) mod p for a, b < p
template <int N> FP_HD U<N> sub(const U<N>& a, const U<N>& b, const Modulus<N>& m) {
    U<N> d, e;
    const uint32_t br = sub_borrow(d, a, b);
    add_carry(e, d, from_limbs(m.p));
    return select(br != 0, e, d);
}
// a b mod p for a, b < p
template <int N> FP_HD U<N> mul(const U<N>& a, const U<N>& b, const Modulus<N>& m) {
    return mont_mul(mont_mul(a, b, m), from_limbs(m.r2), m);
}
// (a b - r) / p for r = a b mod p: exact, below 2^(32N)
template <int N> FP_HD U<N> mul_quotient(const U<N>& a, const U<N>& b, const U<N>& r, const Modulus<N>& m) {
    U<N> d;
    sub_borrow(d, mul_lo(a, b), r);
    return mul_lo(d, from_limbs(m.pinv));
}
// a^(p - 2) mod p: the inverse of a != 0, and 0 for 0 (no branch on the value, no loop that depends on it)
template <int N> FP_HD U<N> inv(const U<N>& a, const Modulus<N>& m) {
    U<N> e;
    sub_borrow(e, from_limbs(m.p), small<N>(2));
    const U<N> am = mont_mul(a, from_limbs(m.r2), m);
    U<N> r = mont_mul(small<N>(1), from_limbs(m.r2), m);
#pragma unroll 1
    for (int step = 0; step < 32 * N; step++) {
        r = mont_mul(r, r, m);
        if (e.w[N - 1] >> 31) r = mont_mul(r, am, m);            // the same bit in every lane: a uniform branch
#pragma unroll
        for (int i = N - 1; i > 0; i--) e.w[i] = (e.w[i] << 1) | (e.w[i - 1] >> 31);
        e.w[0] <<= 1;
    }
    return mont_mul(r, small<N>(1), m);
}

// The derived numbers of an odd modulus given by its limbs (host side, once per modulus; the code is plain enough to run anywhere).
template <int N> FP_HD Modulus<N> make_modulus(const uint32_t (&p)[N]) {
    Modulus<N> m;
    const U<N> pu = from_limbs(p);
    U<N> x = small<N>(1);                                        // p^-1 mod 2^k by Newton's iteration, k doubling from 1
    for (int bits = 1; bits < 32 * N; bits *= 2) {
        U<N> t;
        sub_borrow(t, small<N>(2), mul_lo(pu, x));
        x = mul_lo(x, t);
    }
    for (int i = 0; i < N; i++) m.p[i] = p[i], m.pinv[i] = x.w[i], m.r2[i] = 0;
    m.n0 = 0u - x.w[0];
    U<N> r = small<N>(1);                                        // 2^(64N) mod p by doubling
    for (int i = 0; i < 64 * N; i++) r = add(r, r, m);
    for (int i = 0; i < N; i++) m.r2[i] = r.w[i];
    return m;
}

}  // namespace fp256
}  // namespace sp1hip
