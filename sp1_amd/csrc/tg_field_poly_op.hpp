// sp1_amd/csrc/tg_field_poly_op.hpp — the field columns that tg_field_op.hpp's FieldOpCols does not state, for host and device code
// alike, on byte limbs over a modulus passed as data:
//   FieldInnerProductCols::populate              crates/core/machine/src/operations/field/field_inner_product.rs:L29-L103
//   FieldDenCols::populate                       .../field/field_den.rs:L29-L110
//   FieldOpCols::populate_conditional_op_and_carry   .../field/field_op.rs:L100-L200 (Uint256Ops, modulus 2^256)
// as sp1_amd/machines/riscv_more_trace.py restates them (_ed_field_ops: inner, den; family_shard_from: fill), which the tests compare
// every word with. (FieldSqrtCols needs nothing new: its multiplication shows the root in the result columns while the identity is
// root * root = u / v, which is the `shown` argument of field_mul_cols; its range is a FieldLtCols and its lsb is 0.)
//
// All four are one vanishing polynomial on byte limbs,
//     van(x) = a0(x) b0(x) [+ a1(x) b1(x)] + lin(x) - c(x) m(x),       van(256) = 0,
// whose quotient by (x - 256) is the witness: `lin` holds the terms without a product (minus the result; plus or minus the
// numerator of a denominator column; the sum and the addend of Uint256Ops), below byte 4N. field_poly_witness walks the coefficients
// from the top with constant indices, as field_mul_witness does, with a second product and the linear term.
#pragma once
#include "tg_field_op.hpp"

namespace sp1hip {
namespace tgf {

// One step per coefficient K, from the top down (a template recursion: K is a constant in every step). Coefficients are kept in
// two's complement in uint32_t, as in field_mul_witness: an event outside the preconditions wraps, on the host as on the device.
template <int N, int K, bool TWO, class Lin, class M>
TG_HD void field_poly_witness(Cursor& w, uint32_t acc, const uint32_t (&pa0)[4 * N], const uint32_t (&pb0)[4 * N], const uint32_t (&pa1)[4 * N],
                              const uint32_t (&pb1)[4 * N], const uint32_t (&pc)[4 * N], const Lin& lin, const M& m, uint32_t offset) {
    if constexpr (K >= 1) {
        constexpr int L = 4 * N, ML = M::LIMBS, LO = K < L ? 0 : K - L + 1, HI = K < L ? K : L - 1, MLO = K < ML ? 0 : K - ML + 1;
        uint32_t van = 0;
        if constexpr (K < L) van = lin(K);
#pragma unroll
        for (int i = LO; i <= HI; i++) van += pa0[i] * pb0[K - i];
        if constexpr (TWO) {
#pragma unroll
            for (int i = LO; i <= HI; i++) van += pa1[i] * pb1[K - i];
        }
#pragma unroll
        for (int i = MLO; i <= HI; i++) van -= pc[i] * m.byte(K - i);
        acc = van + 256u * acc;                                                                  // witness[K - 1] = van[K] + 256 witness[K]
        w.val(acc + offset);
        w.back();
        field_poly_witness<N, K - 1, TWO>(w, acc, pa0, pb0, pa1, pb1, pc, lin, m, offset);
    }
}

// result[4N] = shown, carry[4N] = c, witness[4N + M::LIMBS - 2] at column `col`
template <int N, bool TWO, class Lin, class M>
TG_HD void field_poly_cols(Cursor& w, uint32_t col, uint32_t row, const U<N>& shown, const U<N>& a0, const U<N>& b0, const U<N>& a1, const U<N>& b1,
                           const U<N>& c, const Lin& lin, const M& m, uint32_t offset) {
    constexpr int L = 4 * N, WITNESS = L + M::LIMBS - 2;
    w.seek(col, row);
    put_bytes(w, shown);
    put_bytes(w, c);
    uint32_t pa0[L], pb0[L], pa1[L], pb1[L], pc[L];
#pragma unroll
    for (int i = 0; i < L; i++) {
        pa0[i] = byte_of(a0, i), pb0[i] = byte_of(b0, i), pc[i] = byte_of(c, i);
        pa1[i] = TWO ? byte_of(a1, i) : 0u, pb1[i] = TWO ? byte_of(b1, i) : 0u;
    }
    w.seek(col + 2 * L + WITNESS - 1, row);
    field_poly_witness<N, WITNESS, TWO>(w, 0, pa0, pb0, pa1, pb1, pc, lin, m, offset);
}

// the linear terms: coefficient K < 4N of  sign * (plus - minus)
template <int N> struct LinDifference {
    const U<N>&plus, &minus;
    TG_HD uint32_t operator()(int k) const { return byte_of(plus, k) - byte_of(minus, k); }
};
template <int N> struct LinNegated {
    const U<N>& r;
    TG_HD uint32_t operator()(int k) const { return 0u - byte_of(r, k); }
};

// ------------------------------------------------------------------------------------------------------ FieldInnerProductCols
// (a0 b0 + a1 b1) mod p for reduced operands, and the exact quotient (a0 b0 + a1 b1 - r) / p: below 2p, so below 2^(32N), and had
// like fp256::mul_quotient from low halves only
template <int N> TG_HD U<N> inner_product(const U<N>& a0, const U<N>& b0, const U<N>& a1, const U<N>& b1, const Modulus<N>& m) {
    return fp256::add(fp256::mul(a0, b0, m), fp256::mul(a1, b1, m), m);
}
template <int N> TG_HD U<N> inner_product_quotient(const U<N>& a0, const U<N>& b0, const U<N>& a1, const U<N>& b1, const U<N>& r, const Modulus<N>& m) {
    U<N> s, d;
    fp256::add_carry(s, fp256::mul_lo(a0, b0), fp256::mul_lo(a1, b1));
    fp256::sub_borrow(d, s, r);
    return fp256::mul_lo(d, fp256::from_limbs(m.pinv));
}
// The columns of  a0 b0 + a1 b1 = r + c p
template <int N> TG_HD void field_inner_product_cols(Cursor& w, uint32_t col, uint32_t row, const U<N>& a0, const U<N>& b0, const U<N>& a1, const U<N>& b1,
                                                     const U<N>& r, const U<N>& c, const Modulus<N>& m, uint32_t offset) {
    field_poly_cols<N, true>(w, col, row, r, a0, b0, a1, b1, c, LinNegated<N>{r}, ModulusBytes<N>{m.p}, offset);
}

// ------------------------------------------------------------------------------------------------------------- FieldDenCols
// r = a / (1 + b) (sign) or a / (1 - b): the identity is  b r + r = a + c p  or  b r + a = r + c p. The quotient c is below p.
template <int N> TG_HD U<N> den_quotient(const U<N>& a, const U<N>& b, const U<N>& r, bool sign, const Modulus<N>& m) {
    U<N> s, d;
    fp256::add_carry(s, fp256::mul_lo(b, r), fp256::select(sign, r, a));
    fp256::sub_borrow(d, s, fp256::select(sign, a, r));
    return fp256::mul_lo(d, fp256::from_limbs(m.pinv));
}
template <int N> TG_HD void field_den_cols(Cursor& w, uint32_t col, uint32_t row, const U<N>& a, const U<N>& b, const U<N>& r, const U<N>& c, bool sign,
                                           const Modulus<N>& m, uint32_t offset) {
    const U<N> plus = fp256::select(sign, r, a), minus = fp256::select(sign, a, r);
    field_poly_cols<N, false>(w, col, row, r, b, r, b, r, c, LinDifference<N>{plus, minus}, ModulusBytes<N>{m.p}, offset);
}

// ------------------------------------------------------------------------------- the conditional operation with carry (Uint256Ops)
// is_mul a b + is_add (a + b) + c = result + carry 2^(32N): a product term only on a multiplication's row, the sum in the linear
// term on an addition's. The modulus has 4N + 1 byte limbs, [0] * 4N + [1] (ModulusTop of p = 0): 8N - 1 witness columns.
template <int N> struct LinOpAndCarry {
    const U<N>&a, &b, &c, &result;
    bool is_add;
    TG_HD uint32_t operator()(int k) const { return byte_of(c, k) - byte_of(result, k) + (is_add ? byte_of(a, k) + byte_of(b, k) : 0u); }
};
template <int N> TG_HD void field_op_and_carry_cols(Cursor& w, uint32_t col, uint32_t row, const U<N>& a, const U<N>& b, const U<N>& c, const U<N>& result,
                                                    const U<N>& carry, bool is_mul, uint32_t offset) {
    const U<N> zero = fp256::small<N>(0), a_mul = fp256::select(is_mul, a, zero);
    field_poly_cols<N, false>(w, col, row, result, a_mul, b, a_mul, b, carry, LinOpAndCarry<N>{a, b, c, result, !is_mul}, ModulusTop<N>{zero, 1u}, offset);
}

}  // namespace tgf
}  // namespace sp1hip
