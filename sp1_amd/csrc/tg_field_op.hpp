// sp1_amd/csrc/tg_field_op.hpp — the pieces a precompile chip's trace row is made of, for host and device code alike: the cursor a
// lane writes its row with, the memory columns (SyscallAddrOperation, AddrAddOperation, MemoryAccessCols, the u8 form's low
// bytes), FieldOpCols and FieldLtCols over a modulus passed as data (fp256.hpp), and on top of them the whole rows of the two
// Weierstrass chips (point addition and doubling). The definitions followed are
//   FieldOpCols::populate_with_modulus   crates/core/machine/src/operations/field/field_op.rs:L224-L345
//   FieldLtCols::populate                crates/core/machine/src/operations/field/range.rs:L30-L61
//   MemoryAccessCols::populate           crates/core/machine/src/memory/consistency/trace.rs:L36-L101
//   SyscallAddrOperation::populate       crates/core/machine/src/operations/syscall_addr.rs:L27-L46
//   WeierstrassAddAssignChip             crates/core/machine/src/syscall/precompiles/weierstrass/weierstrass_add.rs:L95-L165, L246-L330
//   WeierstrassDoubleAssignChip          .../weierstrass/weierstrass_double.rs:L89-L160, L262-L380
// as sp1_amd/machines/riscv_more_trace.py restates them in Python integers (field_op_columns, _set_field_op, _set_field_lt,
// _syscall_addr_t, _mem_access_t, _low_bytes, secp256k1_{add,double}_shard_from), which the tests compare every word with. The
// column offsets are the #[repr(C)] order that riscv_more.weierstrass_add_chip / weierstrass_double_chip transcribe. The
// multiplication's witness and FieldLtCols also take a modulus that is a row's own data, with one byte limb more than the operands
// (ModulusTop, field_mul_cols_with, field_lt_cols_of): what tg_uint256_rows.hpp builds Uint256MulMod's row on.
//
// A table is column-major [width][height] Montgomery words; one lane (or one host loop iteration) owns one row and stores each
// value as it is made: a row is never held. Limb, byte and coefficient arrays are indexed by constants only (fully unrolled
// loops), so on the device they are registers.
#pragma once
#include "fp256.hpp"
#include "kb31.hpp"

#define TG_HD __host__ __device__ __forceinline__

namespace sp1hip {
namespace tgf {

// The cursor a lane writes its row with: one column per word(), in table order. The word index is (size_t) col * height + row
// (a full shard's table passes 2^30 bytes), kept as a running sum.
struct Cursor {
    uint32_t* out;
    size_t at, height;
    TG_HD void word(uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
        ((__attribute__((address_space(1))) uint32_t*)out)[at] = w;                            // a global store, not a flat one
#else
        out[at] = w;
#endif
        at += height;
    }
    TG_HD void bit(bool b) { word(b ? kb::R1 : 0u); }                                          // 0 or the Montgomery form of 1: a select
    TG_HD void val(uint32_t canonical) { word(kb::to_monty(canonical)); }
    TG_HD void limbs(uint64_t v, int n = 4) {
#pragma unroll
        for (int i = 0; i < 4; i++) if (i < n) val((uint32_t)(v >> (16 * i)) & 0xffffu);
    }
    TG_HD void bits64(uint64_t v) {
#pragma unroll 8
        for (int z = 0; z < 64; z++) bit((v >> z) & 1);
    }
    TG_HD void zeros(int n) {
        for (int i = 0; i < n; i++) word(0u);
    }
    TG_HD void seek(uint32_t col, uint32_t row) { at = (size_t)col * height + row; }
    TG_HD void back() { at -= 2 * height; }                                                    // the next word() goes one column to the left
};

// an event word: a global load on the device
TG_HD uint64_t event_word(const uint64_t* ev, int i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ((const __attribute__((address_space(1))) uint64_t*)ev)[i];
#else
    return ev[i];
#endif
}

// MemoryAccessCols: prev_value[4], prev_high, prev_low, compare_low, diff_low_limb, diff_high_limb. The difference to the previous
// access is taken on the low 24 bits when both stand in the same 2^24 window, on the high limbs otherwise.
TG_HD void memory_access(Cursor& w, uint64_t prev_value, uint64_t t_prev, uint64_t t_cur) {
    const uint32_t ph = (uint32_t)(t_prev >> 24), pl = (uint32_t)t_prev & 0xffffffu, ch = (uint32_t)(t_cur >> 24), cl = (uint32_t)t_cur & 0xffffffu;
    const bool same = ph == ch;
    const uint32_t d = (same ? cl - pl : ch - ph) - 1u;
    w.limbs(prev_value);
    w.val(ph);
    w.val(pl);
    w.bit(same);
    w.val(d & 0xffffu);
    w.val(d >> 16);
}
// MemoryAccessColsU8: the access, then prev_value_u8.low_bytes — the low byte of each 16-bit limb of the previous value
TG_HD void memory_access_u8(Cursor& w, uint64_t prev_value, uint64_t t_prev, uint64_t t_cur) {
    memory_access(w, prev_value, t_prev, t_cur);
#pragma unroll
    for (int k = 0; k < 4; k++) w.val((uint32_t)(prev_value >> (16 * k)) & 0xffu);
}
constexpr int MEMORY_ACCESS_U8_COLS = 13;

// SyscallAddrOperation: addr[3], top_two_limb_min = (addr[1] + addr[2])^-1, IsZero(addr[1] + addr[2] - 2 * 0xffff)
TG_HD void syscall_addr(Cursor& w, uint64_t addr) {
    w.limbs(addr, 3);
    const uint32_t top = ((uint32_t)(addr >> 16) & 0xffffu) + ((uint32_t)(addr >> 32) & 0xffffu);
    w.word(kb::inv(kb::to_monty(top)));                                                          // 0 for 0
    const uint32_t dmax = top == 2u * 0xffffu ? 0u : kb::P - (2u * 0xffffu - top);
    w.word(kb::inv(kb::to_monty(dmax)));
    w.bit(dmax == 0);
}
constexpr int SYSCALL_ADDR_COLS = 6;
// AddrAddOperation: the low three limbs of the sum
TG_HD void addr_add(Cursor& w, uint64_t sum) { w.limbs(sum, 3); }

// ---------------------------------------------------------------------------------------------------------------- field columns
template <int N> using U = fp256::U<N>;
template <int N> using Modulus = fp256::Modulus<N>;

template <int N> TG_HD uint32_t byte_of(const U<N>& a, int i) { return (a.w[i >> 2] >> (8 * (i & 3))) & 0xffu; }
template <int N> TG_HD uint32_t byte_of(const uint32_t (&a)[N], int i) { return (a[i >> 2] >> (8 * (i & 3))) & 0xffu; }
template <int N> TG_HD U<N> from_words(const uint64_t (&v)[N / 2]) {
    U<N> r;
#pragma unroll
    for (int i = 0; i < N / 2; i++) r.w[2 * i] = (uint32_t)v[i], r.w[2 * i + 1] = (uint32_t)(v[i] >> 32);
    return r;
}

// A FieldOpCols of 4N byte limbs: result[4N], carry[4N], witness[8N - 2].
template <int N> struct FieldOp {
    static constexpr int LIMBS = 4 * N, WITNESS = 2 * LIMBS - 2, COLS = 2 * LIMBS + WITNESS;
    static constexpr int RESULT = 0, CARRY = LIMBS, WITNESS_AT = 2 * LIMBS;
};
// A FieldLtCols: byte_flags[4N], lhs_comparison_byte, rhs_comparison_byte.
template <int N> struct FieldLt {
    static constexpr int LIMBS = 4 * N, COLS = LIMBS + 2;
    static constexpr int BYTE_FLAGS = 0, LHS_BYTE = LIMBS, RHS_BYTE = LIMBS + 1;
};

template <int N> TG_HD void put_bytes(Cursor& w, const U<N>& v) {
#pragma unroll
    for (int i = 0; i < 4 * N; i++) w.val(byte_of(v, i));
}

// The columns of the identity  a + b = r + c p  (c = 0 or 1) at column `col`: `shown` in the result columns (the sum for an
// addition; the difference for a subtraction, which is stated as difference + b = minuend), c, and the witness of
// (a + b - r - c p)(x) / (x - 256) on byte limbs, from the top coefficient down, plus `offset`. Above byte 4N - 1 the polynomial
// is zero and so is the quotient.
template <int N> TG_HD void field_add_cols(Cursor& w, uint32_t col, uint32_t row, const U<N>& shown, const U<N>& a, const U<N>& b, const U<N>& r,
                                           uint32_t c, const Modulus<N>& m, uint32_t offset) {
    constexpr int L = 4 * N;
    w.seek(col, row);
    put_bytes(w, shown);
    w.val(c);
    w.zeros(L - 1);
    const uint32_t zero = kb::to_monty(offset);
    w.seek(col + FieldOp<N>::WITNESS_AT + L - 1, row);
    for (int i = L - 1; i < FieldOp<N>::WITNESS; i++) w.word(zero);                             // witness[4N - 1 ..]
    w.seek(col + FieldOp<N>::WITNESS_AT + L - 2, row);
    uint32_t acc = 0;                                                                            // two's complement, see field_mul_witness
#pragma unroll
    for (int k = L - 1; k >= 1; k--) {                                                           // witness[k - 1] = van[k] + 256 witness[k]
        const uint32_t van = byte_of(a, k) + byte_of(b, k) - byte_of(r, k) - c * byte_of(m.p, k);
        acc = van + 256u * acc;
        w.val(acc + offset);
        w.back();
    }
}

// The modulus of a multiplication's witness as byte limbs: the 4N bytes of p, or (ModulusTop) those and one limb more on top, which
// is 1 for the modulus 2^(32N) — p = 0 — and 0 otherwise (Uint256MulMod, tg_uint256_rows.hpp). byte() takes constants only.
template <int N> struct ModulusBytes {
    static constexpr int LIMBS = 4 * N;
    const uint32_t (&p)[N];
    TG_HD uint32_t byte(int j) const { return byte_of(p, j); }
};
template <int N> struct ModulusTop {
    static constexpr int LIMBS = 4 * N + 1;
    const U<N>& p;
    uint32_t top;
    TG_HD uint32_t byte(int j) const { return j < 4 * N ? byte_of(p, j) : top; }
};

// The same for  a b = r + c p  with c a full 4N-byte quotient and p of M::LIMBS byte limbs (4N, or 4N + 1 with ModulusTop): 4N x 4N
// plus 4N x M::LIMBS byte products, 4N + M::LIMBS - 2 witness columns. One step per coefficient K, from the top down, as a template
// recursion: K is a constant in every step, so every byte index is, whatever the compiler's unroll limits.
// The signed coefficients (below 2^23 in magnitude while a b = r + c p holds) are kept in two's complement in uint32_t: an event
// with unreduced operands, for which the identity fails and the running value grows without bound, wraps instead of overflowing
// a signed integer, on the host as on the device.
template <int N, int K, class M> TG_HD void field_mul_witness(Cursor& w, uint32_t acc, const uint32_t (&pa)[4 * N], const uint32_t (&pb)[4 * N],
                                                              const uint32_t (&pc)[4 * N], const U<N>& r, const M& m, uint32_t offset) {
    if constexpr (K >= 1) {
        constexpr int L = 4 * N, ML = M::LIMBS, LO = K < L ? 0 : K - L + 1, HI = K < L ? K : L - 1, MLO = K < ML ? 0 : K - ML + 1;
        uint32_t van = 0;
        if constexpr (K < L) van = 0u - byte_of(r, K);
#pragma unroll
        for (int i = LO; i <= HI; i++) van += pa[i] * pb[K - i];
#pragma unroll
        for (int i = MLO; i <= HI; i++) van -= pc[i] * m.byte(K - i);
        acc = van + 256u * acc;                                                                  // witness[K - 1] = van[K] + 256 witness[K]
        w.val(acc + offset);
        w.back();
        field_mul_witness<N, K - 1>(w, acc, pa, pb, pc, r, m, offset);
    }
}
template <int N, class M> TG_HD void field_mul_cols_with(Cursor& w, uint32_t col, uint32_t row, const U<N>& shown, const U<N>& a, const U<N>& b,
                                                         const U<N>& r, const U<N>& c, const M& m, uint32_t offset) {
    constexpr int L = 4 * N, WITNESS = L + M::LIMBS - 2;
    w.seek(col, row);
    put_bytes(w, shown);
    put_bytes(w, c);
    uint32_t pa[L], pb[L], pc[L];
#pragma unroll
    for (int i = 0; i < L; i++) pa[i] = byte_of(a, i), pb[i] = byte_of(b, i), pc[i] = byte_of(c, i);
    w.seek(col + 2 * L + WITNESS - 1, row);
    field_mul_witness<N, WITNESS>(w, 0, pa, pb, pc, r, m, offset);
}
template <int N> TG_HD void field_mul_cols(Cursor& w, uint32_t col, uint32_t row, const U<N>& shown, const U<N>& a, const U<N>& b, const U<N>& r,
                                           const U<N>& c, const Modulus<N>& m, uint32_t offset) {
    field_mul_cols_with<N>(w, col, row, shown, a, b, r, c, ModulusBytes<N>{m.p}, offset);
}

// FieldLtCols for lhs < rhs (U<N>, or the limbs of a modulus): the flag at the most significant byte where they differ, and the
// two bytes there.
template <int N, class R> TG_HD void field_lt_cols_of(Cursor& w, uint32_t col, uint32_t row, const U<N>& lhs, const R& rhs) {
    constexpr int L = 4 * N;
    int at = L - 1;
    uint32_t lb = byte_of(lhs, L - 1), rb = byte_of(rhs, L - 1);
    bool found = false;
#pragma unroll
    for (int i = L - 1; i >= 0; i--) {
        const uint32_t x = byte_of(lhs, i), y = byte_of(rhs, i);
        const bool hit = !found && x != y;
        at = hit ? i : at;
        lb = hit ? x : lb;
        rb = hit ? y : rb;
        found = found || hit;
    }
    w.seek(col, row);
    for (int i = 0; i < L; i++) w.bit(i == at);
    w.val(lb);
    w.val(rb);
}
template <int N> TG_HD void field_lt_cols(Cursor& w, uint32_t col, uint32_t row, const U<N>& lhs, const Modulus<N>& m) {
    field_lt_cols_of<N>(w, col, row, lhs, m.p);
}

// The field operations of a row: each computes its result from reduced operands and writes its FieldOpCols at `col`.
template <int N> struct FieldOps {
    Cursor& w;
    uint32_t row;
    const Modulus<N>& m;
    uint32_t offset;
    TG_HD U<N> add(uint32_t col, const U<N>& a, const U<N>& b) {
        uint32_t c;
        const U<N> r = fp256::add(a, b, m, &c);
        field_add_cols(w, col, row, r, a, b, r, c, m, offset);
        return r;
    }
    TG_HD U<N> sub(uint32_t col, const U<N>& a, const U<N>& b) {                                 // result + b = a
        uint32_t c;
        const U<N> r = fp256::sub(a, b, m);
        const U<N> sum = fp256::add(r, b, m, &c);
        field_add_cols(w, col, row, r, r, b, sum, c, m, offset);
        return r;
    }
    TG_HD U<N> mul(uint32_t col, const U<N>& a, const U<N>& b) {
        const U<N> r = fp256::mul(a, b, m);
        field_mul_cols(w, col, row, r, a, b, r, fp256::mul_quotient(a, b, r, m), m, offset);
        return r;
    }
    TG_HD U<N> div(uint32_t col, const U<N>& a, const U<N>& b, const U<N>& b_inverse) {          // result * b = a
        const U<N> r = fp256::mul(a, b_inverse, m);
        const U<N> product = fp256::mul(r, b, m);
        field_mul_cols(w, col, row, r, r, b, product, fp256::mul_quotient(r, b, product, m), m, offset);
        return r;
    }
    TG_HD void lt(uint32_t col, const U<N>& lhs) { field_lt_cols(w, col, row, lhs, m); }
};

// ---------------------------------------------------------------------------------------------------- the Weierstrass chips' rows
// An affine point is N u64 words (N / 2 per coordinate, N 32-bit limbs per coordinate). Column offsets in #[repr(C)] order.
template <int N> struct WeierstrassAdd {
    static constexpr int WORDS = N, FO = FieldOp<N>::COLS;
    static constexpr int EVENT_WORDS = 3 + 4 * WORDS + WORDS;      // clk, p_ptr, q_ptr, WORDS x (t, p word), WORDS x (t, q word), WORDS written
    static constexpr int IS_REAL = 0, CLK_HIGH = 1, CLK_LOW = 2, P_PTR = 3, Q_PTR = P_PTR + SYSCALL_ADDR_COLS, P_ADDRS = Q_PTR + SYSCALL_ADDR_COLS,
                         Q_ADDRS = P_ADDRS + 3 * WORDS, P_ACCESS = Q_ADDRS + 3 * WORDS, Q_ACCESS = P_ACCESS + MEMORY_ACCESS_U8_COLS * WORDS,
                         SLOPE_DENOMINATOR = Q_ACCESS + MEMORY_ACCESS_U8_COLS * WORDS, INVERSE_CHECK = SLOPE_DENOMINATOR + FO,
                         SLOPE_NUMERATOR = INVERSE_CHECK + FO, SLOPE = SLOPE_NUMERATOR + FO, SLOPE_SQUARED = SLOPE + FO,
                         P_X_PLUS_Q_X = SLOPE_SQUARED + FO, X3_INS = P_X_PLUS_Q_X + FO, P_X_MINUS_X = X3_INS + FO, Y3_INS = P_X_MINUS_X + FO,
                         SLOPE_TIMES_P_X_MINUS_X = Y3_INS + FO, X3_RANGE = SLOPE_TIMES_P_X_MINUS_X + FO, Y3_RANGE = X3_RANGE + FieldLt<N>::COLS,
                         WIDTH = Y3_RANGE + FieldLt<N>::COLS;
};
template <int N> struct WeierstrassDouble {
    static constexpr int WORDS = N, FO = FieldOp<N>::COLS;
    static constexpr int EVENT_WORDS = 2 + 2 * WORDS + WORDS;      // clk, p_ptr, WORDS x (t, p word), WORDS written
    static constexpr int IS_REAL = 0, CLK_HIGH = 1, CLK_LOW = 2, P_PTR = 3, P_ADDRS = P_PTR + SYSCALL_ADDR_COLS, P_ACCESS = P_ADDRS + 3 * WORDS,
                         SLOPE_DENOMINATOR = P_ACCESS + MEMORY_ACCESS_U8_COLS * WORDS, SLOPE_NUMERATOR = SLOPE_DENOMINATOR + FO,
                         SLOPE = SLOPE_NUMERATOR + FO, P_X_SQUARED = SLOPE + FO, P_X_SQUARED_TIMES_3 = P_X_SQUARED + FO,
                         SLOPE_SQUARED = P_X_SQUARED_TIMES_3 + FO, P_X_PLUS_P_X = SLOPE_SQUARED + FO, X3_INS = P_X_PLUS_P_X + FO,
                         P_X_MINUS_X = X3_INS + FO, Y3_INS = P_X_MINUS_X + FO, SLOPE_TIMES_P_X_MINUS_X = Y3_INS + FO,
                         X3_RANGE = SLOPE_TIMES_P_X_MINUS_X + FO, Y3_RANGE = X3_RANGE + FieldLt<N>::COLS, WIDTH = Y3_RANGE + FieldLt<N>::COLS;
};
static_assert(WeierstrassAdd<8>::WIDTH == 1599 && WeierstrassDouble<8>::WIDTH == 1591 && WeierstrassAdd<8>::EVENT_WORDS == 43 &&
              WeierstrassDouble<8>::EVENT_WORDS == 26 && WeierstrassAdd<12>::WIDTH == 2399 && WeierstrassDouble<12>::WIDTH == 2391, "layouts");

// The head of a row that both chips share: is_real, clk_high, clk_low; zero on a padding row.
TG_HD void row_head(Cursor& w, bool real, uint64_t clk) {
    w.bit(real);
    w.val((uint32_t)(clk >> 24));
    w.val((uint32_t)clk & 0xffffffu);
}

// One row of a curve's AddAssign chip. `ev` = the event's words (the executor's record: clk, p_ptr, q_ptr, the reads of p and q
// with their previous timestamps, the words written), or null for a padding row: the reference's dummy row — the field
// operations on p = (0, 0), q = (1, 1), the dummy access record {value 1, timestamp 1, previous timestamp 0} in q_access[0] and
// q_access[WORDS / 2], zero elsewhere. q is read at clk, p rewritten at clk + 1. x3 and y3 are computed from the words read.
template <int N> TG_HD void weierstrass_add_row(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* ev, const Modulus<N>& m, uint32_t offset) {
    using C = WeierstrassAdd<N>;
    constexpr int W = C::WORDS, H = W / 2;
    const bool real = ev != nullptr;
    Cursor w{out, row, height};
    uint64_t pw[W], qw[W];
#pragma unroll
    for (int i = 0; i < W; i++) {
        pw[i] = real ? event_word(ev, 4 + 2 * i) : 0ull;
        qw[i] = real ? event_word(ev, 4 + 2 * W + 2 * i) : (i % H == 0 ? 1ull : 0ull);
    }
    if (real) {
        const uint64_t clk = event_word(ev, 0), p_ptr = event_word(ev, 1), q_ptr = event_word(ev, 2);
        row_head(w, true, clk);
        syscall_addr(w, p_ptr);
        syscall_addr(w, q_ptr);
        for (uint32_t i = 0; i < (uint32_t)W; i++) addr_add(w, p_ptr + 8u * i);
        for (uint32_t i = 0; i < (uint32_t)W; i++) addr_add(w, q_ptr + 8u * i);
#pragma unroll
        for (int i = 0; i < W; i++) memory_access_u8(w, pw[i], event_word(ev, 3 + 2 * i), clk + 1);
#pragma unroll
        for (int i = 0; i < W; i++) memory_access_u8(w, qw[i], event_word(ev, 3 + 2 * W + 2 * i), clk);
    } else {
        w.zeros(C::Q_ACCESS);
#pragma unroll
        for (int i = 0; i < W; i++) {
            if (i % H == 0) memory_access_u8(w, 1, 0, 1);
            else w.zeros(MEMORY_ACCESS_U8_COLS);
        }
    }
    uint64_t half[H];
#pragma unroll
    for (int i = 0; i < H; i++) half[i] = pw[i];
    const U<N> px = from_words<N>(half);
#pragma unroll
    for (int i = 0; i < H; i++) half[i] = pw[H + i];
    const U<N> py = from_words<N>(half);
#pragma unroll
    for (int i = 0; i < H; i++) half[i] = qw[i];
    const U<N> qx = from_words<N>(half);
#pragma unroll
    for (int i = 0; i < H; i++) half[i] = qw[H + i];
    const U<N> qy = from_words<N>(half);
    FieldOps<N> f{w, row, m, offset};
    const U<N> num = f.sub(C::SLOPE_NUMERATOR, qy, py);
    const U<N> den = f.sub(C::SLOPE_DENOMINATOR, qx, px);
    const U<N> den_inverse = fp256::inv(den, m);                   // one inversion per row
    f.div(C::INVERSE_CHECK, fp256::small<N>(1), den, den_inverse);
    const U<N> slope = f.div(C::SLOPE, num, den, den_inverse);
    const U<N> slope_squared = f.mul(C::SLOPE_SQUARED, slope, slope);
    const U<N> x_sum = f.add(C::P_X_PLUS_Q_X, px, qx);
    const U<N> x3 = f.sub(C::X3_INS, slope_squared, x_sum);
    f.lt(C::X3_RANGE, x3);
    const U<N> dx = f.sub(C::P_X_MINUS_X, px, x3);
    const U<N> sdx = f.mul(C::SLOPE_TIMES_P_X_MINUS_X, slope, dx);
    const U<N> y3 = f.sub(C::Y3_INS, sdx, py);
    f.lt(C::Y3_RANGE, y3);
}

// One row of a curve's DoubleAssign chip (y^2 = x^3 + a x + b: `a` reduced). p is rewritten in place at clk. A padding row (ev
// null) runs the field operations on p = (0, 1) with the dummy access record in p_access[WORDS / 2].
template <int N> TG_HD void weierstrass_double_row(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* ev, const Modulus<N>& m, const U<N>& a,
                                                   uint32_t offset) {
    using C = WeierstrassDouble<N>;
    constexpr int W = C::WORDS, H = W / 2;
    const bool real = ev != nullptr;
    Cursor w{out, row, height};
    uint64_t pw[W];
#pragma unroll
    for (int i = 0; i < W; i++) pw[i] = real ? event_word(ev, 3 + 2 * i) : (i == H ? 1ull : 0ull);
    if (real) {
        const uint64_t clk = event_word(ev, 0), p_ptr = event_word(ev, 1);
        row_head(w, true, clk);
        syscall_addr(w, p_ptr);
        for (uint32_t i = 0; i < (uint32_t)W; i++) addr_add(w, p_ptr + 8u * i);
#pragma unroll
        for (int i = 0; i < W; i++) memory_access_u8(w, pw[i], event_word(ev, 2 + 2 * i), clk);
    } else {
        w.zeros(C::P_ACCESS);
#pragma unroll
        for (int i = 0; i < W; i++) {
            if (i == H) memory_access_u8(w, 1, 0, 1);
            else w.zeros(MEMORY_ACCESS_U8_COLS);
        }
    }
    uint64_t half[H];
#pragma unroll
    for (int i = 0; i < H; i++) half[i] = pw[i];
    const U<N> px = from_words<N>(half);
#pragma unroll
    for (int i = 0; i < H; i++) half[i] = pw[H + i];
    const U<N> py = from_words<N>(half);
    FieldOps<N> f{w, row, m, offset};
    const U<N> xx = f.mul(C::P_X_SQUARED, px, px);
    const U<N> xx3 = f.mul(C::P_X_SQUARED_TIMES_3, xx, fp256::small<N>(3));
    const U<N> num = f.add(C::SLOPE_NUMERATOR, a, xx3);
    const U<N> den = f.mul(C::SLOPE_DENOMINATOR, fp256::small<N>(2), py);
    const U<N> slope = f.div(C::SLOPE, num, den, fp256::inv(den, m));
    const U<N> slope_squared = f.mul(C::SLOPE_SQUARED, slope, slope);
    const U<N> x_sum = f.add(C::P_X_PLUS_P_X, px, px);
    const U<N> x3 = f.sub(C::X3_INS, slope_squared, x_sum);
    f.lt(C::X3_RANGE, x3);
    const U<N> dx = f.sub(C::P_X_MINUS_X, px, x3);
    const U<N> sdx = f.mul(C::SLOPE_TIMES_P_X_MINUS_X, slope, dx);
    const U<N> y3 = f.sub(C::Y3_INS, sdx, py);
    f.lt(C::Y3_RANGE, y3);
}

}  // namespace tgf
}  // namespace sp1hip
