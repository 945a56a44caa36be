// sp1_amd/csrc/tg_field_chip_rows.hpp — the rows of the Weierstrass and Fp / Fp2 precompile chips behind SP1HIP_RV64_FAMILY_* 0..11,
// for host and device code alike, made in TWO PHASES from the pieces of tg_field_op.hpp and fp256.hpp:
//   Secp256r1 / Bn254 / Bls12381 AddAssign, DoubleAssign   weierstrass/weierstrass_add.rs:L95-L165, L246-L330; weierstrass_double.rs:L89-L160, L262-L380
//   Bn254 / Bls12381 FpOpAssign                            fptower/fp.rs:L150-L248
//   Bn254 / Bls12381 Fp2AddSubAssign                       fptower/fp2_addsub.rs:L160-L270
//   Bn254 / Bls12381 Fp2MulAssign                          fptower/fp2_mul.rs:L170-L290
// as sp1_amd/machines/riscv_more_trace.py restates them (family_shard_from, _secp_add_field_ops, _secp_double_field_ops,
// _fp_field_ops), which the tests compare every word with. Column offsets are the #[repr(C)] order that riscv_more.py transcribes.
//
// Why two phases. A whole row per lane as straight-line code (tg_field_op.hpp: weierstrass_add_row) holds ten FieldOpCols' worth of
// unrolled byte products in one function; at N = 12 limbs it needs scratch. Here
//   phase A   one lane per ROW: reads the event (clk, arg1, arg2, syscall code, then (previous timestamp, word) pairs, then the
//             words written — a FOUR-word head), writes the head columns (is_real, clk, selectors, SyscallAddrOperation,
//             AddrAddOperation, MemoryAccessColsU8), does the row's field arithmetic (fp256; one inversion per curve row), writes the
//             FieldLtCols, and leaves one RECORD per FieldOpCols of the row in a work buffer;
//   phase B   one lane per (ROW, FIELD OPERATION): reads its record and writes result, carry and witness with field_add_cols /
//             field_mul_cols. The operation index is uniform over the workgroup; the 4N x 4N byte product is compiled once per N.
// A record is the operands a, b and the reduced value r as FieldOps::add / sub / mul / div pass them to field_add_cols /
// field_mul_cols, then the operation kind: 3N + 1 words. The quotient is NOT stored: phase B recomputes it (an addition's is the
// carry of a + b against p, a product's is fp256::mul_quotient: two low-half products), which is cheaper than N more words written
// and read per operation. The buffer is laid out [op][word][row], so both phases' accesses are coalesced.
//
// A padding row (event null) is the reference's dummy row, made by the same code: curve add p = (0, 0), q = (1, 1) with the dummy
// access record in q_access[0] and q_access[WORDS / 2]; curve double p = (0, 1) with the record in p_access[WORDS / 2]; the tower
// chips the operation on zero operands as an addition (is_add = 1; Fp2Mul has no selector).
#pragma once
#include "tg_field_op.hpp"

namespace sp1hip {
namespace tgc {

using tgf::Cursor;
using tgf::FieldLt;
using tgf::FieldOp;
using tgf::Modulus;
using tgf::U;

enum : uint32_t { KIND_ADD = 0, KIND_SUB = 1, KIND_MUL = 2, KIND_DIV = 3 };     // a record's last word; the low three are an Fp call's code - base

// ------------------------------------------------------------------------------------------------------------ the work buffer
template <int N, int WORDS = 3 * N + 1> struct Work {
    static constexpr int REC = WORDS;                              // a[N], b[N], r[N], kind; EdAddAssign's (tg_ed_uint256_rows.hpp) has five operands
    static size_t words(uint32_t height, uint32_t ops) { return (size_t)ops * REC * height; }
};
TG_HD uint32_t work_word(const uint32_t* work, size_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return ((const __attribute__((address_space(1))) uint32_t*)work)[i];
#else
    return work[i];
#endif
}

// A chip's per-call constants besides the modulus: the curve's a (DoubleAssign), the system-call code of the chip's first
// operation (FpOpAssign: ADD, then SUB, MUL follow; Fp2AddSubAssign: ADD, then SUB), the witness offset
template <int N> struct ChipConsts {
    U<N> a;
    uint32_t code_base, offset;
};
// The column of each FieldOpCols of a chip, in record order: phase B's by-value table
constexpr int MAX_OPS = 11;
struct OpCols {
    uint32_t n, col[MAX_OPS];
};

// ------------------------------------------------------------------------------------------------------------------ head columns
// is_real, clk_high, clk_low, SEL selector columns, one or two SyscallAddrOperation, AddrAddOperation values and MemoryAccessColsU8
// of W words per operand. With two operands y is read at clk and x rewritten at clk + 1; a single operand is rewritten at clk.
template <int W, int SEL, bool TWO> struct Head {
    static constexpr int K = TWO ? 2 : 1;
    static constexpr int IS_REAL = 0, CLK_HIGH = 1, CLK_LOW = 2, SELECT = 3, X_PTR = 3 + SEL, Y_PTR = X_PTR + tgf::SYSCALL_ADDR_COLS,
                         X_ADDRS = X_PTR + K * tgf::SYSCALL_ADDR_COLS, Y_ADDRS = X_ADDRS + 3 * W, X_ACCESS = X_ADDRS + K * 3 * W,
                         Y_ACCESS = X_ACCESS + tgf::MEMORY_ACCESS_U8_COLS * W, END = X_ACCESS + K * tgf::MEMORY_ACCESS_U8_COLS * W;
    static constexpr int EVENT_WORDS = 4 + (TWO ? 5 : 3) * W, X_PAIRS = 4, Y_PAIRS = 4 + 2 * W;
};

// Columns [0, END) of a row. `selected`: the selector column that is 1 (is_add, is_sub, is_mul of SEL = 3; SEL = 1: 0 for is_add,
// anything else for none). dummy_x / dummy_y: the words whose access columns hold the dummy record on a padding row, as bit masks.
template <int W, int SEL, bool TWO>
TG_HD void head_cols(Cursor& w, const uint64_t* ev, const uint64_t (&xw)[W], const uint64_t (&yw)[W], uint32_t selected, uint32_t dummy_x, uint32_t dummy_y) {
    using H = Head<W, SEL, TWO>;
    if (ev != nullptr) {
        const uint64_t clk = tgf::event_word(ev, 0), x_ptr = tgf::event_word(ev, 1), y_ptr = tgf::event_word(ev, 2);
        tgf::row_head(w, true, clk);
#pragma unroll
        for (uint32_t s = 0; s < (uint32_t)SEL; s++) w.bit(s == selected);
        tgf::syscall_addr(w, x_ptr);
        if (TWO) tgf::syscall_addr(w, y_ptr);
        for (uint32_t i = 0; i < (uint32_t)W; i++) tgf::addr_add(w, x_ptr + 8u * i);
        if (TWO)
            for (uint32_t i = 0; i < (uint32_t)W; i++) tgf::addr_add(w, y_ptr + 8u * i);
#pragma unroll
        for (int i = 0; i < W; i++) tgf::memory_access_u8(w, xw[i], tgf::event_word(ev, H::X_PAIRS + 2 * i), TWO ? clk + 1 : clk);
        if (TWO) {
#pragma unroll
            for (int i = 0; i < W; i++) tgf::memory_access_u8(w, yw[i], tgf::event_word(ev, H::Y_PAIRS + 2 * i), clk);
        }
    } else {
        w.zeros(H::SELECT);
#pragma unroll
        for (uint32_t s = 0; s < (uint32_t)SEL; s++) w.bit(s == selected);
        w.zeros(H::X_ACCESS - H::X_PTR);
#pragma unroll
        for (int i = 0; i < W; i++) {
            if ((dummy_x >> i) & 1u) tgf::memory_access_u8(w, 1, 0, 1);
            else w.zeros(tgf::MEMORY_ACCESS_U8_COLS);
        }
        if (TWO) {
#pragma unroll
            for (int i = 0; i < W; i++) {
                if ((dummy_y >> i) & 1u) tgf::memory_access_u8(w, 1, 0, 1);
                else w.zeros(tgf::MEMORY_ACCESS_U8_COLS);
            }
        }
    }
}

// The operand words of a row: the words read of x (and y), or on a padding row `pad_x` / `pad_y` in the word that starts each field
// element selected by the bit mask (bit c: component c is 1, else 0)
template <int N, int W, bool TWO> TG_HD void operand_words(const uint64_t* ev, uint64_t (&xw)[W], uint64_t (&yw)[W], uint32_t pad_x, uint32_t pad_y) {
    using H = Head<W, 0, TWO>;
    constexpr int E = N / 2;                                       // u64 words of a field element
#pragma unroll
    for (int i = 0; i < W; i++) {
        xw[i] = ev ? tgf::event_word(ev, H::X_PAIRS + 1 + 2 * i) : (i % E == 0 ? (uint64_t)((pad_x >> (i / E)) & 1u) : 0ull);
        yw[i] = !TWO ? 0ull : ev ? tgf::event_word(ev, H::Y_PAIRS + 1 + 2 * i) : (i % E == 0 ? (uint64_t)((pad_y >> (i / E)) & 1u) : 0ull);
    }
}
// field element `c` (a constant) of an operand's words
template <int N, int W> TG_HD U<N> element(const uint64_t (&v)[W], int c) {
    U<N> r;
#pragma unroll
    for (int i = 0; i < N / 2; i++) r.w[2 * i] = (uint32_t)v[c * (N / 2) + i], r.w[2 * i + 1] = (uint32_t)(v[c * (N / 2) + i] >> 32);
    return r;
}

// ---------------------------------------------------------------------------------------------------------- phase A's operations
// tgf::FieldOps' interface — each operation computes its result from reduced operands — but instead of the FieldOpCols at `col` it
// leaves the record of operation (col - first) / FieldOp<N>::COLS. lt() writes its FieldLtCols to the table as FieldOps::lt does.
template <int N> struct Recorder {
    Cursor& w;
    uint32_t* work;
    uint32_t height, row;
    const Modulus<N>& m;
    uint32_t first;
    TG_HD void put(uint32_t col, const U<N>& a, const U<N>& b, const U<N>& r, uint32_t kind) {
        Cursor c{work, 0, height};
        c.seek((col - first) / FieldOp<N>::COLS * Work<N>::REC, row);
#pragma unroll
        for (int i = 0; i < N; i++) c.word(a.w[i]);
#pragma unroll
        for (int i = 0; i < N; i++) c.word(b.w[i]);
#pragma unroll
        for (int i = 0; i < N; i++) c.word(r.w[i]);
        c.word(kind);
    }
    TG_HD U<N> add(uint32_t col, const U<N>& a, const U<N>& b) {
        const U<N> r = fp256::add(a, b, m);
        put(col, a, b, r, KIND_ADD);
        return r;
    }
    TG_HD U<N> sub(uint32_t col, const U<N>& a, const U<N>& b) {                                 // result + b = a
        const U<N> r = fp256::sub(a, b, m);
        put(col, r, b, fp256::add(r, b, m), KIND_SUB);
        return r;
    }
    TG_HD U<N> mul(uint32_t col, const U<N>& a, const U<N>& b) {
        const U<N> r = fp256::mul(a, b, m);
        put(col, a, b, r, KIND_MUL);
        return r;
    }
    TG_HD U<N> div(uint32_t col, const U<N>& a, const U<N>& b, const U<N>& b_inverse) {          // result * b = a
        const U<N> r = fp256::mul(a, b_inverse, m);
        put(col, r, b, fp256::mul(r, b, m), KIND_DIV);
        return r;
    }
    TG_HD U<N> variable(uint32_t col, const U<N>& a, const U<N>& b, uint32_t kind) {             // FieldOpCols::populate of a row's own operation
        if (kind == KIND_ADD) return add(col, a, b);
        if (kind == KIND_SUB) return sub(col, a, b);
        return mul(col, a, b);
    }
    TG_HD void lt(uint32_t col, const U<N>& lhs) { tgf::field_lt_cols(w, col, row, lhs, m); }
};

// ------------------------------------------------------------------------------------------------------------------- the shapes
// A shape has LIMBS, WIDTH, EVENT_WORDS, OPS, FIRST_OP (the column of its first FieldOpCols; the others follow it) and
// phase_a(out, height, row, event or null, work, modulus, constants).
template <int N> struct CurveAdd {
    using C = tgf::WeierstrassAdd<N>;
    using H = Head<N, 0, true>;
    static constexpr int LIMBS = N, WIDTH = C::WIDTH, EVENT_WORDS = H::EVENT_WORDS, OPS = 10, FIRST_OP = C::SLOPE_DENOMINATOR;
    static_assert(H::X_PTR == C::P_PTR && H::Y_PTR == C::Q_PTR && H::X_ADDRS == C::P_ADDRS && H::Y_ADDRS == C::Q_ADDRS && H::X_ACCESS == C::P_ACCESS &&
                  H::Y_ACCESS == C::Q_ACCESS && H::END == FIRST_OP && FIRST_OP + OPS * FieldOp<N>::COLS == C::X3_RANGE, "layout");
    static TG_HD void phase_a(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* ev, uint32_t* work, const Modulus<N>& m, const ChipConsts<N>&) {
        Cursor w{out, row, height};
        uint64_t pw[N], qw[N];
        operand_words<N, N, true>(ev, pw, qw, 0u, 3u);                                           // padding: p = (0, 0), q = (1, 1)
        head_cols<N, 0, true>(w, ev, pw, qw, 0u, 0u, 1u | 1u << (N / 2));
        const U<N> px = element<N>(pw, 0), py = element<N>(pw, 1), qx = element<N>(qw, 0), qy = element<N>(qw, 1);
        Recorder<N> f{w, work, height, row, m, (uint32_t)FIRST_OP};
        const U<N> num = f.sub(C::SLOPE_NUMERATOR, qy, py);
        const U<N> den = f.sub(C::SLOPE_DENOMINATOR, qx, px);
        const U<N> den_inverse = fp256::inv(den, m);               // one inversion per row
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
};

template <int N> struct CurveDouble {
    using C = tgf::WeierstrassDouble<N>;
    using H = Head<N, 0, false>;
    static constexpr int LIMBS = N, WIDTH = C::WIDTH, EVENT_WORDS = H::EVENT_WORDS, OPS = 11, FIRST_OP = C::SLOPE_DENOMINATOR;
    static_assert(H::X_PTR == C::P_PTR && H::X_ADDRS == C::P_ADDRS && H::X_ACCESS == C::P_ACCESS && H::END == FIRST_OP &&
                  FIRST_OP + OPS * FieldOp<N>::COLS == C::X3_RANGE, "layout");
    static TG_HD void phase_a(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* ev, uint32_t* work, const Modulus<N>& m, const ChipConsts<N>& k) {
        Cursor w{out, row, height};
        uint64_t pw[N], none[N];
        operand_words<N, N, false>(ev, pw, none, 2u, 0u);                                        // padding: p = (0, 1)
        head_cols<N, 0, false>(w, ev, pw, none, 0u, 1u << (N / 2), 0u);
        const U<N> px = element<N>(pw, 0), py = element<N>(pw, 1);
        Recorder<N> f{w, work, height, row, m, (uint32_t)FIRST_OP};
        const U<N> xx = f.mul(C::P_X_SQUARED, px, px);
        const U<N> xx3 = f.mul(C::P_X_SQUARED_TIMES_3, xx, fp256::small<N>(3));
        const U<N> num = f.add(C::SLOPE_NUMERATOR, k.a, xx3);
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
};

// The operation of a tower row: the system call's low byte (event word 3) minus the chip's first code; a padding row adds
TG_HD uint32_t row_kind(const uint64_t* ev, uint32_t code_base) { return ev ? ((uint32_t)tgf::event_word(ev, 3) & 0xffu) - code_base : KIND_ADD; }

// FpOpAssign: is_add, is_sub, is_mul; x, y of N / 2 words; output, output_range
template <int N> struct FpOp {
    static constexpr int W = N / 2;
    using H = Head<W, 3, true>;
    static constexpr int LIMBS = N, EVENT_WORDS = H::EVENT_WORDS, OPS = 1, FIRST_OP = H::END, OUTPUT = FIRST_OP, OUTPUT_RANGE = OUTPUT + FieldOp<N>::COLS,
                         WIDTH = OUTPUT_RANGE + FieldLt<N>::COLS;
    static TG_HD void phase_a(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* ev, uint32_t* work, const Modulus<N>& m, const ChipConsts<N>& k) {
        Cursor w{out, row, height};
        uint64_t xw[W], yw[W];
        operand_words<N, W, true>(ev, xw, yw, 0u, 0u);
        const uint32_t kind = row_kind(ev, k.code_base);
        head_cols<W, 3, true>(w, ev, xw, yw, kind, 0u, 0u);
        Recorder<N> f{w, work, height, row, m, (uint32_t)FIRST_OP};
        f.lt(OUTPUT_RANGE, f.variable(OUTPUT, element<N>(xw, 0), element<N>(yw, 0), kind));
    }
};

// Fp2AddSubAssign: is_add; x, y of N words (c0, c1); c0, c1, c0_range, c1_range
template <int N> struct Fp2AddSub {
    using H = Head<N, 1, true>;
    static constexpr int LIMBS = N, EVENT_WORDS = H::EVENT_WORDS, OPS = 2, FIRST_OP = H::END, C0 = FIRST_OP, C1 = C0 + FieldOp<N>::COLS,
                         C0_RANGE = C1 + FieldOp<N>::COLS, C1_RANGE = C0_RANGE + FieldLt<N>::COLS, WIDTH = C1_RANGE + FieldLt<N>::COLS;
    static TG_HD void phase_a(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* ev, uint32_t* work, const Modulus<N>& m, const ChipConsts<N>& k) {
        Cursor w{out, row, height};
        uint64_t xw[N], yw[N];
        operand_words<N, N, true>(ev, xw, yw, 0u, 0u);
        const uint32_t kind = row_kind(ev, k.code_base) == KIND_ADD ? KIND_ADD : KIND_SUB;
        head_cols<N, 1, true>(w, ev, xw, yw, kind, 0u, 0u);
        Recorder<N> f{w, work, height, row, m, (uint32_t)FIRST_OP};
        const U<N> c0 = f.variable(C0, element<N>(xw, 0), element<N>(yw, 0), kind);
        const U<N> c1 = f.variable(C1, element<N>(xw, 1), element<N>(yw, 1), kind);
        f.lt(C0_RANGE, c0);
        f.lt(C1_RANGE, c1);
    }
};

// Fp2MulAssign: x, y of N words; a0_mul_b0, a1_mul_b1, a0_mul_b1, a1_mul_b0, c0 = a0 b0 - a1 b1, c1 = a0 b1 + a1 b0, the two ranges
template <int N> struct Fp2Mul {
    using H = Head<N, 0, true>;
    static constexpr int FO = FieldOp<N>::COLS;
    static constexpr int LIMBS = N, EVENT_WORDS = H::EVENT_WORDS, OPS = 6, FIRST_OP = H::END, A0_MUL_B0 = FIRST_OP, A1_MUL_B1 = A0_MUL_B0 + FO,
                         A0_MUL_B1 = A1_MUL_B1 + FO, A1_MUL_B0 = A0_MUL_B1 + FO, C0 = A1_MUL_B0 + FO, C1 = C0 + FO, C0_RANGE = C1 + FO,
                         C1_RANGE = C0_RANGE + FieldLt<N>::COLS, WIDTH = C1_RANGE + FieldLt<N>::COLS;
    static TG_HD void phase_a(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* ev, uint32_t* work, const Modulus<N>& m, const ChipConsts<N>&) {
        Cursor w{out, row, height};
        uint64_t xw[N], yw[N];
        operand_words<N, N, true>(ev, xw, yw, 0u, 0u);
        head_cols<N, 0, true>(w, ev, xw, yw, 0u, 0u, 0u);
        const U<N> a0 = element<N>(xw, 0), a1 = element<N>(xw, 1), b0 = element<N>(yw, 0), b1 = element<N>(yw, 1);
        Recorder<N> f{w, work, height, row, m, (uint32_t)FIRST_OP};
        const U<N> a0b0 = f.mul(A0_MUL_B0, a0, b0);
        const U<N> a1b1 = f.mul(A1_MUL_B1, a1, b1);
        const U<N> a0b1 = f.mul(A0_MUL_B1, a0, b1);
        const U<N> a1b0 = f.mul(A1_MUL_B0, a1, b0);
        const U<N> c0 = f.sub(C0, a0b0, a1b1);
        const U<N> c1 = f.add(C1, a0b1, a1b0);
        f.lt(C0_RANGE, c0);
        f.lt(C1_RANGE, c1);
    }
};

static_assert(CurveAdd<8>::WIDTH == 1599 && CurveDouble<8>::WIDTH == 1591 && CurveAdd<12>::WIDTH == 2399 && CurveDouble<12>::WIDTH == 2391 &&
              FpOp<8>::WIDTH == 306 && FpOp<12>::WIDTH == 450 && Fp2AddSub<8>::WIDTH == 592 && Fp2AddSub<12>::WIDTH == 880 &&
              Fp2Mul<8>::WIDTH == 1095 && Fp2Mul<12>::WIDTH == 1639, "widths");
static_assert(CurveAdd<8>::EVENT_WORDS == 44 && CurveDouble<8>::EVENT_WORDS == 28 && CurveAdd<12>::EVENT_WORDS == 64 && CurveDouble<12>::EVENT_WORDS == 40 &&
              FpOp<8>::EVENT_WORDS == 24 && FpOp<12>::EVENT_WORDS == 34 && Fp2AddSub<8>::EVENT_WORDS == 44 && Fp2AddSub<12>::EVENT_WORDS == 64 &&
              Fp2Mul<8>::EVENT_WORDS == 44 && Fp2Mul<12>::EVENT_WORDS == 64, "event records (rv64_exec.cpp: FAMILY_WORDS)");
static_assert(CurveDouble<8>::OPS <= MAX_OPS, "phase B's table");

template <class Shape> inline OpCols op_cols() {
    OpCols t = {};
    t.n = Shape::OPS;
    for (int i = 0; i < Shape::OPS; i++) t.col[i] = Shape::FIRST_OP + i * FieldOp<Shape::LIMBS>::COLS;
    return t;
}

// ----------------------------------------------------------------------------------------------------------------------- phase B
// The FieldOpCols at `col` of row `row` from record `op`. The kind is the record's own: in FpOpAssign and Fp2AddSubAssign lanes of
// one wave may take the addition's and the product's form.
template <int N>
TG_HD void phase_b(uint32_t* out, uint32_t height, uint32_t row, uint32_t op, uint32_t col, const uint32_t* work, const Modulus<N>& m, uint32_t offset) {
    size_t at = (size_t)op * Work<N>::REC * height + row;
    U<N> a, b, r;
#pragma unroll
    for (int i = 0; i < N; i++, at += height) a.w[i] = work_word(work, at);
#pragma unroll
    for (int i = 0; i < N; i++, at += height) b.w[i] = work_word(work, at);
#pragma unroll
    for (int i = 0; i < N; i++, at += height) r.w[i] = work_word(work, at);
    const uint32_t kind = work_word(work, at);
    Cursor w{out, row, height};
    const U<N> shown = fp256::select(kind == KIND_ADD || kind == KIND_MUL, r, a);              // sub / div: a is the result, r the other side
    if (kind < KIND_MUL) {
        uint32_t c;
        fp256::add(a, b, m, &c);                                                                 // (a + b - r) / p
        tgf::field_add_cols(w, col, row, shown, a, b, r, c, m, offset);
    } else {
        tgf::field_mul_cols(w, col, row, shown, a, b, r, fp256::mul_quotient(a, b, r, m), m, offset);
    }
}

// Both phases on the host: the table of `height` rows from `n` events, with a work buffer of Work<N>::words(height, OPS) words
template <class Shape>
void host_table(uint32_t* out, uint32_t height, const uint64_t* events, uint32_t n, uint32_t* work, const Modulus<Shape::LIMBS>& m,
                const ChipConsts<Shape::LIMBS>& k) {
    const OpCols cols = op_cols<Shape>();
    for (uint32_t row = 0; row < height; row++) Shape::phase_a(out, height, row, row < n ? events + (size_t)row * Shape::EVENT_WORDS : nullptr, work, m, k);
    for (uint32_t op = 0; op < cols.n; op++)
        for (uint32_t row = 0; row < height; row++) phase_b<Shape::LIMBS>(out, height, row, op, cols.col[op], work, m, k.offset);
}

#if defined(__HIPCC__)
// Phase A: one lane per row, 256 rows per workgroup. Phase B: grid (row blocks, operations of the chip).
template <class Shape>
__global__ __launch_bounds__(256) void phase_a_kernel(uint32_t* __restrict__ out, uint32_t height, const uint64_t* __restrict__ events, uint32_t n_events,
                                                      uint32_t* __restrict__ work, const Modulus<Shape::LIMBS> m, const ChipConsts<Shape::LIMBS> k) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    Shape::phase_a(out, height, row, row < n_events ? events + (size_t)row * Shape::EVENT_WORDS : nullptr, work, m, k);
}
template <int N>
__global__ __launch_bounds__(256) void phase_b_kernel(uint32_t* __restrict__ out, uint32_t height, const uint32_t* __restrict__ work, const Modulus<N> m,
                                                      uint32_t offset, const OpCols cols) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x, op = blockIdx.y;
    if (row >= height || op >= cols.n) return;
    phase_b<N>(out, height, row, op, cols.col[op], work, m, offset);
}
template <class Shape>
void launch_table(uint32_t* d_out, uint32_t height, const uint64_t* d_events, uint32_t n, uint32_t* d_work, const Modulus<Shape::LIMBS>& m,
                  const ChipConsts<Shape::LIMBS>& k, hipStream_t stream) {
    const OpCols cols = op_cols<Shape>();
    hipLaunchKernelGGL(phase_a_kernel<Shape>, dim3((height + 255) / 256), dim3(256), 0, stream, d_out, height, d_events, n, d_work, m, k);
    hipLaunchKernelGGL(phase_b_kernel<Shape::LIMBS>, dim3((height + 255) / 256, cols.n), dim3(256), 0, stream, d_out, height, d_work, m, k.offset, cols);
}
#endif

// ------------------------------------------------------------------------------------------------------------------ the families
// SP1HIP_RV64_FAMILY_* 0..11 -> shape, modulus and constants (curves/src/weierstrass/{secp256r1,bn254,bls12_381}.rs; syscall_code.rs:
// L118-L153 for the tower chips' codes). The witness offset is 2^14 at N = 8 and 2^15 at N = 12.
constexpr uint32_t FAMILIES = 12;
inline const uint32_t (&secp256r1_p())[8] {
    static const uint32_t p[8] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000001u, 0xFFFFFFFFu};
    return p;
}
inline const uint32_t (&bn254_p())[8] {
    static const uint32_t p[8] = {0xD87CFD47u, 0x3C208C16u, 0x6871CA8Du, 0x97816A91u, 0x8181585Du, 0xB85045B6u, 0xE131A029u, 0x30644E72u};
    return p;
}
inline const uint32_t (&bls12381_p())[12] {
    static const uint32_t p[12] = {0xFFFFAAABu, 0xB9FEFFFFu, 0xB153FFFFu, 0x1EABFFFEu, 0xF6B0F624u, 0x6730D2A0u,
                                   0xF38512BFu, 0x64774B84u, 0x434BACD7u, 0x4B1BA7B6u, 0x397FE69Au, 0x1A0111EAu};
    return p;
}
constexpr uint32_t BN254_FP_ADD = 0x26, BN254_FP2_ADD = 0x29, BLS12381_FP_ADD = 0x20, BLS12381_FP2_ADD = 0x23;

// Calls f(Shape{}, modulus, constants, chip name) for a family below FAMILIES; false for any other
template <class F> bool with_family(uint32_t family, F&& f) {
    static const Modulus<8> r1 = fp256::make_modulus<8>(secp256r1_p()), bn = fp256::make_modulus<8>(bn254_p());
    static const Modulus<12> bls = fp256::make_modulus<12>(bls12381_p());
    ChipConsts<8> k8 = {fp256::small<8>(0), 0u, 1u << 14};
    ChipConsts<12> k12 = {fp256::small<12>(0), 0u, 1u << 15};
    switch (family) {
    case 0: f(CurveAdd<8>{}, r1, k8, "Secp256r1AddAssign"); return true;
    case 1: fp256::sub_borrow(k8.a, fp256::from_limbs(r1.p), fp256::small<8>(3)); f(CurveDouble<8>{}, r1, k8, "Secp256r1DoubleAssign"); return true;   // a = p - 3
    case 2: f(CurveAdd<8>{}, bn, k8, "Bn254AddAssign"); return true;
    case 3: f(CurveDouble<8>{}, bn, k8, "Bn254DoubleAssign"); return true;
    case 4: f(CurveAdd<12>{}, bls, k12, "Bls12381AddAssign"); return true;
    case 5: f(CurveDouble<12>{}, bls, k12, "Bls12381DoubleAssign"); return true;
    case 6: k8.code_base = BN254_FP_ADD; f(FpOp<8>{}, bn, k8, "Bn254FpOpAssign"); return true;
    case 7: k12.code_base = BLS12381_FP_ADD; f(FpOp<12>{}, bls, k12, "Bls12381FpOpAssign"); return true;
    case 8: k8.code_base = BN254_FP2_ADD; f(Fp2AddSub<8>{}, bn, k8, "Bn254Fp2AddSubAssign"); return true;
    case 9: k12.code_base = BLS12381_FP2_ADD; f(Fp2AddSub<12>{}, bls, k12, "Bls12381Fp2AddSubAssign"); return true;
    case 10: f(Fp2Mul<8>{}, bn, k8, "Bn254Fp2MulAssign"); return true;
    case 11: f(Fp2Mul<12>{}, bls, k12, "Bls12381Fp2MulAssign"); return true;
    default: return false;
    }
}

}  // namespace tgc
}  // namespace sp1hip
