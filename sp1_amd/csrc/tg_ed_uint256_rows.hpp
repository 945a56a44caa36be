// sp1_amd/csrc/tg_ed_uint256_rows.hpp — the rows of the last three chips behind sp1hip_rv64_precompile_events, SP1HIP_RV64_FAMILY_*
// 12..14, for host and device code alike, from the pieces of tg_field_op.hpp, tg_field_poly_op.hpp, tg_field_chip_rows.hpp, fp256.hpp:
//   EdAddAssign    crates/core/machine/src/syscall/precompiles/edwards/ed_add.rs:L94-L130 (populate_field_ops), L330-L470
//   EdDecompress   .../edwards/ed_decompress.rs:L157-L180, L197-L330; curves/src/edwards/ed25519.rs:L75-L120 (ed25519_sqrt)
//   Uint256Ops     .../uint256_ops/air.rs:L117-L402
// as sp1_amd/machines/riscv_more_trace.py restates them (family_shard_from, _ed_field_ops, _ed_decompress_field_ops, fill), which the
// tests compare every word with. Column offsets are the #[repr(C)] order that riscv_more.py transcribes (ed_add_chip,
// ed_decompress_chip, uint256_ops_chip). All three work on byte limbs at N = 8 with witness offset 2^14.
//
// The two Edwards chips are made in the TWO PHASES of tg_field_chip_rows.hpp (a whole row of eight or seven unrolled byte products
// per lane would need scratch): phase A, one lane per row, writes the head and the FieldLtCols, does the field arithmetic and leaves
// one record per FieldOpCols-shaped block; phase B, one lane per (row, block), writes result, carry and witness.
//   EdAddAssign     record = a0, b0, r, a1, b1: 5N words (an inner product has four operands; a product and a denominator use the
//                   first three). The block's form — inner product, product, denominator 1 + b, denominator 1 - b — is a function
//                   of the block index alone, which is uniform over phase B's workgroup, so no kind is stored. The two
//                   denominators 1 + d f and 1 - d f share one inversion: (1 + d f)(1 - d f) is inverted and multiplied back.
//   EdDecompress    its seven blocks are FieldOpCols proper (FieldSqrtCols' multiplication is the record of a division: the root in
//                   the result columns, root * root on the other side), so records and phase B are tg_field_chip_rows.hpp's. Phase A
//                   does one Fermat inversion and one square root — exponent (p + 3) / 8, the multiplication by sqrt(-1) where the
//                   square is -a, negation to the even root —: two exponent chains of 256 steps each, whatever the data.
// Uint256Ops is one lane per row, as Uint256MulMod: one 63-coefficient witness.
//
// A padding row (event null) is the reference's dummy row made by the same code: EdAddAssign on four zero coordinates, EdDecompress
// on y = 0, both with a zero head; Uint256Ops zero except the witness columns, which hold the offset (is_add = is_mul = is_real = 0).
//
// PRECONDITIONS, which the executor guarantees: operands are reduced; EdAddAssign's denominators 1 +- d x1 x2 y1 y2 do not vanish;
// EdDecompress' u / v is a square. An event outside them neither faults nor takes longer (no branch or trip count depends on
// data: a vanishing denominator inverts to 0, a non-square leaves the candidate root as it is); its row satisfies no constraint
// system, and the host and the device form still agree on it.
#pragma once
#include "tg_field_chip_rows.hpp"
#include "tg_field_poly_op.hpp"

namespace sp1hip {
namespace tge {

using tgf::Cursor;
using tgf::FieldLt;
using tgf::FieldOp;
using tgf::Modulus;
using tgf::U;
constexpr int N = 8;                                               // 32-bit limbs of a field element / a 256-bit operand
constexpr uint32_t WITNESS_OFFSET = 1u << 14;
constexpr int FO = FieldOp<N>::COLS, LT = FieldLt<N>::COLS;

// curves/src/edwards/ed25519.rs:L24-L50: p = 2^255 - 19, d, sqrt(-1); (p + 3) / 8 = 2^252 - 2
inline const uint32_t (&ed25519_p())[N] {
    static const uint32_t p[N] = {0xFFFFFFEDu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x7FFFFFFFu};
    return p;
}
TG_HD U<N> ed25519_d() { return U<N>{{0x135978A3u, 0x75EB4DCAu, 0x4141D8ABu, 0x00700A4Du, 0x7779E898u, 0x8CC74079u, 0x2B6FFE73u, 0x52036CEEu}}; }
TG_HD U<N> ed25519_sqrt_m1() { return U<N>{{0x4A0EA0B0u, 0xC4EE1B27u, 0xAD2FE478u, 0x2F431806u, 0x3DFBD7A7u, 0x2B4D0099u, 0x4FC1DF0Bu, 0x2B832480u}}; }
TG_HD U<N> ed25519_sqrt_exponent() { return U<N>{{0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0x0FFFFFFFu}}; }

// a^e mod p for a constant exponent: 32N squarings, the exponent shifted instead of indexed (fp256::inv's loop); the exponent's
// bit is the same in every lane
TG_HD U<N> pow_fixed(const U<N>& a, U<N> e, const Modulus<N>& m) {
    const U<N> am = fp256::mont_mul(a, fp256::from_limbs(m.r2), m);
    U<N> r = fp256::mont_mul(fp256::small<N>(1), fp256::from_limbs(m.r2), m);
#pragma unroll 1
    for (int step = 0; step < 32 * N; step++) {
        r = fp256::mont_mul(r, r, m);
        if (e.w[N - 1] >> 31) r = fp256::mont_mul(r, am, m);
#pragma unroll
        for (int i = N - 1; i > 0; i--) e.w[i] = (e.w[i] << 1) | (e.w[i - 1] >> 31);
        e.w[0] <<= 1;
    }
    return fp256::mont_mul(r, fp256::small<N>(1), m);
}
// ed25519_sqrt: the even square root of a square a. beta = a^((p + 3) / 8) squares to a or to -a; in the second case beta sqrt(-1)
// is a root. A non-square is not detected: the candidate goes on as it is.
TG_HD U<N> ed25519_even_sqrt(const U<N>& a, const Modulus<N>& m) {
    U<N> beta = pow_fixed(a, ed25519_sqrt_exponent(), m);
    const U<N> minus_a = fp256::sub(fp256::small<N>(0), a, m);
    beta = fp256::select(fp256::equal(fp256::mul(beta, beta, m), minus_a), fp256::mul(beta, ed25519_sqrt_m1(), m), beta);
    U<N> negated;
    fp256::sub_borrow(negated, fp256::from_limbs(m.p), beta);      // an odd beta is not 0
    return fp256::select((beta.w[0] & 1u) != 0, negated, beta);
}

// ---------------------------------------------------------------------------------------------------------------- EdAddAssign
struct EdAdd {
    using H = tgc::Head<N, 0, true>;                               // x_ptr, y_ptr, x_addrs, y_addrs, x_access, y_access
    static constexpr int LIMBS = N, EVENT_WORDS = H::EVENT_WORDS, OPS = 8, REC = 5 * N, FIRST_OP = H::END;
    static constexpr int X3_NUMERATOR = FIRST_OP, Y3_NUMERATOR = X3_NUMERATOR + FO, X1_MUL_Y1 = Y3_NUMERATOR + FO, X2_MUL_Y2 = X1_MUL_Y1 + FO, F = X2_MUL_Y2 + FO,
                         D_MUL_F = F + FO, X3_INS = D_MUL_F + FO, Y3_INS = X3_INS + FO, X3_RANGE = Y3_INS + FO, Y3_RANGE = X3_RANGE + LT, WIDTH = Y3_RANGE + LT;
    using Work = tgc::Work<N, REC>;
    enum : uint32_t { INNER_PRODUCT = 0, PRODUCT = 1, DEN_PLUS = 2, DEN_MINUS = 3 };
    static TG_HD uint32_t form(uint32_t op) { return op < 2 ? INNER_PRODUCT : op < 6 ? PRODUCT : op == 6 ? DEN_PLUS : DEN_MINUS; }

    // the record of block `op`: a0, b0, r, then (inner products only) a1, b1
    static TG_HD void put(uint32_t* work, uint32_t height, uint32_t row, uint32_t op, const U<N>& a0, const U<N>& b0, const U<N>& r) {
        Cursor c{work, 0, height};
        c.seek(op * REC, row);
#pragma unroll
        for (int i = 0; i < N; i++) c.word(a0.w[i]);
#pragma unroll
        for (int i = 0; i < N; i++) c.word(b0.w[i]);
#pragma unroll
        for (int i = 0; i < N; i++) c.word(r.w[i]);
    }
    static TG_HD void put_pair(uint32_t* work, uint32_t height, uint32_t row, uint32_t op, const U<N>& a1, const U<N>& b1) {
        Cursor c{work, 0, height};
        c.seek(op * REC + 3 * N, row);
#pragma unroll
        for (int i = 0; i < N; i++) c.word(a1.w[i]);
#pragma unroll
        for (int i = 0; i < N; i++) c.word(b1.w[i]);
    }

    static TG_HD void phase_a(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* ev, uint32_t* work, const Modulus<N>& m) {
        Cursor w{out, row, height};
        uint64_t xw[N], yw[N];
        tgc::operand_words<N, N, true>(ev, xw, yw, 0u, 0u);                                      // padding: four zero coordinates
        tgc::head_cols<N, 0, true>(w, ev, xw, yw, 0u, 0u, 0u);
        const U<N> x1 = tgc::element<N>(xw, 0), y1 = tgc::element<N>(xw, 1), x2 = tgc::element<N>(yw, 0), y2 = tgc::element<N>(yw, 1);
        const U<N> xn = tgf::inner_product(x1, y2, x2, y1, m), yn = tgf::inner_product(y1, y2, x1, x2, m);
        put(work, height, row, 0, x1, y2, xn);
        put_pair(work, height, row, 0, x2, y1);
        put(work, height, row, 1, y1, y2, yn);
        put_pair(work, height, row, 1, x1, x2);
        const U<N> x1y1 = fp256::mul(x1, y1, m), x2y2 = fp256::mul(x2, y2, m), f = fp256::mul(x1y1, x2y2, m), d = ed25519_d(), df = fp256::mul(f, d, m);
        put(work, height, row, 2, x1, y1, x1y1);
        put(work, height, row, 3, x2, y2, x2y2);
        put(work, height, row, 4, x1y1, x2y2, f);
        put(work, height, row, 5, f, d, df);
        const U<N> one = fp256::small<N>(1), plus = fp256::add(one, df, m), minus = fp256::sub(one, df, m);
        const U<N> both = fp256::inv(fp256::mul(plus, minus, m), m);                             // one inversion: 1 / (1 - (d f)^2)
        const U<N> x3 = fp256::mul(xn, fp256::mul(both, minus, m), m), y3 = fp256::mul(yn, fp256::mul(both, plus, m), m);
        put(work, height, row, 6, xn, df, x3);
        put(work, height, row, 7, yn, df, y3);
        tgf::field_lt_cols(w, X3_RANGE, row, x3, m);
        tgf::field_lt_cols(w, Y3_RANGE, row, y3, m);
    }

    // the columns of block `op` of row `row` from its record
    static TG_HD void phase_b(uint32_t* out, uint32_t height, uint32_t row, uint32_t op, const uint32_t* work, const Modulus<N>& m) {
        size_t at = (size_t)op * REC * height + row;
        U<N> a, b, r;
#pragma unroll
        for (int i = 0; i < N; i++, at += height) a.w[i] = tgc::work_word(work, at);
#pragma unroll
        for (int i = 0; i < N; i++, at += height) b.w[i] = tgc::work_word(work, at);
#pragma unroll
        for (int i = 0; i < N; i++, at += height) r.w[i] = tgc::work_word(work, at);
        Cursor w{out, row, height};
        const uint32_t col = FIRST_OP + op * FO, kind = form(op);
        if (kind == INNER_PRODUCT) {
            U<N> a1, b1;
#pragma unroll
            for (int i = 0; i < N; i++, at += height) a1.w[i] = tgc::work_word(work, at);
#pragma unroll
            for (int i = 0; i < N; i++, at += height) b1.w[i] = tgc::work_word(work, at);
            tgf::field_inner_product_cols(w, col, row, a, b, a1, b1, r, tgf::inner_product_quotient(a, b, a1, b1, r, m), m, WITNESS_OFFSET);
        } else if (kind == PRODUCT) {
            tgf::field_mul_cols(w, col, row, r, a, b, r, fp256::mul_quotient(a, b, r, m), m, WITNESS_OFFSET);
        } else {
            const bool sign = kind == DEN_PLUS;
            tgf::field_den_cols(w, col, row, a, b, r, tgf::den_quotient(a, b, r, sign, m), sign, m, WITNESS_OFFSET);
        }
    }

    static void host_table(uint32_t* out, uint32_t height, const uint64_t* events, uint32_t n, uint32_t* work, const Modulus<N>& m) {
        for (uint32_t row = 0; row < height; row++) phase_a(out, height, row, row < n ? events + (size_t)row * EVENT_WORDS : nullptr, work, m);
        for (uint32_t op = 0; op < (uint32_t)OPS; op++)
            for (uint32_t row = 0; row < height; row++) phase_b(out, height, row, op, work, m);
    }
};
static_assert(EdAdd::WIDTH == 1347 && EdAdd::EVENT_WORDS == 44 && EdAdd::FIRST_OP == 271, "EdAddAssign layout");

// --------------------------------------------------------------------------------------------------------------- EdDecompress
struct EdDecompress {
    static constexpr int LIMBS = N, EVENT_WORDS = 24, OPS = 7;     // clk, ptr, sign, code, 4 x (t, x word before), 4 x (t, y word), 4 x words written
    static constexpr int IS_REAL = 0, CLK_HIGH = 1, CLK_LOW = 2, PTR = 3, READ_PTRS = PTR + tgf::SYSCALL_ADDR_COLS, ADDRS = READ_PTRS + 3 * 4, SIGN = ADDRS + 3 * 4,
                         X_ACCESS = SIGN + 1, X_VALUE = X_ACCESS + 9 * 4, Y_ACCESS = X_VALUE + 4 * 4, NEG_X_RANGE = Y_ACCESS + tgf::MEMORY_ACCESS_U8_COLS * 4,
                         Y_RANGE = NEG_X_RANGE + LT, YY = Y_RANGE + LT, U_ = YY + FO, DYY = U_ + FO, V = DYY + FO, U_DIV_V = V + FO, X_MULTIPLICATION = U_DIV_V + FO,
                         X_RANGE = X_MULTIPLICATION + FO, X_LSB = X_RANGE + LT, NEG_X = X_LSB + 1, WIDTH = NEG_X + FO, FIRST_OP = YY;
    using Work = tgc::Work<N>;
    // the column of each block, in record order (record = (column - FIRST_OP) / FO: NEG_X's 35 columns past the sixth round down)
    static tgc::OpCols op_cols() {
        tgc::OpCols t = {};
        t.n = OPS;
        const uint32_t cols[OPS] = {YY, U_, DYY, V, U_DIV_V, X_MULTIPLICATION, NEG_X};
        for (int i = 0; i < OPS; i++) t.col[i] = cols[i];
        return t;
    }

    static TG_HD void phase_a(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* ev, uint32_t* work, const Modulus<N>& m) {
        Cursor w{out, row, height};
        uint64_t yw[4];
#pragma unroll
        for (int i = 0; i < 4; i++) yw[i] = ev ? tgf::event_word(ev, 13 + 2 * i) : 0ull;
        if (ev != nullptr) {
            const uint64_t clk = tgf::event_word(ev, 0), ptr = tgf::event_word(ev, 1);
            tgf::row_head(w, true, clk);
            tgf::syscall_addr(w, ptr);
            for (uint32_t i = 0; i < 4; i++) tgf::addr_add(w, ptr + 32u + 8u * i);                 // read_ptrs: y
            for (uint32_t i = 0; i < 4; i++) tgf::addr_add(w, ptr + 8u * i);                       // addrs: x
            w.bit((tgf::event_word(ev, 2) & 1ull) != 0);
#pragma unroll
            for (int i = 0; i < 4; i++) tgf::memory_access(w, tgf::event_word(ev, 5 + 2 * i), tgf::event_word(ev, 4 + 2 * i), clk + 1);
#pragma unroll
            for (int i = 0; i < 4; i++) w.limbs(tgf::event_word(ev, 20 + i));
#pragma unroll
            for (int i = 0; i < 4; i++) tgf::memory_access_u8(w, yw[i], tgf::event_word(ev, 12 + 2 * i), clk);
        } else {
            w.zeros(NEG_X_RANGE);
        }
        const U<N> y = tgf::from_words<N>(yw), one = fp256::small<N>(1);
        tgc::Recorder<N> f{w, work, height, row, m, (uint32_t)FIRST_OP};
        f.lt(Y_RANGE, y);
        const U<N> yy = f.mul(YY, y, y);
        const U<N> u = f.sub(U_, yy, one);
        const U<N> dyy = f.mul(DYY, ed25519_d(), yy);
        const U<N> v = f.add(V, one, dyy);
        const U<N> u_div_v = f.div(U_DIV_V, u, v, fp256::inv(v, m));
        const U<N> x = ed25519_even_sqrt(u_div_v, m);
        f.put(X_MULTIPLICATION, x, x, fp256::mul(x, x, m), tgc::KIND_DIV);                       // FieldSqrtCols: the root shown, root * root = u / v
        f.lt(X_RANGE, x);
        w.seek(X_LSB, row);
        w.word(0u);
        f.lt(NEG_X_RANGE, f.sub(NEG_X, fp256::small<N>(0), x));
    }

    static void host_table(uint32_t* out, uint32_t height, const uint64_t* events, uint32_t n, uint32_t* work, const Modulus<N>& m) {
        const tgc::OpCols cols = op_cols();
        for (uint32_t row = 0; row < height; row++) phase_a(out, height, row, row < n ? events + (size_t)row * EVENT_WORDS : nullptr, work, m);
        for (uint32_t op = 0; op < cols.n; op++)
            for (uint32_t row = 0; row < height; row++) tgc::phase_b<N>(out, height, row, op, cols.col[op], work, m, WITNESS_OFFSET);
    }
};
static_assert(EdDecompress::WIDTH == 1123 && EdDecompress::YY == 206 && EdDecompress::X_LSB == 996, "EdDecompress layout");
static_assert((EdDecompress::NEG_X - EdDecompress::FIRST_OP) / FO == 6, "NEG_X's record");

// ----------------------------------------------------------------------------------------------------------------- Uint256Ops
// d, e <- the low and high 256 bits of a + b + c (UINT256_ADD_CARRY) or a b + c (UINT256_MUL_CARRY). Event: clk, a_ptr, b_ptr, code,
// the pointers c, d, e (registers x12, x13, x14), those registers' previous timestamps, 4 x (previous timestamp, word before) of each
// of a, b, c, d, e (accessed at clk .. clk + 4), the 4 d and 4 e words written.
struct Uint256Ops {
    static constexpr int EVENT_WORDS = 58, LIMBS = 4 * N, WITNESS = 2 * LIMBS - 1, FIELD_OP_COLS = 2 * LIMBS + WITNESS;
    static constexpr uint32_t MUL_CARRY = 0x31;                    // syscall_code.rs: UINT256_ADD_CARRY = 0x30, UINT256_MUL_CARRY = 0x31
    static constexpr int PTR_BLOCK = tgf::SYSCALL_ADDR_COLS + 3 * 4, REG_BLOCK = PTR_BLOCK + 9;
    static constexpr int CLK_HIGH = 0, CLK_LOW = 1, A_PTR = 2, A_ADDRS = A_PTR + tgf::SYSCALL_ADDR_COLS, B_PTR = A_PTR + PTR_BLOCK, C_PTR = B_PTR + PTR_BLOCK,
                         C_PTR_MEMORY = C_PTR + tgf::SYSCALL_ADDR_COLS, C_ADDRS = C_PTR_MEMORY + 9, D_PTR = C_PTR + REG_BLOCK, E_PTR = D_PTR + REG_BLOCK,
                         A_MEMORY = E_PTR + REG_BLOCK, B_MEMORY = A_MEMORY + 4 * tgf::MEMORY_ACCESS_U8_COLS, C_MEMORY = B_MEMORY + 4 * tgf::MEMORY_ACCESS_U8_COLS,
                         D_MEMORY = C_MEMORY + 4 * tgf::MEMORY_ACCESS_U8_COLS, E_MEMORY = D_MEMORY + 4 * 9, FIELD_OP = E_MEMORY + 4 * 9,
                         FIELD_OP_WITNESS = FIELD_OP + 2 * LIMBS, IS_ADD = FIELD_OP + FIELD_OP_COLS, IS_MUL = IS_ADD + 1, IS_REAL = IS_MUL + 1, WIDTH = IS_REAL + 1;

    // (is_mul ? a b : a + b) + c as sixteen limbs: the low eight are the result, the high eight the carry
    static TG_HD void add_into(uint32_t (&d)[2 * N], const U<N>& v) {
        uint64_t c = 0;
#pragma unroll
        for (int i = 0; i < 2 * N; i++) {
            c += (uint64_t)d[i] + (i < N ? v.w[i] : 0u);
            d[i] = (uint32_t)c;
            c >>= 32;
        }
    }
    static TG_HD void op_and_carry(const U<N>& a, const U<N>& b, const U<N>& c, bool is_mul, U<N>& result, U<N>& carry) {
        const U<N> zero = fp256::small<N>(0), a_mul = fp256::select(is_mul, a, zero);
        uint32_t d[2 * N];
#pragma unroll
        for (int i = 0; i < 2 * N; i++) d[i] = 0;
#pragma unroll
        for (int i = 0; i < N; i++) {
            uint64_t cy = 0;
#pragma unroll
            for (int j = 0; j < N; j++) {
                const uint64_t s = (uint64_t)a_mul.w[j] * b.w[i] + d[i + j] + cy;
                d[i + j] = (uint32_t)s;
                cy = s >> 32;
            }
            d[i + N] = (uint32_t)cy;
        }
        add_into(d, fp256::select(is_mul, zero, a));
        add_into(d, fp256::select(is_mul, zero, b));
        add_into(d, c);
#pragma unroll
        for (int i = 0; i < N; i++) result.w[i] = d[i], carry.w[i] = d[N + i];
    }

    static TG_HD void fill_row(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* ev) {
        Cursor w{out, row, height};
        if (ev == nullptr) {
            w.zeros(FIELD_OP_WITNESS);
            const uint32_t zero = kb::to_monty(WITNESS_OFFSET);
            for (int i = 0; i < WITNESS; i++) w.word(zero);
            w.zeros(WIDTH - IS_ADD);
            return;
        }
        const uint64_t clk = tgf::event_word(ev, 0);
        const bool is_mul = ((uint32_t)tgf::event_word(ev, 3) & 0xffu) == MUL_CARRY;
        w.val((uint32_t)(clk >> 24));
        w.val((uint32_t)clk & 0xffffffu);
#pragma unroll
        for (int k = 0; k < 5; k++) {                                                            // a, b at the arguments; c, d, e in registers
            const uint64_t ptr = tgf::event_word(ev, k < 2 ? 1 + k : 2 + k);
            tgf::syscall_addr(w, ptr);
            if (k >= 2) tgf::memory_access(w, ptr, tgf::event_word(ev, 5 + k), clk);
            for (uint32_t i = 0; i < 4; i++) tgf::addr_add(w, ptr + 8u * i);
        }
        uint64_t aw[4], bw[4], cw[4];
#pragma unroll
        for (int i = 0; i < 4; i++) aw[i] = tgf::event_word(ev, 11 + 2 * i), bw[i] = tgf::event_word(ev, 19 + 2 * i), cw[i] = tgf::event_word(ev, 27 + 2 * i);
#pragma unroll
        for (int i = 0; i < 4; i++) tgf::memory_access_u8(w, aw[i], tgf::event_word(ev, 10 + 2 * i), clk);
#pragma unroll
        for (int i = 0; i < 4; i++) tgf::memory_access_u8(w, bw[i], tgf::event_word(ev, 18 + 2 * i), clk + 1);
#pragma unroll
        for (int i = 0; i < 4; i++) tgf::memory_access_u8(w, cw[i], tgf::event_word(ev, 26 + 2 * i), clk + 2);
#pragma unroll
        for (int i = 0; i < 4; i++) tgf::memory_access(w, tgf::event_word(ev, 35 + 2 * i), tgf::event_word(ev, 34 + 2 * i), clk + 3);
#pragma unroll
        for (int i = 0; i < 4; i++) tgf::memory_access(w, tgf::event_word(ev, 43 + 2 * i), tgf::event_word(ev, 42 + 2 * i), clk + 4);
        const U<N> a = tgf::from_words<N>(aw), b = tgf::from_words<N>(bw), c = tgf::from_words<N>(cw);
        U<N> result, carry;
        op_and_carry(a, b, c, is_mul, result, carry);
        tgf::field_op_and_carry_cols(w, FIELD_OP, row, a, b, c, result, carry, is_mul, WITNESS_OFFSET);
        w.seek(IS_ADD, row);
        w.bit(!is_mul);
        w.bit(is_mul);
        w.bit(true);
    }

    static void host_table(uint32_t* out, uint32_t height, const uint64_t* events, uint32_t n) {
        for (uint32_t r = 0; r < height; r++) fill_row(out, height, r, r < n ? events + (size_t)r * EVENT_WORDS : nullptr);
    }
};
static_assert(Uint256Ops::WIDTH == 477 && Uint256Ops::A_MEMORY == 119 && Uint256Ops::FIELD_OP == 347 && Uint256Ops::C_ADDRS == 53, "Uint256Ops layout");

// ----------------------------------------------------------------------------------------------- the touched words' records
// The MemoryLocal records { addr, initial clk, initial value, final clk, final value } of the words an EdDecompress or a Uint256Ops
// call touched, which sp1hip_precompile_local_records' four segments cannot state (a pointer plus an offset, a register's constant
// address with split value and timestamp words, six runs), in the order riscv_more_trace.family_shard_from hands
// _close_precompile_shard: run after run, event by event inside each run.
//   EdDecompress  8 per call: the 4 x words at ptr + 8 i (pairs at event words 4 + 2 i, final clk + 1, final value word 20 + i), then
//                 the 4 y words at ptr + 32 + 8 i (pairs at 12 + 2 i, final clk, value unchanged)
//   Uint256Ops    23 per call: registers 12, 13, 14 (value word 4 + j, initial clk word 7 + j, final clk, value unchanged), then the
//                 blocks a, b, c, d, e of 4 words (pointers at words 1, 2, 4, 5, 6; pairs at 10 + 8 j + 2 i; final clk + j; a, b, c
//                 unchanged, d takes words 50..53, e words 54..57)
constexpr uint32_t TOUCHED_ED_DECOMPRESS = 13, TOUCHED_UINT256_OPS = 14;                        // SP1HIP_RV64_FAMILY_*
constexpr int MEMORY_LOCAL_RECORD_WORDS = 5;
TG_HD uint32_t touched_event_words(uint32_t family) { return family == TOUCHED_ED_DECOMPRESS ? EdDecompress::EVENT_WORDS : Uint256Ops::EVENT_WORDS; }
TG_HD uint32_t touched_per_event(uint32_t family) { return family == TOUCHED_ED_DECOMPRESS ? 8u : 23u; }

// record q < n_events * touched_per_event(family) of a shard's events
TG_HD void touched_record(uint64_t* rec, const uint64_t* events, uint32_t n_events, uint32_t family, uint64_t q) {
    if (family == TOUCHED_ED_DECOMPRESS) {
        const uint32_t run = (uint32_t)(q / (4ull * n_events)), at = (uint32_t)(q % (4ull * n_events)), i = at % 4u;
        const uint64_t* ev = events + (size_t)(at / 4u) * EdDecompress::EVENT_WORDS;
        const uint32_t pair = (run ? 12u : 4u) + 2u * i;
        rec[0] = ev[1] + (run ? 32u : 0u) + 8u * i;
        rec[1] = ev[pair];
        rec[2] = ev[pair + 1];
        rec[3] = ev[0] + (run ? 0u : 1u);
        rec[4] = run ? ev[pair + 1] : ev[20 + i];
        return;
    }
    if (q < 3ull * n_events) {
        const uint32_t j = (uint32_t)(q % 3u);
        const uint64_t* ev = events + (size_t)(q / 3u) * Uint256Ops::EVENT_WORDS;
        rec[0] = 12u + j;
        rec[1] = ev[7 + j];
        rec[2] = ev[4 + j];
        rec[3] = ev[0];
        rec[4] = ev[4 + j];
        return;
    }
    q -= 3ull * n_events;
    const uint32_t j = (uint32_t)(q / (4ull * n_events)), at = (uint32_t)(q % (4ull * n_events)), i = at % 4u;
    const uint64_t* ev = events + (size_t)(at / 4u) * Uint256Ops::EVENT_WORDS;
    const uint32_t pair = 10u + 8u * j + 2u * i;
    rec[0] = ev[j < 2 ? 1 + j : 2 + j] + 8u * i;
    rec[1] = ev[pair];
    rec[2] = ev[pair + 1];
    rec[3] = ev[0] + j;
    rec[4] = j < 3 ? ev[pair + 1] : ev[50 + 4 * (j - 3) + i];
}
inline void host_touched_records(uint64_t* records, const uint64_t* events, uint32_t n_events, uint32_t family) {
    const uint64_t total = (uint64_t)n_events * touched_per_event(family);
    for (uint64_t q = 0; q < total; q++) touched_record(records + q * MEMORY_LOCAL_RECORD_WORDS, events, n_events, family, q);
}

#if defined(__HIPCC__)
// Phase A: one lane per row, 256 rows per workgroup. Phase B: grid (row blocks, blocks of the chip).
template <class Shape>
__global__ __launch_bounds__(256) void ed_phase_a_kernel(uint32_t* __restrict__ out, uint32_t height, const uint64_t* __restrict__ events, uint32_t n_events,
                                                         uint32_t* __restrict__ work, const Modulus<N> m) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    Shape::phase_a(out, height, row, row < n_events ? events + (size_t)row * Shape::EVENT_WORDS : nullptr, work, m);
}
__global__ __launch_bounds__(256) void ed_add_phase_b_kernel(uint32_t* __restrict__ out, uint32_t height, const uint32_t* __restrict__ work, const Modulus<N> m) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x, op = blockIdx.y;
    if (row >= height || op >= (uint32_t)EdAdd::OPS) return;
    EdAdd::phase_b(out, height, row, op, work, m);
}
__global__ __launch_bounds__(256) void ed_decompress_phase_b_kernel(uint32_t* __restrict__ out, uint32_t height, const uint32_t* __restrict__ work,
                                                                    const Modulus<N> m, const tgc::OpCols cols) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x, op = blockIdx.y;
    if (row >= height || op >= cols.n) return;
    tgc::phase_b<N>(out, height, row, op, cols.col[op], work, m, WITNESS_OFFSET);
}
__global__ __launch_bounds__(256) void uint256_ops_kernel(uint32_t* __restrict__ out, uint32_t height, const uint64_t* __restrict__ events, uint32_t n_events) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    Uint256Ops::fill_row(out, height, row, row < n_events ? events + (size_t)row * Uint256Ops::EVENT_WORDS : nullptr);
}
// One lane per record: [n_records][5] words
__global__ __launch_bounds__(256) void touched_records_kernel(uint64_t* __restrict__ records, uint32_t n_records, const uint64_t* __restrict__ events,
                                                              uint32_t n_events, uint32_t family) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n_records) return;
    uint64_t rec[MEMORY_LOCAL_RECORD_WORDS];
    touched_record(rec, events, n_events, family, q);
#pragma unroll
    for (int i = 0; i < MEMORY_LOCAL_RECORD_WORDS; i++) records[(size_t)q * MEMORY_LOCAL_RECORD_WORDS + i] = rec[i];
}

inline void launch_ed_add(uint32_t* d_out, uint32_t height, const uint64_t* d_events, uint32_t n, uint32_t* d_work, const Modulus<N>& m, hipStream_t stream) {
    hipLaunchKernelGGL(ed_phase_a_kernel<EdAdd>, dim3((height + 255) / 256), dim3(256), 0, stream, d_out, height, d_events, n, d_work, m);
    hipLaunchKernelGGL(ed_add_phase_b_kernel, dim3((height + 255) / 256, EdAdd::OPS), dim3(256), 0, stream, d_out, height, d_work, m);
}
inline void launch_ed_decompress(uint32_t* d_out, uint32_t height, const uint64_t* d_events, uint32_t n, uint32_t* d_work, const Modulus<N>& m, hipStream_t stream) {
    const tgc::OpCols cols = EdDecompress::op_cols();
    hipLaunchKernelGGL(ed_phase_a_kernel<EdDecompress>, dim3((height + 255) / 256), dim3(256), 0, stream, d_out, height, d_events, n, d_work, m);
    hipLaunchKernelGGL(ed_decompress_phase_b_kernel, dim3((height + 255) / 256, cols.n), dim3(256), 0, stream, d_out, height, d_work, m, cols);
}
inline void launch_uint256_ops(uint32_t* d_out, uint32_t height, const uint64_t* d_events, uint32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(uint256_ops_kernel, dim3((height + 255) / 256), dim3(256), 0, stream, d_out, height, d_events, n);
}
inline void launch_touched_records(uint64_t* d_records, uint32_t n_records, const uint64_t* d_events, uint32_t n_events, uint32_t family, hipStream_t stream) {
    hipLaunchKernelGGL(touched_records_kernel, dim3((n_records + 255) / 256), dim3(256), 0, stream, d_records, n_records, d_events, n_events, family);
}
#endif

inline const Modulus<N>& ed25519_modulus() {
    static const Modulus<N> m = fp256::make_modulus<N>(ed25519_p());
    return m;
}

}  // namespace tge
}  // namespace sp1hip
