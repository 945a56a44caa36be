// sp1_amd/csrc/tg_uint256_rows.hpp — the row of the Uint256MulMod chip (UINT256_MUL: x <- x y mod m, or mod 2^256 when m = 0), for
// host and device code alike, on the pieces of tg_field_op.hpp. The definitions followed are
//   Uint256MulChip::generate_trace_into     crates/core/machine/src/syscall/precompiles/uint256/air.rs:L118-L290
//   FieldOpCols::populate_with_modulus      crates/core/machine/src/operations/field/field_op.rs:L224-L345
// as sp1_amd/machines/riscv_more_trace.py restates them (uint256_shard_from, field_op_columns with 33 modulus limbs), which the tests
// compare every word with. The column offsets are the #[repr(C)] order that riscv_more.uint256_mul_chip transcribes.
//
// What fp256.hpp cannot do here: the modulus is the row's own, it may be even (Montgomery's quotient through p^-1 mod 2^256 does not
// exist), zero stands for 2^256, and the operands are not reduced. So the row divides: the 512-bit product by m' = m or 2^256, by a
// restoring shift-subtract of exactly 512 steps (divide_512). One lane owns one row; every limb, byte and coefficient index is a
// constant; nothing is held but the operands and the division's 24 limbs.
#pragma once
#include "tg_field_op.hpp"

namespace sp1hip {
namespace tgu {

using tgf::Cursor;
using tgf::U;
constexpr int N = 8;                                               // 32-bit limbs of a 256-bit operand
constexpr uint32_t WITNESS_OFFSET = 1u << 14;                      // uint256/air.rs: the field operation's witness offset
constexpr int EVENT_WORDS = 31;                                    // clk, x_ptr, y_ptr, 4 x (t, x word), 8 x (t, y / modulus word), 4 words written
constexpr int LIMBS = 4 * N, WITNESS = 2 * LIMBS - 1, FIELD_OP = 2 * LIMBS + WITNESS;      // result[32], carry[32], witness[63]
constexpr int CLK_HIGH = 0, CLK_LOW = 1, X_PTR = 2, Y_PTR = X_PTR + tgf::SYSCALL_ADDR_COLS, X_ADDRS = Y_PTR + tgf::SYSCALL_ADDR_COLS,
              Y_AND_MODULUS_ADDRS = X_ADDRS + 3 * 4, X_MEMORY = Y_AND_MODULUS_ADDRS + 3 * 8, Y_MEMORY = X_MEMORY + 4 * tgf::MEMORY_ACCESS_U8_COLS,
              MODULUS_MEMORY = Y_MEMORY + 4 * tgf::MEMORY_ACCESS_U8_COLS, MODULUS_IS_ZERO = MODULUS_MEMORY + 4 * tgf::MEMORY_ACCESS_U8_COLS,
              MODULUS_IS_NOT_ZERO = MODULUS_IS_ZERO + 2, OUTPUT = MODULUS_IS_NOT_ZERO + 1, OUTPUT_WITNESS = OUTPUT + 2 * LIMBS,
              OUTPUT_RANGE_CHECK = OUTPUT + FIELD_OP, IS_REAL = OUTPUT_RANGE_CHECK + tgf::FieldLt<N>::COLS, WIDTH = IS_REAL + 1;
static_assert(WIDTH == 371 && OUTPUT == 209 && OUTPUT_WITNESS == 273 && OUTPUT_RANGE_CHECK == 336, "Uint256MulMod layout");

// result = x y mod m', carry = (x y / m') mod 2^256, for m' = m in [1, 2^256) — odd or even — and m' = 2^256 when m = 0. Restoring
// division, one quotient bit a step, 512 steps whatever the operands: the 512-bit product d shifts left into the remainder (256 bits
// and the bit shifted out of them, `top`) and takes the quotient bit at its low end, so after 512 steps d is the whole quotient and
// its low eight limbs the carry. The remainder before a step is below m' <= 2^256, so after the shift it is below 2^257: top and
// eight limbs hold it. It is at least m' exactly when top is set (then m' = 2^256 takes top away and leaves the limbs, and m < 2^256
// leaves rem - m mod 2^256, which is the difference since it is below m), or m' < 2^256 and rem - m does not borrow. The chip's
// identity x y = result + carry m' holds where the quotient is below 2^256; beyond that the carry is its low 256 bits.
TG_HD void divide_512(const U<N>& x, const U<N>& y, const U<N>& m, U<N>& result, U<N>& carry) {
    uint32_t d[2 * N];
#pragma unroll
    for (int i = 0; i < 2 * N; i++) d[i] = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
        uint64_t c = 0;
#pragma unroll
        for (int j = 0; j < N; j++) {
            const uint64_t s = (uint64_t)x.w[j] * y.w[i] + d[i + j] + c;
            d[i + j] = (uint32_t)s;
            c = s >> 32;
        }
        d[i + N] = (uint32_t)c;
    }
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < N; i++) any |= m.w[i];
    const bool below = any != 0;                                   // m' < 2^256
    U<N> rem = fp256::small<N>(0);
#pragma unroll 1
    for (int step = 0; step < 64 * N; step++) {
        const bool top = (rem.w[N - 1] >> 31) != 0;
#pragma unroll
        for (int i = N - 1; i >= 1; i--) rem.w[i] = (rem.w[i] << 1) | (rem.w[i - 1] >> 31);
        rem.w[0] = (rem.w[0] << 1) | (d[2 * N - 1] >> 31);
#pragma unroll
        for (int i = 2 * N - 1; i >= 1; i--) d[i] = (d[i] << 1) | (d[i - 1] >> 31);
        d[0] <<= 1;
        U<N> t;
        const uint32_t borrow = fp256::sub_borrow(t, rem, m);
        const bool take = top || (below && !borrow);
        rem = fp256::select(take, t, rem);
        d[0] |= take ? 1u : 0u;
    }
    result = rem;
#pragma unroll
    for (int i = 0; i < N; i++) carry.w[i] = d[i];
}

// One row of Uint256MulMod. `ev` = the event's words, or null for a padding row: zero but for the 63 witness columns, which hold the
// offset (the field operation on zero operands). x is rewritten at clk + 1; y and the modulus are read at clk. The product is
// computed from the words read.
TG_HD void uint256_mul_row(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* ev) {
    Cursor w{out, row, height};
    if (ev == nullptr) {
        w.zeros(OUTPUT_WITNESS);
        const uint32_t zero = kb::to_monty(WITNESS_OFFSET);
        for (int i = 0; i < WITNESS; i++) w.word(zero);
        w.zeros(WIDTH - OUTPUT_RANGE_CHECK);
        return;
    }
    const uint64_t clk = tgf::event_word(ev, 0), x_ptr = tgf::event_word(ev, 1), y_ptr = tgf::event_word(ev, 2);
    uint64_t xw[4], yw[4], mw[4];
#pragma unroll
    for (int i = 0; i < 4; i++) xw[i] = tgf::event_word(ev, 4 + 2 * i), yw[i] = tgf::event_word(ev, 12 + 2 * i), mw[i] = tgf::event_word(ev, 20 + 2 * i);
    w.val((uint32_t)(clk >> 24));
    w.val((uint32_t)clk & 0xffffffu);
    tgf::syscall_addr(w, x_ptr);
    tgf::syscall_addr(w, y_ptr);
    for (uint32_t i = 0; i < 4; i++) tgf::addr_add(w, x_ptr + 8u * i);
    for (uint32_t i = 0; i < 8; i++) tgf::addr_add(w, y_ptr + 8u * i);
#pragma unroll
    for (int i = 0; i < 4; i++) tgf::memory_access_u8(w, xw[i], tgf::event_word(ev, 3 + 2 * i), clk + 1);
#pragma unroll
    for (int i = 0; i < 4; i++) tgf::memory_access_u8(w, yw[i], tgf::event_word(ev, 11 + 2 * i), clk);
#pragma unroll
    for (int i = 0; i < 4; i++) tgf::memory_access_u8(w, mw[i], tgf::event_word(ev, 19 + 2 * i), clk);
    const U<N> x = tgf::from_words<N>(xw), y = tgf::from_words<N>(yw), m = tgf::from_words<N>(mw);
    uint32_t byte_sum = 0;                                         // IsZero over the sum of the modulus' 32 bytes (at most 8160)
#pragma unroll
    for (int i = 0; i < LIMBS; i++) byte_sum += tgf::byte_of(m, i);
    const bool is_zero = byte_sum == 0;
    w.word(kb::inv(kb::to_monty(byte_sum)));                       // 0 for 0
    w.bit(is_zero);
    w.bit(!is_zero);
    U<N> result, carry;
    divide_512(x, y, m, result, carry);
    tgf::field_mul_cols_with<N>(w, OUTPUT, row, result, x, y, result, carry, tgf::ModulusTop<N>{m, is_zero ? 1u : 0u}, WITNESS_OFFSET);
    if (is_zero) {                                                 // no range check against 2^256
        w.seek(OUTPUT_RANGE_CHECK, row);
        w.zeros(tgf::FieldLt<N>::COLS);
    } else {
        tgf::field_lt_cols_of<N>(w, OUTPUT_RANGE_CHECK, row, result, m);
    }
    w.seek(IS_REAL, row);
    w.bit(true);
}

}  // namespace tgu
}  // namespace sp1hip
