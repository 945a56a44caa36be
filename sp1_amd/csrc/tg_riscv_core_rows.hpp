// sp1_amd/csrc/tg_riscv_core_rows.hpp — the rows of the core-shard chips DivRem, AluX0 and MemoryLocal, and the Global events a
// MemoryLocal record sends, for host and device code alike (as tg_riscv_rows.hpp is for the fourteen instruction chips, whose event
// record, Row, CPUState, R / ALU adapters and compare it takes). tracegen_riscv_core.hip calls them one lane per row;
// tests/native/riscv_core_rows.hip runs the same functions on the CPU, so every word can be compared with the host tracer
// (sp1_amd/machines/riscv_trace.py divrem_rows, riscv_exec.py EventTracer) without a GPU.
//
//   DivRem       crates/core/machine/src/alu/divrem/mod.rs:L262-L563 (event_to_row), padding rows L565-L586 (the "0 / 1" row),
//                core/executor/src/utils.rs:L73-L93 (get_quotient_and_remainder), operations/{mul,is_zero_word,lt}.rs
//   AluX0        crates/core/machine/src/alu/alu_x0.rs
//   MemoryLocal  crates/core/machine/src/memory/local.rs (generate_trace_into, generate_dependencies: the two Global events)
//
// DivRem is 246 columns. A kernel that fills the whole row before it stores it gets the row put in scratch (988 bytes per lane), so
// the row is made in four column groups (DIVREM_PARTS): fill_divrem<PART> writes only the columns of its group, from the values
// every group shares (DivRemVals), and the caller stores that group before it asks for the next. fill_divrem<-1> writes them all.
#pragma once
#include "tg_riscv_rows.hpp"

namespace sp1hip {
namespace tg {

enum : uint32_t { OP_DIV = 15, OP_DIVU = 16, OP_REM = 17, OP_REMU = 18, OP_DIVW = 25, OP_DIVUW = 26, OP_REMW = 27, OP_REMUW = 28 };

constexpr int DIVREM_WIDTH = 246, ALU_X0_WIDTH = 34, MEMORY_LOCAL_WIDTH = 20;
constexpr int MEMORY_LOCAL_RECORD_WORDS = 5;
constexpr uint32_t KIND_MEMORY = 1;                           // InteractionKind::Memory

namespace col {
// DivRemCols behind CPUState and the R adapter (0..27)
constexpr int DR_A = 28, DR_B = 32, DR_C = 36, DR_QUOTIENT = 40, DR_QUOTIENT_COMP = 44, DR_REMAINDER_COMP = 48, DR_REMAINDER = 52,
              DR_ABS_REMAINDER = 56, DR_ABS_C = 60, DR_MAX_ABS_C_OR_1 = 64, DR_C_TIMES_QUOTIENT = 68, DR_CTQ_LOWER = 76, DR_CTQ_UPPER = 121,
              DR_C_NEG_OP = 166, DR_REM_NEG_OP = 170, DR_REMAINDER_LT = 174, DR_CARRY = 182, DR_IS_C_0 = 190, DR_IS_DIV = 201, DR_IS_DIVU = 202,
              DR_IS_REM = 203, DR_IS_REMU = 204, DR_IS_DIVW = 205, DR_IS_REMW = 206, DR_IS_DIVUW = 207, DR_IS_REMUW = 208, DR_IS_OVERFLOW = 209,
              DR_IS_OVERFLOW_B = 210, DR_IS_OVERFLOW_C = 221, DR_B_MSB = 232, DR_REM_MSB = 233, DR_C_MSB = 234, DR_QUOT_MSB = 235, DR_B_NEG = 236,
              DR_B_NEG_NOT_OVERFLOW = 237, DR_B_NOT_NEG_NOT_OVERFLOW = 238, DR_IS_REAL_NOT_WORD = 239, DR_REM_NEG = 240, DR_C_NEG = 241,
              DR_ABS_C_ALU_EVENT = 242, DR_ABS_REM_ALU_EVENT = 243, DR_IS_REAL = 244, DR_REMAINDER_CHECK_MULTIPLICITY = 245;
// MulOperation, relative to its first column
constexpr int MUL_CARRY = 0, MUL_PRODUCT = 16, MUL_B_LOW = 32, MUL_C_LOW = 36, MUL_B_MSB = 40, MUL_C_MSB = 41, MUL_PRODUCT_MSB = 42,
              MUL_B_SIGN_EXTEND = 43, MUL_C_SIGN_EXTEND = 44, MUL_WIDTH = 45;
// IsZeroWordOperation, relative: is_zero_limb[4] { inverse, result }, is_zero_first_half, is_zero_second_half, result
constexpr int IZW_LIMB = 0, IZW_FIRST_HALF = 8, IZW_SECOND_HALF = 9, IZW_RESULT = 10;
constexpr int X0_OPCODE = 32, X0_IS_REAL = 33;
constexpr int ML_ADDR = 0, ML_INITIAL_CLK_HIGH = 3, ML_FINAL_CLK_HIGH = 4, ML_INITIAL_CLK_LOW = 5, ML_FINAL_CLK_LOW = 6, ML_INITIAL_VALUE = 7,
              ML_FINAL_VALUE = 11, ML_INITIAL_VALUE_LOWER = 15, ML_INITIAL_VALUE_UPPER = 16, ML_FINAL_VALUE_LOWER = 17, ML_FINAL_VALUE_UPPER = 18,
              ML_IS_REAL = 19;
}  // namespace col

// The column groups DivRem is made and stored in: [DIVREM_PART_AT[p], DIVREM_PART_AT[p + 1])
constexpr int DIVREM_PARTS = 4;
__host__ __device__ constexpr int divrem_part_at(int p) { return p <= 0 ? 0 : p == 1 ? col::DR_CTQ_LOWER : p == 2 ? col::DR_CTQ_UPPER : p == 3 ? col::DR_C_NEG_OP : DIVREM_WIDTH; }

TG_HD uint64_t sext32(uint64_t v) { return (uint64_t)(int64_t)(int32_t)(uint32_t)v; }
// the inverse of canonical x in the field, canonical (0 for 0); the store converts
TG_HD uint32_t inv_canonical(uint32_t x) { return x ? kb::from_monty(kb::inv(kb::to_monty(x))) : 0u; }
// high 64 bits of the 128-bit product, through 32-bit halves (host and device alike)
TG_HD uint64_t mulhi_u64(uint64_t x, uint64_t y) {
    const uint64_t xl = (uint32_t)x, xh = x >> 32, yl = (uint32_t)y, yh = y >> 32;
    const uint64_t ll = xl * yl, lh = xl * yh, hl = xh * yl, hh = xh * yh;
    const uint64_t mid = (ll >> 32) + (uint32_t)lh + (uint32_t)hl;
    return hh + (lh >> 32) + (hl >> 32) + (mid >> 32);
}
TG_HD uint64_t mulhi_i64(uint64_t x, uint64_t y) { return mulhi_u64(x, y) - ((x >> 63) ? y : 0ull) - ((y >> 63) ? x : 0ull); }

// What every column group of a DivRem row is made from
struct DivRemVals {
    uint64_t b, c;                  // the operands as the chip divides them: the W forms sign- or zero-extend the low halves
    uint64_t q, rem;                // quotient and remainder (the W forms sign-extended)
    uint64_t qc, rc;                // quotient_comp / remainder_comp: the unsigned W forms zero-extended
    uint64_t abs_rem, abs_c;
    uint32_t rem_neg, b_neg, c_neg, overflow;
    bool word, sgn;
};

// get_quotient_and_remainder and the sign bookkeeping of event_to_row (riscv_trace.divrem_result / divrem_rows)
TG_HD DivRemVals divrem_values(const Ev& e) {
    DivRemVals d;
    const uint32_t op = (uint32_t)e.ops & 0xff;
    d.word = op == OP_DIVW || op == OP_DIVUW || op == OP_REMW || op == OP_REMUW;
    d.sgn = op == OP_DIV || op == OP_REM || op == OP_DIVW || op == OP_REMW;
    d.b = d.word ? (d.sgn ? sext32(e.b) : e.b & 0xffffffffull) : e.b;
    d.c = d.word ? (d.sgn ? sext32(e.c) : e.c & 0xffffffffull) : e.c;
    if (d.c == 0) {                                            // division by zero: all ones, and the dividend (a W form's sign-extended)
        d.q = ~0ull;
        d.rem = d.word ? sext32(e.b) : e.b;
    } else {                                                   // truncating division through the magnitudes; 2^63 / 1 covers the overflow
        const bool bn = d.sgn && (d.b >> 63), cn = d.sgn && (d.c >> 63);
        const uint64_t mb = bn ? 0ull - d.b : d.b, mc = cn ? 0ull - d.c : d.c;
        const uint64_t mq = mb / mc, mr = mb - mq * mc;
        d.q = bn != cn ? 0ull - mq : mq;
        d.rem = bn ? 0ull - mr : mr;
        if (d.word) { d.q = sext32(d.q); d.rem = sext32(d.rem); }
    }
    const bool zext = d.word && !d.sgn;
    d.qc = zext ? d.q & 0xffffffffull : d.q;
    d.rc = zext ? d.rem & 0xffffffffull : d.rem;
    d.rem_neg = d.b_neg = d.c_neg = d.overflow = 0;
    if (d.sgn && !d.word) {
        d.rem_neg = (uint32_t)(d.rem >> 63); d.b_neg = (uint32_t)(e.b >> 63); d.c_neg = (uint32_t)(e.c >> 63);
        d.overflow = e.b == 1ull << 63 && e.c == ~0ull;
    } else if (d.sgn) {
        d.rem_neg = (uint32_t)(d.rem >> 31) & 1; d.b_neg = (uint32_t)(e.b >> 31) & 1; d.c_neg = (uint32_t)(e.c >> 31) & 1;
        d.overflow = (uint32_t)e.b == 0x80000000u && (uint32_t)e.c == 0xffffffffu;
    }
    d.abs_rem = d.rem_neg ? 0ull - d.rem : d.rc;
    d.abs_c = d.c_neg ? 0ull - d.c : d.c;
    return d;
}

// IsZeroWordOperation::populate_from_field_element at `at` on four field elements given as differences x[i] - y[i] of 16-bit limbs
template <int W> TG_HD uint32_t fill_is_zero_word(Row<W>& r, int at, uint64_t x, uint64_t y) {
    uint32_t res[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint32_t xl = (uint32_t)(x >> (16 * i)) & M16, yl = (uint32_t)(y >> (16 * i)) & M16;
        const uint32_t v = xl >= yl ? xl - yl : kb::P - (yl - xl);
        r.c[at + col::IZW_LIMB + 2 * i] = inv_canonical(v);
        r.c[at + col::IZW_LIMB + 2 * i + 1] = res[i] = v == 0;
    }
    r.c[at + col::IZW_FIRST_HALF] = res[0] & res[1];
    r.c[at + col::IZW_SECOND_HALF] = res[2] & res[3];
    return r.c[at + col::IZW_RESULT] = res[0] & res[1] & res[2] & res[3];
}

// MulOperation::populate at `at` (operations/mul.rs:L54-L137): the low 16 bytes of the 16 x 16 byte product of the operands
// (sign-extended to 128 bits when is_mulh) with their carries; product_msb stays 0
template <int W> TG_HD void fill_mul_operation(Row<W>& r, int at, uint64_t x, uint64_t y, bool is_mulh) {
    const uint32_t x_msb = (uint32_t)(x >> 63), y_msb = (uint32_t)(y >> 63);
    const uint32_t xse = is_mulh ? x_msb : 0u, yse = is_mulh ? y_msb : 0u;
    uint32_t prod[16];
#pragma unroll
    for (int i = 0; i < 16; i++) prod[i] = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t xi = i < 8 ? (uint32_t)(x >> (8 * (i & 7))) & 0xff : xse * 0xffu;
#pragma unroll
        for (int j = 0; j < 16 - i; j++) {
            const uint32_t yj = j < 8 ? (uint32_t)(y >> (8 * (j & 7))) & 0xff : yse * 0xffu;
            prod[i + j] += xi * yj;
        }
    }
    uint32_t carry = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint32_t v = prod[i] + carry;
        carry = v >> 8;
        r.c[at + col::MUL_CARRY + i] = carry;
        r.c[at + col::MUL_PRODUCT + i] = v & 0xff;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        r.c[at + col::MUL_B_LOW + i] = (uint32_t)(x >> (16 * i)) & 0xff;
        r.c[at + col::MUL_C_LOW + i] = (uint32_t)(y >> (16 * i)) & 0xff;
    }
    r.c[at + col::MUL_B_MSB] = x_msb; r.c[at + col::MUL_C_MSB] = y_msb;
    r.c[at + col::MUL_B_SIGN_EXTEND] = xse; r.c[at + col::MUL_C_SIGN_EXTEND] = yse;
}

// The columns of group PART (all of them for PART < 0) of an event's DivRem row; r holds zeros there before
template <int PART> TG_HD void fill_divrem(Row<DIVREM_WIDTH>& r, const Ev& e, const DivRemVals& d) {
    namespace c = col;
    const uint32_t op = (uint32_t)e.ops & 0xff;
    const uint64_t lower = d.qc * d.c, upper = d.sgn ? mulhi_i64(d.qc, d.c) : mulhi_u64(d.qc, d.c);
    if constexpr (PART < 0 || PART == 0) {                    // state | RTypeReader | a .. c_times_quotient
        fill_state(r, e);
        fill_r(r, e);
        const bool div = op == OP_DIV || op == OP_DIVU || op == OP_DIVW || op == OP_DIVUW;
        r.limbs4(c::DR_A, div ? d.q : d.rem);
        r.limbs4(c::DR_B, d.b); r.limbs4(c::DR_C, d.c);
        r.limbs4(c::DR_QUOTIENT, d.q); r.limbs4(c::DR_QUOTIENT_COMP, d.qc);
        r.limbs4(c::DR_REMAINDER_COMP, d.rc); r.limbs4(c::DR_REMAINDER, d.rem);
        r.limbs4(c::DR_ABS_REMAINDER, d.abs_rem); r.limbs4(c::DR_ABS_C, d.abs_c);
        r.limbs4(c::DR_MAX_ABS_C_OR_1, d.abs_c ? d.abs_c : 1ull);
        r.limbs4(c::DR_C_TIMES_QUOTIENT, lower); r.limbs4(c::DR_C_TIMES_QUOTIENT + 4, upper);
    }
    if constexpr (PART < 0 || PART == 1) fill_mul_operation(r, c::DR_CTQ_LOWER, d.qc, d.c, false);
    if constexpr (PART < 0 || PART == 2) {                    // the W forms have no upper product
        if (!d.word) fill_mul_operation(r, c::DR_CTQ_UPPER, d.qc, d.c, d.sgn);
    }
    if constexpr (PART < 0 || PART == 3) {
        if (d.c_neg) r.limbs4(c::DR_C_NEG_OP, d.c + d.abs_c);           // AddOperation values: c + |c| and rem + |rem| wrap to 0
        if (d.rem_neg) r.limbs4(c::DR_REM_NEG_OP, d.rem + d.abs_rem);
        const uint32_t c0 = fill_is_zero_word(r, c::DR_IS_C_0, d.c, 0ull);
        // remainder_lt_operation: |rem| < max(|c|, 1), only when c != 0. fill_lt also writes zeros into the two columns behind its
        // eight (a signed compare's msbs): they are carry[0..1], written below
        if (!c0) fill_lt(r, c::DR_REMAINDER_LT, d.abs_rem, d.abs_c ? d.abs_c : 1ull, false);
        uint32_t prev = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {                          // c * quotient + remainder (sign-extended to 128 bits) in 16-bit limbs
            const uint32_t ctq = (uint32_t)((i < 4 ? lower : upper) >> (16 * (i & 3))) & M16;
            const uint32_t rem16 = i < 4 ? (uint32_t)(d.rc >> (16 * (i & 3))) & M16 : d.rem_neg * M16;
            prev = (ctq + rem16 + prev) >> 16;
            r.c[c::DR_CARRY + i] = prev;
        }
        r.c[c::DR_IS_DIV] = op == OP_DIV; r.c[c::DR_IS_DIVU] = op == OP_DIVU; r.c[c::DR_IS_REM] = op == OP_REM; r.c[c::DR_IS_REMU] = op == OP_REMU;
        r.c[c::DR_IS_DIVW] = op == OP_DIVW; r.c[c::DR_IS_REMW] = op == OP_REMW; r.c[c::DR_IS_DIVUW] = op == OP_DIVUW; r.c[c::DR_IS_REMUW] = op == OP_REMUW;
        r.c[c::DR_IS_OVERFLOW] = d.overflow;
        fill_is_zero_word(r, c::DR_IS_OVERFLOW_B, d.word ? e.b & 0xffffffffull : e.b, d.word ? 1ull << 31 : 1ull << 63);
        fill_is_zero_word(r, c::DR_IS_OVERFLOW_C, d.word ? e.c & 0xffffffffull : e.c, d.word ? 0xffffffffull : ~0ull);
        if (d.word) {
            r.c[c::DR_B_MSB] = (uint32_t)(e.b >> 31) & 1; r.c[c::DR_C_MSB] = (uint32_t)(e.c >> 31) & 1;
            r.c[c::DR_REM_MSB] = (uint32_t)(d.rem >> 31) & 1; r.c[c::DR_QUOT_MSB] = (uint32_t)(d.q >> 31) & 1;
        } else {
            r.c[c::DR_B_MSB] = (uint32_t)(d.b >> 63); r.c[c::DR_C_MSB] = (uint32_t)(d.c >> 63); r.c[c::DR_REM_MSB] = (uint32_t)(d.rem >> 63);
        }
        r.c[c::DR_B_NEG] = d.b_neg;
        r.c[c::DR_B_NEG_NOT_OVERFLOW] = d.b_neg & (1u - d.overflow);
        r.c[c::DR_B_NOT_NEG_NOT_OVERFLOW] = (1u - d.b_neg) & (1u - d.overflow);
        r.c[c::DR_IS_REAL_NOT_WORD] = !d.word;
        r.c[c::DR_REM_NEG] = d.rem_neg; r.c[c::DR_C_NEG] = d.c_neg;
        r.c[c::DR_ABS_C_ALU_EVENT] = d.c_neg; r.c[c::DR_ABS_REM_ALU_EVENT] = d.rem_neg;
        r.c[c::DR_IS_REAL] = 1;
        r.c[c::DR_REMAINDER_CHECK_MULTIPLICITY] = 1u - c0;
    }
}

// The columns of group PART of DivRem's padding row, the reference's "0 / 1" row: DIVU of 0 by 1 without is_real
template <int PART> TG_HD void fill_divrem_padding(Row<DIVREM_WIDTH>& r) {
    namespace c = col;
    if constexpr (PART < 0 || PART == 0) {
        r.c[22] = 1;                                           // adapter.op_c_memory.prev_value
        r.c[c::DR_C] = 1; r.c[c::DR_ABS_C] = 1; r.c[c::DR_MAX_ABS_C_OR_1] = 1;
    }
    if constexpr (PART < 0 || PART == 3) {
        r.c[c::DR_IS_DIVU] = 1;
        r.c[c::DR_B_NOT_NEG_NOT_OVERFLOW] = 1;
        fill_is_zero_word(r, c::DR_IS_C_0, 1ull, 0ull);
    }
}

// AluX0: state | ALUTypeReader | opcode | is_real; padding rows are zero
TG_HD void fill_alu_x0(Row<ALU_X0_WIDTH>& r, const Ev& e) {
    fill_state(r, e);
    fill_alu(r, e);
    r.c[col::X0_OPCODE] = (uint32_t)e.ops & 0xff;
    r.c[col::X0_IS_REAL] = 1;
}

// MemoryLocal from the executor's record { addr, initial clk, initial value, final clk, final value }; padding rows are zero
TG_HD void fill_memory_local(Row<MEMORY_LOCAL_WIDTH>& r, const uint64_t* rec) {
    namespace c = col;
    const uint64_t addr = rec[0], it = rec[1], iv = rec[2], ft = rec[3], fv = rec[4];
    r.limbs3(c::ML_ADDR, addr);
    r.c[c::ML_INITIAL_CLK_HIGH] = (uint32_t)(it >> 24); r.c[c::ML_FINAL_CLK_HIGH] = (uint32_t)(ft >> 24);
    r.c[c::ML_INITIAL_CLK_LOW] = (uint32_t)it & 0xffffffu; r.c[c::ML_FINAL_CLK_LOW] = (uint32_t)ft & 0xffffffu;
    r.limbs4(c::ML_INITIAL_VALUE, iv); r.limbs4(c::ML_FINAL_VALUE, fv);
    r.c[c::ML_INITIAL_VALUE_LOWER] = (uint32_t)(iv >> 32) & 0xff; r.c[c::ML_INITIAL_VALUE_UPPER] = (uint32_t)(iv >> 40) & 0xff;
    r.c[c::ML_FINAL_VALUE_LOWER] = (uint32_t)(fv >> 32) & 0xff; r.c[c::ML_FINAL_VALUE_UPPER] = (uint32_t)(fv >> 40) & 0xff;
    r.c[c::ML_IS_REAL] = 1;
}

// The record's two Global events as sp1hip_tracegen_riscv_global reads them, 9 words each: message[8] = clk_high, clk_low, addr[3],
// value[0] + lower * 2^16, value[1] + upper * 2^16, value[3]; then is_receive | kind << 8. The initial state is received, the final
// one sent, in that order (memory/local.rs generate_dependencies)
TG_HD void memory_local_global_events(int32_t* out, const uint64_t* rec) {
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const uint64_t clk = rec[1 + 2 * k], v = rec[2 + 2 * k];
        int32_t* o = out + GLOBAL_EVENT_WORDS * k;
        o[0] = (int32_t)(clk >> 24); o[1] = (int32_t)((uint32_t)clk & 0xffffffu);
        o[2] = (int32_t)(rec[0] & M16); o[3] = (int32_t)((rec[0] >> 16) & M16); o[4] = (int32_t)((rec[0] >> 32) & M16);
        o[5] = (int32_t)((v & M16) + (((v >> 32) & 0xff) << 16));
        o[6] = (int32_t)(((v >> 16) & M16) + (((v >> 40) & 0xff) << 16));
        o[7] = (int32_t)((v >> 48) & M16);
        o[8] = (int32_t)((k == 0 ? 1u : 0u) | KIND_MEMORY << 8);
    }
}

// One lane's (one host iteration's) whole DivRem row: each column group from its zeros, stored before the next is made. The chip
// keeps this body of its own instead of row_kernel's because a whole 246-word row would go to scratch (above)
template <int PART> TG_HD void divrem_store_part(uint32_t* __restrict__ out, uint32_t height, uint32_t row, bool live, const Ev& e, const DivRemVals& d) {
    constexpr int LO = divrem_part_at(PART), HI = divrem_part_at(PART + 1);
    Row<DIVREM_WIDTH> r;
    zero_cols<LO, HI>(r);
    if (live) fill_divrem<PART>(r, e, d); else fill_divrem_padding<PART>(r);
    store_cols<LO, HI>(out, height, row, r);
}
TG_HD void divrem_row(uint32_t* __restrict__ out, uint32_t height, const Ev* __restrict__ events, uint32_t n, uint32_t row) {
    const bool live = row < n;
    Ev e = {};
    if (live) e = events[row];
    const DivRemVals d = divrem_values(e);
    divrem_store_part<0>(out, height, row, live, e, d);
    divrem_store_part<1>(out, height, row, live, e, d);
    divrem_store_part<2>(out, height, row, live, e, d);
    divrem_store_part<3>(out, height, row, live, e, d);
}

// The chips of row_kernel / host_rows (tg_row_kernel.hpp)
struct AluX0 : ZeroPaddedChip<ALU_X0_WIDTH, Ev> {
    static TG_HD void live(Row<WIDTH>& r, const Ev* __restrict__ events, uint32_t row) { fill_alu_x0(r, events[row]); }
};
// `global_events` (may be null): [2 n][9] words, record i's receive at row 2 i and its send at row 2 i + 1
struct MemoryLocal : ZeroPaddedChip<MEMORY_LOCAL_WIDTH, uint64_t> {
    static TG_HD void live(Row<WIDTH>& r, const uint64_t* __restrict__ records, uint32_t row, int32_t* __restrict__ global_events) {
        uint64_t rec[MEMORY_LOCAL_RECORD_WORDS];
        load_record<MEMORY_LOCAL_RECORD_WORDS>(rec, records, row);
        fill_memory_local(r, rec);
        if (global_events) {
            int32_t ev[2 * GLOBAL_EVENT_WORDS];
            memory_local_global_events(ev, rec);
            store_global_events<2>(global_events, row, ev);
        }
    }
};

}  // namespace tg
}  // namespace sp1hip
