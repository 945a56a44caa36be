// sp1_amd/csrc/tg_riscv_rows.hpp — the rows of the RISC-V instruction chips whose tables tracegen_riscv.hip makes on the device,
// for host and device code alike (as tg_field_op.hpp is for the precompile chips): the event record (a row held as W words is tg_row_kernel.hpp's Row), the
// column groups the chips share (CPUState, the register access columns, the R / I / ALU / J adapters, the signed / unsigned
// compare) and fill_row<CHIP> for each of the fourteen chips. tests/native/riscv_rows.hip runs the same functions on the CPU, so
// every word can be compared with the host tracer (sp1_amd/machines/riscv_trace.py, riscv_exec.py) without a GPU.
//
//   CPUState                 /root/reference/crates/core/machine/src/adapter/state.rs:L26-L69
//   register access columns  crates/core/machine/src/memory/consistency/trace.rs:L22-L33, L104-L127
//   R / I / ALU / J adapters crates/core/machine/src/adapter/register/{r_type,i_type,alu_type,j_type}.rs (populate)
//   Add / Addi / Sub         crates/core/machine/src/alu/add_sub/{add,addi,sub}.rs event_to_row
//   Addw / Subw              crates/core/machine/src/alu/{addw,subw}/mod.rs
//   Mul                      crates/core/machine/src/alu/mul/mod.rs, operations/mul.rs:L54-L137 (MulOperation::populate)
//   ShiftRight               crates/core/machine/src/alu/sr/mod.rs:L239-L312 (padding rows L165-L171)
//   Branch                   crates/core/machine/src/control_flow/branch/{columns,trace}.rs, operations/slt.rs:L50-L174
//   Bitwise                  crates/core/machine/src/alu/bitwise/mod.rs:L180-L191, operations/bitwise_u16.rs:L40-L51
//   Lt                       crates/core/machine/src/alu/lt/mod.rs:L179-L195
//   ShiftLeft                crates/core/machine/src/alu/sll/mod.rs:L224-L286 (padding rows L154-L160)
//   UType                    crates/core/machine/src/utype/mod.rs:L262-L273
//   Jal                      crates/core/machine/src/control_flow/jal/trace.rs:L57-L67
//   Jalr                     crates/core/machine/src/control_flow/jalr/trace.rs:L111-L128
//
// Column order = the reference's #[repr(C)] column structs (sp1_amd/machines/riscv.py transcribes the same structs; its layouts
// are what the tests compare the constants below with). Every index into Row::c and every limb index is a constant (fully
// unrolled loops), so on the device a row is registers.
#pragma once
#include "tg_row_kernel.hpp"

namespace sp1hip {
namespace tg {

// flags of sp1hip_rv64_alu_event_t.ops (bits 32..): operand b / c is an immediate
constexpr uint64_t F_IMM_C = 1ull << 33;                     // (bit 32: operand b is an immediate — JAL, LUI, AUIPC; it travels as b)
constexpr uint32_t POS_C = 2, POS_B = 3, POS_A = 4;         // MemoryAccessPosition (core/executor/src/events/memory.rs:L63-L74)

struct Ev { uint64_t pc, clk, ops, a, b, c, a_prev, a_pts, b_pts, c_pts, aux; };

// Opcode numbers (core/executor/src/opcode.rs:L46-L153, sp1_amd/machines/riscv.py OPC)
enum : uint32_t { OP_SRL = 7, OP_SRA = 8, OP_MUL = 11, OP_MULH = 12, OP_MULHU = 13, OP_MULHSU = 14, OP_SRLW = 22, OP_SRAW = 23, OP_MULW = 24,
                  OP_BEQ = 40, OP_BNE = 41, OP_BLT = 42, OP_BGE = 43, OP_BLTU = 44, OP_BGEU = 45 };
enum : uint32_t { OP_XOR = 3, OP_OR = 4, OP_AND = 5, OP_SLL = 6, OP_SLT = 9, OP_SLTU = 10, OP_SLLW = 21, OP_AUIPC = 48 };

// CPUState at columns 0..5
template <int W> TG_HD void fill_state(Row<W>& r, const Ev& e) {
    r.c[0] = (uint32_t)(e.clk >> 24); r.c[1] = (uint32_t)(e.clk >> 16) & 0xff; r.c[2] = (uint32_t)e.clk & M16;
    r.limbs3(3, e.pc);
}
// RegisterAccessCols at `at`: prev_value[4], prev_low, diff_low_limb. A previous access on the other side of a 2^24 clock
// boundary is bridged by a MemoryBump row (host side, rare): the columns then compare against 0
template <int W> TG_HD void fill_access(Row<W>& r, int at, uint64_t value, uint64_t t_prev, uint64_t t_cur, bool live = true) {
    r.limbs4(at, value);
    const bool cross = (t_prev >> 24) != (t_cur >> 24);
    const uint32_t old = cross ? 0u : (uint32_t)t_prev & 0xffffffu;
    const uint32_t diff = ((uint32_t)t_cur & 0xffffffu) - old - 1u;
    r.c[at + 4] = live ? old : 0u;
    r.c[at + 5] = live ? (diff & M16) : 0u;
}
// the part every adapter shares: op_a, its access, op_a_0 (columns 6..13)
template <int W> TG_HD void fill_a(Row<W>& r, const Ev& e) {
    const uint32_t ra = (uint32_t)(e.ops >> 8) & 0xff;
    r.c[6] = ra;
    fill_access(r, 7, e.a_prev, e.a_pts, e.clk + POS_A);
    r.c[13] = ra == 0;
}
// the part the R / I / ALU adapters share: op_a, its access, op_a_0, op_b, its access (columns 6..20)
template <int W> TG_HD void fill_ab(Row<W>& r, const Ev& e) {
    const uint32_t ra = (uint32_t)(e.ops >> 8) & 0xff, rb = (uint32_t)(e.ops >> 16) & 0xff;
    r.c[6] = ra;
    fill_access(r, 7, e.a_prev, e.a_pts, e.clk + POS_A);
    r.c[13] = ra == 0;
    r.c[14] = rb;
    fill_access(r, 15, e.b, e.b_pts, e.clk + POS_B);
}
// RTypeReader: + op_c, its access (21..27)
template <int W> TG_HD void fill_r(Row<W>& r, const Ev& e) {
    fill_ab(r, e);
    r.c[21] = (uint32_t)(e.ops >> 24) & 0xff;
    fill_access(r, 22, e.c, e.c_pts, e.clk + POS_C);
}
// ITypeReader: + op_c_imm[4] (21..24)
template <int W> TG_HD void fill_i(Row<W>& r, const Ev& e) {
    fill_ab(r, e);
    r.limbs4(21, e.c);
}
// ALUTypeReader: + op_c[4] (a register number or the immediate's limbs), its access (no access for an immediate; prev_value
// holds the operand either way), imm_c (21..31)
template <int W> TG_HD void fill_alu(Row<W>& r, const Ev& e) {
    fill_ab(r, e);
    const bool imm = (e.ops & F_IMM_C) != 0;
    if (imm) r.limbs4(21, e.c); else { r.c[21] = (uint32_t)(e.ops >> 24) & 0xff; r.c[22] = r.c[23] = r.c[24] = 0; }
    fill_access(r, 25, e.c, e.c_pts, e.clk + POS_C, !imm);
    r.c[31] = imm;
}
// JTypeReader: op_a, its access, op_a_0, then op_b_imm[4] (14..17) and op_c_imm[4] (18..21): both operands are immediates, b
// travels as the event's b (bit 32 of ops); c is the same immediate for LUI / AUIPC and zero for JAL (instruction.rs)
template <int W> TG_HD void fill_j(Row<W>& r, const Ev& e, bool c_is_b) {
    fill_a(r, e);
    r.limbs4(14, e.b);
    r.limbs4(18, c_is_b ? e.b : 0ull);
}

// LtOperationSigned / Unsigned::populate at `at`: bit, u16_flags[4], not_eq_inv, comparison_limbs[2], b_msb, c_msb
template <int W> TG_HD void fill_lt(Row<W>& r, int at, uint64_t b, uint64_t c, bool is_signed) {
    uint32_t bl[4], cl[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { bl[i] = (b >> (16 * i)) & M16; cl[i] = (c >> (16 * i)) & M16; }
    r.c[at + 8] = is_signed ? bl[3] >> 15 : 0u;
    r.c[at + 9] = is_signed ? cl[3] >> 15 : 0u;
    if (is_signed) { bl[3] ^= 0x8000u; cl[3] ^= 0x8000u; }
    int idx = -1;
#pragma unroll
    for (int i = 0; i < 4; i++) if (bl[i] != cl[i]) idx = i;               // the most significant limb that differs
    uint32_t bs = 0, cs = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) { r.c[at + 1 + i] = idx == i; if (idx == i) { bs = bl[i]; cs = cl[i]; } }
    r.c[at + 6] = bs; r.c[at + 7] = cs;
    // not_eq_inv = (b_sel - c_sel)^-1 in the field (canonical; the store converts)
    r.c[at + 5] = idx < 0 ? 0u : kb::from_monty(kb::inv(kb::to_monty(bs >= cs ? bs - cs : kb::P - (cs - bs))));
    r.c[at] = bs < cs;
}

enum Chip : int { ADD = 0, ADDI = 1, SUB = 2, ADDW = 3, SUBW = 4, MUL = 5, SHIFT_RIGHT = 6, BRANCH = 7,
                  BITWISE = 8, LT = 9, SHIFT_LEFT = 10, UTYPE = 11, JAL = 12, JALR = 13, N_CHIPS = 14 };
__host__ __device__ constexpr int width_of(int chip) {
    return chip == ADD || chip == SUB ? 33 : chip == ADDI ? 30 : chip == ADDW ? 36 : chip == SUBW ? 32 : chip == MUL ? 82 : chip == SHIFT_RIGHT ? 69 :
           chip == BITWISE ? 51 : chip == LT ? 44 : chip == SHIFT_LEFT ? 65 : chip == UTYPE || chip == JAL ? 31 : chip == JALR ? 35 : 45;
}

// The columns behind the adapter, per chip (what `riscv_rows host layout` prints and the tests compare with riscv.py)
namespace col {
constexpr int BITWISE_B_LOW = 32, BITWISE_C_LOW = 36, BITWISE_RESULT = 40, BITWISE_IS_XOR = 48, BITWISE_IS_OR = 49, BITWISE_IS_AND = 50;
constexpr int LT_IS_SLT = 32, LT_IS_SLTU = 33, LT_LT = 34;
constexpr int SLL_A = 32, SLL_C_BITS = 36, SLL_V_01 = 42, SLL_V_012 = 43, SLL_V_0123 = 44, SLL_SHIFT_U16 = 45, SLL_LOWER = 49, SLL_HIGHER = 53,
              SLL_RESULT = 57, SLL_MSB = 61, SLL_IS_SLL = 62, SLL_IS_SLLW = 63, SLL_IS_SLLW_IMM = 64;
constexpr int UTYPE_ADDEND = 22, UTYPE_VALUE = 25, UTYPE_IS_AUIPC = 29, UTYPE_IS_REAL = 30;
constexpr int JAL_NEXT_PC = 22, JAL_OP_A_VALUE = 26, JAL_IS_REAL = 30;
constexpr int JALR_IS_REAL = 25, JALR_NEXT_PC = 26, JALR_OP_A_VALUE = 30, JALR_LSB = 34;
}  // namespace col

template <int CHIP> TG_HD void fill_row(Row<width_of(CHIP)>& r, const Ev& e) {
    constexpr int W = width_of(CHIP);
    const uint32_t op = (uint32_t)e.ops & 0xff;
    fill_state(r, e);
    if constexpr (CHIP == ADD || CHIP == SUB) {               // state | RTypeReader | value[4] | is_real
        fill_r(r, e);
        r.limbs4(28, e.a);
        r.c[32] = 1;
    } else if constexpr (CHIP == ADDI) {                      // state | ITypeReader | value[4] | is_real
        fill_i(r, e);
        r.limbs4(25, e.a);
        r.c[29] = 1;
    } else if constexpr (CHIP == ADDW) {                      // state | ALUTypeReader | value[2] | msb | is_real
        fill_alu(r, e);
        r.c[32] = e.a & M16; r.c[33] = (e.a >> 16) & M16; r.c[34] = (uint32_t)(e.a >> 31) & 1; r.c[35] = 1;
    } else if constexpr (CHIP == SUBW) {                      // state | RTypeReader | value[2] | msb | is_real
        fill_r(r, e);
        r.c[28] = e.a & M16; r.c[29] = (e.a >> 16) & M16; r.c[30] = (uint32_t)(e.a >> 31) & 1; r.c[31] = 1;
    } else if constexpr (CHIP == MUL) {                       // state | RTypeReader | a[4] | MulOperation | is_mul .. is_mulw
        fill_r(r, e);
        r.limbs4(28, e.a);
        const bool mulh = op == OP_MULH, mulhsu = op == OP_MULHSU, mulw = op == OP_MULW;
        const uint32_t b_msb = (uint32_t)(e.b >> 63), c_msb = (uint32_t)(e.c >> 63);
        const uint32_t bse = (mulh || mulhsu) ? b_msb : 0u, cse = mulh ? c_msb : 0u;
        // 16 x 16 byte product (the operands sign-extended to 128 bits), low 16 bytes with their carries
        uint32_t prod[16];
#pragma unroll
        for (int i = 0; i < 16; i++) prod[i] = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t bi = i < 8 ? (uint32_t)(e.b >> (8 * i)) & 0xff : bse * 0xffu;
#pragma unroll
            for (int j = 0; j < 16 - i; j++) {
                const uint32_t cj = j < 8 ? (uint32_t)(e.c >> (8 * j)) & 0xff : cse * 0xffu;
                prod[i + j] += bi * cj;
            }
        }
        uint32_t carry = 0;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const uint32_t v = prod[i] + carry;
            carry = v >> 8;
            r.c[32 + i] = carry;                              // mul.carry[i]
            r.c[48 + i] = v & 0xff;                           // mul.product[i]
        }
#pragma unroll
        for (int i = 0; i < 4; i++) { r.c[64 + i] = (uint32_t)(e.b >> (16 * i)) & 0xff; r.c[68 + i] = (uint32_t)(e.c >> (16 * i)) & 0xff; }
        r.c[72] = b_msb; r.c[73] = c_msb;
        r.c[74] = mulw ? (uint32_t)(e.a >> 31) & 1 : 0u;      // product_msb
        r.c[75] = bse; r.c[76] = cse;
        r.c[77] = op == OP_MUL; r.c[78] = mulh; r.c[79] = op == OP_MULHU; r.c[80] = mulhsu; r.c[81] = mulw;
    } else if constexpr (CHIP == SHIFT_RIGHT) {               // alu/sr/mod.rs ShiftRightCols
        fill_alu(r, e);
        const bool sra = op == OP_SRA, srlw = op == OP_SRLW, sraw = op == OP_SRAW, w = srlw || sraw;
        r.limbs4(32, e.a);
        const uint32_t c16 = (uint32_t)e.c & M16;
#pragma unroll
        for (int i = 0; i < 6; i++) r.c[38 + i] = (c16 >> i) & 1;
        const uint32_t amount = ((c16 >> 4) & 1) + (w ? 0u : 2 * ((c16 >> 5) & 1)), s = c16 & 15;
#pragma unroll
        for (int i = 0; i < 4; i++) r.c[60 + i] = amount == (uint32_t)i;
        const uint32_t v = 1u << (16 - s);
        r.c[47] = 1u << (4 - (s & 3)); r.c[46] = 1u << (8 - (s & 7)); r.c[45] = v;
        uint32_t bl[4];
#pragma unroll
        for (int i = 0; i < 4; i++) bl[i] = (uint32_t)(e.b >> (16 * i)) & M16;
        const uint32_t msb = sra ? bl[3] >> 15 : sraw ? bl[1] >> 15 : 0u;
        r.c[36] = msb; r.c[44] = msb * v;
        if (w) bl[2] = bl[3] = 0;
        r.c[37] = w ? (uint32_t)(e.a >> 31) & 1 : 0u;         // srw_msb
        uint32_t lower[4], higher[4];
#pragma unroll
        for (int i = 0; i < 4; i++) { lower[i] = bl[i] & ((1u << s) - 1); higher[i] = bl[i] >> s; r.c[48 + i] = lower[i]; r.c[52 + i] = higher[i]; }
#pragma unroll
        for (int i = 0; i < 4; i++) r.c[56 + i] = higher[i] + (i < 3 ? lower[i + 1] * v : 0u);
        r.c[64] = op == OP_SRL; r.c[65] = sra; r.c[66] = srlw; r.c[67] = sraw;
        r.c[68] = w && (e.ops & F_IMM_C);
    } else if constexpr (CHIP == BITWISE) {                   // state | ALUTypeReader | b_low_bytes[4] | c_low_bytes[4] | result[8] | is_xor, is_or, is_and
        fill_alu(r, e);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            r.c[col::BITWISE_B_LOW + i] = (uint32_t)(e.b >> (16 * i)) & 0xff;
            r.c[col::BITWISE_C_LOW + i] = (uint32_t)(e.c >> (16 * i)) & 0xff;
        }
#pragma unroll
        for (int i = 0; i < 8; i++) r.c[col::BITWISE_RESULT + i] = (uint32_t)(e.a >> (8 * i)) & 0xff;
        r.c[col::BITWISE_IS_XOR] = op == OP_XOR; r.c[col::BITWISE_IS_OR] = op == OP_OR; r.c[col::BITWISE_IS_AND] = op == OP_AND;
    } else if constexpr (CHIP == LT) {                        // state | ALUTypeReader | is_slt | is_sltu | LtOperationSigned on (b, c)
        fill_alu(r, e);
        const bool slt = op == OP_SLT;
        r.c[col::LT_IS_SLT] = slt; r.c[col::LT_IS_SLTU] = !slt;
        fill_lt(r, col::LT_LT, e.b, e.c, slt);
    } else if constexpr (CHIP == SHIFT_LEFT) {                // alu/sll/mod.rs ShiftLeftCols
        fill_alu(r, e);
        const bool w = op == OP_SLLW;
        r.limbs4(col::SLL_A, e.a);
        const uint32_t c16 = (uint32_t)e.c & M16;
#pragma unroll
        for (int i = 0; i < 6; i++) r.c[col::SLL_C_BITS + i] = (c16 >> i) & 1;
        const uint32_t amount = ((c16 >> 4) & 1) + (w ? 0u : 2 * ((c16 >> 5) & 1)), s = c16 & 15;
#pragma unroll
        for (int i = 0; i < 4; i++) r.c[col::SLL_SHIFT_U16 + i] = amount == (uint32_t)i;
        r.c[col::SLL_V_01] = 1u << (s & 3); r.c[col::SLL_V_012] = 1u << (s & 7); r.c[col::SLL_V_0123] = 1u << s;
        uint32_t lower[4], higher[4];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t bl = (uint32_t)(e.b >> (16 * i)) & M16;
            lower[i] = bl & ((1u << (16 - s)) - 1); higher[i] = bl >> (16 - s);
            r.c[col::SLL_LOWER + i] = lower[i]; r.c[col::SLL_HIGHER + i] = higher[i];
        }
#pragma unroll
        for (int i = 0; i < 4; i++) r.c[col::SLL_RESULT + i] = (lower[i] << s) + (i > 0 ? higher[i > 0 ? i - 1 : 0] : 0u);
        r.c[col::SLL_MSB] = w ? (uint32_t)(e.a >> 31) & 1 : 0u;
        r.c[col::SLL_IS_SLL] = !w; r.c[col::SLL_IS_SLLW] = w;
        r.c[col::SLL_IS_SLLW_IMM] = w && (e.ops & F_IMM_C);
    } else if constexpr (CHIP == UTYPE) {                     // state | JTypeReader | addend[3] | value[4] | is_auipc | is_real
        fill_j(r, e, true);
        const bool auipc = op == OP_AUIPC;
        r.limbs3(col::UTYPE_ADDEND, auipc ? e.pc : 0ull);
        r.limbs4(col::UTYPE_VALUE, e.a);
        r.c[col::UTYPE_IS_AUIPC] = auipc; r.c[col::UTYPE_IS_REAL] = 1;
    } else if constexpr (CHIP == JAL) {                       // state | JTypeReader | next_pc[4] | op_a_value[4] | is_real
        fill_j(r, e, false);
        const bool rd0 = ((e.ops >> 8) & 0xff) == 0;
        r.limbs4(col::JAL_NEXT_PC, e.pc + e.b);
        r.limbs4(col::JAL_OP_A_VALUE, rd0 ? 0ull : e.pc + 4);   // the link value; nothing is written to x0
        r.c[col::JAL_IS_REAL] = 1;
    } else if constexpr (CHIP == JALR) {                      // state | ITypeReader | is_real | next_pc[4] | op_a_value[4] | lsb
        fill_i(r, e);
        const bool rd0 = ((e.ops >> 8) & 0xff) == 0;
        const uint64_t target = e.b + e.c;                    // before its low bit is cleared
        r.c[col::JALR_IS_REAL] = 1;
        r.limbs4(col::JALR_NEXT_PC, target);
        r.limbs4(col::JALR_OP_A_VALUE, rd0 ? 0ull : e.pc + 4);
        r.c[col::JALR_LSB] = (uint32_t)target & 1;
    } else {                                                  // BRANCH: state | ITypeReader | next_pc[3] | is_beq .. is_bgeu | is_branching | cmp
        fill_i(r, e);
        r.limbs3(25, e.aux);                                  // next_pc: where execution goes on (pc + 4, or pc + offset when taken)
#pragma unroll
        for (int i = 0; i < 6; i++) r.c[28 + i] = op == OP_BEQ + i;
        const bool is_signed = op == OP_BLT || op == OP_BGE;
        const uint64_t av = e.a_prev, bv = e.b;
        const bool eq = av == bv, lt = is_signed ? (int64_t)av < (int64_t)bv : av < bv;
        r.c[34] = op == OP_BEQ ? eq : op == OP_BNE ? !eq : (op == OP_BLT || op == OP_BLTU) ? lt : !lt;
        fill_lt(r, 35, av, bv, is_signed);
    }
    (void)W;
}

// A padding row (row >= n_events) from the all-zero row: the two shift chips have a template, every other chip's is zero
template <int CHIP> TG_HD void fill_padding(Row<width_of(CHIP)>& r) {
    if (CHIP == SHIFT_RIGHT) { r.c[47] = 16; r.c[46] = 256; r.c[45] = 65536; }       // the padded row template (alu/sr/mod.rs:L165-L171)
    if (CHIP == SHIFT_LEFT) { r.c[col::SLL_V_01] = 1; r.c[col::SLL_V_012] = 1; r.c[col::SLL_V_0123] = 1; }   // alu/sll/mod.rs:L154-L160
}

// The chip of row_kernel / host_rows (tg_row_kernel.hpp) for each of the fourteen
template <int CHIP> struct AluChip {
    static constexpr int WIDTH = width_of(CHIP);
    using Rec = Ev;
    static TG_HD void live(Row<WIDTH>& r, const Ev* __restrict__ events, uint32_t row) { fill_row<CHIP>(r, events[row]); }
    static TG_HD void padding(Row<WIDTH>& r) { fill_padding<CHIP>(r); }
};

}  // namespace tg
}  // namespace sp1hip
