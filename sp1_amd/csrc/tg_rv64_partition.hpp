// sp1_amd/csrc/tg_rv64_partition.hpp — where an executed instruction goes and what it becomes there, for host and device code
// alike (as the other tg_* headers are for the rows): the classification of the executor's 20-word event record into the 29 bins of
// sp1hip_rv64_partition_* (include/sp1hip.h has the table) and the packers that make the bins' records. tracegen_rv64_partition.hip
// calls them one lane per event; tests/native/riscv_sys_rows.hip runs the same functions on the CPU, so the routing and every word of
// every record can be compared with riscv_exec.chip_of_events, pack_alu_events and pack_mem_events without a GPU.
//
//   routing     core/executor/src/tracing.rs: emit_alu_event L1153-L1228, emit_mem_instr_event L1096-L1150 (rd = x0 sends an ALU
//               opcode to AluX0 and a load to LoadX0)
//   StateBump   crates/core/machine/src/adapter/bump.rs: a row for every instruction whose clock step carries out of the low 24 bits
//               or whose pc + 4 carries out of the low 16 (branches, jumps and HALT send next_pc in normal form: no pc carry)
//   MemoryBump  crates/core/machine/src/memory/bump.rs: a row for every register access whose previous timestamp lies in another
//               2^24 window — exactly the accesses for which fill_access (tg_riscv_rows.hpp) compares against 0 (`cross`)
#pragma once
#include <stdint.h>

#ifndef TG_HD
#define TG_HD __host__ __device__ __forceinline__
#endif

namespace sp1hip {
namespace tg {

// the executor's record (sp1_amd/csrc/rv64_exec.cpp; riscv_exec.py E_*): 20 u64 words
struct RawEv {
    uint64_t pc, clk, op, op_a, op_b, op_c, flags, a, b, c, a_prev, a_pts, b_pts, c_pts, m_addr, m_pts, m_prev, m_new, next_pc, spare;
};
constexpr int RAW_EV_WORDS = 20;

constexpr int BINS = 29, BIN_SLOTS = 32;                       // a counter row has 32 words: bins 29..31 stay zero
constexpr int BIN_MEM0 = 14, BIN_DIVREM = 23, BIN_ALU_X0 = 24, BIN_SYSCALL_INSTRS = 25, BIN_SYSCALL_CORE = 26, BIN_STATE_BUMP = 27,
              BIN_MEMORY_BUMP = 28, BIN_NONE = 31;
constexpr int ALU_WORDS = 11, MEM_WORDS = 12, STATE_BUMP_WORDS = 4, MEMORY_BUMP_WORDS = 4;
constexpr uint32_t OPC_LAST_ALU = 28, OPC_FIRST_LOAD = 29, OPC_LAST_LOAD = 35, OPC_BEQ = 40, OPC_JALR = 47, OPC_ECALL = 50;
constexpr uint64_t ECALL_CLK_INC = 8 + 256, CLK_INC = 8;       // syscall/instructions/air.rs:L66-L72
constexpr uint64_t LOW24 = 0xffffffull;

__host__ __device__ constexpr int words_of_bin(int bin) {
    return bin < BIN_MEM0 ? ALU_WORDS : bin < BIN_DIVREM ? MEM_WORDS : bin <= BIN_SYSCALL_CORE ? ALU_WORDS : bin == BIN_STATE_BUMP ? STATE_BUMP_WORDS
                                                                                                                              : MEMORY_BUMP_WORDS;
}

// The instruction's bin, 0..25 (BIN_NONE for EBREAK, UNIMP and numbers that are no opcode: the executor records none). The table
// opcode -> bin for a destination other than x0 is five 64-bit constants of twelve 5-bit entries each, picked by opcode / 12: registers
TG_HD int bin_of(uint64_t op64, uint64_t rd) {
    if (op64 > OPC_ECALL) return BIN_NONE;
    const uint32_t op = (uint32_t)op64;
    if (rd == 0 && op <= OPC_LAST_ALU) return BIN_ALU_X0;
    if (rd == 0 && op >= OPC_FIRST_LOAD && op <= OPC_LAST_LOAD) return BIN_MEM0 + 4;     // LoadX0
    // opcode:             ADD ADDI SUB XOR OR AND SLL SRL SRA SLT SLTU MUL
    constexpr uint64_t T0 = 0ull | 1ull << 5 | 2ull << 10 | 8ull << 15 | 8ull << 20 | 8ull << 25 | 10ull << 30 | 6ull << 35 | 6ull << 40 | 9ull << 45 |
                            9ull << 50 | 5ull << 55;
    // MULH MULHU MULHSU DIV DIVU REM REMU ADDW SUBW SLLW SRLW SRAW
    constexpr uint64_t T1 = 5ull | 5ull << 5 | 5ull << 10 | 23ull << 15 | 23ull << 20 | 23ull << 25 | 23ull << 30 | 3ull << 35 | 4ull << 40 | 10ull << 45 |
                            6ull << 50 | 6ull << 55;
    // MULW DIVW DIVUW REMW REMUW LB LH LW LBU LHU LWU LD
    constexpr uint64_t T2 = 5ull | 23ull << 5 | 23ull << 10 | 23ull << 15 | 23ull << 20 | 14ull << 25 | 15ull << 30 | 16ull << 35 | 14ull << 40 |
                            15ull << 45 | 16ull << 50 | 17ull << 55;
    // SB SH SW SD BEQ BNE BLT BGE BLTU BGEU JAL JALR
    constexpr uint64_t T3 = 19ull | 20ull << 5 | 21ull << 10 | 22ull << 15 | 7ull << 20 | 7ull << 25 | 7ull << 30 | 7ull << 35 | 7ull << 40 | 7ull << 45 |
                            12ull << 50 | 13ull << 55;
    // AUIPC LUI ECALL
    constexpr uint64_t T4 = 11ull | 11ull << 5 | 25ull << 10;
    const uint32_t q = op / 12u, r = op - 12u * q;
    const uint64_t t = q == 0 ? T0 : q == 1 ? T1 : q == 2 ? T2 : q == 3 ? T3 : T4;
    return (int)((t >> (5u * r)) & 31u);
}

// The register slots the bin's adapter reads (Tracer.fill_adapter): bit 0 = A, bit 1 = B, bit 2 = C. R: Add, Sub, Subw, Mul, DivRem,
// SyscallInstrs; I: Addi, Branch, Jalr and the nine load and store chips; ALU (C only when it is a register): Addw, ShiftRight,
// Bitwise, Lt, ShiftLeft, AluX0; J: UType, Jal
TG_HD uint32_t slots_of(int bin, bool imm_c) {
    constexpr uint32_t R_BINS = 1u << 0 | 1u << 2 | 1u << 4 | 1u << 5 | 1u << BIN_DIVREM | 1u << BIN_SYSCALL_INSTRS;
    constexpr uint32_t ALU_BINS = 1u << 3 | 1u << 6 | 1u << 8 | 1u << 9 | 1u << 10 | 1u << BIN_ALU_X0;
    constexpr uint32_t J_BINS = 1u << 11 | 1u << 12;
    if (bin >= BIN_SYSCALL_CORE) return 0u;
    const uint32_t b = 1u << bin;
    if (b & R_BINS) return 7u;
    if (b & ALU_BINS) return imm_c ? 3u : 7u;
    if (b & J_BINS) return 1u;
    return 3u;
}

// What an event adds beside its instruction record
struct Extra {
    bool syscall_core, state_bump;
    uint32_t bumps;                 // bit 0 / 1 / 2: the access of slot A / B / C needs a MemoryBump row
};

TG_HD bool crosses(uint64_t t_prev, uint64_t t_cur) { return (t_prev >> 24) != (t_cur >> 24); }

TG_HD Extra extra_of(const RawEv& e, int bin) {
    Extra x;
    const bool ecall = bin == BIN_SYSCALL_INSTRS;
    x.syscall_core = ecall && ((e.a_prev >> 8) & 0xff) == 1;
    const bool halt = ecall && (e.a_prev & 0xff) == 0;
    const bool normal_pc = (e.op >= OPC_BEQ && e.op <= OPC_JALR) || halt;
    const bool pc_carry = !normal_pc && ((e.pc & 0xffff) + 4 > 0xffff);
    const uint64_t inc = ecall ? ECALL_CLK_INC : CLK_INC;
    x.state_bump = bin != BIN_NONE && (pc_carry || (e.clk & LOW24) + inc >= (1ull << 24));
    const uint32_t slots = slots_of(bin, (e.flags & 2) != 0);
    x.bumps = (slots & 1u && crosses(e.a_pts, e.clk + 4) ? 1u : 0u) | (slots & 2u && crosses(e.b_pts, e.clk + 3) ? 2u : 0u) |
              (slots & 4u && crosses(e.c_pts, e.clk + 2) ? 4u : 0u);
    if (bin == BIN_NONE) x.bumps = 0;
    return x;
}

// sp1hip_rv64_alu_event_t, word for word riscv_exec.pack_alu_events
TG_HD void pack_alu(uint64_t* o, const RawEv& e) {
    const uint64_t imm_b = e.flags & 1, imm_c = (e.flags >> 1) & 1;
    o[0] = e.pc; o[1] = e.clk;
    o[2] = e.op | e.op_a << 8 | (imm_b ? 0ull : (e.op_b & 0xff) << 16) | (imm_c ? 0ull : (e.op_c & 0xff) << 24) | (e.flags & 3) << 32;
    o[3] = e.a;
    o[4] = imm_b ? e.op_b : e.b;
    o[5] = imm_c ? e.op_c : e.c;
    o[6] = e.a_prev; o[7] = e.a_pts; o[8] = e.b_pts; o[9] = e.c_pts; o[10] = e.next_pc;
}

// sp1hip_rv64_mem_event_t, word for word riscv_exec.pack_mem_events
TG_HD void pack_mem(uint64_t* o, const RawEv& e) {
    o[0] = e.pc; o[1] = e.clk;
    o[2] = e.op | e.op_a << 8 | (e.op_b & 0xff) << 16;
    o[3] = e.b; o[4] = e.op_c; o[5] = e.a_prev; o[6] = e.a_pts; o[7] = e.b_pts; o[8] = e.m_addr; o[9] = e.m_pts; o[10] = e.m_prev; o[11] = e.m_new;
}

// StateBump's record: clk, pc, next_pc, the clock step | pc_carry << 32
TG_HD void pack_state_bump(uint64_t* o, const RawEv& e, int bin) {
    const bool ecall = bin == BIN_SYSCALL_INSTRS;
    const bool halt = ecall && (e.a_prev & 0xff) == 0;
    const bool normal_pc = (e.op >= OPC_BEQ && e.op <= OPC_JALR) || halt;
    const uint64_t pc_carry = !normal_pc && ((e.pc & 0xffff) + 4 > 0xffff);
    o[0] = e.clk; o[1] = e.pc; o[2] = e.next_pc; o[3] = (ecall ? ECALL_CLK_INC : CLK_INC) | pc_carry << 32;
}

// MemoryBump's record for slot 0 / 1 / 2 = A / B / C: register, previous timestamp, value, the start of the access's window
TG_HD void pack_memory_bump(uint64_t* o, const RawEv& e, int slot) {
    const uint64_t t_cur = e.clk + (slot == 0 ? 4 : slot == 1 ? 3 : 2);
    o[0] = slot == 0 ? e.op_a : slot == 1 ? e.op_b : e.op_c;
    o[1] = slot == 0 ? e.a_pts : slot == 1 ? e.b_pts : e.c_pts;
    o[2] = slot == 0 ? e.a_prev : slot == 1 ? e.b : e.c;
    o[3] = (t_cur >> 24) << 24;
}

}  // namespace tg
}  // namespace sp1hip
