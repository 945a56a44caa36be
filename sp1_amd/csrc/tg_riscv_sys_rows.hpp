// sp1_amd/csrc/tg_riscv_sys_rows.hpp — the rows of the four small chips of a core shard: SyscallInstrs, SyscallCore, StateBump and
// MemoryBump, and the Global event a SyscallCore row sends, for host and device code alike (as tg_riscv_core_rows.hpp is for DivRem,
// AluX0 and MemoryLocal, whose event record, Row, CPUState, R adapter and inverse it takes). tracegen_riscv_sys.hip calls them one
// lane per row; tests/native/riscv_sys_rows.hip runs the same functions on the CPU, so every word can be compared with the host
// tracer (sp1_amd/machines/riscv_trace.py syscall_instrs, _bump_rows; riscv_exec.py EventTracer.state_chain) without a GPU.
//
//   SyscallInstrs  crates/core/machine/src/syscall/instructions/{air,trace}.rs (event_to_row: next_pc is not normalised, HALT jumps
//                  to 1; the five IsZero operations of syscall_id - c; COMMIT / COMMIT_DEFERRED_PROOFS index bitmap and digest word)
//   SyscallCore    crates/core/machine/src/syscall/chip.rs (generate_trace_into; its Global send L299-L420)
//   StateBump      crates/core/machine/src/adapter/bump.rs
//   MemoryBump     crates/core/machine/src/memory/bump.rs
//
// The records are the bins 25..28 of sp1hip_rv64_partition_scatter (tg_rv64_partition.hpp packs them).
#pragma once
#include "tg_riscv_core_rows.hpp"

namespace sp1hip {
namespace tg {

constexpr int SYSCALL_INSTRS_WIDTH = 65, SYSCALL_CORE_WIDTH = 10, STATE_BUMP_WIDTH = 14, MEMORY_BUMP_WIDTH = 15;
constexpr int STATE_BUMP_RECORD_WORDS = 4, MEMORY_BUMP_RECORD_WORDS = 4;
constexpr uint32_t KIND_SYSCALL = 8;                          // InteractionKind::Syscall
constexpr uint32_t SYSCALL_HALT = 0x00, SYSCALL_ENTER_UNCONSTRAINED = 0x03, SYSCALL_COMMIT = 0x10, SYSCALL_COMMIT_DEFERRED_PROOFS = 0x1A,
                   SYSCALL_HINT_LEN = 0xF0;
constexpr uint32_t TOP_LIMB = (kb::P - 1) >> 16;              // a 16-bit limb 1 below this keeps a three-limb value under the modulus

namespace col {
// SyscallInstrs behind CPUState and the R adapter (0..27)
constexpr int SI_NEXT_PC = 28, SI_IS_HALT = 31, SI_OP_A_VALUE = 32, SI_A_LOW_BYTES = 36, SI_IS_ENTER_UNCONSTRAINED = 40, SI_IS_HINT_LEN = 42,
              SI_IS_HALT_CHECK = 44, SI_IS_COMMIT = 46, SI_IS_COMMIT_DEFERRED_PROOFS = 48, SI_INDEX_BITMAP = 50, SI_EXPECTED_DIGEST = 58,
              SI_OP_B_RANGE_CHECK = 62, SI_OP_C_RANGE_CHECK = 63, SI_IS_REAL = 64;
constexpr int SC_CLK_HIGH = 0, SC_CLK_LOW = 1, SC_SYSCALL_ID = 2, SC_ARG1 = 3, SC_ARG2 = 6, SC_IS_REAL = 9;
constexpr int SB_NEXT_CLK_32_48 = 0, SB_NEXT_CLK_24_32 = 1, SB_NEXT_CLK_16_24 = 2, SB_NEXT_CLK_0_16 = 3, SB_CLK_HIGH = 4, SB_CLK_LOW = 5,
              SB_NEXT_PC = 6, SB_PC = 9, SB_IS_CLK = 12, SB_IS_REAL = 13;
constexpr int MB_PREV_VALUE = 0, MB_PREV_HIGH = 4, MB_PREV_LOW = 5, MB_COMPARE_LOW = 6, MB_DIFF_LOW_LIMB = 7, MB_DIFF_HIGH_LIMB = 8, MB_CLK_32_48 = 9,
              MB_CLK_24_32 = 10, MB_CLK_16_24 = 11, MB_CLK_0_16 = 12, MB_ADDR = 13, MB_IS_REAL = 14;
}  // namespace col

// IsZeroOperation at `at` on sid - c: inverse, result
template <int W> TG_HD void fill_is_zero_of(Row<W>& r, int at, uint32_t sid, uint32_t c) {
    const uint32_t d = sid >= c ? sid - c : kb::P - (c - sid);
    r.c[at] = inv_canonical(d);
    r.c[at + 1] = d == 0;
}

// SyscallInstrs from the ECALL's sp1hip_rv64_alu_event_t (a_prev = the syscall code in t0, b / c = a0 / a1, a = the value written
// to t0); padding rows are zero
TG_HD void fill_syscall_instrs(Row<SYSCALL_INSTRS_WIDTH>& r, const Ev& e) {
    namespace c = col;
    fill_state(r, e);
    fill_r(r, e);
    const uint64_t code = e.a_prev;
    const uint32_t sid = (uint32_t)code & 0xff;
    const bool halt = sid == SYSCALL_HALT, commit = sid == SYSCALL_COMMIT, cdp = sid == SYSCALL_COMMIT_DEFERRED_PROOFS;
    r.limbs3(c::SI_NEXT_PC, e.pc);
    r.c[c::SI_NEXT_PC] += 4;                                   // not normalised: limb 0 = pc[0] + 4
    if (halt) { r.c[c::SI_NEXT_PC] = 1; r.c[c::SI_NEXT_PC + 1] = 0; r.c[c::SI_NEXT_PC + 2] = 0; }
    r.c[c::SI_IS_HALT] = halt;
    r.limbs4(c::SI_OP_A_VALUE, e.a);
#pragma unroll
    for (int i = 0; i < 4; i++) r.c[c::SI_A_LOW_BYTES + i] = (uint32_t)(code >> (16 * i)) & 0xff;
    fill_is_zero_of(r, c::SI_IS_ENTER_UNCONSTRAINED, sid, SYSCALL_ENTER_UNCONSTRAINED);
    fill_is_zero_of(r, c::SI_IS_HINT_LEN, sid, SYSCALL_HINT_LEN);
    fill_is_zero_of(r, c::SI_IS_HALT_CHECK, sid, SYSCALL_HALT);
    fill_is_zero_of(r, c::SI_IS_COMMIT, sid, SYSCALL_COMMIT);
    fill_is_zero_of(r, c::SI_IS_COMMIT_DEFERRED_PROOFS, sid, SYSCALL_COMMIT_DEFERRED_PROOFS);
    const uint32_t idx = (uint32_t)e.b & 7u;
#pragma unroll
    for (int i = 0; i < 8; i++) r.c[c::SI_INDEX_BITMAP + i] = (commit || cdp) && idx == (uint32_t)i;
#pragma unroll
    for (int i = 0; i < 4; i++) r.c[c::SI_EXPECTED_DIGEST + i] = commit ? (uint32_t)(e.c >> (8 * i)) & 0xff : 0u;
    r.c[c::SI_OP_B_RANGE_CHECK] = halt && ((uint32_t)(e.b >> 16) & M16) < TOP_LIMB;
    r.c[c::SI_OP_C_RANGE_CHECK] = cdp && ((uint32_t)(e.c >> 16) & M16) < TOP_LIMB;
    r.c[c::SI_IS_REAL] = 1;
}

// SyscallCore from the same record (an ECALL whose code asks for a send); padding rows are zero
TG_HD void fill_syscall_core(Row<SYSCALL_CORE_WIDTH>& r, const Ev& e) {
    namespace c = col;
    r.c[c::SC_CLK_HIGH] = (uint32_t)(e.clk >> 24); r.c[c::SC_CLK_LOW] = (uint32_t)e.clk & 0xffffffu;
    r.c[c::SC_SYSCALL_ID] = (uint32_t)e.a_prev & 0xff;
    r.limbs3(c::SC_ARG1, e.b); r.limbs3(c::SC_ARG2, e.c);
    r.c[c::SC_IS_REAL] = 1;
}

// The row's Global event as sp1hip_tracegen_riscv_global reads it, 9 words: message = clk_high, clk_low, syscall_id + arg1[0] * 2^8,
// arg1[1], arg1[2], arg2[3]; then is_receive | kind << 8 — a send of kind Syscall
TG_HD void syscall_core_global_event(int32_t* o, const Ev& e) {
    o[0] = (int32_t)(e.clk >> 24); o[1] = (int32_t)((uint32_t)e.clk & 0xffffffu);
    o[2] = (int32_t)(((uint32_t)e.a_prev & 0xff) + (((uint32_t)e.b & M16) << 8));
    o[3] = (int32_t)((e.b >> 16) & M16); o[4] = (int32_t)((e.b >> 32) & M16);
    o[5] = (int32_t)(e.c & M16); o[6] = (int32_t)((e.c >> 16) & M16); o[7] = (int32_t)((e.c >> 32) & M16);
    o[8] = (int32_t)(KIND_SYSCALL << 8);
}

// StateBump from { clk, pc, next_pc, clock step | pc_carry << 32 }; padding rows are zero
TG_HD void fill_state_bump(Row<STATE_BUMP_WIDTH>& r, const uint64_t* rec) {
    namespace c = col;
    const uint64_t clk = rec[0], pc = rec[1], next_pc = rec[2], inc = rec[3] & 0xffffffffull;
    const bool pc_carry = (rec[3] >> 32) & 1;
    const uint64_t next = clk + inc;
    r.c[c::SB_NEXT_CLK_32_48] = (uint32_t)(next >> 32); r.c[c::SB_NEXT_CLK_24_32] = (uint32_t)(next >> 24) & 0xff;
    r.c[c::SB_NEXT_CLK_16_24] = (uint32_t)(next >> 16) & 0xff; r.c[c::SB_NEXT_CLK_0_16] = (uint32_t)next & M16;
    r.c[c::SB_CLK_HIGH] = (uint32_t)(clk >> 24);
    r.c[c::SB_CLK_LOW] = ((uint32_t)clk & 0xffffffu) + (uint32_t)inc;
    r.limbs3(c::SB_NEXT_PC, next_pc);
    r.limbs3(c::SB_PC, pc_carry ? pc : next_pc);
    if (pc_carry) r.c[c::SB_PC] += 4;                          // the pc as the instruction's row sent it: limb 0 = pc[0] + 4
    r.c[c::SB_IS_CLK] = (next >> 24) != (clk >> 24);
    r.c[c::SB_IS_REAL] = 1;
}

// MemoryBump from { register, previous timestamp, value, the start of the access's 2^24 window }; padding rows are zero
TG_HD void fill_memory_bump(Row<MEMORY_BUMP_WIDTH>& r, const uint64_t* rec) {
    namespace c = col;
    const uint64_t reg = rec[0], tp = rec[1], val = rec[2], tc = rec[3];
    r.limbs4(c::MB_PREV_VALUE, val);
    const uint64_t ph = tp >> 24, d = (tc >> 24) - ph - 1;
    r.c[c::MB_PREV_HIGH] = (uint32_t)ph; r.c[c::MB_PREV_LOW] = (uint32_t)tp & 0xffffffu;
    r.c[c::MB_DIFF_LOW_LIMB] = (uint32_t)d & M16; r.c[c::MB_DIFF_HIGH_LIMB] = (uint32_t)(d >> 16);
    r.c[c::MB_CLK_32_48] = (uint32_t)(tc >> 32); r.c[c::MB_CLK_24_32] = (uint32_t)(tc >> 24) & 0xff;
    r.c[c::MB_ADDR] = (uint32_t)reg;
    r.c[c::MB_IS_REAL] = 1;
}

// The chips of row_kernel / host_rows (tg_row_kernel.hpp)
struct SyscallInstrs : ZeroPaddedChip<SYSCALL_INSTRS_WIDTH, Ev> {
    static TG_HD void live(Row<WIDTH>& r, const Ev* __restrict__ events, uint32_t row) { fill_syscall_instrs(r, events[row]); }
};
// `global_events` (may be null): [n][9] words, row i's send at row i
struct SyscallCore : ZeroPaddedChip<SYSCALL_CORE_WIDTH, Ev> {
    static TG_HD void live(Row<WIDTH>& r, const Ev* __restrict__ events, uint32_t row, int32_t* __restrict__ global_events) {
        const Ev e = events[row];
        fill_syscall_core(r, e);
        if (global_events) {
            int32_t ev[GLOBAL_EVENT_WORDS];
            syscall_core_global_event(ev, e);
            store_global_events<1>(global_events, row, ev);
        }
    }
};
struct StateBump : ZeroPaddedChip<STATE_BUMP_WIDTH, uint64_t> {
    static TG_HD void live(Row<WIDTH>& r, const uint64_t* __restrict__ records, uint32_t row) {
        uint64_t rec[STATE_BUMP_RECORD_WORDS];
        load_record<STATE_BUMP_RECORD_WORDS>(rec, records, row);
        fill_state_bump(r, rec);
    }
};
struct MemoryBump : ZeroPaddedChip<MEMORY_BUMP_WIDTH, uint64_t> {
    static TG_HD void live(Row<WIDTH>& r, const uint64_t* __restrict__ records, uint32_t row) {
        uint64_t rec[MEMORY_BUMP_RECORD_WORDS];
        load_record<MEMORY_BUMP_RECORD_WORDS>(rec, records, row);
        fill_memory_bump(r, rec);
    }
};

}  // namespace tg
}  // namespace sp1hip
