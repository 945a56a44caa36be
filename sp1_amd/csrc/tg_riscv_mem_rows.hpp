// sp1_amd/csrc/tg_riscv_mem_rows.hpp — the rows of the nine load and store chips of a core shard, whose tables
// tracegen_riscv_mem.hip makes on the device, for host and device code alike: the event record, the column groups the nine share
// (CPUState and the I adapter of tg_riscv_rows.hpp, included unchanged; AddressOperation; MemoryAccessCols) and fill_mem_row<CHIP>.
// tests/native/riscv_mem_rows.hip runs the same functions on the CPU, so every word can be compared with the host tracer
// (riscv_trace.Tracer.fill_mem_chip driven by riscv_exec.EventTracer.memory_instructions) without a GPU.
//
//   AddressOperation         crates/core/machine/src/operations/address.rs:L29-L75 (populate L38)
//   MemoryAccessCols         crates/core/machine/src/memory/consistency/columns.rs:L10-L37, trace.rs:L36-L47, L65-L99 (populate_timestamp)
//   LoadByte                 crates/core/machine/src/memory/instructions/load/load_byte.rs:L48-L80, L189 (event_to_row)
//   LoadHalf                 .../load/load_half.rs:L47, L181
//   LoadWord                 .../load/load_word.rs:L46, L180
//   LoadDouble               .../load/load_double.rs:L47, L170
//   LoadX0                   .../load/load_x0.rs:L44, L186
//   StoreByte                .../store/store_byte.rs:L47, L187-L223
//   StoreHalf                .../store/store_half.rs:L44, L172
//   StoreWord                .../store/store_word.rs:L44, L172
//   StoreDouble              .../store/store_double.rs:L45, L168
//
// The address, the word found there and the word left there travel in the event as the executor recorded them (E_MADDR, E_M_PREV,
// E_M_NEW of sp1_amd/machines/riscv_exec.py): nothing here re-derives what a load or a store does to memory. Column order = the
// reference's #[repr(C)] column structs (transcribed in sp1_amd/machines/riscv.py, whose layouts the tests compare the constants
// below with). Every index into Row::c is a constant, so on the device a row is registers.
#pragma once
#include "tg_riscv_rows.hpp"

namespace sp1hip {
namespace tg {

// sp1hip_rv64_mem_event_t (include/sp1hip.h)
struct MemEv { uint64_t pc, clk, ops, b, imm, a_prev, a_pts, b_pts, m_addr, m_pts, m_prev, m_new; };

constexpr uint32_t POS_M = 1;                                  // MemoryAccessPosition::Memory (core/executor/src/events/memory.rs:L63-L74)
enum : uint32_t { OP_LB = 29, OP_LH = 30, OP_LW = 31, OP_LBU = 32, OP_LHU = 33, OP_LWU = 34, OP_LD = 35 };   // opcode.rs, riscv.py OPC

enum MemChip : int { LOAD_BYTE = 0, LOAD_HALF = 1, LOAD_WORD = 2, LOAD_DOUBLE = 3, LOAD_X0 = 4, STORE_BYTE = 5, STORE_HALF = 6, STORE_WORD = 7,
                     STORE_DOUBLE = 8, N_MEM_CHIPS = 9 };
__host__ __device__ constexpr int mem_width_of(int chip) {
    return chip == LOAD_BYTE ? 47 : chip == LOAD_HALF || chip == LOAD_WORD || chip == STORE_WORD ? 44 : chip == LOAD_X0 ? 48 : chip == STORE_BYTE ? 50 :
           chip == STORE_HALF ? 45 : 39;
}

// The columns behind the I adapter (0..24): what `riscv_mem_rows host layout` prints and the tests compare with riscv.py
namespace col {
constexpr int MEM_ADDRESS = 25, MEM_ADDRESS_INV = 28;                                       // address.value[3], address.top_two_limb_inv
constexpr int MEM_PREV_VALUE = 29, MEM_PREV_HIGH = 33, MEM_PREV_LOW = 34, MEM_COMPARE_LOW = 35, MEM_DIFF_LOW = 36, MEM_DIFF_HIGH = 37;
constexpr int MEM_OWN = 38;                                                                 // offset_bit, or is_real of the Double chips
constexpr int LB_SELECTED_LIMB = 41, LB_SELECTED_LIMB_LOW_BYTE = 42, LB_SELECTED_BYTE = 43, LB_MSB = 44, LB_IS_LB = 45, LB_IS_LBU = 46;
constexpr int LH_SELECTED_HALF = 40, LH_MSB = 41, LH_IS_LH = 42, LH_IS_LHU = 43;
constexpr int LW_SELECTED_WORD = 39, LW_MSB = 41, LW_IS_LW = 42, LW_IS_LWU = 43;
constexpr int LX0_IS_LB = 41;                                                               // is_lb, is_lbu, is_lh, is_lhu, is_lw, is_lwu, is_ld
constexpr int SB_MEM_LIMB = 41, SB_MEM_LIMB_LOW_BYTE = 42, SB_REGISTER_LOW_BYTE = 43, SB_INCREMENT = 44, SB_STORE_VALUE = 45, SB_IS_REAL = 49;
constexpr int SH_STORE_VALUE = 40, SH_IS_REAL = 44;
constexpr int SW_STORE_VALUE = 39, SW_IS_REAL = 43;
}  // namespace col

// AddressOperation at 25..28: the address's three low limbs, and the field inverse of limb 1 + limb 2 (0 for 0): the AIR's proof
// that the address is not below 2^16
template <int W> TG_HD void fill_address(Row<W>& r, uint64_t addr) {
    r.limbs3(col::MEM_ADDRESS, addr);
    const uint32_t top = ((uint32_t)(addr >> 16) & M16) + ((uint32_t)(addr >> 32) & M16);
    r.c[col::MEM_ADDRESS_INV] = top ? kb::from_monty(kb::inv(kb::to_monty(top))) : 0u;
}
// MemoryAccessCols at 29..37: prev_value[4], then MemoryAccessTimestamp. Unlike a register access, a memory access compares the
// windows themselves when they differ, so there is no bump row and nothing is left to the host
template <int W> TG_HD void fill_mem_access(Row<W>& r, uint64_t prev_value, uint64_t t_prev, uint64_t t_cur) {
    r.limbs4(col::MEM_PREV_VALUE, prev_value);
    const uint32_t ph = (uint32_t)(t_prev >> 24), pl = (uint32_t)t_prev & 0xffffffu, ch = (uint32_t)(t_cur >> 24), cl = (uint32_t)t_cur & 0xffffffu;
    const bool same = ph == ch;
    const uint32_t d = (same ? cl - pl : ch - ph) - 1u;
    r.c[col::MEM_PREV_HIGH] = ph; r.c[col::MEM_PREV_LOW] = pl; r.c[col::MEM_COMPARE_LOW] = same;
    r.c[col::MEM_DIFF_LOW] = d & M16; r.c[col::MEM_DIFF_HIGH] = d >> 16;
}
// the 16-bit limb of `v` that holds the byte / half at `addr`, without a dynamic index
TG_HD uint32_t limb_at(uint64_t v, uint64_t addr) { return (uint32_t)(v >> (16 * ((uint32_t)(addr >> 1) & 3))) & M16; }

template <int CHIP> TG_HD void fill_mem_row(Row<mem_width_of(CHIP)>& r, const MemEv& m) {
    const uint32_t op = (uint32_t)m.ops & 0xff;
    const Ev e = {m.pc, m.clk, m.ops, 0, m.b, m.imm, m.a_prev, m.a_pts, m.b_pts, 0, 0};
    fill_state(r, e);                                         // state | ITypeReader | address | memory_access | the chip's own
    fill_i(r, e);
    fill_address(r, m.m_addr);
    fill_mem_access(r, m.m_prev, m.m_pts, m.clk + POS_M);
    const uint32_t b0 = (uint32_t)m.m_addr & 1, b1 = (uint32_t)(m.m_addr >> 1) & 1, b2 = (uint32_t)(m.m_addr >> 2) & 1;
    const uint32_t limb = limb_at(m.m_prev, m.m_addr);
    if constexpr (CHIP == LOAD_BYTE || CHIP == LOAD_X0 || CHIP == STORE_BYTE) { r.c[col::MEM_OWN] = b0; r.c[col::MEM_OWN + 1] = b1; r.c[col::MEM_OWN + 2] = b2; }
    else if constexpr (CHIP == LOAD_HALF || CHIP == STORE_HALF) { r.c[col::MEM_OWN] = b1; r.c[col::MEM_OWN + 1] = b2; }
    else if constexpr (CHIP == LOAD_WORD || CHIP == STORE_WORD) r.c[col::MEM_OWN] = b2;
    else r.c[col::MEM_OWN] = 1;                               // LoadDouble / StoreDouble: is_real
    if constexpr (CHIP == LOAD_BYTE) {                        // selected_limb | selected_limb_low_byte | selected_byte | msb | is_lb | is_lbu
        const uint32_t byte = (limb >> (8 * b0)) & 0xff;
        const bool lb = op == OP_LB;
        r.c[col::LB_SELECTED_LIMB] = limb; r.c[col::LB_SELECTED_LIMB_LOW_BYTE] = limb & 0xff; r.c[col::LB_SELECTED_BYTE] = byte;
        r.c[col::LB_MSB] = lb ? byte >> 7 : 0u;
        r.c[col::LB_IS_LB] = lb; r.c[col::LB_IS_LBU] = !lb;
    } else if constexpr (CHIP == LOAD_HALF) {                 // selected_half | msb | is_lh | is_lhu
        const bool lh = op == OP_LH;
        r.c[col::LH_SELECTED_HALF] = limb;
        r.c[col::LH_MSB] = lh ? limb >> 15 : 0u;
        r.c[col::LH_IS_LH] = lh; r.c[col::LH_IS_LHU] = !lh;
    } else if constexpr (CHIP == LOAD_WORD) {                 // selected_word[2] | msb | is_lw | is_lwu
        const bool lw = op == OP_LW;
        const uint32_t word = (uint32_t)(m.m_prev >> (32 * b2));
        r.c[col::LW_SELECTED_WORD] = word & M16; r.c[col::LW_SELECTED_WORD + 1] = word >> 16;
        r.c[col::LW_MSB] = lw ? word >> 31 : 0u;
        r.c[col::LW_IS_LW] = lw; r.c[col::LW_IS_LWU] = !lw;
    } else if constexpr (CHIP == LOAD_X0) {                   // is_lb .. is_ld: any load whose destination is x0
        r.c[col::LX0_IS_LB] = op == OP_LB; r.c[col::LX0_IS_LB + 1] = op == OP_LBU; r.c[col::LX0_IS_LB + 2] = op == OP_LH; r.c[col::LX0_IS_LB + 3] = op == OP_LHU;
        r.c[col::LX0_IS_LB + 4] = op == OP_LW; r.c[col::LX0_IS_LB + 5] = op == OP_LWU; r.c[col::LX0_IS_LB + 6] = op == OP_LD;
    } else if constexpr (CHIP == STORE_BYTE) {                // mem_limb | mem_limb_low_byte | register_low_byte | increment | store_value[4] | is_real
        const uint32_t rl = (uint32_t)m.a_prev & 0xff, ml = limb & 0xff, mh = limb >> 8;
        // what the store adds to the limb, as a field element: the register's byte minus the byte it replaces, in that byte's place
        const int32_t inc = b0 ? 256 * ((int32_t)rl - (int32_t)mh) : (int32_t)rl - (int32_t)ml;
        r.c[col::SB_MEM_LIMB] = limb; r.c[col::SB_MEM_LIMB_LOW_BYTE] = ml; r.c[col::SB_REGISTER_LOW_BYTE] = rl;
        r.c[col::SB_INCREMENT] = inc < 0 ? kb::P - (uint32_t)(-inc) : (uint32_t)inc;
        r.limbs4(col::SB_STORE_VALUE, m.m_new);
        r.c[col::SB_IS_REAL] = 1;
    } else if constexpr (CHIP == STORE_HALF) {                // store_value[4] | is_real
        r.limbs4(col::SH_STORE_VALUE, m.m_new);
        r.c[col::SH_IS_REAL] = 1;
    } else if constexpr (CHIP == STORE_WORD) {
        r.limbs4(col::SW_STORE_VALUE, m.m_new);
        r.c[col::SW_IS_REAL] = 1;
    }
    (void)limb; (void)b0; (void)b1; (void)op;
}

// A padding row (row >= n_events) of all nine chips is the zero row: each chip's generate_trace_into clears the rows behind its
// events with write_bytes(.., 0, ..) (load_byte.rs:L135-L141 and the same lines of the eight others), and the host tracer's
// tables start as zeros (riscv_trace.Table); the tests compare the padding rows word for word

// The chip of row_kernel / host_rows (tg_row_kernel.hpp) for each of the nine
template <int CHIP> struct LoadStoreChip : ZeroPaddedChip<mem_width_of(CHIP), MemEv> {
    static TG_HD void live(Row<mem_width_of(CHIP)>& r, const MemEv* __restrict__ events, uint32_t row) { fill_mem_row<CHIP>(r, events[row]); }
};

}  // namespace tg
}  // namespace sp1hip
