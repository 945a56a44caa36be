// sp1_amd/csrc/tracegen_riscv.hip — device trace generation for the RISC-V instruction chips that make up a core shard
// (VERDICT r5 #6): Add, Addi, Sub, Addw, Subw, Mul, ShiftRight, Branch — 99.6 % of the rows of a shard
// of the reference's fibonacci guest — and Bitwise, Lt, ShiftLeft, UType, Jal, Jalr, another million rows of a shard of a real
// program (rsp), from compact EVENT records instead of host-made tables.
//
// The reference fills these tables on the host, row by row, from its executor's events and copies them to the device
// (`generate_trace_into` / `event_to_row` of each chip, then sp1-gpu's `device_main_tracegen`,
// /root/reference/sp1-gpu/crates/jagged_tracegen/src/lib.rs:L819-L835); its device tracegen covers the recursion chips and
// the Global chip. Here one lane fills one row: an event is 88 bytes, a row 120-328, and the fields are a few dozen integer
// operations each, so the kernels run at the rate the table can be written.
//
// The rows themselves — the event record, the column groups, fill_row<CHIP> with the reference's files and lines at each chip —
// are tg_riscv_rows.hpp, host and device code alike (tests/native/riscv_rows.hip runs them on the CPU); the kernel and its launch
// are tg_row_kernel.hpp. This file is the launch switch and the ABI. Output: column-major [width][height] Montgomery words, rows
// >= n_events are the chip's padding rows.
#include "device_ctx.hpp"
#include "tg_riscv_rows.hpp"

using namespace sp1hip;
static_assert(sizeof(tg::Ev) == sizeof(sp1hip_rv64_alu_event_t), "event layout");

extern "C" {

int sp1hip_tracegen_riscv_alu_width(int chip) { return chip >= 0 && chip < tg::N_CHIPS ? tg::width_of(chip) : -1; }

int sp1hip_tracegen_riscv_alu(int chip, uint32_t* d_table, uint32_t height, const sp1hip_rv64_alu_event_t* d_events, uint32_t n_events,
                              sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(chip >= 0 && chip < tg::N_CHIPS, "unknown chip");
    const tg::Ev* ev = reinterpret_cast<const tg::Ev*>(d_events);
    switch (chip) {
#define SP1HIP_TG(C) case tg::C: return tg::launch_rows(__func__, tg::row_kernel<tg::AluChip<tg::C>>, d_table, height, ev, n_events, stream)
        SP1HIP_TG(ADD); SP1HIP_TG(ADDI); SP1HIP_TG(SUB); SP1HIP_TG(ADDW); SP1HIP_TG(SUBW); SP1HIP_TG(MUL); SP1HIP_TG(SHIFT_RIGHT); SP1HIP_TG(BRANCH);
        SP1HIP_TG(BITWISE); SP1HIP_TG(LT); SP1HIP_TG(SHIFT_LEFT); SP1HIP_TG(UTYPE); SP1HIP_TG(JAL); SP1HIP_TG(JALR);
#undef SP1HIP_TG
    }
    return SP1HIP_ERROR_INVALID_ARGUMENT;                    // not reached: every chip of the range has its case
}

}  // extern "C"
