// sp1_amd/csrc/tracegen_riscv_sys.hip — device trace generation for the four small chips of a core shard: SyscallInstrs, SyscallCore
// (with the Global events its rows send, in the 9-word form sp1hip_tracegen_riscv_global reads), StateBump and MemoryBump. They are
// a handful of rows per shard; they are made here so that a core shard needs no host table at all: their records are the bins 25..28
// of sp1hip_rv64_partition_scatter, already in device memory.
//
// The reference fills the four on the host (`generate_trace_into` of crates/core/machine/src/syscall/{instructions/trace,chip}.rs,
// adapter/bump.rs, memory/bump.rs). Here one lane fills one row. The rows themselves are tg_riscv_sys_rows.hpp, host and device code
// alike (tests/native/riscv_sys_rows.hip runs them on the CPU); the kernel and its launch are tg_row_kernel.hpp. This file is the
// ABI. Output: column-major [width][height] Montgomery words, zero padding rows.
#include "device_ctx.hpp"
#include "tg_riscv_sys_rows.hpp"

using namespace sp1hip;
static_assert(sizeof(tg::Ev) == sizeof(sp1hip_rv64_alu_event_t), "event layout");

static const tg::Ev* ev(const sp1hip_rv64_alu_event_t* d_events) { return reinterpret_cast<const tg::Ev*>(d_events); }

extern "C" {

int sp1hip_tracegen_riscv_syscall_instrs_width(void) { return tg::SYSCALL_INSTRS_WIDTH; }
int sp1hip_tracegen_riscv_syscall_core_width(void) { return tg::SYSCALL_CORE_WIDTH; }
int sp1hip_tracegen_riscv_state_bump_width(void) { return tg::STATE_BUMP_WIDTH; }
int sp1hip_tracegen_riscv_memory_bump_width(void) { return tg::MEMORY_BUMP_WIDTH; }

int sp1hip_tracegen_riscv_syscall_instrs(uint32_t* d_table, uint32_t height, const sp1hip_rv64_alu_event_t* d_events, uint32_t n_events,
                                         sp1hip_stream_t stream) {
    return tg::launch_rows(__func__, tg::row_kernel<tg::SyscallInstrs>, d_table, height, ev(d_events), n_events, stream);
}

int sp1hip_tracegen_riscv_syscall_core(uint32_t* d_table, uint32_t height, const sp1hip_rv64_alu_event_t* d_events, uint32_t n_events,
                                       int32_t* d_global_events, sp1hip_stream_t stream) {
    return tg::launch_rows(__func__, tg::row_kernel<tg::SyscallCore, int32_t*>, d_table, height, ev(d_events), n_events, stream, d_global_events);
}

int sp1hip_tracegen_riscv_state_bump(uint32_t* d_table, uint32_t height, const uint64_t* d_records, uint32_t n_records, sp1hip_stream_t stream) {
    return tg::launch_rows(__func__, tg::row_kernel<tg::StateBump>, d_table, height, d_records, n_records, stream);
}

int sp1hip_tracegen_riscv_memory_bump(uint32_t* d_table, uint32_t height, const uint64_t* d_records, uint32_t n_records, sp1hip_stream_t stream) {
    return tg::launch_rows(__func__, tg::row_kernel<tg::MemoryBump>, d_table, height, d_records, n_records, stream);
}

}  // extern "C"
