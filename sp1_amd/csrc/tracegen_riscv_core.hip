// sp1_amd/csrc/tracegen_riscv_core.hip — device trace generation for four more tables of a core shard: DivRem, AluX0 and
// MemoryLocal from event records, and with MemoryLocal the Global events its rows send, in the 9-word form
// sp1hip_tracegen_riscv_global reads — so that the Global table of an executed program is made on the device from records that
// never were a host table.
//
// The reference fills DivRem, AluX0 and MemoryLocal on the host (`generate_trace_into` / `event_to_row` of
// crates/core/machine/src/alu/divrem/mod.rs, alu/alu_x0.rs, memory/local.rs) and copies them to the device. Here one lane fills one
// row. DivRem and AluX0 read the 88-byte sp1hip_rv64_alu_event_t of tracegen_riscv.hip, MemoryLocal a 40-byte record of five words.
//
// The rows themselves are tg_riscv_core_rows.hpp, host and device code alike (tests/native/riscv_core_rows.hip runs them on the
// CPU); the kernel and its launch are tg_row_kernel.hpp. This file is DivRem's kernel and the ABI. Output: column-major
// [width][height] Montgomery words. A DivRem row is 246 words: it is made and stored in four column groups (divrem_row), so that a
// lane never holds more than one group (no scratch: DESIGN.md has the figures).
#include "device_ctx.hpp"
#include "tg_riscv_core_rows.hpp"

namespace sp1hip {
namespace tg {

static_assert(sizeof(Ev) == sizeof(sp1hip_rv64_alu_event_t), "event layout");

__global__ __launch_bounds__(256) void tracegen_divrem_kernel(uint32_t* __restrict__ out, uint32_t height, const Ev* __restrict__ events, uint32_t n) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row < height) divrem_row(out, height, events, n, row);
}

static const Ev* ev(const sp1hip_rv64_alu_event_t* d_events) { return reinterpret_cast<const Ev*>(d_events); }

}  // namespace tg
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

int sp1hip_tracegen_riscv_divrem_width(void) { return tg::DIVREM_WIDTH; }
int sp1hip_tracegen_riscv_alu_x0_width(void) { return tg::ALU_X0_WIDTH; }
int sp1hip_tracegen_riscv_memory_local_width(void) { return tg::MEMORY_LOCAL_WIDTH; }

int sp1hip_tracegen_riscv_divrem(uint32_t* d_table, uint32_t height, const sp1hip_rv64_alu_event_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    return tg::launch_rows(__func__, tg::tracegen_divrem_kernel, d_table, height, tg::ev(d_events), n_events, stream);
}

int sp1hip_tracegen_riscv_alu_x0(uint32_t* d_table, uint32_t height, const sp1hip_rv64_alu_event_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    return tg::launch_rows(__func__, tg::row_kernel<tg::AluX0>, d_table, height, tg::ev(d_events), n_events, stream);
}

int sp1hip_tracegen_riscv_memory_local(uint32_t* d_table, uint32_t height, const uint64_t* d_records, uint32_t n_records, int32_t* d_global_events,
                                       sp1hip_stream_t stream) {
    return tg::launch_rows(__func__, tg::row_kernel<tg::MemoryLocal, int32_t*>, d_table, height, d_records, n_records, stream, d_global_events);
}

}  // extern "C"
