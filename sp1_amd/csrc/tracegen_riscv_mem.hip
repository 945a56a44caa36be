// sp1_amd/csrc/tracegen_riscv_mem.hip — device trace generation for the nine load and store chips of a core shard: LoadByte,
// LoadHalf, LoadWord, LoadDouble, LoadX0, StoreByte, StoreHalf, StoreWord, StoreDouble, from 96-byte event records instead of
// host-made tables. In the reference's recorded core shard these hold 2.57 M rows, about as many cells as the fourteen chips of
// tracegen_riscv.hip together.
//
// The reference fills these tables on the host (`generate_trace_into` / `event_to_row` of
// crates/core/machine/src/memory/instructions/{load,store}/*.rs) and copies them to the device. Here one lane fills one row: an
// event is 96 bytes, a row 156-200, and a row is a few dozen integer operations and one field inversion, so the kernels run at the
// rate the table can be written.
//
// The rows themselves are tg_riscv_mem_rows.hpp, host and device code alike (tests/native/riscv_mem_rows.hip runs them on the
// CPU); the kernel and its launch are tg_row_kernel.hpp. This file is the launch switch and the ABI. Output: column-major
// [width][height] Montgomery words, rows >= n_events are zero rows.
#include "device_ctx.hpp"
#include "tg_riscv_mem_rows.hpp"

using namespace sp1hip;
static_assert(sizeof(tg::MemEv) == sizeof(sp1hip_rv64_mem_event_t), "event layout");

extern "C" {

int sp1hip_tracegen_riscv_mem_width(int chip) { return chip >= 0 && chip < tg::N_MEM_CHIPS ? tg::mem_width_of(chip) : -1; }

int sp1hip_tracegen_riscv_mem(int chip, uint32_t* d_table, uint32_t height, const sp1hip_rv64_mem_event_t* d_events, uint32_t n_events,
                              sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(chip >= 0 && chip < tg::N_MEM_CHIPS, "unknown chip");
    const tg::MemEv* ev = reinterpret_cast<const tg::MemEv*>(d_events);
    switch (chip) {
#define SP1HIP_TG(C) case tg::C: return tg::launch_rows(__func__, tg::row_kernel<tg::LoadStoreChip<tg::C>>, d_table, height, ev, n_events, stream)
        SP1HIP_TG(LOAD_BYTE); SP1HIP_TG(LOAD_HALF); SP1HIP_TG(LOAD_WORD); SP1HIP_TG(LOAD_DOUBLE); SP1HIP_TG(LOAD_X0);
        SP1HIP_TG(STORE_BYTE); SP1HIP_TG(STORE_HALF); SP1HIP_TG(STORE_WORD); SP1HIP_TG(STORE_DOUBLE);
#undef SP1HIP_TG
    }
    return SP1HIP_ERROR_INVALID_ARGUMENT;                    // not reached: every chip of the range has its case
}

}  // extern "C"
