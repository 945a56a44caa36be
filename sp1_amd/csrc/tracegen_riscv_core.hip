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
// CPU). This file is the kernels and the ABI. Output: column-major [width][height] Montgomery words. A DivRem row is 246 words: it is
// made and stored in four column groups, so that a lane never holds more than one group (no scratch: DESIGN.md has the figures).
#include "device_ctx.hpp"
#include "tg_riscv_core_rows.hpp"

namespace sp1hip {
namespace tg {

static_assert(sizeof(Ev) == sizeof(sp1hip_rv64_alu_event_t), "event layout");

template <int PART>
__device__ __forceinline__ void divrem_store_part(uint32_t* __restrict__ out, uint32_t height, uint32_t row, bool live, const Ev& e, const DivRemVals& d) {
    constexpr int LO = divrem_part_at(PART), HI = divrem_part_at(PART + 1);
    Row<DIVREM_WIDTH> r;
#pragma unroll
    for (int c = LO; c < HI; c++) r.c[c] = 0;
    if (live) fill_divrem<PART>(r, e, d); else fill_divrem_padding<PART>(r);
#pragma unroll
    for (int c = LO; c < HI; c++) gptr(out)[(size_t)c * height + row] = r.c[c] ? kb::to_monty(r.c[c]) : 0u;
}

__global__ __launch_bounds__(256) void tracegen_divrem_kernel(uint32_t* __restrict__ out, uint32_t height, const Ev* __restrict__ events, uint32_t n) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    const bool live = row < n;
    Ev e = {};
    if (live) e = events[row];
    const DivRemVals d = divrem_values(e);
    divrem_store_part<0>(out, height, row, live, e, d);
    divrem_store_part<1>(out, height, row, live, e, d);
    divrem_store_part<2>(out, height, row, live, e, d);
    divrem_store_part<3>(out, height, row, live, e, d);
}

__global__ __launch_bounds__(256) void tracegen_alu_x0_kernel(uint32_t* __restrict__ out, uint32_t height, const Ev* __restrict__ events, uint32_t n) {
    constexpr int W = ALU_X0_WIDTH;
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    Row<W> r;
#pragma unroll
    for (int c = 0; c < W; c++) r.c[c] = 0;
    if (row < n) fill_alu_x0(r, events[row]);
#pragma unroll
    for (int c = 0; c < W; c++) gptr(out)[(size_t)c * height + row] = r.c[c] ? kb::to_monty(r.c[c]) : 0u;
}

// `global_events` (may be null): [2 n][9] words, record i's receive at row 2 i and its send at row 2 i + 1
__global__ __launch_bounds__(256) void tracegen_memory_local_kernel(uint32_t* __restrict__ out, uint32_t height, const uint64_t* __restrict__ records,
                                                                    uint32_t n, int32_t* __restrict__ global_events) {
    constexpr int W = MEMORY_LOCAL_WIDTH;
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    Row<W> r;
#pragma unroll
    for (int c = 0; c < W; c++) r.c[c] = 0;
    if (row < n) {
        uint64_t rec[MEMORY_LOCAL_RECORD_WORDS];
#pragma unroll
        for (int i = 0; i < MEMORY_LOCAL_RECORD_WORDS; i++) rec[i] = records[(size_t)row * MEMORY_LOCAL_RECORD_WORDS + i];
        fill_memory_local(r, rec);
        if (global_events) {
            int32_t ev[2 * GLOBAL_EVENT_WORDS];
            memory_local_global_events(ev, rec);
#pragma unroll
            for (int i = 0; i < 2 * GLOBAL_EVENT_WORDS; i++) global_events[(size_t)row * (2 * GLOBAL_EVENT_WORDS) + i] = ev[i];
        }
    }
#pragma unroll
    for (int c = 0; c < W; c++) gptr(out)[(size_t)c * height + row] = r.c[c] ? kb::to_monty(r.c[c]) : 0u;
}

}  // namespace tg
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

int sp1hip_tracegen_riscv_divrem_width(void) { return tg::DIVREM_WIDTH; }
int sp1hip_tracegen_riscv_alu_x0_width(void) { return tg::ALU_X0_WIDTH; }
int sp1hip_tracegen_riscv_memory_local_width(void) { return tg::MEMORY_LOCAL_WIDTH; }

int sp1hip_tracegen_riscv_divrem(uint32_t* d_table, uint32_t height, const sp1hip_rv64_alu_event_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(n_events <= height && (d_table || height == 0) && (d_events || n_events == 0), "bad argument");
    if (height == 0) return SP1HIP_SUCCESS;
    hipLaunchKernelGGL(tg::tracegen_divrem_kernel, dim3((height + 255) / 256), dim3(256), 0, S(stream), d_table, height,
                       reinterpret_cast<const tg::Ev*>(d_events), n_events);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}

int sp1hip_tracegen_riscv_alu_x0(uint32_t* d_table, uint32_t height, const sp1hip_rv64_alu_event_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(n_events <= height && (d_table || height == 0) && (d_events || n_events == 0), "bad argument");
    if (height == 0) return SP1HIP_SUCCESS;
    hipLaunchKernelGGL(tg::tracegen_alu_x0_kernel, dim3((height + 255) / 256), dim3(256), 0, S(stream), d_table, height,
                       reinterpret_cast<const tg::Ev*>(d_events), n_events);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}

int sp1hip_tracegen_riscv_memory_local(uint32_t* d_table, uint32_t height, const uint64_t* d_records, uint32_t n_records, int32_t* d_global_events,
                                       sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(n_records <= height && (d_table || height == 0) && (d_records || n_records == 0), "bad argument");
    if (height == 0) return SP1HIP_SUCCESS;
    hipLaunchKernelGGL(tg::tracegen_memory_local_kernel, dim3((height + 255) / 256), dim3(256), 0, S(stream), d_table, height, d_records, n_records,
                       d_global_events);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}

}  // extern "C"
