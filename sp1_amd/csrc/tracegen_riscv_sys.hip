// sp1_amd/csrc/tracegen_riscv_sys.hip — device trace generation for the four small chips of a core shard: SyscallInstrs, SyscallCore
// (with the Global events its rows send, in the 9-word form sp1hip_tracegen_riscv_global reads), StateBump and MemoryBump. They are
// a handful of rows per shard; they are made here so that a core shard needs no host table at all: their records are the bins 25..28
// of sp1hip_rv64_partition_scatter, already in device memory.
//
// The reference fills the four on the host (`generate_trace_into` of crates/core/machine/src/syscall/{instructions/trace,chip}.rs,
// adapter/bump.rs, memory/bump.rs). Here one lane fills one row. The rows themselves are tg_riscv_sys_rows.hpp, host and device code
// alike (tests/native/riscv_sys_rows.hip runs them on the CPU). This file is the kernels and the ABI. Output: column-major
// [width][height] Montgomery words, zero padding rows.
#include "device_ctx.hpp"
#include "tg_riscv_sys_rows.hpp"

namespace sp1hip {
namespace tg {

static_assert(sizeof(Ev) == sizeof(sp1hip_rv64_alu_event_t), "event layout");

template <int W> __device__ __forceinline__ void store_row(uint32_t* __restrict__ out, uint32_t height, uint32_t row, const Row<W>& r) {
#pragma unroll
    for (int c = 0; c < W; c++) gptr(out)[(size_t)c * height + row] = r.c[c] ? kb::to_monty(r.c[c]) : 0u;
}

__global__ __launch_bounds__(256) void tracegen_syscall_instrs_kernel(uint32_t* __restrict__ out, uint32_t height, const Ev* __restrict__ events, uint32_t n) {
    constexpr int W = SYSCALL_INSTRS_WIDTH;
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    Row<W> r;
#pragma unroll
    for (int c = 0; c < W; c++) r.c[c] = 0;
    if (row < n) fill_syscall_instrs(r, events[row]);
    store_row(out, height, row, r);
}

// `global_events` (may be null): [n][9] words, row i's send at row i
__global__ __launch_bounds__(256) void tracegen_syscall_core_kernel(uint32_t* __restrict__ out, uint32_t height, const Ev* __restrict__ events, uint32_t n,
                                                                    int32_t* __restrict__ global_events) {
    constexpr int W = SYSCALL_CORE_WIDTH;
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    Row<W> r;
#pragma unroll
    for (int c = 0; c < W; c++) r.c[c] = 0;
    if (row < n) {
        const Ev e = events[row];
        fill_syscall_core(r, e);
        if (global_events) {
            int32_t ev[GLOBAL_EVENT_WORDS];
            syscall_core_global_event(ev, e);
#pragma unroll
            for (int i = 0; i < GLOBAL_EVENT_WORDS; i++) gptr(global_events)[(size_t)row * GLOBAL_EVENT_WORDS + i] = ev[i];
        }
    }
    store_row(out, height, row, r);
}

// StateBump (BUMP = 0) and MemoryBump (BUMP = 1): four-word records
template <int BUMP> __global__ __launch_bounds__(256) void tracegen_bump_kernel(uint32_t* __restrict__ out, uint32_t height,
                                                                                const uint64_t* __restrict__ records, uint32_t n) {
    constexpr int W = BUMP ? MEMORY_BUMP_WIDTH : STATE_BUMP_WIDTH;
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    Row<W> r;
#pragma unroll
    for (int c = 0; c < W; c++) r.c[c] = 0;
    if (row < n) {
        uint64_t rec[4];
#pragma unroll
        for (int i = 0; i < 4; i++) rec[i] = gptr(records)[(size_t)row * 4 + i];
        if constexpr (BUMP) fill_memory_bump(r, rec); else fill_state_bump(r, rec);
    }
    store_row(out, height, row, r);
}

}  // namespace tg
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

int sp1hip_tracegen_riscv_syscall_instrs_width(void) { return tg::SYSCALL_INSTRS_WIDTH; }
int sp1hip_tracegen_riscv_syscall_core_width(void) { return tg::SYSCALL_CORE_WIDTH; }
int sp1hip_tracegen_riscv_state_bump_width(void) { return tg::STATE_BUMP_WIDTH; }
int sp1hip_tracegen_riscv_memory_bump_width(void) { return tg::MEMORY_BUMP_WIDTH; }

int sp1hip_tracegen_riscv_syscall_instrs(uint32_t* d_table, uint32_t height, const sp1hip_rv64_alu_event_t* d_events, uint32_t n_events,
                                         sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(n_events <= height && (d_table || height == 0) && (d_events || n_events == 0), "bad argument");
    if (height == 0) return SP1HIP_SUCCESS;
    hipLaunchKernelGGL(tg::tracegen_syscall_instrs_kernel, dim3((height + 255) / 256), dim3(256), 0, S(stream), d_table, height,
                       reinterpret_cast<const tg::Ev*>(d_events), n_events);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}

int sp1hip_tracegen_riscv_syscall_core(uint32_t* d_table, uint32_t height, const sp1hip_rv64_alu_event_t* d_events, uint32_t n_events,
                                       int32_t* d_global_events, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(n_events <= height && (d_table || height == 0) && (d_events || n_events == 0), "bad argument");
    if (height == 0) return SP1HIP_SUCCESS;
    hipLaunchKernelGGL(tg::tracegen_syscall_core_kernel, dim3((height + 255) / 256), dim3(256), 0, S(stream), d_table, height,
                       reinterpret_cast<const tg::Ev*>(d_events), n_events, d_global_events);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}

int sp1hip_tracegen_riscv_state_bump(uint32_t* d_table, uint32_t height, const uint64_t* d_records, uint32_t n_records, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(n_records <= height && (d_table || height == 0) && (d_records || n_records == 0), "bad argument");
    if (height == 0) return SP1HIP_SUCCESS;
    hipLaunchKernelGGL(tg::tracegen_bump_kernel<0>, dim3((height + 255) / 256), dim3(256), 0, S(stream), d_table, height, d_records, n_records);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}

int sp1hip_tracegen_riscv_memory_bump(uint32_t* d_table, uint32_t height, const uint64_t* d_records, uint32_t n_records, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(n_records <= height && (d_table || height == 0) && (d_records || n_records == 0), "bad argument");
    if (height == 0) return SP1HIP_SUCCESS;
    hipLaunchKernelGGL(tg::tracegen_bump_kernel<1>, dim3((height + 255) / 256), dim3(256), 0, S(stream), d_table, height, d_records, n_records);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}

}  // extern "C"
