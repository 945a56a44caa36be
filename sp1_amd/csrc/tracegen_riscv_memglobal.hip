// sp1_amd/csrc/tracegen_riscv_memglobal.hip — device trace generation for the chips that close the shards without instructions:
// MemoryGlobalInit / MemoryGlobalFinalize of a memory shard, SyscallPrecompile of a precompile shard, the Global events their rows
// stand for in the 9-word form sp1hip_tracegen_riscv_global reads, and the MemoryLocal records of the words a precompile's calls
// touched — so that a memory shard and a precompile shard are made on the device from the executor's records, as a core shard is.
//
// The reference fills these tables on the host (`generate_trace_into` of crates/core/machine/src/memory/global.rs and
// syscall/chip.rs; memory/local.rs for the records' rows) and copies them to the device. Here one lane fills one row. The rows
// themselves are tg_riscv_memglobal_rows.hpp, host and device code alike (tests/native/riscv_memglobal_rows.hip runs them on the
// CPU); the kernel and its launch are tg_row_kernel.hpp. This file is the kernel of the MemoryLocal records and the ABI. Output:
// column-major [width][height] Montgomery words, every column stored once, 64 consecutive words per wave.
#include "device_ctx.hpp"
#include "tg_riscv_memglobal_rows.hpp"

namespace sp1hip {
namespace tg {

// One lane per MemoryLocal record: [n_records][5] words
__global__ __launch_bounds__(256) void precompile_local_records_kernel(uint64_t* __restrict__ records, uint32_t n_records, const uint64_t* __restrict__ events,
                                                                       uint32_t n_events, uint32_t words_per_event, LocalSegments segs) {
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n_records) return;
    LocalSegment seg;
    uint32_t event, word;
    if (!precompile_local_locate(segs, n_events, q, seg, event, word)) return;
    uint64_t rec[MEMORY_LOCAL_RECORD_WORDS];
    precompile_local_record(rec, events + (size_t)event * words_per_event, seg, word);
#pragma unroll
    for (int i = 0; i < MEMORY_LOCAL_RECORD_WORDS; i++) records[(size_t)q * MEMORY_LOCAL_RECORD_WORDS + i] = rec[i];
}

}  // namespace tg
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

int sp1hip_tracegen_riscv_memory_global_width(void) { return tg::MEMORY_GLOBAL_WIDTH; }
int sp1hip_tracegen_riscv_syscall_precompile_width(void) { return tg::SYSCALL_PRECOMPILE_WIDTH; }

int sp1hip_tracegen_riscv_memory_global(int finalize, uint32_t* d_table, uint32_t height, const uint64_t* d_records, uint32_t n_records,
                                        uint64_t previous_addr, int32_t* d_global_events, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(finalize == 0 || finalize == 1, "bad argument: finalize is 0 or 1");
    return tg::launch_rows(__func__, tg::row_kernel<tg::MemoryGlobal, uint64_t, int, int32_t*>, d_table, height, d_records, n_records, stream, previous_addr,
                           finalize, d_global_events);
}

int sp1hip_tracegen_riscv_syscall_precompile(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, uint32_t words_per_event,
                                             uint32_t syscall_id, int32_t arg2_word, int32_t* d_global_events, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(words_per_event >= 2 && words_per_event <= 65536 && syscall_id < 256 && arg2_word >= -1 && arg2_word < (int32_t)words_per_event,
                   "bad event shape: need 2 <= words_per_event <= 65536, syscall_id < 256, -1 <= arg2_word < words_per_event");
    return tg::launch_rows(__func__, tg::row_kernel<tg::SyscallPrecompile, uint32_t, uint32_t, int, int32_t*>, d_table, height, d_events, n_events, stream,
                           words_per_event, syscall_id, arg2_word, d_global_events);
}

int sp1hip_tracegen_riscv_syscall_precompile_coded(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, uint32_t words_per_event,
                                                   uint32_t code_word, int32_t arg2_word, int32_t* d_global_events, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(words_per_event >= 2 && words_per_event <= 65536 && code_word < words_per_event && arg2_word >= -1 && arg2_word < (int32_t)words_per_event,
                   "bad event shape: need 2 <= words_per_event <= 65536, code_word < words_per_event, -1 <= arg2_word < words_per_event");
    return tg::launch_rows(__func__, tg::row_kernel<tg::SyscallPrecompileCoded, uint32_t, uint32_t, int, int32_t*>, d_table, height, d_events, n_events, stream,
                           words_per_event, code_word, arg2_word, d_global_events);
}

int sp1hip_precompile_local_records(uint64_t* d_records, uint64_t records_capacity, const uint64_t* d_events, uint32_t n_events, uint32_t words_per_event,
                                    const uint32_t* segments, uint32_t n_segments, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(segments && n_segments >= 1 && n_segments <= (uint32_t)tg::PRECOMPILE_MAX_SEGMENTS, "need 1 to 4 segments");
    SP1HIP_REQUIRE(words_per_event >= 2 && words_per_event <= 65536, "bad event shape: need 2 <= words_per_event <= 65536");
    tg::LocalSegments segs = {};
    segs.n = n_segments;
    uint64_t total = 0;
    for (uint32_t k = 0; k < n_segments; k++) {
        const uint32_t* w = segments + 5 * k;
        const tg::LocalSegment s = {w[0], w[1], w[2], w[3], w[4]};
        SP1HIP_REQUIRE(s.count >= 1 && s.count <= words_per_event && s.ptr_word < words_per_event && s.pairs_word <= words_per_event &&
                       (uint64_t)s.pairs_word + (s.final_word == tg::PRECOMPILE_QUAD_WORDS ? 4ull : 2ull) * s.count <= words_per_event &&
                       (s.final_word == tg::PRECOMPILE_NO_WORD || s.final_word == tg::PRECOMPILE_QUAD_WORDS ||
                        (uint64_t)s.final_word + s.count <= words_per_event),
                       "a segment reads behind the event record");
        segs.s[k] = s;
        total += (uint64_t)n_events * s.count;
    }
    SP1HIP_REQUIRE(total <= 0x7fffffffull, "too many records");
    SP1HIP_REQUIRE(total <= records_capacity && (d_records || total == 0) && (d_events || n_events == 0), "bad argument");
    if (total == 0) return SP1HIP_SUCCESS;
    hipLaunchKernelGGL(tg::precompile_local_records_kernel, dim3((uint32_t)((total + 255) / 256)), dim3(256), 0, S(stream), d_records, (uint32_t)total,
                       d_events, n_events, words_per_event, segs);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}

}  // extern "C"
