// sp1_amd/csrc/tracegen_sha256.hip — device trace generation for the four chips of the SHA_EXTEND and SHA_COMPRESS precompile shards:
// ShaExtend (128 columns, 48 rows per call), ShaExtendControl (18, one row per call), ShaCompress (206, 80 rows per call) and
// ShaCompressControl (53, one row per call), from the executor's event records (sp1hip_rv64_sha_extend_events: 786 u64,
// sp1hip_rv64_sha_compress_events: 155 u64) instead of host-made tables. A SHA_EXTEND call's rows are 24.6 KB of table for a 6.3 KB
// event, a SHA_COMPRESS call's 65.9 KB for 1.2 KB.
//
// The reference fills the four tables on the host and has no device filler for them. The rows, their definitions in the reference
// and the column offsets are in tg_sha256_rows.hpp, host and device code alike (tests/native/sha_rows.hip runs the same row
// functions on the CPU against the Python fillers).
//
// Lane mapping. One lane owns one ROW in all four kernels, 256 rows per workgroup, so every store of a column goes to consecutive
// rows from consecutive lanes (256 B per wave instruction) and the table is written exactly once. A row is never held: each value
// goes to memory through the cursor as it is made. ShaExtend's row 48 e + r reads the 11 record words of step r of event e and
// nothing else. ShaCompress's row 80 e + j needs the working state entering its round: the lane loads the event's eight h words
// and runs rounds 0 .. j - 9 on them in eight registers (at most 64 rounds of ~30 32-bit operations against 206 stores per row; w[t]
// and K[t] are loads at an address that depends on the round, not indices into a lane's array: no scratch), so no lane reads a row
// another lane wrote. ShaCompress's padding rows are not zero: octet, octet_num, index and k cycle by row mod 80 on every row.
#include "device_ctx.hpp"
#include "tg_row_kernel.hpp"
#include "tg_sha256_rows.hpp"

namespace sp1hip {
namespace tgs {

static_assert(EXTEND_EVENT_WORDS == SP1HIP_RV64_SHA_EXTEND_WORDS && COMPRESS_EVENT_WORDS == SP1HIP_RV64_SHA_COMPRESS_WORDS, "event records");

#define SP1HIP_SHA_ROW_KERNEL(name, row_function)                                                                                              \
    __global__ __launch_bounds__(256) void name(uint32_t* __restrict__ out, uint32_t height, const uint64_t* __restrict__ events, uint32_t n_events) { \
        const uint32_t row = blockIdx.x * 256u + threadIdx.x;                                                                                  \
        if (row >= height) return;                                                                                                             \
        row_function(out, height, row, events, n_events);                                                                                      \
    }
SP1HIP_SHA_ROW_KERNEL(sha_extend_kernel, sha_extend_row)
SP1HIP_SHA_ROW_KERNEL(sha_extend_control_kernel, sha_extend_control_row)
SP1HIP_SHA_ROW_KERNEL(sha_compress_kernel, sha_compress_row)
SP1HIP_SHA_ROW_KERNEL(sha_compress_control_kernel, sha_compress_control_row)
#undef SP1HIP_SHA_ROW_KERNEL

}  // namespace tgs
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

int sp1hip_tracegen_riscv_sha_extend_width(void) { return tgs::ext::WIDTH; }
int sp1hip_tracegen_riscv_sha_extend_control_width(void) { return tgs::ext::CONTROL_WIDTH; }
int sp1hip_tracegen_riscv_sha_compress_width(void) { return tgs::cmp::WIDTH; }
int sp1hip_tracegen_riscv_sha_compress_control_width(void) { return tgs::cmp::CONTROL_WIDTH; }

int sp1hip_tracegen_riscv_sha_extend(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE((uint64_t)n_events * tgs::EXTEND_ROWS <= height, "the events' rows (48 each) exceed the height");
    return tg::launch_rows(__func__, tgs::sha_extend_kernel, d_table, height, d_events, n_events, stream);
}

int sp1hip_tracegen_riscv_sha_extend_control(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    return tg::launch_rows(__func__, tgs::sha_extend_control_kernel, d_table, height, d_events, n_events, stream);
}

int sp1hip_tracegen_riscv_sha_compress(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE((uint64_t)n_events * tgs::COMPRESS_ROWS <= height, "the events' rows (80 each) exceed the height");
    return tg::launch_rows(__func__, tgs::sha_compress_kernel, d_table, height, d_events, n_events, stream);
}

int sp1hip_tracegen_riscv_sha_compress_control(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    return tg::launch_rows(__func__, tgs::sha_compress_control_kernel, d_table, height, d_events, n_events, stream);
}

}  // extern "C"
