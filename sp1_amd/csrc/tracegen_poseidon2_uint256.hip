// sp1_amd/csrc/tracegen_poseidon2_uint256.hip — device trace generation for the chips of the POSEIDON2 and UINT256_MUL precompile
// shards: Poseidon2 (348 columns) and Uint256MulMod (371 columns), one row per system call, from the executor's event records
// (sp1hip_rv64_poseidon2_events: 26 u64, sp1hip_rv64_uint256_events: 31 u64) instead of host-made tables. With them every kind of
// shard the executor records is made on the device.
//
// The reference fills both tables on the host and has no device filler for them. The rows, their definitions in the reference and
// the column offsets are in tg_poseidon2_rows.hpp and tg_uint256_rows.hpp, host and device code alike (tests/native/p2u_rows.hip runs
// the same row functions on the CPU against the Python fillers).
//
// Lane mapping. One lane owns one ROW in both kernels, 256 rows per workgroup, so every store of a column goes to consecutive rows
// from consecutive lanes (256 B per wave instruction) and the table is written exactly once. A row is never held: each value goes
// to memory through the cursor as it is made. A Poseidon2 lane carries the sixteen state words through the permutation (perm_rows,
// the walk of the Global chip's lift kernel; the round constants are the device context's). A Uint256MulMod lane divides its
// 512-bit product by its own modulus in 512 shift-subtract steps (divide_512: 24 limbs, constant indices, a fixed trip count) and
// writes the 63-coefficient witness from the top down, as the curve chips do.
#include "device_ctx.hpp"
#include "tg_poseidon2_rows.hpp"
#include "tg_row_kernel.hpp"
#include "tg_uint256_rows.hpp"

namespace sp1hip {
namespace tgpu {

static_assert(tgp::EVENT_WORDS == SP1HIP_RV64_POSEIDON2_WORDS && tgu::EVENT_WORDS == SP1HIP_RV64_UINT256_WORDS, "event records");
static_assert(tgp::WIDTH == 348 && tgu::WIDTH == 371, "widths");

__global__ __launch_bounds__(256) void poseidon2_kernel(uint32_t* __restrict__ out, uint32_t height, const uint64_t* __restrict__ events, uint32_t n_events,
                                                        const p2::RoundConstants* __restrict__ rc) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    tgp::poseidon2_row(out, height, row, row < n_events ? events + (size_t)row * tgp::EVENT_WORDS : nullptr, rc);
}

__global__ __launch_bounds__(256) void uint256_mul_kernel(uint32_t* __restrict__ out, uint32_t height, const uint64_t* __restrict__ events, uint32_t n_events) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    tgu::uint256_mul_row(out, height, row, row < n_events ? events + (size_t)row * tgu::EVENT_WORDS : nullptr);
}

}  // namespace tgpu
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

int sp1hip_tracegen_riscv_poseidon2_width(void) { return tgp::WIDTH; }
int sp1hip_tracegen_riscv_uint256_mul_width(void) { return tgu::WIDTH; }

int sp1hip_tracegen_riscv_poseidon2(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    const p2::RoundConstants* rc = nullptr;
    if (height && n_events <= height && d_table && (d_events || n_events == 0)) {         // the context only for a call that launches
        const DeviceCtx* ctx;
        SP1HIP_TRY(get_device_ctx(&ctx));
        rc = ctx->d_rc;
    }
    return tg::launch_rows(__func__, tgpu::poseidon2_kernel, d_table, height, d_events, n_events, stream, rc);
}

int sp1hip_tracegen_riscv_uint256_mul(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    return tg::launch_rows(__func__, tgpu::uint256_mul_kernel, d_table, height, d_events, n_events, stream);
}

}  // extern "C"
