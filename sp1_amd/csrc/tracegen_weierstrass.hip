// sp1_amd/csrc/tracegen_weierstrass.hip — device trace generation for the secp256k1 point-addition and point-doubling precompile
// chips: Secp256k1AddAssign (1,599 columns) and Secp256k1DoubleAssign (1,591 columns), one row per system call, from the
// executor's event records (sp1hip_rv64_secp256k1_add_events: 43 u64, _double_events: 26 u64) instead of host-made tables. A row
// is ten / eleven FieldOpCols — a 32 x 32 byte convolution and a division by (x - 256) each — and one modular inversion: pure
// integer arithmetic on a 344- / 208-byte event, 6.4 KB of table.
//
// The reference fills both tables on the host and has no device filler for them. The row's pieces, their definitions in the
// reference and the column offsets are in tg_field_op.hpp, the 256-bit arithmetic in fp256.hpp; both compile for the host too
// (tests/native/secp_rows.hip runs the same row functions on the CPU against the Python filler).
//
// Lane mapping. One lane owns one ROW, so every store of a column goes to consecutive rows from consecutive lanes (256 B per
// wave instruction) and the table is written exactly once. A 1,599-word row is never held: each FieldOpCols goes to memory as it
// is made, witness from the top coefficient down. Limbs, bytes and coefficients are indexed by constants only (no scratch for
// them). The modulus is a kernel argument — its limbs, -p^-1 mod 2^32, R^2 mod p, p^-1 mod 2^256 — read with constant indices, so
// it sits in scalar registers; nothing in the kernels knows secp256k1's form. A padding row (row >= n_events) is the reference's
// dummy row, computed by the same code from p = (0, 0), q = (1, 1) (doubling: p = (0, 1)).
#include "device_ctx.hpp"
#include "tg_field_op.hpp"
#include "tg_row_kernel.hpp"

namespace sp1hip {
namespace tgw {

constexpr int N = 8;                                               // 32-bit limbs of a secp256k1 field element
using Add = tgf::WeierstrassAdd<N>;
using Double = tgf::WeierstrassDouble<N>;
constexpr uint32_t WITNESS_OFFSET = 1u << 14;                      // curves/src/weierstrass/secp256k1.rs: WITNESS_OFFSET
static_assert(Add::EVENT_WORDS == SP1HIP_RV64_SECP_ADD_WORDS && Double::EVENT_WORDS == SP1HIP_RV64_SECP_DOUBLE_WORDS, "event records");

// p = 2^256 - 2^32 - 977 (curves/src/weierstrass/secp256k1.rs:L29-L45), a = 0
static const fp256::Modulus<N>& secp256k1() {
    static const uint32_t P[N] = {0xFFFFFC2Fu, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    static const fp256::Modulus<N> m = fp256::make_modulus<N>(P);
    return m;
}

__global__ __launch_bounds__(256) void weierstrass_add_kernel(uint32_t* __restrict__ out, uint32_t height, const uint64_t* __restrict__ events,
                                                              uint32_t n_events, const fp256::Modulus<N> m) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    tgf::weierstrass_add_row<N>(out, height, row, row < n_events ? events + (size_t)row * Add::EVENT_WORDS : nullptr, m, WITNESS_OFFSET);
}

__global__ __launch_bounds__(256) void weierstrass_double_kernel(uint32_t* __restrict__ out, uint32_t height, const uint64_t* __restrict__ events,
                                                                 uint32_t n_events, const fp256::Modulus<N> m, const fp256::U<N> a) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    tgf::weierstrass_double_row<N>(out, height, row, row < n_events ? events + (size_t)row * Double::EVENT_WORDS : nullptr, m, a, WITNESS_OFFSET);
}

}  // namespace tgw
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

int sp1hip_tracegen_riscv_secp256k1_add_width(void) { return tgw::Add::WIDTH; }
int sp1hip_tracegen_riscv_secp256k1_double_width(void) { return tgw::Double::WIDTH; }

int sp1hip_tracegen_riscv_secp256k1_add(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    return tg::launch_rows(__func__, tgw::weierstrass_add_kernel, d_table, height, d_events, n_events, stream, tgw::secp256k1());
}

int sp1hip_tracegen_riscv_secp256k1_double(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    return tg::launch_rows(__func__, tgw::weierstrass_double_kernel, d_table, height, d_events, n_events, stream, tgw::secp256k1(), fp256::small<tgw::N>(0));
}

}  // extern "C"
