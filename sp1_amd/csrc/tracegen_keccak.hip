// sp1_amd/csrc/tracegen_keccak.hip — device trace generation for the two chips of a KECCAK_PERMUTE precompile shard:
// KeccakPermute (24 rows of 2,640 columns per system call) and KeccakPermuteControl (one row of 634 columns per call), from the
// executor's 77-word event records (sp1hip_rv64_keccak_events) instead of host-made tables. A call's rows are 253 KB of table
// for a 616-byte event, so what crosses the bus shrinks by a factor of ~400.
//
// The reference fills both tables on the host (it has no device filler for them); the definitions followed here are
//   KeccakPermuteChip::generate_trace_into          crates/core/machine/src/syscall/precompiles/keccak256/trace.rs:L63-L162
//   KeccakPermuteControlChip::generate_trace_into   .../keccak256/controller.rs:L155-L237
//   MemoryAccessCols::populate                      crates/core/machine/src/memory/consistency/trace.rs:L36-L101
//   SyscallAddrOperation::populate                  crates/core/machine/src/operations/syscall_addr.rs:L27-L46
// and the column order is the one sp1_amd/machines/riscv_more.py transcribes (keccak_permute_chip / keccak_control_chip), which
// tests/test_gpu_tracegen_keccak.py compares every word with.
//
// Lane mapping. One lane owns one ROW in both kernels, so every store of a column goes to consecutive rows from consecutive
// lanes (256 B per wave instruction), and the table is written exactly once. A 2,640-word row does not fit a lane's registers,
// so no row image exists anywhere: the lane that owns row 24 e + r loads the 25 lanes of event e's state, runs rounds 0 .. r - 1
// on them in registers (the round body is fully unrolled, the state never indexed at run time: no scratch), and then walks the
// columns in table order, computing c, c', a', a'' of round r as 64-bit values and storing their bits and limbs as it goes. The
// recomputation is at most 23 rounds of ~150 64-bit operations per row against 2,640 stores per row: the kernel stays bound by
// the table's write. Padding rows run the same code on the zero state (trace.rs:L88-L122: a trailing chunk takes the first rows
// of the zero state's permutation, so padding row q is its round q mod 24) with is_real = 0.
#include "device_ctx.hpp"
#include "tg_field_op.hpp"
#include "tg_row_kernel.hpp"

namespace sp1hip {
namespace tgk {

constexpr int EVENT_WORDS = SP1HIP_RV64_KECCAK_WORDS;          // clk, state pointer, 25 x (previous timestamp, word read), 25 words written
constexpr int ROUNDS = 24;
constexpr int PERMUTE_WIDTH = 24 + 1 + 100 + 100 + 320 + 320 + 1600 + 100 + 64 + 4 + 7;
constexpr int CONTROL_WIDTH = 2 + 6 + 75 + 1 + 225 + 225 + 100;
static_assert(EVENT_WORDS == 77 && PERMUTE_WIDTH == 2640 && CONTROL_WIDTH == 634, "layouts");

__constant__ uint64_t RC[ROUNDS] = {
    0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808Aull, 0x8000000080008000ull, 0x000000000000808Bull, 0x0000000080000001ull,
    0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008Aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000Aull,
    0x000000008000808Bull, 0x800000000000008Bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
    0x000000000000800Aull, 0x800000008000000Aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};

// rotation offsets r[x][y] (FIPS 202 §3.2.2), as a function so that every use folds to a constant
__host__ __device__ constexpr int rot_of(int x, int y) {
    constexpr int R[5][5] = {{0, 36, 3, 41, 18}, {1, 44, 10, 45, 2}, {62, 6, 43, 15, 61}, {28, 55, 25, 21, 56}, {27, 20, 39, 8, 14}};
    return R[x][y];
}
template <int N> __device__ __forceinline__ uint64_t rotl(uint64_t v) {
    if constexpr (N == 0) return v; else return (v << N) | (v >> (64 - N));
}

// The cursor a lane writes its row with (one column per put, in table order) is tg_field_op.hpp's, as are the memory columns below.
using tgf::Cursor;
using tgf::memory_access;

// a[x + 5 y]: theta's column parities c and c', a' = a ^ c ^ c' (p3-keccak-air's names; sp1_amd/machines/riscv_more_trace.py keccak_f_rows)
__device__ __forceinline__ void theta(const uint64_t (&a)[25], uint64_t (&c)[5], uint64_t (&cp)[5]) {
#pragma unroll
    for (int x = 0; x < 5; x++) c[x] = a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20];
#pragma unroll
    for (int x = 0; x < 5; x++) cp[x] = c[x] ^ c[(x + 4) % 5] ^ rotl<1>(c[(x + 1) % 5]);
}
// rho and pi (B[y, 2x + 3y] = ROT(A'[x, y], r[x][y])), then chi: a''[x + 5 y] from a'[x + 5 y]
template <int X, int Y> __device__ __forceinline__ void rho_pi_one(const uint64_t (&ap)[25], uint64_t (&b)[25]) {
    b[Y + 5 * ((2 * X + 3 * Y) % 5)] = rotl<rot_of(X, Y)>(ap[X + 5 * Y]);
}
template <int I> __device__ __forceinline__ void rho_pi_all(const uint64_t (&ap)[25], uint64_t (&b)[25]) {
    if constexpr (I < 25) { rho_pi_one<I % 5, I / 5>(ap, b); rho_pi_all<I + 1>(ap, b); }
}
__device__ __forceinline__ void rho_pi_chi(const uint64_t (&ap)[25], uint64_t (&app)[25]) {
    uint64_t b[25];
    rho_pi_all<0>(ap, b);
#pragma unroll
    for (int y = 0; y < 5; y++)
#pragma unroll
        for (int x = 0; x < 5; x++) app[x + 5 * y] = b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & b[(x + 2) % 5 + 5 * y]);
}
__device__ __forceinline__ void round_in_place(uint64_t (&a)[25], uint64_t rc) {
    uint64_t c[5], cp[5], ap[25];
    theta(a, c, cp);
#pragma unroll
    for (int i = 0; i < 25; i++) ap[i] = a[i] ^ c[i % 5] ^ cp[i % 5];
    rho_pi_chi(ap, a);
    a[0] ^= rc;
}

__global__ __launch_bounds__(256) void keccak_permute_kernel(uint32_t* __restrict__ out, uint32_t height, const uint64_t* __restrict__ events, uint32_t n_events) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    const uint32_t e = row / ROUNDS, r = row - e * ROUNDS;
    const bool real = e < n_events;
    const uint64_t* ev = events + (size_t)(real ? e : 0u) * EVENT_WORDS;                       // read on real rows only
    uint64_t a[25];
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] = real ? gptr(ev)[3 + 2 * i] : 0ull;
    const uint64_t clk = real ? gptr(ev)[0] : 0ull, addr = real ? gptr(ev)[1] : 0ull;
    Cursor w{out, row, height};
    // step_flags[24], export
    for (uint32_t i = 0; i < ROUNDS; i++) w.bit(i == r);
    w.bit(r == ROUNDS - 1);
    // preimage: the state the call read, on every row of the call
#pragma unroll
    for (int i = 0; i < 25; i++) w.limbs(a[i]);
    // the state entering round r
    for (uint32_t i = 0; i < r; i++) round_in_place(a, RC[i]);
#pragma unroll
    for (int i = 0; i < 25; i++) w.limbs(a[i]);
    uint64_t c[5], cp[5];
    theta(a, c, cp);
#pragma unroll
    for (int x = 0; x < 5; x++) w.bits64(c[x]);
#pragma unroll
    for (int x = 0; x < 5; x++) w.bits64(cp[x]);
#pragma unroll
    for (int i = 0; i < 25; i++) a[i] ^= c[i % 5] ^ cp[i % 5];                                  // a'
#pragma unroll
    for (int i = 0; i < 25; i++) w.bits64(a[i]);
    uint64_t app[25];
    rho_pi_chi(a, app);
#pragma unroll
    for (int i = 0; i < 25; i++) w.limbs(app[i]);
    w.bits64(app[0]);
    w.limbs(app[0] ^ RC[r]);
    // clk_high, clk_low, state_addr[3], index, is_real (zero on padding rows: clk and addr are)
    w.val((uint32_t)(clk >> 24));
    w.val((uint32_t)clk & 0xffffffu);
    w.limbs(addr, 3);
    w.val(real ? r : 0u);
    w.bit(real);
}

__global__ __launch_bounds__(256) void keccak_control_kernel(uint32_t* __restrict__ out, uint32_t height, const uint64_t* __restrict__ events, uint32_t n_events) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    Cursor w{out, row, height};
    if (row >= n_events) {                                                                      // padding rows are zero
        for (int c = 0; c < CONTROL_WIDTH; c++) w.word(0u);
        return;
    }
    const uint64_t* ev = events + (size_t)row * EVENT_WORDS;
    const uint64_t clk = gptr(ev)[0], addr = gptr(ev)[1];
    w.val((uint32_t)(clk >> 24));
    w.val((uint32_t)clk & 0xffffffu);
    tgf::syscall_addr(w, addr);                                                                 // SyscallAddrOperation
    for (uint32_t i = 0; i < 25; i++) tgf::addr_add(w, addr + 8u * i);                          // AddrAddOperation x 25
    w.bit(true);                                                                                // is_real
    // the reads at clk against the words' previous accesses, the writes at clk + 1 against the reads
    for (uint32_t i = 0; i < 25; i++) memory_access(w, gptr(ev)[3 + 2 * i], gptr(ev)[2 + 2 * i], clk);
    for (uint32_t i = 0; i < 25; i++) memory_access(w, gptr(ev)[3 + 2 * i], clk, clk + 1);
    for (uint32_t i = 0; i < 25; i++) w.limbs(gptr(ev)[52 + i]);                                // final_value
}

}  // namespace tgk
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

int sp1hip_tracegen_riscv_keccak_width(void) { return tgk::PERMUTE_WIDTH; }
int sp1hip_tracegen_riscv_keccak_control_width(void) { return tgk::CONTROL_WIDTH; }

int sp1hip_tracegen_riscv_keccak(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE((uint64_t)n_events * tgk::ROUNDS <= height, "the events' rows (24 each) exceed the height");
    return tg::launch_rows(__func__, tgk::keccak_permute_kernel, d_table, height, d_events, n_events, stream);
}

int sp1hip_tracegen_riscv_keccak_control(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    return tg::launch_rows(__func__, tgk::keccak_control_kernel, d_table, height, d_events, n_events, stream);
}

}  // extern "C"
