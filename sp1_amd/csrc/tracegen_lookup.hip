// sp1_amd/csrc/tracegen_lookup.hip — the Byte, Range and Program multiplicities of a shard counted on the device, from the
// column-major tables the prover already holds: the reference's `generate_dependencies` of its Byte and Range chips
// (crates/core/machine/src/bytes/trace.rs:L50-L66, range/trace.rs:L54-L95) and the Program chip's count of executed pcs
// (program/trusted.rs). Generic over the chip: a chip is its interaction description, compiled by tg_lookup_counts.hpp, which also
// holds the row function (host and device code alike; tests/native/lookup_counts.hip runs it on the CPU). This file is the three
// kernels, the launches and the ABI.
//
// Count kernel: one lane one row, lanes of a wave on consecutive rows (every column load is 64 consecutive words), grid-stride. The
// walk over the sends and their terms is the same in every lane, so the description is read with wave-uniform addresses. Counts
// are u32 and added with no-return device-scope atomics. The messages are very uneven — a zero high limb, the (0, 0) byte pair:
// whole waves address one cell — so before the atomics the lanes that hold the cell of the first pending lane become ONE add of
// their summed multiplicities, up to LC_COMBINE_ROUNDS times or until a round finds a cell nobody shares; what is left is added
// lane by lane. No LDS, no per-lane arrays.
#include "device_ctx.hpp"
#include "tg_lookup_counts.hpp"

namespace sp1hip {
namespace tg {

constexpr int LC_COMBINE_ROUNDS = 4;
constexpr unsigned LC_MAX_BLOCKS = 2048;

__device__ __forceinline__ void lc_atomic_add(uint32_t* p, uint32_t v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The first offender is the one that draws 0 from the counter (a returning atomic, on the error path only).
__device__ __forceinline__ void lc_report(uint32_t* status, uint32_t what, uint32_t send, uint32_t row, uint32_t tag) {
    if (__hip_atomic_fetch_add(&status[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) {
        status[1] = what;
        status[2] = send;
        status[3] = row;
        status[4] = tag;
    }
}

__device__ __forceinline__ uint32_t lc_wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// counts[key] += m for the lanes with `pending`, lanes of one key combined first. Called by whole waves (no divergence around it).
__device__ __forceinline__ void lc_add_combined(uint32_t* counts, bool pending, uint32_t key, uint32_t m) {
    const uint32_t lane = __lane_id();
    uint64_t todo = __ballot(pending);
    for (int round = 0; round < LC_COMBINE_ROUNDS && todo; round++) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t k = __shfl(key, leader, 64), m0 = __shfl(m, leader, 64);
        const bool same = pending && key == k;
        const uint64_t group = __ballot(same);
        // the usual multiplicity is a flag: every lane of the group holds the leader's
        uint32_t sum = m0 * (uint32_t)__popcll(group);
        if (__ballot(same && m != m0)) sum = lc_wave_sum(same ? m : 0u);
        if (lane == leader) lc_atomic_add(counts + k, sum);
        pending = pending && !same;
        todo &= ~group;
        if ((group & (group - 1)) == 0) break;         // nobody shared the leader's cell: take the rest as they are
    }
    if (pending) lc_atomic_add(counts + key, m);
}

__global__ __launch_bounds__(256) void lookup_count_sends_kernel(const uint32_t* __restrict__ prog, const uint32_t* __restrict__ main,
                                                                 const uint32_t* __restrict__ prep, uint32_t rows, uint32_t* __restrict__ byte_counts,
                                                                 uint32_t* __restrict__ range_counts, uint32_t* __restrict__ status, uint32_t tag) {
    const uint32_t n_sends = prog[0];
    for (uint32_t base = blockIdx.x * 256u; base < rows; base += gridDim.x * 256u) {
        const uint32_t row = base + threadIdx.x;
        const bool live = row < rows;
        const uint32_t at = live ? row : rows - 1;     // a lane past the end reads the last row and sends nothing
        const uint32_t* send = prog + 1;
        for (uint32_t s = 0; s < n_sends; s++, send += send[1]) {
            LcMsg msg = lc_message(send, main, prep, rows, at);
            if (!live) msg.where = LC_SKIP;
            if (msg.where == LC_BAD) lc_report(status, LC_WHAT_MESSAGE, send[0], row, tag);
            if (__ballot(msg.where == LC_BYTE)) lc_add_combined(byte_counts, msg.where == LC_BYTE, msg.cell, msg.m);
            if (__ballot(msg.where == LC_RANGE)) lc_add_combined(range_counts, msg.where == LC_RANGE, msg.cell, msg.m);
        }
    }
}

// counts[(pc - pc_base) >> 2] += 1 for n executed pcs, pc i = pcs[i * stride] (u64 words: column E_PC of the [n, 20] event matrix,
// or word 0 of the 11- and 12-word packed records). A loop body is the same few pcs millions of times: combined as above.
__global__ __launch_bounds__(256) void lookup_count_program_kernel(const uint64_t* __restrict__ pcs, uint64_t stride, uint32_t n, uint64_t pc_base,
                                                                   uint32_t n_instructions, uint32_t* __restrict__ counts, uint32_t* __restrict__ status,
                                                                   uint32_t tag) {
    for (uint32_t base = blockIdx.x * 256u; base < n; base += gridDim.x * 256u) {
        const uint32_t i = base + threadIdx.x;
        const bool live = i < n;
        const uint64_t pc = pcs[(size_t)(live ? i : n - 1) * stride];
        uint32_t cell;
        const bool good = lc_program_cell(pc, pc_base, n_instructions, cell);
        if (live && !good) lc_report(status, LC_WHAT_PC, 0u, i, tag);
        lc_add_combined(counts, live && good, cell, 1u);
    }
}

// Counts -> Montgomery words, in place or into `table`. A count at or above the modulus is no field element.
__global__ __launch_bounds__(256) void lookup_counts_finish_kernel(const uint32_t* counts, uint32_t* table, uint64_t n_cells, uint32_t* __restrict__ status) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n_cells; i += (uint64_t)gridDim.x * 256u) {
        const uint32_t v = counts[i];
        if (v >= kb::P) lc_report(status, LC_WHAT_COUNT, 0u, (uint32_t)i, 0u);
        table[i] = v < kb::P ? (v ? kb::to_monty(v) : 0u) : 0u;
    }
}

static unsigned lc_blocks(uint64_t n) { return (unsigned)((n + 255) / 256 < LC_MAX_BLOCKS ? (n + 255) / 256 : LC_MAX_BLOCKS); }

}  // namespace tg
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

int sp1hip_lookup_count_sends(const uint32_t* interactions, uint64_t n_words, uint32_t main_width, uint32_t prep_width, const uint32_t* d_main,
                              const uint32_t* d_prep, uint32_t rows, uint32_t* d_byte_counts, uint32_t* d_range_counts, uint32_t* d_status, uint32_t tag,
                              sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(interactions && n_words >= 1, "no interaction words");
    std::vector<uint32_t> prog;
    const char* why = tg::lc_compile(interactions, n_words, main_width, prep_width, prog);
    SP1HIP_REQUIRE(why == nullptr, why);
    SP1HIP_REQUIRE(d_byte_counts && d_range_counts && d_status, "null count or status buffer");
    SP1HIP_REQUIRE((d_main || main_width == 0 || rows == 0) && (d_prep || prep_width == 0 || rows == 0), "null table");
    SP1HIP_REQUIRE(rows <= (1u << 30), "a table taller than 2^30");
    if (rows == 0 || prog[0] == 0) return SP1HIP_SUCCESS;
    hipStream_t s = S(stream);
    const size_t bytes = prog.size() * 4;
    void* d_prog = nullptr;
    SP1HIP_TRY(arena_alloc(&d_prog, bytes, s));
    // pageable source: the copy has left `prog` when the call returns
    hipError_t e = hipMemcpyAsync(d_prog, prog.data(), bytes, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(tg::lookup_count_sends_kernel, dim3(tg::lc_blocks(rows)), dim3(256), 0, s, (const uint32_t*)d_prog, d_main, d_prep, rows,
                           d_byte_counts, d_range_counts, d_status, tag);
        e = hipGetLastError();
    }
    arena_free(d_prog, bytes, s);                      // stream-ordered: reused only behind the kernel
    SP1HIP_HIP(e);
    return SP1HIP_SUCCESS;
}

int sp1hip_lookup_count_program(const uint64_t* d_pcs, uint64_t stride_words, uint32_t n, uint64_t pc_base, uint32_t n_instructions,
                                uint32_t* d_program_counts, uint32_t* d_status, uint32_t tag, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE((d_pcs || n == 0) && d_program_counts && d_status, "null buffer");
    SP1HIP_REQUIRE(stride_words >= 1 && stride_words <= 4096, "a stride of 0 or more than 4096 words");
    if (n == 0) return SP1HIP_SUCCESS;
    hipLaunchKernelGGL(tg::lookup_count_program_kernel, dim3(tg::lc_blocks(n)), dim3(256), 0, S(stream), d_pcs, stride_words, n, pc_base, n_instructions,
                       d_program_counts, d_status, tag);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}

int sp1hip_lookup_counts_finish(uint32_t* d_counts, uint64_t n_cells, uint32_t* d_table_or_null, uint32_t* d_status, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE((d_counts || n_cells == 0) && d_status, "null buffer");
    SP1HIP_REQUIRE(n_cells < ((uint64_t)1 << 32), "more than 2^32 cells");
    hipStream_t s = S(stream);
    if (n_cells) {
        hipLaunchKernelGGL(tg::lookup_counts_finish_kernel, dim3(tg::lc_blocks(n_cells)), dim3(256), 0, s, (const uint32_t*)d_counts,
                           d_table_or_null ? d_table_or_null : d_counts, n_cells, d_status);
        SP1HIP_LAUNCH_CHECK();
    }
    uint32_t st[tg::LC_STATUS_WORDS] = {0};
    SP1HIP_HIP(hipMemcpyAsync(st, d_status, sizeof st, hipMemcpyDeviceToHost, s));
    SP1HIP_HIP(hipStreamSynchronize(s));
    if (st[0] != 0) {
        if (st[1] == tg::LC_WHAT_MESSAGE)
            set_error("%s: %u byte messages are no row of the table they address, or have a multiplicity of 2^16 or more; the first: send %u, row %u of "
                      "call %u", __func__, st[0], st[2], st[3], st[4]);
        else if (st[1] == tg::LC_WHAT_PC)
            set_error("%s: %u executed pcs are outside the program or not on an instruction; the first: pc %u of call %u", __func__, st[0], st[3], st[4]);
        else
            set_error("%s: %u counts at or above the modulus; the first: cell %u", __func__, st[0], st[3]);
        return SP1HIP_ERROR_INVALID_ARGUMENT;
    }
    return SP1HIP_SUCCESS;
}

}  // extern "C"
