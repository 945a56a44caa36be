// sp1_amd/csrc/tracegen_rv64_partition.hip — a stable partition of a core shard's executed instructions ON THE DEVICE: from the
// executor's [n][20] u64 records to one record stream per chip, in execution order inside each stream, packed as the chips' kernels
// read them (sp1hip_rv64_alu_event_t / sp1hip_rv64_mem_event_t and the short records of StateBump and MemoryBump). The host does this
// with a pass over object arrays and one fancy-indexed gather per chip (riscv_exec.chip_of_events, pack_alu_events, pack_mem_events).
//
// Where an event goes and what it becomes there is tg_rv64_partition.hpp, host and device code alike (tests/native/riscv_sys_rows.hip
// runs it on the CPU). This file is the launch structure and the ABI. No workgroup waits on another and no atomic decides a
// position, so the result is the same bytes on every run — the three-phase form of tracegen_global.hip's scan:
//
//   partition_count_kernel    one lane per event. A wave matches the lanes of one bin with a ballot (one ballot per bin PRESENT in the
//                             wave, not per bin) and counts them with a population count; the four waves' counts meet in LDS and the
//                             workgroup's 32 counters go to scratch[workgroup][32]
//   partition_scan_kernel     ONE workgroup of 1024 lanes = 32 bins x 32 slices of the workgroups: exclusive offsets per bin over the
//                             workgroups, in place (serial over a slice, the slice totals through LDS), and the 29 totals
//   partition_scatter_kernel  one lane per event again: its bin recomputed, its destination = the bin's start in the arena + the
//                             workgroup's offset + the earlier waves' counts (LDS) + its rank in the wave (the ballot below the
//                             lane; for MemoryBump a prefix sum of the 0..3 records of the lanes below), then the record packed and
//                             stored. Every store is checked against the arena's size.
//
// An event is read with ten 16-byte loads (the count pass reads the five it needs); about 420 bytes move per event over both passes.
#include "device_ctx.hpp"
#include "tg_rv64_partition.hpp"

namespace sp1hip {
namespace tg {

static_assert(sizeof(RawEv) == 8 * RAW_EV_WORDS, "event layout");
static_assert(BINS == SP1HIP_RV64_BINS, "bins");

constexpr uint32_t PART_WG = SP1HIP_RV64_PARTITION_WORKGROUP, PART_WAVES = PART_WG / 64;
constexpr uint32_t SCAN_SLICES = SP1HIP_RV64_PARTITION_SCAN_SLICES, SCAN_LANES = SCAN_SLICES * BIN_SLOTS;

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// words 2 k, 2 k + 1 of event i
__device__ __forceinline__ u64x2 ld_pair(const uint64_t* __restrict__ events, uint64_t i, int k) {
    return gptr(reinterpret_cast<const u64x2*>(events))[i * (RAW_EV_WORDS / 2) + k];
}

// what the routing reads: pc, clk, op, op_a, flags, a_prev and the three previous timestamps
__device__ __forceinline__ RawEv load_head(const uint64_t* __restrict__ events, uint64_t i) {
    RawEv e = {};
    const u64x2 p0 = ld_pair(events, i, 0), p1 = ld_pair(events, i, 1), p3 = ld_pair(events, i, 3), p5 = ld_pair(events, i, 5), p6 = ld_pair(events, i, 6);
    e.pc = p0.x; e.clk = p0.y; e.op = p1.x; e.op_a = p1.y; e.flags = p3.x; e.a = p3.y; e.a_prev = p5.x; e.a_pts = p5.y; e.b_pts = p6.x; e.c_pts = p6.y;
    return e;
}

__device__ __forceinline__ RawEv load_event(const uint64_t* __restrict__ events, uint64_t i) {
    RawEv e;
    const u64x2 p0 = ld_pair(events, i, 0), p1 = ld_pair(events, i, 1), p2 = ld_pair(events, i, 2), p3 = ld_pair(events, i, 3), p4 = ld_pair(events, i, 4),
                p5 = ld_pair(events, i, 5), p6 = ld_pair(events, i, 6), p7 = ld_pair(events, i, 7), p8 = ld_pair(events, i, 8), p9 = ld_pair(events, i, 9);
    e.pc = p0.x; e.clk = p0.y; e.op = p1.x; e.op_a = p1.y; e.op_b = p2.x; e.op_c = p2.y; e.flags = p3.x; e.a = p3.y; e.b = p4.x; e.c = p4.y;
    e.a_prev = p5.x; e.a_pts = p5.y; e.b_pts = p6.x; e.c_pts = p6.y; e.m_addr = p7.x; e.m_pts = p7.y; e.m_prev = p8.x; e.m_new = p8.y;
    e.next_pc = p9.x; e.spare = p9.y;
    return e;
}

// The lane's place among the lanes of its wave in each stream it adds to, and the wave's counts into counts[32] (LDS, zero before).
// `bin` is BIN_NONE for a lane without an event
struct Ranks { uint32_t main, syscall_core, state_bump, memory_bump; };

__device__ __forceinline__ Ranks wave_ranks(int bin, const Extra& x, uint32_t* __restrict__ counts) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t below = (1ull << lane) - 1ull;
    Ranks r = {0u, 0u, 0u, 0u};
    uint64_t todo = __ballot(bin != BIN_NONE);                        // the lanes whose bin has not been matched yet: wave-uniform
    while (todo) {
        const int leader = __ffsll((unsigned long long)todo) - 1;
        const int b = __shfl(bin, leader);
        const uint64_t m = __ballot(bin == b);
        if (bin == b) r.main = (uint32_t)__popcll(m & below);
        if ((int)lane == leader) counts[b] = (uint32_t)__popcll(m);
        todo &= ~m;
    }
    const uint64_t m_sc = __ballot(x.syscall_core), m_sb = __ballot(x.state_bump);
    const uint64_t m_a = __ballot((x.bumps & 1u) != 0), m_b = __ballot((x.bumps & 2u) != 0), m_c = __ballot((x.bumps & 4u) != 0);
    r.syscall_core = (uint32_t)__popcll(m_sc & below);
    r.state_bump = (uint32_t)__popcll(m_sb & below);
    r.memory_bump = (uint32_t)(__popcll(m_a & below) + __popcll(m_b & below) + __popcll(m_c & below));
    if (lane == 0) {
        counts[BIN_SYSCALL_CORE] = (uint32_t)__popcll(m_sc);
        counts[BIN_STATE_BUMP] = (uint32_t)__popcll(m_sb);
        counts[BIN_MEMORY_BUMP] = (uint32_t)(__popcll(m_a) + __popcll(m_b) + __popcll(m_c));
    }
    return r;
}

__global__ __launch_bounds__(PART_WG) void partition_count_kernel(const uint64_t* __restrict__ events, uint64_t n, uint32_t* __restrict__ scratch) {
    __shared__ uint32_t sh[PART_WAVES][BIN_SLOTS];
    const uint32_t t = threadIdx.x;
    if (t < PART_WAVES * BIN_SLOTS) sh[t / BIN_SLOTS][t % BIN_SLOTS] = 0u;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * PART_WG + t;
    int bin = BIN_NONE;
    Extra x = {false, false, 0u};
    if (i < n) {
        const RawEv e = load_head(events, i);
        bin = bin_of(e.op, e.op_a);
        x = extra_of(e, bin);
    }
    wave_ranks(bin, x, sh[t >> 6]);
    __syncthreads();
    if (t < BIN_SLOTS) {
        uint32_t total = 0;
#pragma unroll
        for (uint32_t w = 0; w < PART_WAVES; w++) total += sh[w][t];
        gptr(scratch)[(size_t)blockIdx.x * BIN_SLOTS + t] = t < (uint32_t)BINS ? total : 0u;
    }
}

// lane = slice * 32 + bin: slice s holds the workgroups [s per, (s + 1) per)
__global__ __launch_bounds__(SCAN_LANES) void partition_scan_kernel(uint32_t* __restrict__ scratch, uint32_t workgroups, uint32_t* __restrict__ counts) {
    __shared__ uint32_t sh[SCAN_SLICES][BIN_SLOTS];
    const uint32_t bin = threadIdx.x % BIN_SLOTS, slice = threadIdx.x / BIN_SLOTS;
    const uint32_t per = (workgroups + SCAN_SLICES - 1) / SCAN_SLICES;
    const uint64_t lo = (uint64_t)slice * per, end = lo + per, hi = end < workgroups ? end : workgroups;
    uint32_t acc = 0;
    for (uint64_t w = lo; w < hi; w++) {
        const uint32_t v = gptr(scratch)[w * BIN_SLOTS + bin];
        gptr(scratch)[w * BIN_SLOTS + bin] = acc;
        acc += v;
    }
    sh[slice][bin] = acc;
    __syncthreads();
    uint32_t before = 0, total = 0;
    for (uint32_t s = 0; s < SCAN_SLICES; s++) {
        const uint32_t v = sh[s][bin];
        before += s < slice ? v : 0u;
        total += v;
    }
    if (before)
        for (uint64_t w = lo; w < hi; w++) gptr(scratch)[w * BIN_SLOTS + bin] += before;
    if (slice == 0 && bin < (uint32_t)BINS) gptr(counts)[bin] = total;
}

template <int W> __device__ __forceinline__ void store_record(uint64_t* __restrict__ records, uint64_t records_words, uint64_t at, const uint64_t (&o)[W]) {
    if (at + W > records_words) return;                            // counts that are not this stream's: nothing is written out of bounds
#pragma unroll
    for (int k = 0; k < W; k++) gptr(records)[at + k] = o[k];
}

__global__ __launch_bounds__(PART_WG) void partition_scatter_kernel(const uint64_t* __restrict__ events, uint64_t n, const uint32_t* __restrict__ scratch,
                                                                   const uint32_t* __restrict__ counts, uint64_t* __restrict__ records,
                                                                   uint64_t records_words) {
    __shared__ uint32_t sh[PART_WAVES][BIN_SLOTS];
    __shared__ uint64_t start[BIN_SLOTS];                          // the word a bin's stream starts at
    __shared__ uint32_t offset[BIN_SLOTS];                         // this workgroup's first record in the stream
    const uint32_t t = threadIdx.x, wave = t >> 6;
    if (t < PART_WAVES * BIN_SLOTS) sh[t / BIN_SLOTS][t % BIN_SLOTS] = 0u;
    if (t < BIN_SLOTS) {
        uint64_t at = 0;
        for (uint32_t b = 0; b < t && b < (uint32_t)BINS; b++) at += (uint64_t)gptr(counts)[b] * (uint32_t)words_of_bin((int)b);
        start[t] = at;
        offset[t] = gptr(scratch)[(size_t)blockIdx.x * BIN_SLOTS + t];
    }
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * PART_WG + t;
    int bin = BIN_NONE;
    Extra x = {false, false, 0u};
    RawEv e = {};
    if (i < n) {
        e = load_event(events, i);
        bin = bin_of(e.op, e.op_a);
        x = extra_of(e, bin);
    }
    const Ranks r = wave_ranks(bin, x, sh[wave]);
    __syncthreads();
    auto place = [&](int b, uint32_t rank) {                       // the record's first word
        uint32_t idx = offset[b] + rank;
        for (uint32_t w = 0; w < wave; w++) idx += sh[w][b];
        return start[b] + (uint64_t)idx * (uint32_t)words_of_bin(b);
    };
    if (bin == BIN_NONE) return;
    if (bin >= BIN_MEM0 && bin < BIN_DIVREM) {
        uint64_t o[MEM_WORDS];
        pack_mem(o, e);
        store_record(records, records_words, place(bin, r.main), o);
    } else {
        uint64_t o[ALU_WORDS];
        pack_alu(o, e);
        store_record(records, records_words, place(bin, r.main), o);
        if (x.syscall_core) store_record(records, records_words, place(BIN_SYSCALL_CORE, r.syscall_core), o);
    }
    if (x.state_bump) {
        uint64_t o[STATE_BUMP_WORDS];
        pack_state_bump(o, e, bin);
        store_record(records, records_words, place(BIN_STATE_BUMP, r.state_bump), o);
    }
    if (x.bumps) {
        uint64_t at = place(BIN_MEMORY_BUMP, r.memory_bump);
#pragma unroll
        for (int slot = 0; slot < 3; slot++) {
            if (x.bumps & (1u << slot)) {
                uint64_t o[MEMORY_BUMP_WORDS];
                pack_memory_bump(o, e, slot);
                store_record(records, records_words, at, o);
                at += MEMORY_BUMP_WORDS;
            }
        }
    }
}

constexpr uint64_t PART_MAX_EVENTS = 1ull << 30;                   // three MemoryBump records per event still count in 32 bits
inline uint64_t part_workgroups(uint64_t n) { return (n + PART_WG - 1) / PART_WG; }

}  // namespace tg
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

uint64_t sp1hip_rv64_partition_scratch_bytes(uint64_t n_events) {
    const uint64_t wgs = tg::part_workgroups(n_events);
    return (wgs ? wgs : 1) * tg::BIN_SLOTS * sizeof(uint32_t);
}

int sp1hip_rv64_partition_count(const uint64_t* d_events, uint64_t n_events, uint32_t* d_scratch, uint32_t* d_counts, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(n_events <= tg::PART_MAX_EVENTS, "more than 2^30 events");
    SP1HIP_REQUIRE(n_events == 0 || (d_events && d_scratch && d_counts), "null buffer");
    SP1HIP_REQUIRE(((uintptr_t)d_events & 15u) == 0 && ((uintptr_t)d_scratch & 3u) == 0 && ((uintptr_t)d_counts & 3u) == 0, "misaligned buffer");
    if (n_events == 0) return SP1HIP_SUCCESS;
    const uint32_t wgs = (uint32_t)tg::part_workgroups(n_events);
    hipLaunchKernelGGL(tg::partition_count_kernel, dim3(wgs), dim3(tg::PART_WG), 0, S(stream), d_events, n_events, d_scratch);
    SP1HIP_LAUNCH_CHECK();
    hipLaunchKernelGGL(tg::partition_scan_kernel, dim3(1), dim3(tg::SCAN_LANES), 0, S(stream), d_scratch, wgs, d_counts);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}

int sp1hip_rv64_partition_scatter(const uint64_t* d_events, uint64_t n_events, const uint32_t* d_scratch, const uint32_t* d_counts, uint64_t* d_records,
                                  uint64_t records_words, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(n_events <= tg::PART_MAX_EVENTS, "more than 2^30 events");
    SP1HIP_REQUIRE(n_events == 0 || (d_events && d_scratch && d_counts), "null buffer");
    SP1HIP_REQUIRE(d_records || records_words == 0, "null record arena");
    SP1HIP_REQUIRE(((uintptr_t)d_events & 15u) == 0 && ((uintptr_t)d_scratch & 3u) == 0 && ((uintptr_t)d_counts & 3u) == 0 && ((uintptr_t)d_records & 7u) == 0,
                   "misaligned buffer");
    if (n_events == 0) return SP1HIP_SUCCESS;
    const uint32_t wgs = (uint32_t)tg::part_workgroups(n_events);
    hipLaunchKernelGGL(tg::partition_scatter_kernel, dim3(wgs), dim3(tg::PART_WG), 0, S(stream), d_events, n_events, d_scratch, d_counts, d_records,
                       records_words);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}

}  // extern "C"
