// sp1_amd/csrc/col_dot.hpp — sum_r eq[r] * col_c[r] over one row chunk for the (up to) four base-field columns of a workgroup: the
// inner loop that the trace openings (gkr::open_columns_kernel) and the column evaluations (eval_columns_partial_kernel) share.
// Both stream the whole trace once against an eq table and are nowhere near VALU-bound (kb::dot_add is ~15 instructions per word), so
// what decides their speed is how many bytes a lane has in flight: one row per lane and step was eight 4-byte loads. (ld_rows4 is
// also what batch_kernel loads with.)
#pragma once
#include "common.hpp"
#include "kb31.hpp"

namespace sp1hip {

constexpr int COL_DOT_COLS = 4;            // columns per workgroup: 4 x 16 VGPRs of unreduced accumulators
constexpr uint32_t COL_DOT_ROWS = 16384;   // rows per workgroup: 16 row groups = 64 terms per lane and accumulator (<= 2^16)
static_assert(COL_DOT_ROWS % (4 * 256) == 0, "a row chunk is whole row groups for every lane, so only a table's last chunk has a tail");

// Rows r .. r+3 of a column (or of one coordinate plane of eq), r % 4 == 0: one 16-byte load where the column's base is 16-byte
// aligned, four 4-byte loads where it is not (an odd column of a table whose height is no multiple of 4).
// `base` is workgroup-uniform and r a 32-bit lane offset, so the eight loads of a step share one offset register.
template <bool ALIGNED>
__device__ __forceinline__ q4_t ld_rows4(const uint32_t* base, uint32_t r) {
    if (ALIGNED) return gptr(reinterpret_cast<const q4_t*>(base))[r >> 2];
    const auto* w = gptr(base);
    return q4_t{w[r], w[r + 1], w[r + 2], w[r + 3]};
}
__host__ __device__ __forceinline__ bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The whole row groups of the chunk: a lane takes groups of four consecutive rows and issues the eight loads of a step (4 eq planes
// + NC columns, 16 bytes each) before the first multiply-add: 116 VGPRs, four waves per SIMD, 128 KB in flight per CU. (Two groups
// per step, sixteen loads, is 150 VGPRs and three waves; held to 128 it spills 100 bytes per lane to scratch.)
template <int NC, bool ALIGNED>
__device__ __forceinline__ void col_dot_groups(const uint32_t* const (&col)[NC], const uint32_t* eq, size_t eq_len, uint32_t r0,
                                               uint32_t groups, kb::DotAcc (&acc)[NC]) {
    for (uint32_t g = threadIdx.x; g < groups; g += 256) {
        q4_t e[4], v[NC];
#pragma unroll
        for (int k = 0; k < 4; k++) e[k] = ld_rows4<ALIGNED>(eq + k * eq_len + r0, 4 * g);
#pragma unroll
        for (int c = 0; c < NC; c++) v[c] = ld_rows4<ALIGNED>(col[c] + r0, 4 * g);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const kb::Ext ej{{e[0][j], e[1][j], e[2][j], e[3][j]}};
#pragma unroll
            for (int c = 0; c < NC; c++) kb::dot_add(acc[c], ej, v[c][j]);
        }
    }
}

// acc[c] += sum over rows r0 <= r < r1 of eq[r] * col[c][r]; eq is four coordinate planes of eq_len words, r0 % 4 == 0,
// r1 - r0 <= COL_DOT_ROWS. `aligned` (workgroup-uniform): eq, its planes and every col[c] are 16-byte aligned. The (r1 - r0) % 4
// last rows of a table go one row per lane.
template <int NC>
__device__ __forceinline__ void col_dot_rows(const uint32_t* const (&col)[NC], const uint32_t* eq, size_t eq_len, uint32_t r0,
                                             uint32_t r1, bool aligned, kb::DotAcc (&acc)[NC]) {
    const uint32_t groups = (r1 - r0) >> 2;
    if (aligned) col_dot_groups<NC, true>(col, eq, eq_len, r0, groups, acc);
    else col_dot_groups<NC, false>(col, eq, eq_len, r0, groups, acc);
    const size_t r = r0 + 4 * (size_t)groups + threadIdx.x;
    if (r < r1) {
        const kb::Ext e{{gptr(eq)[r], gptr(eq)[eq_len + r], gptr(eq)[2 * eq_len + r], gptr(eq)[3 * eq_len + r]}};
#pragma unroll
        for (int c = 0; c < NC; c++) kb::dot_add(acc[c], e, gptr(col[c])[r]);
    }
}

}  // namespace sp1hip
