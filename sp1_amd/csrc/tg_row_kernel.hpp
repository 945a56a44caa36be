// sp1_amd/csrc/tg_row_kernel.hpp — one lane, one row: what every RISC-V trace generator does around its chip's row function, written
// once for host and device code alike. A row held as W words, the zero row, the Montgomery store of a row into the column-major
// table, the store of a row's Global events, the kernel that does this for a chip given as a traits type, the launch with its
// argument check, and the same loop over the rows on the host (tests/native/riscv_*_rows.hip: the CPU tests run the zero, fill and
// store code the kernel runs, not a copy of it).
//
// A chip is a type with
//   static constexpr int WIDTH;  using Rec = <the record type `records` points to>;
//   static void live(Row<WIDTH>& r, const Rec* records, uint32_t row, extra...);     the row of record `row`, from the zero row
//   static void padding(Row<WIDTH>& r);                                             a row behind the records, from the zero row
// next to the row functions it wraps (tg_riscv_rows.hpp, tg_riscv_{mem,core,sys,memglobal}_rows.hpp). `extra...` are the
// kernel's further arguments, passed on as they are: the pointer the row's Global events go to, a call's constants.
//
// The branch `row < n ? live : padding` stands in the kernel's body and must stay there. Handed to the chip as a flag (a functor
// chip(r, row, live), a static Chip::fill(r, records, row, live), a lambda given to a helper) it costs ShiftLeft 12 bytes of
// scratch per lane: DESIGN.md, "One row-per-lane kernel", has the figures.
#pragma once
#include "common.hpp"
#include "kb31.hpp"

#ifndef TG_HD
#define TG_HD __host__ __device__ __forceinline__
#endif
// the table and the Global events are device memory on the device: say so at the store (common.hpp gptr)
#if defined(__HIP_DEVICE_COMPILE__)
#define TG_GLOBAL(p) gptr(p)
#else
#define TG_GLOBAL(p) (p)
#endif

namespace sp1hip {
namespace tg {

constexpr uint32_t M16 = 0xffffu;
constexpr int GLOBAL_EVENT_WORDS = 9;                         // message[8], then is_receive | kind << 8 (sp1hip_tracegen_riscv_global)

// Every index into Row::c is a constant (fully unrolled loops), so on the device a row is registers
template <int W> struct Row {
    uint32_t c[W];
    TG_HD void limbs4(int at, uint64_t v) { c[at] = v & M16; c[at + 1] = (v >> 16) & M16; c[at + 2] = (v >> 32) & M16; c[at + 3] = (v >> 48) & M16; }
    TG_HD void limbs3(int at, uint64_t v) { c[at] = v & M16; c[at + 1] = (v >> 16) & M16; c[at + 2] = (v >> 32) & M16; }
};

// Columns [LO, HI) of a row: zeroed, and stored as Montgomery words at out[c * height + row] (DivRem makes its row in four such
// groups; every other chip uses the whole row)
template <int LO, int HI, int W> TG_HD void zero_cols(Row<W>& r) {
#pragma unroll
    for (int c = LO; c < HI; c++) r.c[c] = 0;
}
template <int LO, int HI, int W> TG_HD void store_cols(uint32_t* __restrict__ out, uint32_t height, uint32_t row, const Row<W>& r) {
#pragma unroll
    for (int c = LO; c < HI; c++) TG_GLOBAL(out)[(size_t)c * height + row] = r.c[c] ? kb::to_monty(r.c[c]) : 0u;
}
template <int W> TG_HD void zero_row(Row<W>& r) { zero_cols<0, W>(r); }
template <int W> TG_HD void store_row(uint32_t* __restrict__ out, uint32_t height, uint32_t row, const Row<W>& r) { store_cols<0, W>(out, height, row, r); }

// The K Global events of row `row`, 9 words each, at global_events[row * K * 9 ...]
template <int K> TG_HD void store_global_events(int32_t* __restrict__ global_events, uint32_t row, const int32_t* ev) {
#pragma unroll
    for (int i = 0; i < K * GLOBAL_EVENT_WORDS; i++) TG_GLOBAL(global_events)[(size_t)row * (K * GLOBAL_EVENT_WORDS) + i] = ev[i];
}

// Record `row` of WORDS-word records
template <int WORDS> TG_HD void load_record(uint64_t* rec, const uint64_t* __restrict__ records, uint32_t row) {
#pragma unroll
    for (int i = 0; i < WORDS; i++) rec[i] = records[(size_t)row * WORDS + i];
}

// What a chip with zero padding rows starts from
template <int W, class R> struct ZeroPaddedChip {
    static constexpr int WIDTH = W;
    using Rec = R;
    static TG_HD void padding(Row<W>&) {}
};

// The same on the host: the table of `height` rows from `n` records
template <class Chip, class... Extra> void host_rows(uint32_t* out, uint32_t height, const typename Chip::Rec* records, uint32_t n, Extra... extra) {
    for (uint32_t row = 0; row < height; row++) {
        Row<Chip::WIDTH> r;
        zero_row(r);
        if (row < n) Chip::live(r, records, row, extra...); else Chip::padding(r);
        store_row(out, height, row, r);
    }
}

#if defined(__HIPCC__)
template <class Chip, class... Extra>
__global__ __launch_bounds__(256) void row_kernel(uint32_t* __restrict__ out, uint32_t height, const typename Chip::Rec* __restrict__ records, uint32_t n,
                                                  Extra... extra) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    Row<Chip::WIDTH> r;
    zero_row(r);
    if (row < n) Chip::live(r, records, row, extra...); else Chip::padding(r);
    store_row(out, height, row, r);
}

template <class T> struct AsDeclared { using type = T; };      // keeps `extra...` below out of deduction: the kernel's own types hold

// Launches a kernel of one lane per row, 256 rows per workgroup: row_kernel, or one with the same head that keeps a body of its own
// (DivRem, the Keccak and Weierstrass chips). `entry` is the ABI function's name for the error message.
template <class Rec, class... Extra>
int launch_rows(const char* entry, void (*kernel)(uint32_t*, uint32_t, const Rec*, uint32_t, Extra...), uint32_t* d_table, uint32_t height, const Rec* d_records,
                uint32_t n, sp1hip_stream_t stream, typename AsDeclared<Extra>::type... extra) {
    if (!(n <= height && (d_table || height == 0) && (d_records || n == 0))) {
        set_error("%s: bad argument: more records than rows, or a null pointer with rows to write or records to read", entry);
        return SP1HIP_ERROR_INVALID_ARGUMENT;
    }
    if (height == 0) return SP1HIP_SUCCESS;
    hipLaunchKernelGGL(kernel, dim3((height + 255) / 256), dim3(256), 0, S(stream), d_table, height, d_records, n, extra...);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}
#endif

}  // namespace tg
}  // namespace sp1hip
