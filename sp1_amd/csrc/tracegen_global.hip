// sp1_amd/csrc/tracegen_global.hip — trace generation ON THE DEVICE for the RISC-V machine's Global chip.
//
// The Global chip is a third of a core shard's cells: one row per global interaction event with a Poseidon2 permutation of the
// message, the lift of its digest onto the septic curve, and the running sum of the lifted points. The reference generates it on
// the GPU (/root/reference/sp1-gpu/crates/sys/lib/tracegen/riscv/global.cu:L1-L252: a decompress kernel, a scan of curve points,
// a finalize kernel; CPU definition crates/core/machine/src/global/mod.rs:L131-L260, operations/global_interaction.rs:L33-L103,
// operations/global_accumulation.rs:L28-L54, hypercube/src/septic_{extension,curve,digest}.rs). This is the MI355X counterpart:
//
// The field, the curve, the lift and the row of one event are septic.hpp (KB_HD, shared with tests/native/septic_ops.hip); this
// file holds the kernels' launch structure and the scan.
//
//   global_lift_kernel     one lane per event: for offset = 0, 1, ...: m = message (kind folded into word 0, offset into word 7),
//                          h = Poseidon2(m), x = h[0..7] in F_p^7 = F_p[z] / (z^7 - 3 z - 5); if x^3 + 45 x + 41 z^3 is a square
//                          whose root y has y_6 (or -y_6) in [1, 63 2^24], the point is (x, +-y) — a receive takes the root in
//                          that range, a send its negative — and the row gets message, flags, limbs, x, y, offset, the byte
//                          decomposition of the range check and the 179 columns of the permutation (`populate_perm`).
//                          Square roots take the norm route (septic.py: n^((r+1)/2) / sqrt_p(N(n)), Frobenius maps from a table
//                          COMPUTED on the host at first use, Tonelli-Shanks in F_p).
//   global_chunk_sum / global_scan_totals / global_finalize
//                          cumulative_sum[i] = start + P_0 + ... + P_i by a three-phase scan over the group law (16 points per
//                          lane, one workgroup over the chunk totals), initial_digest[i] = cumulative_sum[i - 1] (start for i = 0);
//                          padding rows: the dummy point, start and start + dummy, the permutation of the zero state
//                          (global/mod.rs:L213-L236).
//
// Events: `GlobalInteractionEvent { message: [u32; 8], is_receive: bool, kind: u8 }` as 9 u32 words per event (the Rust struct's
// `#[repr(C)]` image: word 8 = is_receive | kind << 8). Output: the column-major [241][height] table of Montgomery words the
// prover consumes (column order: sp1_amd/machines/riscv.py::global_chip). Bit-identical to the host trace of
// sp1_amd/machines/{riscv_trace.py, septic.py} (tests/test_gpu_tracegen_global.py).
#include <memory>
#include <mutex>
#include <unordered_map>

#include "device_ctx.hpp"
#include "poseidon2.hpp"
#include "septic.hpp"

namespace sp1hip {
namespace {

using namespace septic;

struct GlobalCtx {
    FrobTables* d_ft = nullptr;
    Pt start, dummy, start_plus_dummy;          // Montgomery
};

// one lane per row: the event's row and its point (septic.hpp: global_event_row), or the padding row
__global__ __launch_bounds__(256) void global_lift_kernel(uint32_t* __restrict__ trace, uint64_t height, const uint32_t* __restrict__ events,
                                                          uint64_t n_events, const p2::RoundConstants* __restrict__ rc,
                                                          const FrobTables* __restrict__ ftp, Pt dummy, Pt* __restrict__ points,
                                                          uint32_t* __restrict__ failed) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= height) return;
    auto put = [&](int col, uint32_t v) { trace[(size_t)col * height + r] = v; };
    if (r >= n_events) {                                              // padding row; global_finalize_kernel writes the accumulation columns
        for (int c = G_INIT_X; c < G_WIDTH; c++) put(c, 0u);
        global_padding_row(rc, dummy, put);
        return;
    }
    if (!global_event_row(events + r * G_EVENT_WORDS, (uint32_t)r, rc, *ftp, put, points + r)) atomicAdd(failed, 1u);
}

constexpr uint32_t G_CHUNK = 16;                                      // points one lane sums sequentially

// totals[c] = Q_{16 c} + ... (Q_0 = start + P_0, Q_i = P_i)
__global__ __launch_bounds__(256) void global_chunk_sum_kernel(const Pt* __restrict__ points, uint64_t n, Pt start, const FrobTables* __restrict__ ftp,
                                                               Pt* __restrict__ totals) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t lo = c * G_CHUNK;
    if (lo >= n) return;
    const FrobTables& ft = *ftp;
    Pt acc = points[lo];
    if (lo == 0) acc = ec_add(ft, start, acc);
    for (uint64_t i = lo + 1; i < lo + G_CHUNK && i < n; i++) acc = ec_add(ft, acc, points[i]);
    totals[c] = acc;
}

// inclusive scan of the chunk totals in place, ONE workgroup of 1024 lanes: serial over a lane's slice, Hillis-Steele over the
// slice totals in LDS, slice prefixes applied
__global__ __launch_bounds__(1024) void global_scan_totals_kernel(Pt* __restrict__ totals, uint64_t n_chunks, const FrobTables* __restrict__ ftp) {
    __shared__ Pt sh[1024];
    const FrobTables& ft = *ftp;
    const uint32_t t = threadIdx.x;
    const uint64_t per = (n_chunks + 1023) / 1024;
    const uint64_t lo = (uint64_t)t * per, hi = lo + per < n_chunks ? lo + per : n_chunks;
    const bool has = lo < n_chunks;
    Pt acc;
    if (has) {
        acc = totals[lo];
        for (uint64_t i = lo + 1; i < hi; i++) { acc = ec_add(ft, acc, totals[i]); totals[i] = acc; }
        sh[t] = acc;
    }
    __syncthreads();
    const uint32_t live = (uint32_t)((n_chunks + per - 1) / per);      // lanes with a slice
    for (uint32_t d = 1; d < live; d <<= 1) {
        Pt v;
        const bool take = has && t >= d;
        if (take) v = ec_add(ft, sh[t - d], sh[t]);
        __syncthreads();
        if (take) sh[t] = v;
        __syncthreads();
    }
    if (has && t > 0) {
        const Pt pre = sh[t - 1];                                     // everything before this lane's slice
        for (uint64_t i = lo; i < hi; i++) totals[i] = ec_add(ft, pre, totals[i]);
    }
}

__global__ __launch_bounds__(256) void global_finalize_kernel(uint32_t* __restrict__ trace, uint64_t height, const Pt* __restrict__ points, uint64_t n,
                                                              const Pt* __restrict__ totals, Pt start, Pt start_plus_dummy,
                                                              const FrobTables* __restrict__ ftp) {
    const uint64_t c = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t lo = c * G_CHUNK;
    if (lo >= height) return;
    const FrobTables& ft = *ftp;
    auto put_pt = [&](uint64_t r, int cx, int cy, const Pt& p) {
        for (int i = 0; i < 7; i++) { trace[(size_t)(cx + i) * height + r] = p.x.c[i]; trace[(size_t)(cy + i) * height + r] = p.y.c[i]; }
    };
    Pt prev = (c == 0 || lo >= n) ? start : totals[c - 1];            // cumulative sum before this chunk (padding-only chunks never use it)
    for (uint64_t r = lo; r < lo + G_CHUNK && r < height; r++) {
        if (r < n) {
            const Pt cur = ec_add(ft, prev, points[r]);
            put_pt(r, G_INIT_X, G_INIT_Y, prev);
            put_pt(r, G_CUM_X, G_CUM_Y, cur);
            prev = cur;
        } else {
            put_pt(r, G_INIT_X, G_INIT_Y, start);
            put_pt(r, G_CUM_X, G_CUM_Y, start_plus_dummy);
        }
    }
}

int get_global_ctx(const GlobalCtx** out) {
    static std::mutex g;
    static std::unordered_map<int, GlobalCtx*> per_device;
    int dev = 0;
    SP1HIP_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g);
    GlobalCtx*& c = per_device[dev];
    if (!c) {
        std::unique_ptr<GlobalCtx> fresh(new GlobalCtx());
        const FrobTables ft = make_frob_tables();
        fresh->start = global_start_point();
        fresh->dummy = global_dummy_point();
        fresh->start_plus_dummy = ec_add(ft, fresh->start, fresh->dummy);
        SP1HIP_HIP(hipMalloc((void**)&fresh->d_ft, sizeof ft));
        const hipError_t e = hipMemcpy(fresh->d_ft, &ft, sizeof ft, hipMemcpyHostToDevice);
        if (e != hipSuccess) { (void)hipFree(fresh->d_ft); return map_hip_error(e, "uploading the Frobenius tables"); }
        c = fresh.release();
    }
    *out = c;
    return SP1HIP_SUCCESS;
}

}  // namespace
}  // namespace sp1hip

using namespace sp1hip;

extern "C" int sp1hip_tracegen_riscv_global(uint32_t* d_trace, uint64_t height, const uint32_t* d_events, uint64_t n_events,
                                            sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(d_trace && (d_events || n_events == 0), "null buffer");
    SP1HIP_REQUIRE(n_events <= height && height < ((uint64_t)1 << 31), "more events than rows, or a table taller than 2^31");
    if (height == 0) return SP1HIP_SUCCESS;
    hipStream_t s = S(stream);
    const DeviceCtx* ctx;
    SP1HIP_TRY(get_device_ctx(&ctx));
    const GlobalCtx* g;
    SP1HIP_TRY(get_global_ctx(&g));
    const uint64_t n_chunks = (n_events + G_CHUNK - 1) / G_CHUNK;
    Pt *d_points = nullptr, *d_totals = nullptr;
    uint32_t* d_failed = nullptr;
    const size_t pts_bytes = std::max<uint64_t>(n_events, 1) * sizeof(Pt), tot_bytes = std::max<uint64_t>(n_chunks, 1) * sizeof(Pt);
    SP1HIP_TRY(arena_alloc((void**)&d_points, pts_bytes, s));
    struct Free { void* p; size_t b; hipStream_t s; ~Free() { arena_free(p, b, s); } } f1{d_points, pts_bytes, s};
    SP1HIP_TRY(arena_alloc((void**)&d_totals, tot_bytes, s));
    Free f2{d_totals, tot_bytes, s};
    SP1HIP_TRY(arena_alloc((void**)&d_failed, 256, s));
    Free f3{d_failed, 256, s};
    SP1HIP_HIP(hipMemsetAsync(d_failed, 0, 4, s));
    hipLaunchKernelGGL(global_lift_kernel, dim3((unsigned)((height + 255) / 256)), dim3(256), 0, s, d_trace, height, d_events, n_events, ctx->d_rc,
                       g->d_ft, g->dummy, d_points, d_failed);
    SP1HIP_LAUNCH_CHECK();
    if (n_events) {
        hipLaunchKernelGGL(global_chunk_sum_kernel, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, s, d_points, n_events, g->start, g->d_ft, d_totals);
        SP1HIP_LAUNCH_CHECK();
        hipLaunchKernelGGL(global_scan_totals_kernel, dim3(1), dim3(1024), 0, s, d_totals, n_chunks, g->d_ft);
        SP1HIP_LAUNCH_CHECK();
    }
    const uint64_t fin_chunks = (height + G_CHUNK - 1) / G_CHUNK;
    hipLaunchKernelGGL(global_finalize_kernel, dim3((unsigned)((fin_chunks + 255) / 256)), dim3(256), 0, s, d_trace, height, d_points, n_events, d_totals,
                       g->start, g->start_plus_dummy, g->d_ft);
    SP1HIP_LAUNCH_CHECK();
    uint32_t failed = 0;
    SP1HIP_HIP(hipMemcpyAsync(&failed, d_failed, 4, hipMemcpyDeviceToHost, s));
    SP1HIP_HIP(hipStreamSynchronize(s));
    SP1HIP_REQUIRE(failed == 0, "an event has no curve point within 256 offsets");
    return SP1HIP_SUCCESS;
}
