// sp1_amd/csrc/tracegen_ed_uint256_ops.hip — device trace generation for the last three chips behind sp1hip_rv64_precompile_events,
// SP1HIP_RV64_FAMILY_* 12..14: EdAddAssign (1,347 columns), EdDecompress (1,123) and Uint256Ops (477), one row per system call, from
// the executor's event records instead of host-made tables, and the MemoryLocal records of the words an EdDecompress or a Uint256Ops
// call touched. The reference fills these tables on the host and has no device filler for them.
//
// The rows, their definitions in the reference, the column offsets and the preconditions are in tg_ed_uint256_rows.hpp, host and
// device code alike (tests/native/ed_u256_rows.hip runs the same functions on the CPU against the Python fillers). The two Edwards
// tables are made in two launches through a work buffer — 8 x 40 (EdAddAssign) or 7 x 25 (EdDecompress) words per row,
// [block][word][row] — that is allocated and released inside the call, in stream order; Uint256Ops is one launch, one lane per row.
#include "device_ctx.hpp"
#include "tg_ed_uint256_rows.hpp"
#include "tg_row_kernel.hpp"

using namespace sp1hip;

static_assert(tge::TOUCHED_ED_DECOMPRESS == SP1HIP_RV64_FAMILY_ED_DECOMPRESS && tge::TOUCHED_UINT256_OPS == SP1HIP_RV64_FAMILY_UINT256_OPS, "families");

namespace {

// The argument check of tg::launch_rows, then the two phases around a work buffer of `work_words` words
template <class Launch>
int two_phase_table(const char* entry, uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, size_t work_words, sp1hip_stream_t stream,
                    Launch&& launch) {
    if (!(n_events <= height && (d_table || height == 0) && (d_events || n_events == 0))) {
        set_error("%s: bad argument: more events than rows, or a null pointer with rows to write or events to read", entry);
        return SP1HIP_ERROR_INVALID_ARGUMENT;
    }
    if (height == 0) return SP1HIP_SUCCESS;
    uint32_t* d_work = nullptr;
    SP1HIP_TRY(sp1hip_malloc_async((void**)&d_work, work_words * sizeof(uint32_t), stream));
    launch(d_work);
    const hipError_t launched = hipGetLastError();
    const int freed = sp1hip_free_async(d_work, stream);
    return launched != hipSuccess ? map_hip_error(launched, entry) : freed;
}

}  // namespace

extern "C" {

int sp1hip_tracegen_riscv_ed_add_width(void) { return tge::EdAdd::WIDTH; }
int sp1hip_tracegen_riscv_ed_decompress_width(void) { return tge::EdDecompress::WIDTH; }
int sp1hip_tracegen_riscv_uint256_ops_width(void) { return tge::Uint256Ops::WIDTH; }

int sp1hip_tracegen_riscv_ed_add(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    return two_phase_table(__func__, d_table, height, d_events, n_events, tge::EdAdd::Work::words(height, tge::EdAdd::OPS), stream, [&](uint32_t* d_work) {
        tge::launch_ed_add(d_table, height, d_events, n_events, d_work, tge::ed25519_modulus(), S(stream));
    });
}

int sp1hip_tracegen_riscv_ed_decompress(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    return two_phase_table(__func__, d_table, height, d_events, n_events, tge::EdDecompress::Work::words(height, tge::EdDecompress::OPS), stream,
                           [&](uint32_t* d_work) { tge::launch_ed_decompress(d_table, height, d_events, n_events, d_work, tge::ed25519_modulus(), S(stream)); });
}

int sp1hip_tracegen_riscv_uint256_ops(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    return tg::launch_rows(__func__, tge::uint256_ops_kernel, d_table, height, d_events, n_events, stream);
}

int sp1hip_precompile_touched_records(uint64_t* d_records, uint64_t records_capacity, const uint64_t* d_events, uint32_t n_events, uint32_t family,
                                      sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(family == tge::TOUCHED_ED_DECOMPRESS || family == tge::TOUCHED_UINT256_OPS,
                   "family: SP1HIP_RV64_FAMILY_ED_DECOMPRESS (13) or SP1HIP_RV64_FAMILY_UINT256_OPS (14); sp1hip_precompile_local_records states every other kind");
    const uint64_t total = (uint64_t)n_events * tge::touched_per_event(family);
    SP1HIP_REQUIRE(total <= 0x7fffffffull, "too many records");
    SP1HIP_REQUIRE(total <= records_capacity && (d_records || total == 0) && (d_events || n_events == 0), "bad argument");
    if (total == 0) return SP1HIP_SUCCESS;
    tge::launch_touched_records(d_records, (uint32_t)total, d_events, n_events, family, S(stream));
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}

}  // extern "C"
