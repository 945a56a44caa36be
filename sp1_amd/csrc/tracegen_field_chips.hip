// sp1_amd/csrc/tracegen_field_chips.hip — device trace generation for the twelve Weierstrass and Fp / Fp2 precompile chips behind
// SP1HIP_RV64_FAMILY_* 0..11 (Secp256r1 / Bn254 / Bls12381 AddAssign and DoubleAssign; Bn254 / Bls12381 FpOpAssign, Fp2AddSubAssign,
// Fp2MulAssign), one row per system call, from the executor's event records (sp1hip_rv64_precompile_events) instead of host-made
// tables. The reference fills these tables on the host and has no device filler for them.
//
// A table is made in two launches (tg_field_chip_rows.hpp has the rows and says why): phase A, one lane per row, writes the head
// columns and the FieldLtCols and leaves one record per FieldOpCols in a work buffer; phase B, one lane per (row, field operation),
// writes result, carry and witness from the records. The work buffer — (3N + 1) words per row and operation, [op][word][row] — is
// allocated and released inside the call, in stream order. The moduli, the curve's a and the witness offset are kernel arguments;
// nothing in the kernels knows a curve's form.
#include "device_ctx.hpp"
#include "tg_field_chip_rows.hpp"

using namespace sp1hip;

extern "C" {

int sp1hip_tracegen_riscv_field_chip_width(uint32_t family) {
    int width = -1;
    tgc::with_family(family, [&](auto shape, const auto&, const auto&, const char*) { width = decltype(shape)::WIDTH; });
    return width;
}

int sp1hip_tracegen_riscv_field_chip(uint32_t family, uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream) {
    if (family >= tgc::FAMILIES) {
        set_error("%s: family %u has no device filler: SP1HIP_RV64_FAMILY_* 0..11 (the curve and Fp / Fp2 chips) are made here, ed_add, ed_decompress and "
                  "uint256_ops (12..14) are not", __func__, family);
        return SP1HIP_ERROR_INVALID_ARGUMENT;
    }
    if (!(n_events <= height && (d_table || height == 0) && (d_events || n_events == 0))) {
        set_error("%s: bad argument: more events than rows, or a null pointer with rows to write or events to read", __func__);
        return SP1HIP_ERROR_INVALID_ARGUMENT;
    }
    if (height == 0) return SP1HIP_SUCCESS;
    int status = SP1HIP_SUCCESS;
    tgc::with_family(family, [&](auto shape, const auto& m, const auto& k, const char*) {
        using Shape = decltype(shape);
        uint32_t* d_work = nullptr;
        status = sp1hip_malloc_async((void**)&d_work, tgc::Work<Shape::LIMBS>::words(height, Shape::OPS) * sizeof(uint32_t), stream);
        if (status != SP1HIP_SUCCESS) return;
        tgc::launch_table<Shape>(d_table, height, d_events, n_events, d_work, m, k, S(stream));
        const hipError_t launched = hipGetLastError();
        const int freed = sp1hip_free_async(d_work, stream);
        status = launched != hipSuccess ? map_hip_error(launched, "field chip kernels") : freed;
    });
    return status;
}

}  // extern "C"
