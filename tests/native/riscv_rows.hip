// tests/native/riscv_rows.hip — the row functions of sp1_amd/csrc/tg_riscv_rows.hpp (included unchanged) behind a file interface, in
// one of two forms: `host` (the __host__ __device__ code compiled for the CPU; never opens a GPU, never loads the library) and
// `device` (the real kernels: sp1hip_tracegen_riscv_alu of sp1_amd/lib/libsp1hip.so, loaded at run time from beside this program's
// tree). tests/test_tracegen_riscv_host.py (CPU) and tests/test_gpu_tracegen_riscv_more.py write the inputs and check every word.
//
//   riscv_rows FORM rows CHIP EVENTS HEIGHT OUT   the table of chip number CHIP (SP1HIP_RV64_CHIP_*: 0..13)
//       EVENTS: n x 11 u64 (sp1hip_rv64_alu_event_t records, little-endian; n = file size / 88, n <= HEIGHT <= 2^20)
//       OUT:    width x HEIGHT u32, column-major [width][height], Montgomery words; rows >= n are the chip's padding rows
//   riscv_rows host layout                        the column constants of all fourteen chips as text lines "chip key column"
//   riscv_rows host width                         "chip width" lines
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc -Iinclude ...
#include <string.h>

#include "rows_io.hpp"
#include "sp1hip.h"
#include "tg_riscv_rows.hpp"

namespace tg = sp1hip::tg;
static_assert(sizeof(tg::Ev) == sizeof(sp1hip_rv64_alu_event_t), "event layout");

static const char* const NAMES[tg::N_CHIPS] = {"Add", "Addi", "Sub", "Addw", "Subw", "Mul", "ShiftRight", "Branch",
                                               "Bitwise", "Lt", "ShiftLeft", "UType", "Jal", "Jalr"};

// what the kernel does for its lanes, as a host loop: tg::host_rows (tg_row_kernel.hpp)
static void host_rows_of(int chip, uint32_t* out, uint32_t height, const tg::Ev* events, uint32_t n) {
    switch (chip) {
#define ROWS(C) case tg::C: tg::host_rows<tg::AluChip<tg::C>>(out, height, events, n); break
        ROWS(ADD); ROWS(ADDI); ROWS(SUB); ROWS(ADDW); ROWS(SUBW); ROWS(MUL); ROWS(SHIFT_RIGHT); ROWS(BRANCH);
        ROWS(BITWISE); ROWS(LT); ROWS(SHIFT_LEFT); ROWS(UTYPE); ROWS(JAL); ROWS(JALR);
#undef ROWS
    }
}

static void put(const char* chip, const char* key, int v) { printf("%s %s %d\n", chip, key, v); }

// The column constants the row functions use. The shared groups and the eight first chips are written as literals in
// tg_riscv_rows.hpp (fill_state .. fill_lt and the heads of fill_row's branches): they are restated here; the six later chips use
// the names of tg::col.
static void lt_cols(const char* n, const char* name, int at) {
    char key[64];
    const char* const parts[] = {"result.bit", "result.u16_flags", "result.not_eq_inv", "result.comparison_limbs", "b_msb", "c_msb"};
    const int off[] = {0, 1, 5, 6, 8, 9};
    for (int i = 0; i < 6; i++) { snprintf(key, sizeof key, "%s.%s", name, parts[i]); put(n, key, at + off[i]); }
}
static void access_cols(const char* n, const char* name, int at) {
    char key[64];
    snprintf(key, sizeof key, "adapter.%s.prev_value", name); put(n, key, at);
    snprintf(key, sizeof key, "adapter.%s.prev_low", name); put(n, key, at + 4);
    snprintf(key, sizeof key, "adapter.%s.diff_low_limb", name); put(n, key, at + 5);
}
static int layout() {
    for (int chip = 0; chip < tg::N_CHIPS; chip++) {
        const char* n = NAMES[chip];
        put(n, "width", tg::width_of(chip));
        put(n, "state.clk_high", 0); put(n, "state.clk_16_24", 1); put(n, "state.clk_0_16", 2); put(n, "state.pc", 3);
        put(n, "adapter.op_a", 6); access_cols(n, "op_a_memory", 7); put(n, "adapter.op_a_0", 13);
        const bool j = chip == tg::UTYPE || chip == tg::JAL;
        const bool r = chip == tg::ADD || chip == tg::SUB || chip == tg::SUBW || chip == tg::MUL;
        const bool i = chip == tg::ADDI || chip == tg::BRANCH || chip == tg::JALR;
        if (j) { put(n, "adapter.op_b_imm", 14); put(n, "adapter.op_c_imm", 18); }
        else { put(n, "adapter.op_b", 14); access_cols(n, "op_b_memory", 15); }
        if (r) { put(n, "adapter.op_c", 21); access_cols(n, "op_c_memory", 22); }
        else if (i) put(n, "adapter.op_c_imm", 21);
        else if (!j) { put(n, "adapter.op_c", 21); access_cols(n, "op_c_memory", 25); put(n, "adapter.imm_c", 31); }
    }
    put("Add", "value", 28); put("Add", "is_real", 32);
    put("Sub", "value", 28); put("Sub", "is_real", 32);
    put("Addi", "value", 25); put("Addi", "is_real", 29);
    put("Addw", "value", 32); put("Addw", "msb", 34); put("Addw", "is_real", 35);
    put("Subw", "value", 28); put("Subw", "msb", 30); put("Subw", "is_real", 31);
    put("Mul", "a", 28); put("Mul", "mul.carry", 32); put("Mul", "mul.product", 48); put("Mul", "mul.b_lower_byte.low_bytes", 64);
    put("Mul", "mul.c_lower_byte.low_bytes", 68); put("Mul", "mul.b_msb", 72); put("Mul", "mul.c_msb", 73); put("Mul", "mul.product_msb", 74);
    put("Mul", "mul.b_sign_extend", 75); put("Mul", "mul.c_sign_extend", 76); put("Mul", "is_mul", 77); put("Mul", "is_mulh", 78);
    put("Mul", "is_mulhu", 79); put("Mul", "is_mulhsu", 80); put("Mul", "is_mulw", 81);
    const char* s = "ShiftRight";
    put(s, "a", 32); put(s, "b_msb", 36); put(s, "srw_msb", 37); put(s, "c_bits", 38); put(s, "sra_msb_v0123", 44); put(s, "v_0123", 45);
    put(s, "v_012", 46); put(s, "v_01", 47); put(s, "lower_limb", 48); put(s, "higher_limb", 52); put(s, "limb_result", 56); put(s, "shift_u16", 60);
    put(s, "is_srl", 64); put(s, "is_sra", 65); put(s, "is_srlw", 66); put(s, "is_sraw", 67); put(s, "is_w_imm", 68);
    s = "Branch";
    put(s, "next_pc", 25); put(s, "is_beq", 28); put(s, "is_bne", 29); put(s, "is_blt", 30); put(s, "is_bge", 31); put(s, "is_bltu", 32);
    put(s, "is_bgeu", 33); put(s, "is_branching", 34); lt_cols(s, "cmp", 35);
    namespace c = tg::col;
    s = "Bitwise";
    put(s, "b_low_bytes.low_bytes", c::BITWISE_B_LOW); put(s, "c_low_bytes.low_bytes", c::BITWISE_C_LOW); put(s, "result", c::BITWISE_RESULT);
    put(s, "is_xor", c::BITWISE_IS_XOR); put(s, "is_or", c::BITWISE_IS_OR); put(s, "is_and", c::BITWISE_IS_AND);
    s = "Lt";
    put(s, "is_slt", c::LT_IS_SLT); put(s, "is_sltu", c::LT_IS_SLTU); lt_cols(s, "lt", c::LT_LT);
    s = "ShiftLeft";
    put(s, "a", c::SLL_A); put(s, "c_bits", c::SLL_C_BITS); put(s, "v_01", c::SLL_V_01); put(s, "v_012", c::SLL_V_012); put(s, "v_0123", c::SLL_V_0123);
    put(s, "shift_u16", c::SLL_SHIFT_U16); put(s, "lower_limb", c::SLL_LOWER); put(s, "higher_limb", c::SLL_HIGHER); put(s, "limb_result", c::SLL_RESULT);
    put(s, "sllw_msb", c::SLL_MSB); put(s, "is_sll", c::SLL_IS_SLL); put(s, "is_sllw", c::SLL_IS_SLLW); put(s, "is_sllw_imm", c::SLL_IS_SLLW_IMM);
    s = "UType";
    put(s, "addend", c::UTYPE_ADDEND); put(s, "value", c::UTYPE_VALUE); put(s, "is_auipc", c::UTYPE_IS_AUIPC); put(s, "is_real", c::UTYPE_IS_REAL);
    s = "Jal";
    put(s, "next_pc", c::JAL_NEXT_PC); put(s, "op_a_value", c::JAL_OP_A_VALUE); put(s, "is_real", c::JAL_IS_REAL);
    s = "Jalr";
    put(s, "is_real", c::JALR_IS_REAL); put(s, "next_pc", c::JALR_NEXT_PC); put(s, "op_a_value", c::JALR_OP_A_VALUE); put(s, "lsb", c::JALR_LSB);
    return 0;
}

static int usage(const char* me) {
    fprintf(stderr, "usage: %s host|device rows CHIP EVENTS HEIGHT OUT\n       %s host layout|width\n", me, me);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 3) return usage(argv[0]);
    const char *form = argv[1], *what = argv[2];
    const bool host = !strcmp(form, "host"), device = !strcmp(form, "device");
    if (!host && !device) { fprintf(stderr, "unknown form %s\n", form); return 1; }
    if (host && argc == 3 && !strcmp(what, "layout")) return layout();
    if (host && argc == 3 && !strcmp(what, "width")) {
        for (int chip = 0; chip < tg::N_CHIPS; chip++) printf("%s %d\n", NAMES[chip], tg::width_of(chip));
        return 0;
    }
    if (strcmp(what, "rows") || argc != 7) return usage(argv[0]);
#if !defined(__HIPCC__)
    if (device) { fprintf(stderr, "built without a device compiler: only the host form\n"); return 1; }
#endif
    char* end = nullptr;
    const long chip = strtol(argv[3], &end, 10);
    if (*end || end == argv[3] || chip < 0 || chip >= tg::N_CHIPS) { fprintf(stderr, "unknown chip %s\n", argv[3]); return 1; }
    uint32_t height, n;
    std::vector<uint64_t> words;
    if (!read_rows_input(argv[5], argv[4], sizeof(tg::Ev) / 8, height, words, n)) return 1;
    const int width = tg::width_of((int)chip);
    std::vector<uint32_t> out((size_t)width * height, 0xeeeeeeeeu);
    int st = 0;
    if (host) host_rows_of((int)chip, out.data(), height, reinterpret_cast<const tg::Ev*>(words.data()), n);
#if defined(__HIPCC__)
    else if (height) st = device_rows("sp1hip_tracegen_riscv_alu", (int)chip, out, height, words, n);
#endif
    if (st) return st;
    if (write_out(argv[6], out.data(), out.size() * 4)) return 1;
    fprintf(stderr, "riscv_rows %s rows %s: %d x %u words\n", form, NAMES[chip], width, height);
    return 0;
}
