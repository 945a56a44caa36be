// tests/native/riscv_core_rows.hip — the row functions of sp1_amd/csrc/tg_riscv_core_rows.hpp (included unchanged) behind a file
// interface, in their `host` form: the __host__ __device__ code compiled for the CPU. It never opens a GPU and never loads the
// library. tests/test_tracegen_riscv_core_host.py writes the inputs and checks every word; the device side is checked through
// sp1_amd.api by tests/test_gpu_tracegen_riscv_core.py.
//
//   riscv_core_rows host rows CHIP IN HEIGHT OUT      the table of CHIP = DivRem | AluX0 | MemoryLocal
//       IN:  DivRem, AluX0: n x 11 u64 (sp1hip_rv64_alu_event_t records); MemoryLocal: n x 5 u64 { addr, initial clk, initial
//            value, final clk, final value }; little-endian, n = file size / record size, n <= HEIGHT <= 2^20
//       OUT: width x HEIGHT u32, column-major [width][height], Montgomery words; rows >= n are the chip's padding rows
//   riscv_core_rows host global IN OUT                 the Global events of MemoryLocal records: 2 n x 9 i32, record i at rows 2 i, 2 i + 1
//   riscv_core_rows host layout                        the column constants of the three chips as text lines "chip key column"
//   riscv_core_rows host width                         "chip width" lines
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc -Iinclude ...
#include <string.h>

#include "rows_io.hpp"
#include "sp1hip.h"
#include "tg_riscv_core_rows.hpp"

namespace tg = sp1hip::tg;
static_assert(sizeof(tg::Ev) == sizeof(sp1hip_rv64_alu_event_t), "event layout");

enum { DIVREM = 0, ALU_X0 = 1, MEMORY_LOCAL = 2, N_CORE_CHIPS = 3 };
static const char* const NAMES[N_CORE_CHIPS] = {"DivRem", "AluX0", "MemoryLocal"};
static const int WIDTHS[N_CORE_CHIPS] = {tg::DIVREM_WIDTH, tg::ALU_X0_WIDTH, tg::MEMORY_LOCAL_WIDTH};
static const size_t RECORD_WORDS[N_CORE_CHIPS] = {11, 11, tg::MEMORY_LOCAL_RECORD_WORDS};

// what the kernels do for their lanes, as a host loop: tg::host_rows (tg_row_kernel.hpp), and for DivRem the kernel's own body
static void host_rows(int chip, uint32_t* out, uint32_t height, const uint64_t* in, uint32_t n) {
    const tg::Ev* ev = reinterpret_cast<const tg::Ev*>(in);
    if (chip == DIVREM) for (uint32_t row = 0; row < height; row++) tg::divrem_row(out, height, ev, n, row);
    else if (chip == ALU_X0) tg::host_rows<tg::AluX0>(out, height, ev, n);
    else tg::host_rows<tg::MemoryLocal>(out, height, in, n, (int32_t*)nullptr);
}

static void put(const char* chip, const char* key, int v) { printf("%s %s %d\n", chip, key, v); }

static void access_cols(const char* n, const char* name, int at) {
    char key[64];
    snprintf(key, sizeof key, "adapter.%s.prev_value", name); put(n, key, at);
    snprintf(key, sizeof key, "adapter.%s.prev_low", name); put(n, key, at + 4);
    snprintf(key, sizeof key, "adapter.%s.diff_low_limb", name); put(n, key, at + 5);
}
static void state_and_ab(const char* n) {
    put(n, "state.clk_high", 0); put(n, "state.clk_16_24", 1); put(n, "state.clk_0_16", 2); put(n, "state.pc", 3);
    put(n, "adapter.op_a", 6); access_cols(n, "op_a_memory", 7); put(n, "adapter.op_a_0", 13);
    put(n, "adapter.op_b", 14); access_cols(n, "op_b_memory", 15); put(n, "adapter.op_c", 21);
}
static void mul_cols(const char* n, const char* name, int at) {
    namespace c = tg::col;
    const struct { const char* key; int off; } cols[] = {{"carry", c::MUL_CARRY}, {"product", c::MUL_PRODUCT}, {"b_lower_byte.low_bytes", c::MUL_B_LOW},
        {"c_lower_byte.low_bytes", c::MUL_C_LOW}, {"b_msb", c::MUL_B_MSB}, {"c_msb", c::MUL_C_MSB}, {"product_msb", c::MUL_PRODUCT_MSB},
        {"b_sign_extend", c::MUL_B_SIGN_EXTEND}, {"c_sign_extend", c::MUL_C_SIGN_EXTEND}};
    char key[96];
    for (const auto& k : cols) { snprintf(key, sizeof key, "%s.%s", name, k.key); put(n, key, at + k.off); }
}
static void is_zero_word_cols(const char* n, const char* name, int at) {
    namespace c = tg::col;
    char key[96];
    for (int i = 0; i < 4; i++) {
        snprintf(key, sizeof key, "%s.is_zero_limb.%d.inverse", name, i); put(n, key, at + c::IZW_LIMB + 2 * i);
        snprintf(key, sizeof key, "%s.is_zero_limb.%d.result", name, i); put(n, key, at + c::IZW_LIMB + 2 * i + 1);
    }
    snprintf(key, sizeof key, "%s.is_zero_first_half", name); put(n, key, at + c::IZW_FIRST_HALF);
    snprintf(key, sizeof key, "%s.is_zero_second_half", name); put(n, key, at + c::IZW_SECOND_HALF);
    snprintf(key, sizeof key, "%s.result", name); put(n, key, at + c::IZW_RESULT);
}
// The column constants the row functions use: CPUState and the R / ALU adapters are literals of tg_riscv_rows.hpp (fill_state,
// fill_r, fill_alu), restated here; LtOperationUnsigned is fill_lt's order; everything else has a name in tg::col.
static int layout() {
    namespace c = tg::col;
    const char* n = "DivRem";
    put(n, "width", tg::DIVREM_WIDTH);
    state_and_ab(n); access_cols(n, "op_c_memory", 22);
    put(n, "a", c::DR_A); put(n, "b", c::DR_B); put(n, "c", c::DR_C); put(n, "quotient", c::DR_QUOTIENT); put(n, "quotient_comp", c::DR_QUOTIENT_COMP);
    put(n, "remainder_comp", c::DR_REMAINDER_COMP); put(n, "remainder", c::DR_REMAINDER); put(n, "abs_remainder", c::DR_ABS_REMAINDER);
    put(n, "abs_c", c::DR_ABS_C); put(n, "max_abs_c_or_1", c::DR_MAX_ABS_C_OR_1); put(n, "c_times_quotient", c::DR_C_TIMES_QUOTIENT);
    mul_cols(n, "c_times_quotient_lower", c::DR_CTQ_LOWER); mul_cols(n, "c_times_quotient_upper", c::DR_CTQ_UPPER);
    put(n, "c_neg_operation.value", c::DR_C_NEG_OP); put(n, "rem_neg_operation.value", c::DR_REM_NEG_OP);
    put(n, "remainder_lt_operation.bit", c::DR_REMAINDER_LT); put(n, "remainder_lt_operation.u16_flags", c::DR_REMAINDER_LT + 1);
    put(n, "remainder_lt_operation.not_eq_inv", c::DR_REMAINDER_LT + 5); put(n, "remainder_lt_operation.comparison_limbs", c::DR_REMAINDER_LT + 6);
    put(n, "carry", c::DR_CARRY);
    is_zero_word_cols(n, "is_c_0", c::DR_IS_C_0);
    put(n, "is_div", c::DR_IS_DIV); put(n, "is_divu", c::DR_IS_DIVU); put(n, "is_rem", c::DR_IS_REM); put(n, "is_remu", c::DR_IS_REMU);
    put(n, "is_divw", c::DR_IS_DIVW); put(n, "is_remw", c::DR_IS_REMW); put(n, "is_divuw", c::DR_IS_DIVUW); put(n, "is_remuw", c::DR_IS_REMUW);
    put(n, "is_overflow", c::DR_IS_OVERFLOW);
    is_zero_word_cols(n, "is_overflow_b", c::DR_IS_OVERFLOW_B); is_zero_word_cols(n, "is_overflow_c", c::DR_IS_OVERFLOW_C);
    put(n, "b_msb", c::DR_B_MSB); put(n, "rem_msb", c::DR_REM_MSB); put(n, "c_msb", c::DR_C_MSB); put(n, "quot_msb", c::DR_QUOT_MSB);
    put(n, "b_neg", c::DR_B_NEG); put(n, "b_neg_not_overflow", c::DR_B_NEG_NOT_OVERFLOW); put(n, "b_not_neg_not_overflow", c::DR_B_NOT_NEG_NOT_OVERFLOW);
    put(n, "is_real_not_word", c::DR_IS_REAL_NOT_WORD); put(n, "rem_neg", c::DR_REM_NEG); put(n, "c_neg", c::DR_C_NEG);
    put(n, "abs_c_alu_event", c::DR_ABS_C_ALU_EVENT); put(n, "abs_rem_alu_event", c::DR_ABS_REM_ALU_EVENT); put(n, "is_real", c::DR_IS_REAL);
    put(n, "remainder_check_multiplicity", c::DR_REMAINDER_CHECK_MULTIPLICITY);
    n = "AluX0";
    put(n, "width", tg::ALU_X0_WIDTH);
    state_and_ab(n); access_cols(n, "op_c_memory", 25); put(n, "adapter.imm_c", 31);
    put(n, "opcode", c::X0_OPCODE); put(n, "is_real", c::X0_IS_REAL);
    n = "MemoryLocal";
    put(n, "width", tg::MEMORY_LOCAL_WIDTH);
    put(n, "addr", c::ML_ADDR); put(n, "initial_clk_high", c::ML_INITIAL_CLK_HIGH); put(n, "final_clk_high", c::ML_FINAL_CLK_HIGH);
    put(n, "initial_clk_low", c::ML_INITIAL_CLK_LOW); put(n, "final_clk_low", c::ML_FINAL_CLK_LOW); put(n, "initial_value", c::ML_INITIAL_VALUE);
    put(n, "final_value", c::ML_FINAL_VALUE); put(n, "initial_value_lower", c::ML_INITIAL_VALUE_LOWER);
    put(n, "initial_value_upper", c::ML_INITIAL_VALUE_UPPER); put(n, "final_value_lower", c::ML_FINAL_VALUE_LOWER);
    put(n, "final_value_upper", c::ML_FINAL_VALUE_UPPER); put(n, "is_real", c::ML_IS_REAL);
    return 0;
}

static int usage(const char* me) {
    fprintf(stderr, "usage: %s host rows CHIP IN HEIGHT OUT\n       %s host global IN OUT\n       %s host layout|width\n", me, me, me);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 3) return usage(argv[0]);
    const char* what = argv[2];
    if (strcmp(argv[1], "host")) { fprintf(stderr, "unknown form %s: this program has only the host form\n", argv[1]); return 1; }
    if (argc == 3 && !strcmp(what, "layout")) return layout();
    if (argc == 3 && !strcmp(what, "width")) {
        for (int chip = 0; chip < N_CORE_CHIPS; chip++) printf("%s %d\n", NAMES[chip], WIDTHS[chip]);
        return 0;
    }
    if (argc == 5 && !strcmp(what, "global")) {
        std::vector<uint64_t> rec;
        if (!read_records(argv[3], tg::MEMORY_LOCAL_RECORD_WORDS, rec)) return 1;
        const uint32_t n = (uint32_t)(rec.size() / tg::MEMORY_LOCAL_RECORD_WORDS);
        std::vector<int32_t> ev((size_t)n * 2 * tg::GLOBAL_EVENT_WORDS);
        std::vector<uint32_t> table((size_t)tg::MEMORY_LOCAL_WIDTH * n);       // the events come with the rows
        tg::host_rows<tg::MemoryLocal>(table.data(), n, rec.data(), n, ev.data());
        return write_out(argv[4], ev.data(), ev.size() * 4);
    }
    if (strcmp(what, "rows") || argc != 7) return usage(argv[0]);
    int chip = -1;
    for (int k = 0; k < N_CORE_CHIPS; k++) if (!strcmp(argv[3], NAMES[k])) chip = k;
    if (chip < 0) { fprintf(stderr, "unknown chip %s\n", argv[3]); return 1; }
    uint32_t height, n;
    std::vector<uint64_t> in;
    if (!read_rows_input(argv[5], argv[4], RECORD_WORDS[chip], height, in, n)) return 1;
    std::vector<uint32_t> out((size_t)WIDTHS[chip] * height, 0xeeeeeeeeu);
    host_rows(chip, out.data(), height, in.data(), n);
    if (write_out(argv[6], out.data(), out.size() * 4)) return 1;
    fprintf(stderr, "riscv_core_rows host rows %s: %d x %u words\n", NAMES[chip], WIDTHS[chip], height);
    return 0;
}
