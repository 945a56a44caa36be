// tests/native/riscv_mem_rows.hip — the row functions of sp1_amd/csrc/tg_riscv_mem_rows.hpp (included unchanged) behind a file
// interface, in one of two forms: `host` (the __host__ __device__ code compiled for the CPU; never opens a GPU, never loads the
// library) and `device` (the real kernels: sp1hip_tracegen_riscv_mem of sp1_amd/lib/libsp1hip.so, loaded at run time from beside
// this program's tree). tests/test_tracegen_riscv_mem_host.py (CPU) and tests/test_gpu_tracegen_riscv_mem.py write the inputs and
// check every word.
//
//   riscv_mem_rows FORM rows CHIP EVENTS HEIGHT OUT   the table of chip number CHIP (SP1HIP_RV64_MEM_CHIP_*: 0..8)
//       EVENTS: n x 12 u64 (sp1hip_rv64_mem_event_t records, little-endian; n = file size / 96, n <= HEIGHT <= 2^20)
//       OUT:    width x HEIGHT u32, column-major [width][height], Montgomery words; rows >= n are zero rows
//   riscv_mem_rows host layout                        the column constants of all nine chips as text lines "chip key column"
//   riscv_mem_rows host width                         "chip width" lines
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc -Iinclude ...
#include <string.h>

#include "rows_io.hpp"
#include "sp1hip.h"
#include "tg_riscv_mem_rows.hpp"

namespace tg = sp1hip::tg;
static_assert(sizeof(tg::MemEv) == sizeof(sp1hip_rv64_mem_event_t), "event layout");

static const char* const NAMES[tg::N_MEM_CHIPS] = {"LoadByte", "LoadHalf", "LoadWord", "LoadDouble", "LoadX0", "StoreByte", "StoreHalf", "StoreWord",
                                                   "StoreDouble"};

// what the kernel does for its lanes, as a host loop: tg::host_rows (tg_row_kernel.hpp)
static void host_rows_of(int chip, uint32_t* out, uint32_t height, const tg::MemEv* events, uint32_t n) {
    switch (chip) {
#define ROWS(C) case tg::C: tg::host_rows<tg::LoadStoreChip<tg::C>>(out, height, events, n); break
        ROWS(LOAD_BYTE); ROWS(LOAD_HALF); ROWS(LOAD_WORD); ROWS(LOAD_DOUBLE); ROWS(LOAD_X0);
        ROWS(STORE_BYTE); ROWS(STORE_HALF); ROWS(STORE_WORD); ROWS(STORE_DOUBLE);
#undef ROWS
    }
}

static void put(const char* chip, const char* key, int v) { printf("%s %s %d\n", chip, key, v); }

static void access_cols(const char* n, const char* name, int at) {
    char key[64];
    snprintf(key, sizeof key, "adapter.%s.prev_value", name); put(n, key, at);
    snprintf(key, sizeof key, "adapter.%s.prev_low", name); put(n, key, at + 4);
    snprintf(key, sizeof key, "adapter.%s.diff_low_limb", name); put(n, key, at + 5);
}
// The column constants the row functions use: CPUState and the I adapter are literals of tg_riscv_rows.hpp (fill_state, fill_i),
// restated here; everything behind them has a name in tg::col.
static int layout() {
    namespace c = tg::col;
    for (int chip = 0; chip < tg::N_MEM_CHIPS; chip++) {
        const char* n = NAMES[chip];
        put(n, "width", tg::mem_width_of(chip));
        put(n, "state.clk_high", 0); put(n, "state.clk_16_24", 1); put(n, "state.clk_0_16", 2); put(n, "state.pc", 3);
        put(n, "adapter.op_a", 6); access_cols(n, "op_a_memory", 7); put(n, "adapter.op_a_0", 13);
        put(n, "adapter.op_b", 14); access_cols(n, "op_b_memory", 15); put(n, "adapter.op_c_imm", 21);
        put(n, "address.value", c::MEM_ADDRESS); put(n, "address.top_two_limb_inv", c::MEM_ADDRESS_INV);
        put(n, "memory_access.prev_value", c::MEM_PREV_VALUE); put(n, "memory_access.prev_high", c::MEM_PREV_HIGH);
        put(n, "memory_access.prev_low", c::MEM_PREV_LOW); put(n, "memory_access.compare_low", c::MEM_COMPARE_LOW);
        put(n, "memory_access.diff_low_limb", c::MEM_DIFF_LOW); put(n, "memory_access.diff_high_limb", c::MEM_DIFF_HIGH);
        put(n, chip == tg::LOAD_DOUBLE || chip == tg::STORE_DOUBLE ? "is_real" : "offset_bit", c::MEM_OWN);
    }
    const char* s = "LoadByte";
    put(s, "selected_limb", c::LB_SELECTED_LIMB); put(s, "selected_limb_low_byte", c::LB_SELECTED_LIMB_LOW_BYTE); put(s, "selected_byte", c::LB_SELECTED_BYTE);
    put(s, "msb", c::LB_MSB); put(s, "is_lb", c::LB_IS_LB); put(s, "is_lbu", c::LB_IS_LBU);
    s = "LoadHalf";
    put(s, "selected_half", c::LH_SELECTED_HALF); put(s, "msb", c::LH_MSB); put(s, "is_lh", c::LH_IS_LH); put(s, "is_lhu", c::LH_IS_LHU);
    s = "LoadWord";
    put(s, "selected_word", c::LW_SELECTED_WORD); put(s, "msb", c::LW_MSB); put(s, "is_lw", c::LW_IS_LW); put(s, "is_lwu", c::LW_IS_LWU);
    s = "LoadX0";
    const char* const loads[] = {"is_lb", "is_lbu", "is_lh", "is_lhu", "is_lw", "is_lwu", "is_ld"};
    for (int i = 0; i < 7; i++) put(s, loads[i], c::LX0_IS_LB + i);
    s = "StoreByte";
    put(s, "mem_limb", c::SB_MEM_LIMB); put(s, "mem_limb_low_byte", c::SB_MEM_LIMB_LOW_BYTE); put(s, "register_low_byte", c::SB_REGISTER_LOW_BYTE);
    put(s, "increment", c::SB_INCREMENT); put(s, "store_value", c::SB_STORE_VALUE); put(s, "is_real", c::SB_IS_REAL);
    s = "StoreHalf";
    put(s, "store_value", c::SH_STORE_VALUE); put(s, "is_real", c::SH_IS_REAL);
    s = "StoreWord";
    put(s, "store_value", c::SW_STORE_VALUE); put(s, "is_real", c::SW_IS_REAL);
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
        for (int chip = 0; chip < tg::N_MEM_CHIPS; chip++) printf("%s %d\n", NAMES[chip], tg::mem_width_of(chip));
        return 0;
    }
    if (strcmp(what, "rows") || argc != 7) return usage(argv[0]);
#if !defined(__HIPCC__)
    if (device) { fprintf(stderr, "built without a device compiler: only the host form\n"); return 1; }
#endif
    char* end = nullptr;
    const long chip = strtol(argv[3], &end, 10);
    if (*end || end == argv[3] || chip < 0 || chip >= tg::N_MEM_CHIPS) { fprintf(stderr, "unknown chip %s\n", argv[3]); return 1; }
    uint32_t height, n;
    std::vector<uint64_t> words;
    if (!read_rows_input(argv[5], argv[4], sizeof(tg::MemEv) / 8, height, words, n)) return 1;
    const int width = tg::mem_width_of((int)chip);
    std::vector<uint32_t> out((size_t)width * height, 0xeeeeeeeeu);
    int st = 0;
    if (host) host_rows_of((int)chip, out.data(), height, reinterpret_cast<const tg::MemEv*>(words.data()), n);
#if defined(__HIPCC__)
    else if (height) st = device_rows("sp1hip_tracegen_riscv_mem", (int)chip, out, height, words, n);
#endif
    if (st) return st;
    if (write_out(argv[6], out.data(), out.size() * 4)) return 1;
    fprintf(stderr, "riscv_mem_rows %s rows %s: %d x %u words\n", form, NAMES[chip], width, height);
    return 0;
}
