// tests/native/riscv_sys_rows.hip — the event partition of sp1_amd/csrc/tg_rv64_partition.hpp and the row functions of
// sp1_amd/csrc/tg_riscv_sys_rows.hpp (both included unchanged) behind a file interface, in their `host` form: the __host__
// __device__ code compiled for the CPU. It never opens a GPU and never loads the library. tests/test_rv64_partition_host.py and
// tests/test_tracegen_riscv_sys_host.py write the inputs and check every word; the device side is checked through sp1_amd.api by
// tests/test_gpu_rv64_partition.py and tests/test_gpu_device_core_shard.py.
//
//   riscv_sys_rows host partition IN OUT              the partition of n x 20 u64 executor records (little-endian)
//       OUT: 29 u64 record counts, then the record arena: bin b's records at the sum of the earlier bins' count x words
//   riscv_sys_rows host rows CHIP IN HEIGHT OUT       the table of CHIP = SyscallInstrs | SyscallCore | StateBump | MemoryBump
//       IN:  SyscallInstrs, SyscallCore: n x 11 u64 (sp1hip_rv64_alu_event_t); StateBump, MemoryBump: n x 4 u64; n <= HEIGHT <= 2^20
//       OUT: width x HEIGHT u32, column-major [width][height], Montgomery words; rows >= n are zero
//   riscv_sys_rows host global IN OUT                 the Global events of SyscallCore records: n x 9 i32
//   riscv_sys_rows host layout                        the column constants of the four chips as text lines "chip key column"
//   riscv_sys_rows host width                         "chip width" lines
//   riscv_sys_rows host bins                          "bin words" lines
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc -Iinclude ...
#include <string.h>

#include "rows_io.hpp"
#include "sp1hip.h"
#include "tg_riscv_sys_rows.hpp"
#include "tg_rv64_partition.hpp"

namespace tg = sp1hip::tg;
static_assert(sizeof(tg::Ev) == sizeof(sp1hip_rv64_alu_event_t), "event layout");
static_assert(sizeof(tg::RawEv) == 8 * tg::RAW_EV_WORDS, "event layout");
static_assert(tg::BINS == SP1HIP_RV64_BINS, "bins");

enum { SYSCALL_INSTRS = 0, SYSCALL_CORE = 1, STATE_BUMP = 2, MEMORY_BUMP = 3, N_SYS_CHIPS = 4 };
static const char* const NAMES[N_SYS_CHIPS] = {"SyscallInstrs", "SyscallCore", "StateBump", "MemoryBump"};
static const int WIDTHS[N_SYS_CHIPS] = {tg::SYSCALL_INSTRS_WIDTH, tg::SYSCALL_CORE_WIDTH, tg::STATE_BUMP_WIDTH, tg::MEMORY_BUMP_WIDTH};
static const size_t RECORD_WORDS[N_SYS_CHIPS] = {11, 11, tg::STATE_BUMP_RECORD_WORDS, tg::MEMORY_BUMP_RECORD_WORDS};

// what the kernels do for their lanes, as a host loop: tg::host_rows (tg_row_kernel.hpp)
static void host_rows(int chip, uint32_t* out, uint32_t height, const uint64_t* in, uint32_t n) {
    const tg::Ev* ev = reinterpret_cast<const tg::Ev*>(in);
    if (chip == SYSCALL_INSTRS) tg::host_rows<tg::SyscallInstrs>(out, height, ev, n);
    else if (chip == SYSCALL_CORE) tg::host_rows<tg::SyscallCore>(out, height, ev, n, (int32_t*)nullptr);
    else if (chip == STATE_BUMP) tg::host_rows<tg::StateBump>(out, height, in, n);
    else tg::host_rows<tg::MemoryBump>(out, height, in, n);
}

// the partition by its definition: every event in order, each record appended to its bin
static void host_partition(const uint64_t* in, size_t n, std::vector<uint64_t> (&bins)[tg::BINS]) {
    for (size_t i = 0; i < n; i++) {
        tg::RawEv e;
        memcpy(&e, in + i * tg::RAW_EV_WORDS, sizeof e);
        const int bin = tg::bin_of(e.op, e.op_a);
        if (bin == tg::BIN_NONE) continue;
        const tg::Extra x = tg::extra_of(e, bin);
        uint64_t o[tg::MEM_WORDS];
        if (bin >= tg::BIN_MEM0 && bin < tg::BIN_DIVREM) {
            tg::pack_mem(o, e);
            bins[bin].insert(bins[bin].end(), o, o + tg::MEM_WORDS);
        } else {
            tg::pack_alu(o, e);
            bins[bin].insert(bins[bin].end(), o, o + tg::ALU_WORDS);
            if (x.syscall_core) bins[tg::BIN_SYSCALL_CORE].insert(bins[tg::BIN_SYSCALL_CORE].end(), o, o + tg::ALU_WORDS);
        }
        if (x.state_bump) {
            tg::pack_state_bump(o, e, bin);
            bins[tg::BIN_STATE_BUMP].insert(bins[tg::BIN_STATE_BUMP].end(), o, o + tg::STATE_BUMP_WORDS);
        }
        for (int slot = 0; slot < 3; slot++)
            if (x.bumps & (1u << slot)) {
                tg::pack_memory_bump(o, e, slot);
                bins[tg::BIN_MEMORY_BUMP].insert(bins[tg::BIN_MEMORY_BUMP].end(), o, o + tg::MEMORY_BUMP_WORDS);
            }
    }
}

static void put(const char* chip, const char* key, int v) { printf("%s %s %d\n", chip, key, v); }

static void access_cols(const char* n, const char* name, int at) {
    char key[64];
    snprintf(key, sizeof key, "adapter.%s.prev_value", name); put(n, key, at);
    snprintf(key, sizeof key, "adapter.%s.prev_low", name); put(n, key, at + 4);
    snprintf(key, sizeof key, "adapter.%s.diff_low_limb", name); put(n, key, at + 5);
}
static void is_zero_cols(const char* n, const char* name, int at) {
    char key[64];
    snprintf(key, sizeof key, "%s.inverse", name); put(n, key, at);
    snprintf(key, sizeof key, "%s.result", name); put(n, key, at + 1);
}
// The column constants the row functions use: CPUState and the R adapter are literals of tg_riscv_rows.hpp (fill_state, fill_r),
// restated here; everything else has a name in tg::col.
static int layout() {
    namespace c = tg::col;
    const char* n = "SyscallInstrs";
    put(n, "width", tg::SYSCALL_INSTRS_WIDTH);
    put(n, "state.clk_high", 0); put(n, "state.clk_16_24", 1); put(n, "state.clk_0_16", 2); put(n, "state.pc", 3);
    put(n, "adapter.op_a", 6); access_cols(n, "op_a_memory", 7); put(n, "adapter.op_a_0", 13);
    put(n, "adapter.op_b", 14); access_cols(n, "op_b_memory", 15); put(n, "adapter.op_c", 21); access_cols(n, "op_c_memory", 22);
    put(n, "next_pc", c::SI_NEXT_PC); put(n, "is_halt", c::SI_IS_HALT); put(n, "op_a_value", c::SI_OP_A_VALUE);
    put(n, "a_low_bytes.low_bytes", c::SI_A_LOW_BYTES);
    is_zero_cols(n, "is_enter_unconstrained", c::SI_IS_ENTER_UNCONSTRAINED); is_zero_cols(n, "is_hint_len", c::SI_IS_HINT_LEN);
    is_zero_cols(n, "is_halt_check", c::SI_IS_HALT_CHECK); is_zero_cols(n, "is_commit", c::SI_IS_COMMIT);
    is_zero_cols(n, "is_commit_deferred_proofs", c::SI_IS_COMMIT_DEFERRED_PROOFS);
    put(n, "index_bitmap", c::SI_INDEX_BITMAP); put(n, "expected_public_values_digest", c::SI_EXPECTED_DIGEST);
    put(n, "op_b_range_check", c::SI_OP_B_RANGE_CHECK); put(n, "op_c_range_check", c::SI_OP_C_RANGE_CHECK); put(n, "is_real", c::SI_IS_REAL);
    n = "SyscallCore";
    put(n, "width", tg::SYSCALL_CORE_WIDTH);
    put(n, "clk_high", c::SC_CLK_HIGH); put(n, "clk_low", c::SC_CLK_LOW); put(n, "syscall_id", c::SC_SYSCALL_ID); put(n, "arg1", c::SC_ARG1);
    put(n, "arg2", c::SC_ARG2); put(n, "is_real", c::SC_IS_REAL);
    n = "StateBump";
    put(n, "width", tg::STATE_BUMP_WIDTH);
    put(n, "next_clk_32_48", c::SB_NEXT_CLK_32_48); put(n, "next_clk_24_32", c::SB_NEXT_CLK_24_32); put(n, "next_clk_16_24", c::SB_NEXT_CLK_16_24);
    put(n, "next_clk_0_16", c::SB_NEXT_CLK_0_16); put(n, "clk_high", c::SB_CLK_HIGH); put(n, "clk_low", c::SB_CLK_LOW); put(n, "next_pc", c::SB_NEXT_PC);
    put(n, "pc", c::SB_PC); put(n, "is_clk", c::SB_IS_CLK); put(n, "is_real", c::SB_IS_REAL);
    n = "MemoryBump";
    put(n, "width", tg::MEMORY_BUMP_WIDTH);
    put(n, "access.prev_value", c::MB_PREV_VALUE); put(n, "access.prev_high", c::MB_PREV_HIGH); put(n, "access.prev_low", c::MB_PREV_LOW);
    put(n, "access.compare_low", c::MB_COMPARE_LOW); put(n, "access.diff_low_limb", c::MB_DIFF_LOW_LIMB); put(n, "access.diff_high_limb", c::MB_DIFF_HIGH_LIMB);
    put(n, "clk_32_48", c::MB_CLK_32_48); put(n, "clk_24_32", c::MB_CLK_24_32); put(n, "clk_16_24", c::MB_CLK_16_24); put(n, "clk_0_16", c::MB_CLK_0_16);
    put(n, "addr", c::MB_ADDR); put(n, "is_real", c::MB_IS_REAL);
    return 0;
}

static int usage(const char* me) {
    fprintf(stderr, "usage: %s host partition IN OUT\n       %s host rows CHIP IN HEIGHT OUT\n       %s host global IN OUT\n       %s host layout|width|bins\n", me,
            me, me, me);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 3) return usage(argv[0]);
    const char* what = argv[2];
    if (strcmp(argv[1], "host")) { fprintf(stderr, "unknown form %s: this program has only the host form\n", argv[1]); return 1; }
    if (argc == 3 && !strcmp(what, "layout")) return layout();
    if (argc == 3 && !strcmp(what, "width")) {
        for (int chip = 0; chip < N_SYS_CHIPS; chip++) printf("%s %d\n", NAMES[chip], WIDTHS[chip]);
        return 0;
    }
    if (argc == 3 && !strcmp(what, "bins")) {
        for (int bin = 0; bin < tg::BINS; bin++) printf("%d %d\n", bin, tg::words_of_bin(bin));
        return 0;
    }
    if (argc == 5 && !strcmp(what, "partition")) {
        std::vector<uint64_t> in;
        if (!read_records(argv[3], tg::RAW_EV_WORDS, in)) return 1;
        std::vector<uint64_t> bins[tg::BINS];
        host_partition(in.data(), in.size() / tg::RAW_EV_WORDS, bins);
        std::vector<uint64_t> out;
        for (int b = 0; b < tg::BINS; b++) out.push_back(bins[b].size() / (size_t)tg::words_of_bin(b));
        for (int b = 0; b < tg::BINS; b++) out.insert(out.end(), bins[b].begin(), bins[b].end());
        return write_out(argv[4], out.data(), out.size() * 8);
    }
    if (argc == 5 && !strcmp(what, "global")) {
        std::vector<uint64_t> rec;
        if (!read_records(argv[3], 11, rec)) return 1;
        const uint32_t n = (uint32_t)(rec.size() / 11);
        std::vector<int32_t> ev((size_t)n * tg::GLOBAL_EVENT_WORDS);
        std::vector<uint32_t> table((size_t)tg::SYSCALL_CORE_WIDTH * n);       // the events come with the rows
        tg::host_rows<tg::SyscallCore>(table.data(), n, reinterpret_cast<const tg::Ev*>(rec.data()), n, ev.data());
        return write_out(argv[4], ev.data(), ev.size() * 4);
    }
    if (strcmp(what, "rows") || argc != 7) return usage(argv[0]);
    int chip = -1;
    for (int k = 0; k < N_SYS_CHIPS; k++) if (!strcmp(argv[3], NAMES[k])) chip = k;
    if (chip < 0) { fprintf(stderr, "unknown chip %s\n", argv[3]); return 1; }
    uint32_t height, n;
    std::vector<uint64_t> in;
    if (!read_rows_input(argv[5], argv[4], RECORD_WORDS[chip], height, in, n)) return 1;
    std::vector<uint32_t> out((size_t)WIDTHS[chip] * height, 0xeeeeeeeeu);
    host_rows(chip, out.data(), height, in.data(), n);
    if (write_out(argv[6], out.data(), out.size() * 4)) return 1;
    fprintf(stderr, "riscv_sys_rows host rows %s: %d x %u words\n", NAMES[chip], WIDTHS[chip], height);
    return 0;
}
