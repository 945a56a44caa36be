// tests/native/riscv_memglobal_rows.hip — the row functions of sp1_amd/csrc/tg_riscv_memglobal_rows.hpp (included unchanged) behind a
// file interface, in their `host` form: the __host__ __device__ code compiled for the CPU. It never opens a GPU and never loads the
// library. tests/test_tracegen_memglobal_host.py writes the inputs and checks every word; the device side is checked through
// sp1_amd.api by tests/test_gpu_tracegen_memglobal.py.
//
//   riscv_memglobal_rows host rows CHIP IN HEIGHT OUT [ARGS]    the table of CHIP
//       CHIP = MemoryGlobalInit | MemoryGlobalFinalize, ARGS = PREVIOUS_ADDR; IN: n x 3 u64 { addr, value, timestamp }
//       CHIP = SyscallPrecompile, ARGS = WORDS_PER_EVENT SYSCALL_ID ARG2_WORD (-1: none); IN: n x WORDS_PER_EVENT u64 event records
//       little-endian, n = file size / record size, n <= HEIGHT <= 2^20
//       OUT: width x HEIGHT u32, column-major [width][height], Montgomery words; rows >= n are zero
//   riscv_memglobal_rows host global CHIP IN OUT [ARGS]          the rows' Global events: n x 9 i32 (ARGS as above, without PREVIOUS_ADDR)
//   riscv_memglobal_rows host records IN WORDS_PER_EVENT OUT SEGMENT...   the MemoryLocal records of precompile events: sum of n *
//       count records x 5 u64; SEGMENT = ptr_word,count,pairs_word,final_word,final_clk_delta (final_word -1: the words are only read)
//   riscv_memglobal_rows host layout                             the column constants as text lines "chip key column"
//   riscv_memglobal_rows host width                              "chip width" lines
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc -Iinclude ...
#include <string.h>

#include "rows_io.hpp"
#include "sp1hip.h"
#include "tg_riscv_memglobal_rows.hpp"

namespace tg = sp1hip::tg;

static void put(const char* chip, const char* key, int v) { printf("%s %s %d\n", chip, key, v); }

static int layout() {
    namespace c = tg::col;
    for (const char* n : {"MemoryGlobalInit", "MemoryGlobalFinalize"}) {
        put(n, "width", tg::MEMORY_GLOBAL_WIDTH);
        put(n, "clk_high", c::MG_CLK_HIGH); put(n, "clk_low", c::MG_CLK_LOW); put(n, "index", c::MG_INDEX); put(n, "prev_addr", c::MG_PREV_ADDR);
        put(n, "addr", c::MG_ADDR); put(n, "lt_cols.bit", c::MG_LT_BIT); put(n, "lt_cols.u16_flags", c::MG_LT_U16_FLAGS);
        put(n, "lt_cols.not_eq_inv", c::MG_LT_NOT_EQ_INV); put(n, "lt_cols.comparison_limbs", c::MG_LT_COMPARISON_LIMBS);
        put(n, "value", c::MG_VALUE); put(n, "value_lower", c::MG_VALUE_LOWER); put(n, "value_upper", c::MG_VALUE_UPPER);
        put(n, "is_real", c::MG_IS_REAL); put(n, "is_comp", c::MG_IS_COMP); put(n, "prev_valid", c::MG_PREV_VALID);
        put(n, "is_prev_addr_zero.inverse", c::MG_IS_PREV_ADDR_ZERO); put(n, "is_prev_addr_zero.result", c::MG_IS_PREV_ADDR_ZERO + 1);
        put(n, "is_index_zero.inverse", c::MG_IS_INDEX_ZERO); put(n, "is_index_zero.result", c::MG_IS_INDEX_ZERO + 1);
    }
    const char* n = "SyscallPrecompile";
    put(n, "width", tg::SYSCALL_PRECOMPILE_WIDTH);
    put(n, "clk_high", c::SP_CLK_HIGH); put(n, "clk_low", c::SP_CLK_LOW); put(n, "syscall_id", c::SP_SYSCALL_ID); put(n, "arg1", c::SP_ARG1);
    put(n, "arg2", c::SP_ARG2); put(n, "is_real", c::SP_IS_REAL);
    return 0;
}

static int usage(const char* me) {
    fprintf(stderr, "usage: %s host rows CHIP IN HEIGHT OUT ARGS...\n       %s host global CHIP IN OUT ARGS...\n"
                    "       %s host records IN WORDS_PER_EVENT OUT SEGMENT...\n       %s host layout|width\n", me, me, me, me);
    return 1;
}

static bool number(const char* s, long long lo, long long hi, long long& v) {
    char* end = nullptr;
    v = strtoll(s, &end, 0);
    if (*end || end == s || v < lo || v > hi) { fprintf(stderr, "bad number %s: need %lld <= value <= %lld\n", s, lo, hi); return false; }
    return true;
}

// CHIP and its trailing arguments: kind 0 / 1 = MemoryGlobalInit / Finalize, 2 = SyscallPrecompile
struct Chip { int kind; uint64_t previous; uint32_t words, syscall_id; int arg2_word; };

static bool parse_chip(const char* name, char** args, int n_args, bool with_previous, Chip& c) {
    c = {};
    long long v;
    if (!strcmp(name, "MemoryGlobalInit") || !strcmp(name, "MemoryGlobalFinalize")) {
        c.kind = !strcmp(name, "MemoryGlobalFinalize");
        c.words = tg::MEMORY_GLOBAL_RECORD_WORDS;
        if (n_args != (with_previous ? 1 : 0)) return false;
        if (with_previous) { c.previous = strtoull(args[0], nullptr, 0); }
        return true;
    }
    if (strcmp(name, "SyscallPrecompile") || n_args != 3) { fprintf(stderr, "unknown chip %s or wrong arguments\n", name); return false; }
    c.kind = 2;
    if (!number(args[0], 2, 65536, v)) return false;
    c.words = (uint32_t)v;
    if (!number(args[1], 0, 255, v)) return false;
    c.syscall_id = (uint32_t)v;
    if (!number(args[2], -1, (long long)c.words - 1, v)) return false;
    c.arg2_word = (int)v;
    return true;
}

// what the kernels do for their lanes, as a host loop: tg::host_rows (tg_row_kernel.hpp); `global_events` may be null
static void host_rows(const Chip& chip, uint32_t* out, uint32_t height, const uint64_t* in, uint32_t n, int32_t* global_events) {
    if (chip.kind == 2) tg::host_rows<tg::SyscallPrecompile>(out, height, in, n, chip.words, chip.syscall_id, chip.arg2_word, global_events);
    else tg::host_rows<tg::MemoryGlobal>(out, height, in, n, chip.previous, chip.kind, global_events);
}
static int width_of(const Chip& chip) { return chip.kind == 2 ? tg::SYSCALL_PRECOMPILE_WIDTH : tg::MEMORY_GLOBAL_WIDTH; }

int main(int argc, char** argv) {
    if (argc < 3) return usage(argv[0]);
    const char* what = argv[2];
    if (strcmp(argv[1], "host")) { fprintf(stderr, "unknown form %s: this program has only the host form\n", argv[1]); return 1; }
    if (argc == 3 && !strcmp(what, "layout")) return layout();
    if (argc == 3 && !strcmp(what, "width")) {
        printf("MemoryGlobalInit %d\nMemoryGlobalFinalize %d\nSyscallPrecompile %d\n", tg::MEMORY_GLOBAL_WIDTH, tg::MEMORY_GLOBAL_WIDTH, tg::SYSCALL_PRECOMPILE_WIDTH);
        return 0;
    }
    long long v;
    if (!strcmp(what, "records") && argc >= 7 && argc <= 6 + tg::PRECOMPILE_MAX_SEGMENTS) {
        if (!number(argv[4], 2, 65536, v)) return 1;
        const uint32_t words = (uint32_t)v;
        tg::LocalSegments segs = {};
        for (int k = 6; k < argc; k++) {
            long long w[5];
            if (sscanf(argv[k], "%lld,%lld,%lld,%lld,%lld", &w[0], &w[1], &w[2], &w[3], &w[4]) != 5) { fprintf(stderr, "bad segment %s\n", argv[k]); return 1; }
            const bool ok = w[0] >= 0 && w[0] < words && w[1] >= 1 && w[2] >= 0 && w[2] + 2 * w[1] <= words && (w[3] == -1 || (w[3] >= 0 && w[3] + w[1] <= words)) &&
                            w[4] >= 0 && w[4] <= 0xffffffffll;
            if (!ok) { fprintf(stderr, "segment %s reads behind the event record\n", argv[k]); return 1; }
            segs.s[segs.n++] = {(uint32_t)w[0], (uint32_t)w[1], (uint32_t)w[2], w[3] < 0 ? tg::PRECOMPILE_NO_WORD : (uint32_t)w[3], (uint32_t)w[4]};
        }
        std::vector<uint64_t> ev;
        if (!read_records(argv[3], words, ev)) return 1;
        const uint32_t n = (uint32_t)(ev.size() / words);
        uint64_t total = 0;
        for (uint32_t k = 0; k < segs.n; k++) total += (uint64_t)n * segs.s[k].count;
        std::vector<uint64_t> rec(total * tg::MEMORY_LOCAL_RECORD_WORDS);
        for (uint64_t q = 0; q < total; q++) {                  // what precompile_local_records_kernel does for its lane
            tg::LocalSegment seg;
            uint32_t event, word;
            if (!tg::precompile_local_locate(segs, n, q, seg, event, word)) { fprintf(stderr, "record %llu has no segment\n", (unsigned long long)q); return 1; }
            tg::precompile_local_record(rec.data() + q * tg::MEMORY_LOCAL_RECORD_WORDS, ev.data() + (size_t)event * words, seg, word);
        }
        return write_out(argv[5], rec.data(), rec.size() * 8);
    }
    if (!strcmp(what, "global") && argc >= 6) {
        Chip chip;
        if (!parse_chip(argv[3], argv + 6, argc - 6, false, chip)) return usage(argv[0]);
        std::vector<uint64_t> in;
        if (!read_records(argv[4], chip.words, in)) return 1;
        const uint32_t n = (uint32_t)(in.size() / chip.words);
        std::vector<int32_t> ev((size_t)n * tg::GLOBAL_EVENT_WORDS);
        std::vector<uint32_t> table((size_t)width_of(chip) * n);               // the events come with the rows
        host_rows(chip, table.data(), n, in.data(), n, ev.data());
        return write_out(argv[5], ev.data(), ev.size() * 4);
    }
    if (strcmp(what, "rows") || argc < 7) return usage(argv[0]);
    Chip chip;
    if (!parse_chip(argv[3], argv + 7, argc - 7, true, chip)) return usage(argv[0]);
    uint32_t height, n;
    std::vector<uint64_t> in;
    if (!read_rows_input(argv[5], argv[4], chip.words, height, in, n)) return 1;
    const int width = width_of(chip);
    std::vector<uint32_t> out((size_t)width * height, 0xeeeeeeeeu);
    host_rows(chip, out.data(), height, in.data(), n, nullptr);
    if (write_out(argv[6], out.data(), out.size() * 4)) return 1;
    fprintf(stderr, "riscv_memglobal_rows host rows %s: %d x %u words\n", argv[3], width, height);
    return 0;
}
