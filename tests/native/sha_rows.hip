// tests/native/sha_rows.hip — the row functions of sp1_amd/csrc/tg_sha256_rows.hpp and the MemoryLocal record function of
// tg_riscv_memglobal_rows.hpp (both included unchanged) behind a file interface, in one of two forms: `host` (the __host__ __device__
// code compiled for the CPU in a plain loop over the rows; never opens a GPU and never loads the library) and `device` (the kernels
// of tracegen_sha256.hip through the library's entry points). tests/test_tracegen_sha_host.py (CPU) writes the inputs and checks
// every output word.
//
//   sha_rows FORM rows CHIP IN HEIGHT OUT     the table of CHIP = ShaExtend | ShaExtendControl | ShaCompress | ShaCompressControl
//       IN:  n x 786 (ShaExtend*) or n x 155 (ShaCompress*) u64 event records, little-endian, n = file size / record size;
//            48 n (ShaExtend), 80 n (ShaCompress) or n <= HEIGHT <= 2^20
//       OUT: width x HEIGHT u32, column-major [width][height], Montgomery words
//   sha_rows host records IN WORDS_PER_EVENT OUT SEGMENT...   the MemoryLocal records of precompile events: sum of n * count records
//       x 5 u64; SEGMENT = ptr_word,count,pairs_word,final_word,final_clk_delta (final_word -1: the words are only read; -2: the quad
//       form, four record words per word from pairs_word on)
//   sha_rows host layout                      the column constants as text lines "chip key column"
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc -Iinclude ...
#include <string.h>

#include "rows_io.hpp"
#include "sp1hip.h"
#include "tg_riscv_memglobal_rows.hpp"
#include "tg_sha256_rows.hpp"

namespace tg = sp1hip::tg;
namespace tgs = sp1hip::tgs;

struct Chip { const char* name; int width, words, rows_per_event; const char* entry; };
static const Chip CHIPS[] = {{"ShaExtend", tgs::ext::WIDTH, tgs::EXTEND_EVENT_WORDS, tgs::EXTEND_ROWS, "sp1hip_tracegen_riscv_sha_extend"},
                             {"ShaExtendControl", tgs::ext::CONTROL_WIDTH, tgs::EXTEND_EVENT_WORDS, 1, "sp1hip_tracegen_riscv_sha_extend_control"},
                             {"ShaCompress", tgs::cmp::WIDTH, tgs::COMPRESS_EVENT_WORDS, tgs::COMPRESS_ROWS, "sp1hip_tracegen_riscv_sha_compress"},
                             {"ShaCompressControl", tgs::cmp::CONTROL_WIDTH, tgs::COMPRESS_EVENT_WORDS, 1, "sp1hip_tracegen_riscv_sha_compress_control"}};

// what the kernels do for their lanes, as a host loop
static void host_rows(int chip, uint32_t* out, uint32_t height, const uint64_t* events, uint32_t n) {
    for (uint32_t row = 0; row < height; row++) {
        switch (chip) {
        case 0: tgs::sha_extend_row(out, height, row, events, n); break;
        case 1: tgs::sha_extend_control_row(out, height, row, events, n); break;
        case 2: tgs::sha_compress_row(out, height, row, events, n); break;
        default: tgs::sha_compress_control_row(out, height, row, events, n); break;
        }
    }
}

#if defined(__HIPCC__)
// the table from the real kernels, through the library's entry point (table, height, events, n, stream), loaded at run time
static int device_rows(const char* entry, std::vector<uint32_t>& out, uint32_t height, const std::vector<uint64_t>& words, uint32_t n) {
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)
    const std::string path = library_path();
    void* lib = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!lib) { fprintf(stderr, "cannot load %s: %s\n", path.c_str(), dlerror()); return 2; }
    using Fn = int (*)(uint32_t*, uint32_t, const uint64_t*, uint32_t, sp1hip_stream_t);
    using Err = const char* (*)();
    const Fn run = (Fn)dlsym(lib, entry);
    const Err last_error = (Err)dlsym(lib, "sp1hip_last_error");
    if (!run) { fprintf(stderr, "%s has no %s\n", path.c_str(), entry); return 2; }
    uint64_t* d_ev = nullptr;
    uint32_t* d_out = nullptr;
    CHECK(hipMalloc(&d_ev, words.size() * 8 + 8));
    CHECK(hipMalloc(&d_out, out.size() * 4 + 8));
    CHECK(hipMemcpy(d_ev, words.data(), words.size() * 8, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xee, out.size() * 4 + 8));
    const int st = run(d_out, height, d_ev, n, nullptr);
    if (st != 0) { fprintf(stderr, "%s: %d %s\n", entry, st, last_error ? last_error() : ""); return 2; }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_ev));
    CHECK(hipFree(d_out));
    return 0;
#undef CHECK
}
#endif

static void put(const char* chip, const char* key, int v) { printf("%s %s %d\n", chip, key, v); }

static int layout() {
    namespace e = tgs::ext;
    namespace c = tgs::cmp;
    const char* n = "ShaExtend";
    put(n, "width", e::WIDTH); put(n, "clk_high", e::CLK_HIGH); put(n, "clk_low", e::CLK_LOW); put(n, "next_clk.next_clk_16_24", e::NEXT_CLK);
    put(n, "next_clk.next_clk_0_16", e::NEXT_CLK + 1); put(n, "next_clk.is_overflow", e::NEXT_CLK + 2); put(n, "w_ptr", e::W_PTR_COL);
    put(n, "w_i_minus_15_ptr.value", e::W_I_MINUS_15_PTR); put(n, "w_i_minus_2_ptr.value", e::W_I_MINUS_2_PTR);
    put(n, "w_i_minus_16_ptr.value", e::W_I_MINUS_16_PTR); put(n, "w_i_minus_7_ptr.value", e::W_I_MINUS_7_PTR); put(n, "w_i_ptr.value", e::W_I_PTR);
    put(n, "i", e::I); put(n, "w_i_minus_15.prev_value", e::W_I_MINUS_15); put(n, "w_i_minus_15_rr_7.value", e::W_I_MINUS_15_RR_7);
    put(n, "w_i_minus_15_rr_18.higher_limb", e::W_I_MINUS_15_RR_7 + tgs::FIXED_ROT + 2); put(n, "w_i_minus_15_rs_3.value", e::W_I_MINUS_15_RR_7 + 2 * tgs::FIXED_ROT);
    put(n, "s0_intermediate.b_low_bytes.low_bytes", e::S0_INTERMEDIATE); put(n, "s0.b_low_bytes.low_bytes", e::S0); put(n, "s0.value", e::S0 + 4);
    put(n, "w_i_minus_2.prev_value", e::W_I_MINUS_2); put(n, "w_i_minus_2_rr_17.value", e::W_I_MINUS_2_RR_17);
    put(n, "w_i_minus_2_rr_19.value", e::W_I_MINUS_2_RR_17 + tgs::FIXED_ROT); put(n, "w_i_minus_15_rr_18.value", e::W_I_MINUS_15_RR_7 + tgs::FIXED_ROT);
    put(n, "w_i_minus_2_rs_10.value", e::W_I_MINUS_2_RR_17 + 2 * tgs::FIXED_ROT); put(n, "s1_intermediate.b_low_bytes.low_bytes", e::S1_INTERMEDIATE);
    put(n, "s1.c_low_bytes.low_bytes", e::S1 + 2); put(n, "w_i_minus_16.prev_value", e::W_I_MINUS_16); put(n, "w_i_minus_7.prev_value", e::W_I_MINUS_7);
    put(n, "s2.value", e::S2); put(n, "w_i.prev_value", e::W_I); put(n, "w_i.diff_high_limb", e::W_I + 8); put(n, "is_real", e::IS_REAL);
    n = "ShaExtendControl";
    put(n, "width", e::CONTROL_WIDTH); put(n, "clk_high", 0); put(n, "clk_low", 1); put(n, "w_ptr.addr", 2);
    put(n, "w_ptr.top_two_limb_min", 5); put(n, "w_ptr.top_two_limb_max.inverse", 6); put(n, "w_ptr.top_two_limb_max.result", 7);
    put(n, "w_16th_addr.value", 2 + sp1hip::tgf::SYSCALL_ADDR_COLS); put(n, "w_17th_addr.value", 5 + sp1hip::tgf::SYSCALL_ADDR_COLS);
    put(n, "w_64th_addr.value", 8 + sp1hip::tgf::SYSCALL_ADDR_COLS); put(n, "is_real", e::CONTROL_WIDTH - 1);
    n = "ShaCompress";
    put(n, "width", c::WIDTH); put(n, "clk_high", c::CLK_HIGH); put(n, "clk_low", c::CLK_LOW); put(n, "w_ptr", c::W_PTR_COL); put(n, "h_ptr", c::H_PTR_COL);
    put(n, "index", c::INDEX); put(n, "octet", c::OCTET); put(n, "octet_num", c::OCTET_NUM); put(n, "mem.prev_value", c::MEM); put(n, "mem_value", c::MEM_VALUE);
    put(n, "mem_addr", c::MEM_ADDR); put(n, "mem_addr_init.value", c::MEM_ADDR_INIT); put(n, "mem_addr_compress.value", c::MEM_ADDR_COMPRESS);
    put(n, "mem_addr_finalize.value", c::MEM_ADDR_FINALIZE); put(n, "a", c::A); put(n, "b", c::A + 2); put(n, "c", c::A + 4); put(n, "d", c::A + 6);
    put(n, "e", c::A + 8); put(n, "f", c::A + 10); put(n, "g", c::A + 12); put(n, "h", c::A + 14); put(n, "e_rr_11.value", c::E_RR_6 + tgs::FIXED_ROT);
    put(n, "a_rr_13.value", c::A_RR_2 + tgs::FIXED_ROT); put(n, "k", c::K); put(n, "e_rr_6.value", c::E_RR_6);
    put(n, "e_rr_25.higher_limb", c::E_RR_6 + 2 * tgs::FIXED_ROT + 2); put(n, "s1_intermediate.b_low_bytes.low_bytes", c::S1_INTERMEDIATE);
    put(n, "s1.value", c::S1 + 4); put(n, "e_and_f.value", c::E_AND_F + 4); put(n, "e_not.value", c::E_NOT); put(n, "e_not_and_g.value", c::E_NOT_AND_G + 4);
    put(n, "ch.value", c::CH + 4); put(n, "temp1.value", c::TEMP1); put(n, "a_rr_2.value", c::A_RR_2); put(n, "a_rr_22.value", c::A_RR_2 + 2 * tgs::FIXED_ROT);
    put(n, "s0_intermediate.value", c::S0_INTERMEDIATE + 4); put(n, "s0.value", c::S0 + 4); put(n, "a_and_b.value", c::A_AND_B + 4);
    put(n, "a_and_c.value", c::A_AND_C + 4); put(n, "b_and_c.value", c::B_AND_C + 4); put(n, "maj_intermediate.value", c::MAJ_INTERMEDIATE + 4);
    put(n, "maj.value", c::MAJ + 4); put(n, "temp2.value", c::TEMP2); put(n, "d_add_temp1.value", c::D_ADD_TEMP1);
    put(n, "temp1_add_temp2.value", c::TEMP1_ADD_TEMP2); put(n, "finalized_operand", c::FINALIZED_OPERAND); put(n, "finalize_add.value", c::FINALIZE_ADD);
    put(n, "is_initialize", c::IS_INITIALIZE); put(n, "is_compression", c::IS_COMPRESSION); put(n, "is_finalize", c::IS_FINALIZE); put(n, "is_real", c::IS_REAL);
    n = "ShaCompressControl";
    put(n, "width", c::CONTROL_WIDTH); put(n, "clk_high", 0); put(n, "clk_low", 1); put(n, "w_ptr.addr", 2); put(n, "h_ptr.addr", 2 + sp1hip::tgf::SYSCALL_ADDR_COLS);
    put(n, "w_ptr.top_two_limb_min", 5); put(n, "w_ptr.top_two_limb_max.inverse", 6); put(n, "w_ptr.top_two_limb_max.result", 7);
    put(n, "h_ptr.top_two_limb_min", 11); put(n, "h_ptr.top_two_limb_max.inverse", 12); put(n, "h_ptr.top_two_limb_max.result", 13);
    put(n, "w_slice_end.value", 2 + 2 * sp1hip::tgf::SYSCALL_ADDR_COLS); put(n, "h_slice_end.value", 5 + 2 * sp1hip::tgf::SYSCALL_ADDR_COLS);
    put(n, "is_real", 8 + 2 * sp1hip::tgf::SYSCALL_ADDR_COLS); put(n, "initial_state", 9 + 2 * sp1hip::tgf::SYSCALL_ADDR_COLS);
    put(n, "final_state", 25 + 2 * sp1hip::tgf::SYSCALL_ADDR_COLS);
    return 0;
}

static int usage(const char* me) {
    fprintf(stderr, "usage: %s host|device rows CHIP IN HEIGHT OUT\n       %s host records IN WORDS_PER_EVENT OUT SEGMENT...\n       %s host layout\n", me, me, me);
    return 1;
}

static bool number(const char* s, long long lo, long long hi, long long& v) {
    char* end = nullptr;
    v = strtoll(s, &end, 0);
    if (*end || end == s || v < lo || v > hi) { fprintf(stderr, "bad number %s: need %lld <= value <= %lld\n", s, lo, hi); return false; }
    return true;
}

// the MemoryLocal records of the events of IN: what precompile_local_records_kernel does for its lanes, with its entry point's checks
static int records(int argc, char** argv) {
    long long v;
    if (!number(argv[4], 2, 65536, v)) return 1;
    const uint32_t words = (uint32_t)v;
    tg::LocalSegments segs = {};
    for (int k = 6; k < argc; k++) {
        long long w[5];
        if (sscanf(argv[k], "%lld,%lld,%lld,%lld,%lld", &w[0], &w[1], &w[2], &w[3], &w[4]) != 5) { fprintf(stderr, "bad segment %s\n", argv[k]); return 1; }
        const bool quad = w[3] == -2;
        const bool ok = w[0] >= 0 && w[0] < words && w[1] >= 1 && w[2] >= 0 && w[2] + (quad ? 4 : 2) * w[1] <= words &&
                        (w[3] == -1 || quad || (w[3] >= 0 && w[3] + w[1] <= words)) && w[4] >= 0 && w[4] <= 0xffffffffll;
        if (!ok) { fprintf(stderr, "segment %s reads behind the event record\n", argv[k]); return 1; }
        const uint32_t final_word = w[3] == -1 ? tg::PRECOMPILE_NO_WORD : quad ? tg::PRECOMPILE_QUAD_WORDS : (uint32_t)w[3];
        segs.s[segs.n++] = {(uint32_t)w[0], (uint32_t)w[1], (uint32_t)w[2], final_word, (uint32_t)w[4]};
    }
    std::vector<uint64_t> ev;
    if (!read_records(argv[3], words, ev)) return 1;
    const uint32_t n = (uint32_t)(ev.size() / words);
    uint64_t total = 0;
    for (uint32_t k = 0; k < segs.n; k++) total += (uint64_t)n * segs.s[k].count;
    std::vector<uint64_t> rec(total * tg::MEMORY_LOCAL_RECORD_WORDS);
    for (uint64_t q = 0; q < total; q++) {
        tg::LocalSegment seg;
        uint32_t event, word;
        if (!tg::precompile_local_locate(segs, n, q, seg, event, word)) { fprintf(stderr, "record %llu has no segment\n", (unsigned long long)q); return 1; }
        tg::precompile_local_record(rec.data() + q * tg::MEMORY_LOCAL_RECORD_WORDS, ev.data() + (size_t)event * words, seg, word);
    }
    return write_out(argv[5], rec.data(), rec.size() * 8);
}

int main(int argc, char** argv) {
    if (argc < 3) return usage(argv[0]);
    const char *form = argv[1], *what = argv[2];
    const bool host = !strcmp(form, "host"), device = !strcmp(form, "device");
    if (!host && !device) { fprintf(stderr, "unknown form %s\n", form); return 1; }
    if (host && argc == 3 && !strcmp(what, "layout")) return layout();
    if (host && !strcmp(what, "records") && argc >= 7 && argc <= 6 + tg::PRECOMPILE_MAX_SEGMENTS) return records(argc, argv);
    if (strcmp(what, "rows") || argc != 7) return usage(argv[0]);
    int chip = -1;
    for (int k = 0; k < 4; k++) if (!strcmp(argv[3], CHIPS[k].name)) chip = k;
    if (chip < 0) { fprintf(stderr, "unknown chip %s\n", argv[3]); return 1; }
    const Chip& c = CHIPS[chip];
    uint32_t height, n;
    std::vector<uint64_t> in;
    if (!read_rows_input(argv[5], argv[4], (size_t)c.words, height, in, n)) return 1;
    if ((uint64_t)n * c.rows_per_event > height) { fprintf(stderr, "the events' rows (%d each) exceed height = %u\n", c.rows_per_event, height); return 1; }
    std::vector<uint32_t> out((size_t)c.width * height, 0xeeeeeeeeu);
    if (host) {
        host_rows(chip, out.data(), height, in.data(), n);
    } else {
#if defined(__HIPCC__)
        const int st = device_rows(c.entry, out, height, in, n);
        if (st) return st;
#else
        fprintf(stderr, "built without a device compiler: only the host form\n");
        return 1;
#endif
    }
    if (write_out(argv[6], out.data(), out.size() * 4)) return 1;
    fprintf(stderr, "sha_rows %s rows %s: %d x %u words\n", form, c.name, c.width, height);
    return 0;
}
