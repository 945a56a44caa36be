// tests/native/ed_u256_rows.hip — the rows of sp1_amd/csrc/tg_ed_uint256_rows.hpp (included unchanged: EdAddAssign, EdDecompress,
// Uint256Ops and the touched words' records) behind a file interface, in one of two forms: `host` (the __host__ __device__ code
// compiled for the CPU, both phases as loops; never opens a GPU) and `device` (the header's gfx950 kernels, launched as libsp1hip.so
// launches them, with a work buffer of this program's own). tests/test_tracegen_ed_u256_host.py (CPU) and
// tests/test_gpu_tracegen_ed_u256.py write the inputs and check every word.
//
//   ed_u256_rows FORM ed_add|ed_decompress|uint256_ops IN OUT     the chip's table of an event file
//       IN:  u32 n_events, u32 height, then n_events x (44 / 24 / 58) u64   (little-endian)
//       OUT: width x height u32, column-major [width][height], Montgomery words
//   ed_u256_rows FORM records_ed_decompress|records_uint256_ops IN OUT     the MemoryLocal records of the words the calls touched
//       OUT: n_events x (8 / 23) x 5 u64
//   ed_u256_rows host layout - OUT      the column constants of the three chips as text lines "chip key offset"
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc ...
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "tg_ed_uint256_rows.hpp"

namespace tge = sp1hip::tge;
namespace tgf = sp1hip::tgf;

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

static bool read_exact(FILE* f, void* to, size_t bytes) { return bytes == 0 || fread(to, 1, bytes, f) == bytes; }

static int write_out(const char* path, const void* data, size_t bytes) {
    const bool to_stdout = !strcmp(path, "-");
    FILE* g = to_stdout ? stdout : fopen(path, "wb");
    if (!g) { fprintf(stderr, "cannot open %s\n", path); return 1; }
    const size_t put = bytes ? fwrite(data, 1, bytes, g) : 0;
    if (!to_stdout) fclose(g); else fflush(g);
    if (put != bytes) { fprintf(stderr, "short write\n"); return 1; }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------------- layout
struct Text {
    std::string s;
    void put(const char* chip, const std::string& key, int v) { s += std::string(chip) + " " + key + " " + std::to_string(v) + "\n"; }
    void field_op(const char* chip, const char* name, int col, int limbs = 32) {
        put(chip, std::string(name) + ".result", col);
        put(chip, std::string(name) + ".carry", col + limbs);
        put(chip, std::string(name) + ".witness", col + 2 * limbs);
    }
    void field_lt(const char* chip, const char* name, int col) {
        put(chip, std::string(name) + ".byte_flags", col + tgf::FieldLt<8>::BYTE_FLAGS);
        put(chip, std::string(name) + ".lhs_comparison_byte", col + tgf::FieldLt<8>::LHS_BYTE);
        put(chip, std::string(name) + ".rhs_comparison_byte", col + tgf::FieldLt<8>::RHS_BYTE);
    }
};

static int layout(const char* path) {
    Text t;
    {
        using S = tge::EdAdd;
        const char* c = "EdAddAssign";
        t.put(c, "width", S::WIDTH); t.put(c, "event_words", S::EVENT_WORDS); t.put(c, "ops", S::OPS);
        t.put(c, "is_real", S::H::IS_REAL); t.put(c, "clk_high", S::H::CLK_HIGH); t.put(c, "clk_low", S::H::CLK_LOW);
        t.put(c, "x_ptr.addr", S::H::X_PTR); t.put(c, "y_ptr.addr", S::H::Y_PTR); t.put(c, "x_addrs.0.value", S::H::X_ADDRS); t.put(c, "y_addrs.0.value", S::H::Y_ADDRS);
        t.put(c, "x_access.0.memory_access.prev_value", S::H::X_ACCESS); t.put(c, "y_access.0.memory_access.prev_value", S::H::Y_ACCESS);
        t.put(c, "y_access.7.prev_value_u8.low_bytes", S::H::Y_ACCESS + 7 * tgf::MEMORY_ACCESS_U8_COLS + 9);
        t.field_op(c, "x3_numerator", S::X3_NUMERATOR); t.field_op(c, "y3_numerator", S::Y3_NUMERATOR); t.field_op(c, "x1_mul_y1", S::X1_MUL_Y1);
        t.field_op(c, "x2_mul_y2", S::X2_MUL_Y2); t.field_op(c, "f", S::F); t.field_op(c, "d_mul_f", S::D_MUL_F); t.field_op(c, "x3_ins", S::X3_INS);
        t.field_op(c, "y3_ins", S::Y3_INS); t.field_lt(c, "x3_range", S::X3_RANGE); t.field_lt(c, "y3_range", S::Y3_RANGE);
    }
    {
        using S = tge::EdDecompress;
        const char* c = "EdDecompress";
        t.put(c, "width", S::WIDTH); t.put(c, "event_words", S::EVENT_WORDS); t.put(c, "ops", S::OPS);
        t.put(c, "is_real", S::IS_REAL); t.put(c, "clk_high", S::CLK_HIGH); t.put(c, "clk_low", S::CLK_LOW); t.put(c, "ptr.addr", S::PTR);
        t.put(c, "read_ptrs.0.value", S::READ_PTRS); t.put(c, "addrs.0.value", S::ADDRS); t.put(c, "sign", S::SIGN);
        t.put(c, "x_access.0.prev_value", S::X_ACCESS); t.put(c, "x_access.3.diff_high_limb", S::X_ACCESS + 35); t.put(c, "x_value.0", S::X_VALUE);
        t.put(c, "x_value.3", S::X_VALUE + 12); t.put(c, "y_access.0.memory_access.prev_value", S::Y_ACCESS);
        t.put(c, "y_access.3.prev_value_u8.low_bytes", S::Y_ACCESS + 3 * tgf::MEMORY_ACCESS_U8_COLS + 9);
        t.field_lt(c, "neg_x_range", S::NEG_X_RANGE); t.field_lt(c, "y_range", S::Y_RANGE);
        t.field_op(c, "yy", S::YY); t.field_op(c, "u", S::U_); t.field_op(c, "dyy", S::DYY); t.field_op(c, "v", S::V); t.field_op(c, "u_div_v", S::U_DIV_V);
        t.field_op(c, "x.multiplication", S::X_MULTIPLICATION); t.field_lt(c, "x.range", S::X_RANGE); t.put(c, "x.lsb", S::X_LSB); t.field_op(c, "neg_x", S::NEG_X);
    }
    {
        using S = tge::Uint256Ops;
        const char* c = "Uint256Ops";
        t.put(c, "width", S::WIDTH); t.put(c, "event_words", S::EVENT_WORDS);
        t.put(c, "clk_high", S::CLK_HIGH); t.put(c, "clk_low", S::CLK_LOW); t.put(c, "a_ptr.addr", S::A_PTR); t.put(c, "a_addrs.0.value", S::A_ADDRS);
        t.put(c, "b_ptr.addr", S::B_PTR); t.put(c, "c_ptr.addr", S::C_PTR); t.put(c, "c_ptr_memory.prev_value", S::C_PTR_MEMORY); t.put(c, "c_addrs.0.value", S::C_ADDRS);
        t.put(c, "d_ptr.addr", S::D_PTR); t.put(c, "d_ptr_memory.prev_value", S::D_PTR + 6); t.put(c, "e_ptr.addr", S::E_PTR); t.put(c, "e_addrs.3.value", S::E_PTR + 15 + 9);
        t.put(c, "a_memory.0.memory_access.prev_value", S::A_MEMORY); t.put(c, "b_memory.0.memory_access.prev_value", S::B_MEMORY);
        t.put(c, "c_memory.3.prev_value_u8.low_bytes", S::C_MEMORY + 3 * tgf::MEMORY_ACCESS_U8_COLS + 9); t.put(c, "d_memory.0.prev_value", S::D_MEMORY);
        t.put(c, "e_memory.0.prev_value", S::E_MEMORY); t.put(c, "e_memory.3.diff_high_limb", S::E_MEMORY + 35);
        t.field_op(c, "field_op", S::FIELD_OP); t.put(c, "is_add", S::IS_ADD); t.put(c, "is_mul", S::IS_MUL); t.put(c, "is_real", S::IS_REAL);
    }
    t.put("all", "witness_offset", (int)tge::WITNESS_OFFSET);
    return write_out(path, t.s.data(), t.s.size());
}

// ----------------------------------------------------------------------------------------------------------------------- tables
enum What { ED_ADD, ED_DECOMPRESS, UINT256_OPS, RECORDS_ED_DECOMPRESS, RECORDS_UINT256_OPS };

static int run(What what, bool host, FILE* f, std::vector<uint8_t>& bytes) {
    uint32_t head[2] = {0, 0};
    if (!read_exact(f, head, 8) || head[0] > head[1] || head[1] > (1u << 20)) { fprintf(stderr, "bad header: need n_events <= height <= 2^20\n"); return 1; }
    const uint32_t n = head[0], height = head[1];
    const bool records = what >= RECORDS_ED_DECOMPRESS;
    const uint32_t family = what == RECORDS_ED_DECOMPRESS ? tge::TOUCHED_ED_DECOMPRESS : tge::TOUCHED_UINT256_OPS;
    const uint32_t event_words = what == ED_ADD ? tge::EdAdd::EVENT_WORDS : what == ED_DECOMPRESS || what == RECORDS_ED_DECOMPRESS ? tge::EdDecompress::EVENT_WORDS
                                                                                                                                 : tge::Uint256Ops::EVENT_WORDS;
    const uint32_t width = what == ED_ADD ? tge::EdAdd::WIDTH : what == ED_DECOMPRESS ? tge::EdDecompress::WIDTH : tge::Uint256Ops::WIDTH;
    std::vector<uint64_t> events((size_t)n * event_words);
    if (!read_exact(f, events.data(), events.size() * 8)) { fprintf(stderr, "short input\n"); return 1; }
    const size_t n_records = records ? (size_t)n * tge::touched_per_event(family) : 0;
    bytes.assign(records ? n_records * tge::MEMORY_LOCAL_RECORD_WORDS * 8 : (size_t)width * height * 4, 0xee);
    const size_t work_words = what == ED_ADD ? tge::EdAdd::Work::words(height, tge::EdAdd::OPS)
                              : what == ED_DECOMPRESS ? tge::EdDecompress::Work::words(height, tge::EdDecompress::OPS) : 0;
    const sp1hip::tgf::Modulus<8>& m = tge::ed25519_modulus();
    uint32_t* out = (uint32_t*)bytes.data();
    if (host) {
        std::vector<uint32_t> work(work_words, 0xeeeeeeeeu);
        if (what == ED_ADD) tge::EdAdd::host_table(out, height, events.data(), n, work.data(), m);
        else if (what == ED_DECOMPRESS) tge::EdDecompress::host_table(out, height, events.data(), n, work.data(), m);
        else if (what == UINT256_OPS) tge::Uint256Ops::host_table(out, height, events.data(), n);
        else tge::host_touched_records((uint64_t*)bytes.data(), events.data(), n, family);
        return 0;
    }
    if (bytes.empty()) return 0;
#if defined(__HIPCC__)
    uint64_t* d_events = nullptr;
    uint32_t *d_out = nullptr, *d_work = nullptr;
    CHECK(hipMalloc(&d_events, events.size() * 8 + 8));
    CHECK(hipMalloc(&d_out, bytes.size()));
    CHECK(hipMalloc(&d_work, work_words * 4 + 4));
    CHECK(hipMemcpy(d_events, events.data(), events.size() * 8, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xee, bytes.size()));
    CHECK(hipMemset(d_work, 0xee, work_words * 4 + 4));
    if (what == ED_ADD) tge::launch_ed_add(d_out, height, d_events, n, d_work, m, 0);
    else if (what == ED_DECOMPRESS) tge::launch_ed_decompress(d_out, height, d_events, n, d_work, m, 0);
    else if (what == UINT256_OPS) tge::launch_uint256_ops(d_out, height, d_events, n, 0);
    else tge::launch_touched_records((uint64_t*)d_out, (uint32_t)n_records, d_events, n, family, 0);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(bytes.data(), d_out, bytes.size(), hipMemcpyDeviceToHost));
    CHECK(hipFree(d_events));
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_work));
    return 0;
#else
    return 1;
#endif
}

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: %s host|device ed_add|ed_decompress|uint256_ops|records_ed_decompress|records_uint256_ops|layout IN|- OUT|-\n", argv[0]);
        return 1;
    }
    const char *form = argv[1], *name = argv[2];
    const bool host = !strcmp(form, "host"), device = !strcmp(form, "device");
    if (!host && !device) { fprintf(stderr, "unknown form %s\n", form); return 1; }
#if !defined(__HIPCC__)
    if (device) { fprintf(stderr, "built without a device compiler: only the host form\n"); return 1; }
#endif
    if (!strcmp(name, "layout")) return layout(argv[4]);
    static const char* names[] = {"ed_add", "ed_decompress", "uint256_ops", "records_ed_decompress", "records_uint256_ops"};
    int what = -1;
    for (int i = 0; i < 5; i++) if (!strcmp(name, names[i])) what = i;
    if (what < 0) { fprintf(stderr, "unknown table %s\n", name); return 1; }
    const bool from_stdin = !strcmp(argv[3], "-");
    FILE* f = from_stdin ? stdin : fopen(argv[3], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[3]); return 1; }
    std::vector<uint8_t> bytes;
    int st = run((What)what, host, f, bytes);
    if (!from_stdin) fclose(f);
    if (st) return st;
    st = write_out(argv[4], bytes.data(), bytes.size());
    if (!st) fprintf(stderr, "ed_u256_rows %s %s: %zu bytes\n", form, name, bytes.size());
    return st;
}
