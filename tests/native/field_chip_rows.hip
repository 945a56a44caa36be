// tests/native/field_chip_rows.hip — the two-phase rows of sp1_amd/csrc/tg_field_chip_rows.hpp (included unchanged) behind a file
// interface, in one of two forms: `host` (both phases as loops over the __host__ __device__ code compiled for the CPU; never opens a
// GPU) and `device` (the header's gfx950 kernels, launched as libsp1hip.so launches them, with a work buffer of this program's own).
// tests/test_tracegen_field_chips_host.py (CPU) and tests/test_gpu_tracegen_field_chips.py write the inputs and check every word.
//
//   field_chip_rows FORM FAMILY IN OUT     the table of SP1HIP_RV64_FAMILY_* FAMILY (0..11) of an event file
//       IN:  u32 n_events, u32 height, then n_events x (the family's event words) u64   (little-endian)
//       OUT: width x height u32, column-major [width][height], Montgomery words
//   field_chip_rows host layout - OUT      the column constants of the twelve chips as text lines "chip key offset"
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc ...
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "tg_field_chip_rows.hpp"

namespace tgc = sp1hip::tgc;
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
};
template <int N> static void field_ops(Text& t, const char* chip, int first, std::initializer_list<const char*> names) {
    int col = first;
    for (const char* name : names) {
        t.put(chip, std::string(name) + ".result", col + tgf::FieldOp<N>::RESULT);
        t.put(chip, std::string(name) + ".carry", col + tgf::FieldOp<N>::CARRY);
        t.put(chip, std::string(name) + ".witness", col + tgf::FieldOp<N>::WITNESS_AT);
        col += tgf::FieldOp<N>::COLS;
    }
}
template <int N> static void field_lts(Text& t, const char* chip, int first, std::initializer_list<const char*> names) {
    int col = first;
    for (const char* name : names) {
        t.put(chip, std::string(name) + ".byte_flags", col + tgf::FieldLt<N>::BYTE_FLAGS);
        t.put(chip, std::string(name) + ".lhs_comparison_byte", col + tgf::FieldLt<N>::LHS_BYTE);
        t.put(chip, std::string(name) + ".rhs_comparison_byte", col + tgf::FieldLt<N>::RHS_BYTE);
        col += tgf::FieldLt<N>::COLS;
    }
}
template <class H, int W> static void head(Text& t, const char* chip, const char* x, const char* y) {
    t.put(chip, "is_real", H::IS_REAL); t.put(chip, "clk_high", H::CLK_HIGH); t.put(chip, "clk_low", H::CLK_LOW);
    const std::string last = "." + std::to_string(W - 1);
    t.put(chip, std::string(x) + "_ptr.addr", H::X_PTR); t.put(chip, std::string(x) + "_addrs.0.value", H::X_ADDRS);
    t.put(chip, std::string(x) + "_addrs" + last + ".value", H::X_ADDRS + 3 * (W - 1));
    t.put(chip, std::string(x) + "_access.0.memory_access.prev_value", H::X_ACCESS);
    t.put(chip, std::string(x) + "_access" + last + ".prev_value_u8.low_bytes", H::X_ACCESS + (W - 1) * tgf::MEMORY_ACCESS_U8_COLS + 9);
    if (y) {
        t.put(chip, std::string(y) + "_ptr.addr", H::Y_PTR); t.put(chip, std::string(y) + "_addrs.0.value", H::Y_ADDRS);
        t.put(chip, std::string(y) + "_access.0.memory_access.prev_value", H::Y_ACCESS);
        t.put(chip, std::string(y) + "_access" + last + ".prev_value_u8.low_bytes", H::Y_ACCESS + (W - 1) * tgf::MEMORY_ACCESS_U8_COLS + 9);
    }
}
template <int N> static void describe(Text& t, tgc::CurveAdd<N>, const char* chip) {
    using S = tgc::CurveAdd<N>;
    head<typename S::H, N>(t, chip, "p", "q");
    field_ops<N>(t, chip, S::FIRST_OP, {"slope_denominator", "inverse_check", "slope_numerator", "slope", "slope_squared", "p_x_plus_q_x", "x3_ins",
                                         "p_x_minus_x", "y3_ins", "slope_times_p_x_minus_x"});
    field_lts<N>(t, chip, S::C::X3_RANGE, {"x3_range", "y3_range"});
}
template <int N> static void describe(Text& t, tgc::CurveDouble<N>, const char* chip) {
    using S = tgc::CurveDouble<N>;
    head<typename S::H, N>(t, chip, "p", nullptr);
    field_ops<N>(t, chip, S::FIRST_OP, {"slope_denominator", "slope_numerator", "slope", "p_x_squared", "p_x_squared_times_3", "slope_squared",
                                         "p_x_plus_p_x", "x3_ins", "p_x_minus_x", "y3_ins", "slope_times_p_x_minus_x"});
    field_lts<N>(t, chip, S::C::X3_RANGE, {"x3_range", "y3_range"});
}
template <int N> static void describe(Text& t, tgc::FpOp<N>, const char* chip) {
    using S = tgc::FpOp<N>;
    head<typename S::H, S::W>(t, chip, "x", "y");
    t.put(chip, "is_add", S::H::SELECT); t.put(chip, "is_sub", S::H::SELECT + 1); t.put(chip, "is_mul", S::H::SELECT + 2);
    field_ops<N>(t, chip, S::OUTPUT, {"output"});
    field_lts<N>(t, chip, S::OUTPUT_RANGE, {"output_range"});
}
template <int N> static void describe(Text& t, tgc::Fp2AddSub<N>, const char* chip) {
    using S = tgc::Fp2AddSub<N>;
    head<typename S::H, N>(t, chip, "x", "y");
    t.put(chip, "is_add", S::H::SELECT);
    field_ops<N>(t, chip, S::C0, {"c0", "c1"});
    field_lts<N>(t, chip, S::C0_RANGE, {"c0_range", "c1_range"});
}
template <int N> static void describe(Text& t, tgc::Fp2Mul<N>, const char* chip) {
    using S = tgc::Fp2Mul<N>;
    head<typename S::H, N>(t, chip, "x", "y");
    field_ops<N>(t, chip, S::A0_MUL_B0, {"a0_mul_b0", "a1_mul_b1", "a0_mul_b1", "a1_mul_b0", "c0", "c1"});
    field_lts<N>(t, chip, S::C0_RANGE, {"c0_range", "c1_range"});
}

static int layout(const char* path) {
    Text t;
    for (uint32_t family = 0; family < tgc::FAMILIES; family++)
        tgc::with_family(family, [&](auto shape, const auto&, const auto& k, const char* chip) {
            using Shape = decltype(shape);
            t.put(chip, "width", Shape::WIDTH);
            t.put(chip, "event_words", Shape::EVENT_WORDS);
            t.put(chip, "ops", Shape::OPS);
            t.put(chip, "witness_offset", (int)k.offset);
            describe(t, shape, chip);
        });
    return write_out(path, t.s.data(), t.s.size());
}

// ----------------------------------------------------------------------------------------------------------------------- tables
template <class Shape, class M, class K>
static int table(bool host, FILE* f, std::vector<uint32_t>& out, const M& m, const K& k) {
    uint32_t head[2] = {0, 0};
    if (!read_exact(f, head, 8) || head[0] > head[1] || head[1] > (1u << 20)) { fprintf(stderr, "bad header: need n_events <= height <= 2^20\n"); return 1; }
    const uint32_t n = head[0], height = head[1];
    std::vector<uint64_t> events((size_t)n * Shape::EVENT_WORDS);
    if (!read_exact(f, events.data(), events.size() * 8)) { fprintf(stderr, "short input\n"); return 1; }
    out.assign((size_t)Shape::WIDTH * height, 0xeeeeeeeeu);
    const size_t work_words = tgc::Work<Shape::LIMBS>::words(height, Shape::OPS);
    if (host) {
        std::vector<uint32_t> work(work_words, 0xeeeeeeeeu);
        tgc::host_table<Shape>(out.data(), height, events.data(), n, work.data(), m, k);
        return 0;
    }
    if (height == 0) return 0;
#if defined(__HIPCC__)
    uint64_t* d_events = nullptr;
    uint32_t *d_out = nullptr, *d_work = nullptr;
    CHECK(hipMalloc(&d_events, events.size() * 8 + 8));
    CHECK(hipMalloc(&d_out, out.size() * 4));
    CHECK(hipMalloc(&d_work, work_words * 4));
    CHECK(hipMemcpy(d_events, events.data(), events.size() * 8, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xee, out.size() * 4));
    CHECK(hipMemset(d_work, 0xee, work_words * 4));
    tgc::launch_table<Shape>(d_out, height, d_events, n, d_work, m, k, 0);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
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
        fprintf(stderr, "usage: %s host|device FAMILY|layout IN|- OUT|-\n", argv[0]);
        return 1;
    }
    const char *form = argv[1], *what = argv[2];
    const bool host = !strcmp(form, "host"), device = !strcmp(form, "device");
    if (!host && !device) { fprintf(stderr, "unknown form %s\n", form); return 1; }
#if !defined(__HIPCC__)
    if (device) { fprintf(stderr, "built without a device compiler: only the host form\n"); return 1; }
#endif
    if (!strcmp(what, "layout")) return layout(argv[4]);
    char* end = nullptr;
    const unsigned long family = strtoul(what, &end, 10);
    if (end == what || *end || family >= tgc::FAMILIES) { fprintf(stderr, "unknown family %s: 0..11\n", what); return 1; }
    const bool from_stdin = !strcmp(argv[3], "-");
    FILE* f = from_stdin ? stdin : fopen(argv[3], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[3]); return 1; }
    int st = 1;
    std::vector<uint32_t> out;
    tgc::with_family((uint32_t)family, [&](auto shape, const auto& m, const auto& k, const char*) { st = table<decltype(shape)>(host, f, out, m, k); });
    if (!from_stdin) fclose(f);
    if (st) return st;
    st = write_out(argv[4], out.data(), out.size() * 4);
    if (!st) fprintf(stderr, "field_chip_rows %s %s: %zu words\n", form, what, out.size());
    return st;
}
