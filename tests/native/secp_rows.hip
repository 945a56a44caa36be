// tests/native/secp_rows.hip — the row functions of sp1_amd/csrc/tg_field_op.hpp and the arithmetic of sp1_amd/csrc/fp256.hpp (both
// included unchanged) behind a file interface, in one of two forms: `host` (the __host__ __device__ code compiled for the CPU;
// never opens a GPU) and `device` (gfx950 kernels, one lane per row / record, as libsp1hip.so launches them).
// tests/test_tracegen_secp_host.py (CPU) and tests/test_gpu_tracegen_secp.py write the inputs and check every output word.
//
//   secp_rows FORM add|double IN OUT     the Secp256k1AddAssign / Secp256k1DoubleAssign table of an event file
//       IN:  u32 n_events, u32 height, then n_events x 43 (add) or 26 (double) u64   (little-endian)
//       OUT: width x height u32, column-major [width][height], Montgomery words
//   secp_rows FORM fp IN OUT             fp256 on operand records, modulo a modulus given as data
//       IN:  u32 n, 8 u32 limbs of an odd modulus p, then n records of 17 u32: op (0 add, 1 sub, 2 mul, 3 inv), a[8], b[8]; a, b < p
//       OUT: n x 16 u32: result[8], then the quotient ((a + b - result) / p or (a b - result) / p; 0 for sub and inv)
//   secp_rows host layout - OUT          the column constants of both chips as text lines "chip key offset"
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc ...
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "fp256.hpp"
#include "tg_field_op.hpp"

namespace fp = sp1hip::fp256;
namespace tgf = sp1hip::tgf;

constexpr int N = 8;
constexpr uint32_t OFFSET = 1u << 14;
using Add = tgf::WeierstrassAdd<N>;
using Double = tgf::WeierstrassDouble<N>;
constexpr int FP_REC = 1 + 2 * N, FP_RES = 2 * N;

static fp::Modulus<N> secp256k1() {
    const uint32_t p[N] = {0xFFFFFC2Fu, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    return fp::make_modulus<N>(p);
}

__host__ __device__ inline void fp_eval(const uint32_t* rec, const fp::Modulus<N>& m, uint32_t* out) {
    fp::U<N> a, b, r = fp::small<N>(0), q = fp::small<N>(0);
    for (int i = 0; i < N; i++) a.w[i] = rec[1 + i], b.w[i] = rec[1 + N + i];
    uint32_t c = 0;
    switch (rec[0]) {
    case 0: r = fp::add(a, b, m, &c); q = fp::small<N>(c); break;
    case 1: r = fp::sub(a, b, m); break;
    case 2: r = fp::mul(a, b, m); q = fp::mul_quotient(a, b, r, m); break;
    case 3: r = fp::inv(a, m); break;
    default: r = fp::small<N>(0xffffffffu); break;
    }
    for (int i = 0; i < N; i++) out[i] = r.w[i], out[N + i] = q.w[i];
}

__host__ __device__ inline void row_eval(bool add, uint32_t* out, uint32_t height, uint32_t row, const uint64_t* events, uint32_t n,
                                         const fp::Modulus<N>& m) {
    if (add) tgf::weierstrass_add_row<N>(out, height, row, row < n ? events + (size_t)row * Add::EVENT_WORDS : nullptr, m, OFFSET);
    else tgf::weierstrass_double_row<N>(out, height, row, row < n ? events + (size_t)row * Double::EVENT_WORDS : nullptr, m, fp::small<N>(0), OFFSET);
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(256) void add_rows_kernel(uint32_t* __restrict__ out, uint32_t height, const uint64_t* __restrict__ events, uint32_t n,
                                                       const fp::Modulus<N> m) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row < height) row_eval(true, out, height, row, events, n, m);
}
__global__ __launch_bounds__(256) void double_rows_kernel(uint32_t* __restrict__ out, uint32_t height, const uint64_t* __restrict__ events, uint32_t n,
                                                          const fp::Modulus<N> m) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row < height) row_eval(false, out, height, row, events, n, m);
}
__global__ __launch_bounds__(256) void fp_kernel(const uint32_t* __restrict__ in, uint32_t n, const fp::Modulus<N> m, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t rec[FP_REC], res[FP_RES];
    for (int k = 0; k < FP_REC; k++) rec[k] = in[(size_t)i * FP_REC + k];
    fp_eval(rec, m, res);
    for (int k = 0; k < FP_RES; k++) out[(size_t)i * FP_RES + k] = res[k];
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

// in: `in_bytes` bytes copied to the device; the kernel writes out.size() words
template <class Launch> static int run_device(const void* in, size_t in_bytes, std::vector<uint32_t>& out, Launch launch) {
    void* d_in = nullptr;
    uint32_t* d_out = nullptr;
    CHECK(hipMalloc(&d_in, in_bytes + 8));
    CHECK(hipMalloc(&d_out, out.size() * 4 + 8));
    CHECK(hipMemcpy(d_in, in, in_bytes, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xee, out.size() * 4 + 8));
    launch(d_in, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));
    return 0;
}
#endif

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

static int layout(const char* path) {
    std::vector<char> text(1 << 14);
    size_t at = 0;
    auto put = [&](const char* chip, const char* key, int v) { at += snprintf(text.data() + at, text.size() - at, "%s %s %d\n", chip, key, v); };
    auto field_op = [&](const char* chip, const char* name, int col) {
        char key[96];
        snprintf(key, sizeof key, "%s.result", name); put(chip, key, col + tgf::FieldOp<N>::RESULT);
        snprintf(key, sizeof key, "%s.carry", name); put(chip, key, col + tgf::FieldOp<N>::CARRY);
        snprintf(key, sizeof key, "%s.witness", name); put(chip, key, col + tgf::FieldOp<N>::WITNESS_AT);
    };
    auto field_lt = [&](const char* chip, const char* name, int col) {
        char key[96];
        snprintf(key, sizeof key, "%s.byte_flags", name); put(chip, key, col + tgf::FieldLt<N>::BYTE_FLAGS);
        snprintf(key, sizeof key, "%s.lhs_comparison_byte", name); put(chip, key, col + tgf::FieldLt<N>::LHS_BYTE);
        snprintf(key, sizeof key, "%s.rhs_comparison_byte", name); put(chip, key, col + tgf::FieldLt<N>::RHS_BYTE);
    };
    const char* a = "Secp256k1AddAssign";
    put(a, "width", Add::WIDTH); put(a, "is_real", Add::IS_REAL); put(a, "clk_high", Add::CLK_HIGH); put(a, "clk_low", Add::CLK_LOW);
    put(a, "p_ptr.addr", Add::P_PTR); put(a, "q_ptr.addr", Add::Q_PTR); put(a, "p_addrs.0.value", Add::P_ADDRS); put(a, "q_addrs.0.value", Add::Q_ADDRS);
    put(a, "p_access.0.memory_access.prev_value", Add::P_ACCESS); put(a, "q_access.0.memory_access.prev_value", Add::Q_ACCESS);
    put(a, "q_access.7.prev_value_u8.low_bytes", Add::Q_ACCESS + 7 * tgf::MEMORY_ACCESS_U8_COLS + 9);
    field_op(a, "slope_denominator", Add::SLOPE_DENOMINATOR); field_op(a, "inverse_check", Add::INVERSE_CHECK);
    field_op(a, "slope_numerator", Add::SLOPE_NUMERATOR); field_op(a, "slope", Add::SLOPE); field_op(a, "slope_squared", Add::SLOPE_SQUARED);
    field_op(a, "p_x_plus_q_x", Add::P_X_PLUS_Q_X); field_op(a, "x3_ins", Add::X3_INS); field_op(a, "p_x_minus_x", Add::P_X_MINUS_X);
    field_op(a, "y3_ins", Add::Y3_INS); field_op(a, "slope_times_p_x_minus_x", Add::SLOPE_TIMES_P_X_MINUS_X);
    field_lt(a, "x3_range", Add::X3_RANGE); field_lt(a, "y3_range", Add::Y3_RANGE);
    const char* d = "Secp256k1DoubleAssign";
    put(d, "width", Double::WIDTH); put(d, "is_real", Double::IS_REAL); put(d, "clk_high", Double::CLK_HIGH); put(d, "clk_low", Double::CLK_LOW);
    put(d, "p_ptr.addr", Double::P_PTR); put(d, "p_addrs.0.value", Double::P_ADDRS); put(d, "p_access.0.memory_access.prev_value", Double::P_ACCESS);
    put(d, "p_access.7.prev_value_u8.low_bytes", Double::P_ACCESS + 7 * tgf::MEMORY_ACCESS_U8_COLS + 9);
    field_op(d, "slope_denominator", Double::SLOPE_DENOMINATOR); field_op(d, "slope_numerator", Double::SLOPE_NUMERATOR); field_op(d, "slope", Double::SLOPE);
    field_op(d, "p_x_squared", Double::P_X_SQUARED); field_op(d, "p_x_squared_times_3", Double::P_X_SQUARED_TIMES_3);
    field_op(d, "slope_squared", Double::SLOPE_SQUARED); field_op(d, "p_x_plus_p_x", Double::P_X_PLUS_P_X); field_op(d, "x3_ins", Double::X3_INS);
    field_op(d, "p_x_minus_x", Double::P_X_MINUS_X); field_op(d, "y3_ins", Double::Y3_INS);
    field_op(d, "slope_times_p_x_minus_x", Double::SLOPE_TIMES_P_X_MINUS_X);
    field_lt(d, "x3_range", Double::X3_RANGE); field_lt(d, "y3_range", Double::Y3_RANGE);
    return write_out(path, text.data(), at);
}

int main(int argc, char** argv) {
    if (argc != 5) {
        fprintf(stderr, "usage: %s host|device add|double|fp|layout IN|- OUT|-\n", argv[0]);
        return 1;
    }
    const char *form = argv[1], *what = argv[2];
    const bool host = !strcmp(form, "host"), device = !strcmp(form, "device");
    if (!host && !device) { fprintf(stderr, "unknown form %s\n", form); return 1; }
#if !defined(__HIPCC__)
    if (device) { fprintf(stderr, "built without a device compiler: only the host form\n"); return 1; }
#endif
    if (!strcmp(what, "layout")) return layout(argv[4]);
    const bool from_stdin = !strcmp(argv[3], "-");
    FILE* f = from_stdin ? stdin : fopen(argv[3], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[3]); return 1; }
    int st = 1;
    std::vector<uint32_t> out;
    if (!strcmp(what, "add") || !strcmp(what, "double")) {
        const bool add = !strcmp(what, "add");
        const int words = add ? Add::EVENT_WORDS : Double::EVENT_WORDS, width = add ? Add::WIDTH : Double::WIDTH;
        uint32_t head[2] = {0, 0};
        std::vector<uint64_t> events;
        if (!read_exact(f, head, 8) || head[0] > head[1] || head[1] > (1u << 20)) { fprintf(stderr, "bad header: need n_events <= height <= 2^20\n"); goto done; }
        events.resize((size_t)head[0] * words);
        if (!read_exact(f, events.data(), events.size() * 8)) { fprintf(stderr, "short input\n"); goto done; }
        out.assign((size_t)width * head[1], 0xeeeeeeeeu);
        {
            const fp::Modulus<N> m = secp256k1();
            const uint32_t n = head[0], height = head[1];
            if (host) {
                for (uint32_t row = 0; row < height; row++) row_eval(add, out.data(), height, row, events.data(), n, m);
                st = 0;
            } else if (height == 0) {
                st = 0;
            } else {
#if defined(__HIPCC__)
                st = run_device(events.data(), events.size() * 8, out, [&](void* d_in, uint32_t* d_out) {
                    if (add) hipLaunchKernelGGL(add_rows_kernel, dim3((height + 255) / 256), dim3(256), 0, 0, d_out, height, (const uint64_t*)d_in, n, m);
                    else hipLaunchKernelGGL(double_rows_kernel, dim3((height + 255) / 256), dim3(256), 0, 0, d_out, height, (const uint64_t*)d_in, n, m);
                });
#endif
            }
        }
    } else if (!strcmp(what, "fp")) {
        uint32_t n = 0, p[N];
        std::vector<uint32_t> in;
        if (!read_exact(f, &n, 4) || !read_exact(f, p, sizeof p) || n == 0 || n > (1u << 20) || !(p[0] & 1)) { fprintf(stderr, "bad header: need 0 < n <= 2^20, p odd\n"); goto done; }
        in.resize((size_t)n * FP_REC);
        if (!read_exact(f, in.data(), in.size() * 4)) { fprintf(stderr, "short input\n"); goto done; }
        out.assign((size_t)n * FP_RES, 0);
        {
            const fp::Modulus<N> m = fp::make_modulus<N>(p);
            if (host) {
                for (uint32_t i = 0; i < n; i++) fp_eval(in.data() + (size_t)i * FP_REC, m, out.data() + (size_t)i * FP_RES);
                st = 0;
            } else {
#if defined(__HIPCC__)
                st = run_device(in.data(), in.size() * 4, out, [&](void* d_in, uint32_t* d_out) {
                    hipLaunchKernelGGL(fp_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, (const uint32_t*)d_in, n, m, d_out);
                });
#endif
            }
        }
    } else {
        fprintf(stderr, "unknown table %s\n", what);
    }
done:
    if (!from_stdin) fclose(f);
    if (st) return st;
    st = write_out(argv[4], out.data(), out.size() * 4);
    if (!st) fprintf(stderr, "secp_rows %s %s: %zu words\n", form, what, out.size());
    return st;
}
