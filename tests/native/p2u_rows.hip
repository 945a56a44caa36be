// tests/native/p2u_rows.hip — the row functions of sp1_amd/csrc/tg_poseidon2_rows.hpp and tg_uint256_rows.hpp and the division of the
// latter (both included unchanged) behind a file interface, in one of two forms: `host` (the __host__ __device__ code compiled for
// the CPU in a plain loop over the rows; never opens a GPU and never loads the library) and `device` (rows: the kernels of
// tracegen_poseidon2_uint256.hip through the library's entry points; div: a gfx950 kernel of this program, one lane per record).
// tests/test_tracegen_p2u_host.py (CPU) and tests/test_gpu_tracegen_p2u.py write the inputs and check every output word.
//
//   p2u_rows FORM rows CHIP IN HEIGHT OUT     the table of CHIP = Poseidon2 | Uint256MulMod
//       IN:  n x 26 (Poseidon2) or n x 31 (Uint256MulMod) u64 event records, little-endian, n = file size / record size <= HEIGHT <= 2^20
//       OUT: width x HEIGHT u32, column-major [width][height], Montgomery words
//   p2u_rows FORM div IN OUT                  the division alone
//       IN:  n records of 24 u32: x[8], y[8], m[8] (little-endian limbs; m = 0 stands for 2^256), n = file size / 96 <= 2^20
//       OUT: n x 16 u32: (x y mod m')[8], (x y / m' mod 2^256)[8]
//   p2u_rows host layout                      the column constants as text lines "chip key column"
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc -Iinclude ...
#include <string.h>

#include "poseidon2.hpp"
#include "rows_io.hpp"
#include "sp1hip.h"
#include "tg_poseidon2_rows.hpp"
#include "tg_uint256_rows.hpp"

namespace tgp = sp1hip::tgp;
namespace tgu = sp1hip::tgu;
namespace tgf = sp1hip::tgf;

struct Chip { const char* name; int width, words; const char* entry; };
static const Chip CHIPS[] = {{"Poseidon2", tgp::WIDTH, tgp::EVENT_WORDS, "sp1hip_tracegen_riscv_poseidon2"},
                             {"Uint256MulMod", tgu::WIDTH, tgu::EVENT_WORDS, "sp1hip_tracegen_riscv_uint256_mul"}};
constexpr int DIV_REC = 3 * tgu::N, DIV_RES = 2 * tgu::N;

// what the kernels do for their lanes, as a host loop
static void host_rows(int chip, uint32_t* out, uint32_t height, const uint64_t* events, uint32_t n) {
    const p2::RoundConstants rc = p2::make_round_constants();
    for (uint32_t row = 0; row < height; row++) {
        if (chip == 0) tgp::poseidon2_row(out, height, row, row < n ? events + (size_t)row * tgp::EVENT_WORDS : nullptr, &rc);
        else tgu::uint256_mul_row(out, height, row, row < n ? events + (size_t)row * tgu::EVENT_WORDS : nullptr);
    }
}

__host__ __device__ inline void div_eval(const uint32_t* rec, uint32_t* out) {
    tgf::U<tgu::N> x, y, m, result, carry;
    for (int i = 0; i < tgu::N; i++) x.w[i] = rec[i], y.w[i] = rec[tgu::N + i], m.w[i] = rec[2 * tgu::N + i];
    tgu::divide_512(x, y, m, result, carry);
    for (int i = 0; i < tgu::N; i++) out[i] = result.w[i], out[tgu::N + i] = carry.w[i];
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(256) void div_kernel(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    uint32_t rec[DIV_REC], res[DIV_RES];
    for (int k = 0; k < DIV_REC; k++) rec[k] = in[(size_t)i * DIV_REC + k];
    div_eval(rec, res);
    for (int k = 0; k < DIV_RES; k++) out[(size_t)i * DIV_RES + k] = res[k];
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

static int device_div(const std::vector<uint32_t>& in, uint32_t n, std::vector<uint32_t>& out) {
    uint32_t *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc(&d_in, in.size() * 4 + 8));
    CHECK(hipMalloc(&d_out, out.size() * 4 + 8));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xee, out.size() * 4 + 8));
    hipLaunchKernelGGL(div_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d_in, n, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));
    return 0;
}

// the table from the real kernels, through the library's entry point (table, height, events, n, stream), loaded at run time
static int device_rows(const char* entry, std::vector<uint32_t>& out, uint32_t height, const std::vector<uint64_t>& words, uint32_t n) {
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
}
#undef CHECK
#endif

static void put(const char* chip, const char* key, int v) { printf("%s %s %d\n", chip, key, v); }

static int layout() {
    const char* n = "Poseidon2";
    put(n, "width", tgp::WIDTH); put(n, "clk_high", tgp::CLK_HIGH); put(n, "clk_low", tgp::CLK_LOW); put(n, "ptr.addr", tgp::PTR);
    put(n, "addrs.0.value", tgp::ADDRS); put(n, "memory.0.prev_value", tgp::MEMORY); put(n, "hash_result.0", tgp::HASH_RESULT);
    put(n, "hash_result_range_checkers", tgp::HASH_RESULT_RANGE_CHECKERS); put(n, "input_range_checkers", tgp::INPUT_RANGE_CHECKERS);
    put(n, "permutation", tgp::PERMUTATION); put(n, "is_real", tgp::IS_REAL);
    n = "Uint256MulMod";
    put(n, "width", tgu::WIDTH); put(n, "clk_high", tgu::CLK_HIGH); put(n, "clk_low", tgu::CLK_LOW); put(n, "x_ptr.addr", tgu::X_PTR);
    put(n, "y_ptr.addr", tgu::Y_PTR); put(n, "x_addrs.0.value", tgu::X_ADDRS); put(n, "y_and_modulus_addrs.0.value", tgu::Y_AND_MODULUS_ADDRS);
    put(n, "x_memory.0.memory_access.prev_value", tgu::X_MEMORY); put(n, "y_memory.0.memory_access.prev_value", tgu::Y_MEMORY);
    put(n, "modulus_memory.0.memory_access.prev_value", tgu::MODULUS_MEMORY); put(n, "modulus_is_zero.inverse", tgu::MODULUS_IS_ZERO);
    put(n, "modulus_is_zero.result", tgu::MODULUS_IS_ZERO + 1); put(n, "modulus_is_not_zero", tgu::MODULUS_IS_NOT_ZERO);
    put(n, "output.result", tgu::OUTPUT); put(n, "output.carry", tgu::OUTPUT + tgu::LIMBS); put(n, "output.witness", tgu::OUTPUT_WITNESS);
    put(n, "output_range_check.byte_flags", tgu::OUTPUT_RANGE_CHECK); put(n, "output_range_check.lhs_comparison_byte", tgu::OUTPUT_RANGE_CHECK + tgu::LIMBS);
    put(n, "output_range_check.rhs_comparison_byte", tgu::OUTPUT_RANGE_CHECK + tgu::LIMBS + 1); put(n, "is_real", tgu::IS_REAL);
    return 0;
}

static int usage(const char* me) {
    fprintf(stderr, "usage: %s host|device rows CHIP IN HEIGHT OUT\n       %s host|device div IN OUT\n       %s host layout\n", me, me, me);
    return 1;
}

static int divide(bool host, const char* in_path, const char* out_path) {
    std::vector<uint64_t> raw;
    if (!read_records(in_path, DIV_REC / 2, raw)) return 1;
    const size_t n = raw.size() / (DIV_REC / 2);
    if (n > (1u << 20)) { fprintf(stderr, "more than 2^20 records\n"); return 1; }
    std::vector<uint32_t> in(n * DIV_REC), out(n * DIV_RES, 0xeeeeeeeeu);
    if (n) memcpy(in.data(), raw.data(), in.size() * 4);
    if (host) {
        for (size_t i = 0; i < n; i++) div_eval(in.data() + i * DIV_REC, out.data() + i * DIV_RES);
    } else if (n) {
#if defined(__HIPCC__)
        const int st = device_div(in, (uint32_t)n, out);
        if (st) return st;
#else
        fprintf(stderr, "built without a device compiler: only the host form\n");
        return 1;
#endif
    }
    if (write_out(out_path, out.data(), out.size() * 4)) return 1;
    fprintf(stderr, "p2u_rows %s div: %zu records\n", host ? "host" : "device", n);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return usage(argv[0]);
    const char *form = argv[1], *what = argv[2];
    const bool host = !strcmp(form, "host"), device = !strcmp(form, "device");
    if (!host && !device) { fprintf(stderr, "unknown form %s\n", form); return 1; }
    if (host && argc == 3 && !strcmp(what, "layout")) return layout();
    if (!strcmp(what, "div") && argc == 5) return divide(host, argv[3], argv[4]);
    if (strcmp(what, "rows") || argc != 7) return usage(argv[0]);
    int chip = -1;
    for (int k = 0; k < 2; k++) if (!strcmp(argv[3], CHIPS[k].name)) chip = k;
    if (chip < 0) { fprintf(stderr, "unknown chip %s\n", argv[3]); return 1; }
    const Chip& c = CHIPS[chip];
    uint32_t height, n;
    std::vector<uint64_t> in;
    if (!read_rows_input(argv[5], argv[4], (size_t)c.words, height, in, n)) return 1;
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
    fprintf(stderr, "p2u_rows %s rows %s: %d x %u words\n", form, c.name, c.width, height);
    return 0;
}
