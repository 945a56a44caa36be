// tests/native/bb31_ops.hip — every operation of sp1_amd/csrc/bb31.hpp (included unchanged) on operand records, in one of two
// forms: `host` (the BB_HD code compiled for the CPU; never opens a GPU) and `device` (a gfx950 kernel, one lane per record).
// tests/test_bb31_arith.py writes the operands and checks every result word against Python integers.
//
//   bb31_ops FORM IN OUT          ("-" for IN reads stdin, "-" for OUT writes stdout)
//   IN:  u32 n, then n records of 20 u32: op, n, x_lo, x_hi, s[16]   (little-endian words; a = s[0], b = s[1])
//   OUT: n results of 16 u32 (a scalar result in word 0, the other words 0; an unknown op: all words 0xffffffff)
//
// to_monty, pow and two_adic_generator are host functions in the header (the library calls them on the host only): in the
// device form their records are evaluated by the host after the kernel has run, and the kernel leaves them untouched.
// The round constants of `permute` come from the header's make_round_constants on the host, as in the library.
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc ...
// The host form alone also builds with a plain C++ compiler: g++ -x c++ -D__HIP_PLATFORM_AMD__ -I<rocm>/include ...
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bb31.hpp"

namespace bb = sp1hip::bb;

enum Op : uint32_t {
    OP_ADD, OP_SUB, OP_MUL, OP_REDUCE, OP_TO_MONTY, OP_POW, OP_GEN, OP_EXTERNAL, OP_INTERNAL, OP_SBOX, OP_PERMUTE, OP_COUNT
};
constexpr int REC = 20, RES = 16;

BB_HD bool host_only(uint32_t op) { return op == OP_TO_MONTY || op == OP_POW || op == OP_GEN; }

BB_HD void eval(const uint32_t* rec, const bb::RoundConstants* rc, uint32_t* out) {
    const uint32_t n = rec[1];
    const uint64_t x = (uint64_t)rec[2] | ((uint64_t)rec[3] << 32);
    uint32_t s[16];
    for (int i = 0; i < 16; i++) s[i] = rec[4 + i];
    uint32_t r = 0;
    bool scalar = true;
    switch (rec[0]) {
    case OP_ADD: r = bb::add(s[0], s[1]); break;
    case OP_SUB: r = bb::sub(s[0], s[1]); break;
    case OP_MUL: r = bb::mul(s[0], s[1]); break;
    case OP_REDUCE: r = bb::monty_reduce(x); break;
    case OP_SBOX: r = bb::sbox(s[0]); break;
#if !defined(__HIP_DEVICE_COMPILE__)
    case OP_TO_MONTY: r = bb::to_monty(s[0]); break;
    case OP_POW: r = bb::pow(s[0], x); break;
    case OP_GEN: r = n <= (uint32_t)bb::TWO_ADICITY ? bb::two_adic_generator((int)n) : 0xffffffffu; break;
#endif
    case OP_EXTERNAL: bb::external_linear(s); scalar = false; break;
    case OP_INTERNAL: bb::internal_linear(s); scalar = false; break;
    case OP_PERMUTE: bb::permute(s, rc); scalar = false; break;
    default: for (int i = 0; i < 16; i++) s[i] = 0xffffffffu; scalar = false; break;
    }
    for (int i = 0; i < RES; i++) out[i] = scalar ? (i == 0 ? r : 0u) : s[i];
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(256) void ops_kernel(const uint32_t* __restrict__ in, uint32_t n, const bb::RoundConstants* __restrict__ rc,
                                                  uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (host_only(in[(size_t)i * REC])) return;
    uint32_t r[RES];
    eval(in + (size_t)i * REC, rc, r);
    for (int k = 0; k < RES; k++) out[(size_t)i * RES + k] = r[k];
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

static int run_device(const std::vector<uint32_t>& in, uint32_t n, const bb::RoundConstants& rc, std::vector<uint32_t>& out) {
    uint32_t *d_in = nullptr, *d_out = nullptr;
    bb::RoundConstants* d_rc = nullptr;
    CHECK(hipMalloc(&d_in, in.size() * 4 + 4));
    CHECK(hipMalloc(&d_out, (size_t)n * RES * 4 + 4));
    CHECK(hipMalloc(&d_rc, sizeof rc));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_rc, &rc, sizeof rc, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0, (size_t)n * RES * 4 + 4));
    hipLaunchKernelGGL(ops_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d_in, n, d_rc, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, (size_t)n * RES * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));
    CHECK(hipFree(d_rc));
    return 0;
}
#endif

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s host|device IN|- OUT|-\n", argv[0]);
        return 1;
    }
    const char* form = argv[1];
    const bool from_stdin = !strcmp(argv[2], "-"), to_stdout = !strcmp(argv[3], "-");
    FILE* f = from_stdin ? stdin : fopen(argv[2], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n == 0 || n > (1u << 24)) { fprintf(stderr, "bad record count\n"); if (!from_stdin) fclose(f); return 1; }
    std::vector<uint32_t> in((size_t)n * REC);
    const size_t got = fread(in.data(), 4, in.size(), f);
    if (!from_stdin) fclose(f);
    if (got != in.size()) { fprintf(stderr, "short input: %zu of %zu words\n", got, in.size()); return 1; }
    std::vector<uint32_t> out((size_t)n * RES);
    const bb::RoundConstants rc = bb::make_round_constants();
    if (!strcmp(form, "host")) {
        for (uint32_t i = 0; i < n; i++) eval(in.data() + (size_t)i * REC, &rc, out.data() + (size_t)i * RES);
    } else if (!strcmp(form, "device")) {
#if defined(__HIPCC__)
        const int st = run_device(in, n, rc, out);
        if (st) return st;
        for (uint32_t i = 0; i < n; i++)
            if (host_only(in[(size_t)i * REC])) eval(in.data() + (size_t)i * REC, &rc, out.data() + (size_t)i * RES);
#else
        fprintf(stderr, "built without a device compiler: only the host form\n");
        return 1;
#endif
    } else {
        fprintf(stderr, "unknown form %s\n", form);
        return 1;
    }
    FILE* g = to_stdout ? stdout : fopen(argv[3], "wb");
    if (!g) { fprintf(stderr, "cannot open %s\n", argv[3]); return 1; }
    const size_t put = fwrite(out.data(), 4, out.size(), g);
    if (!to_stdout) fclose(g); else fflush(g);
    if (put != out.size()) { fprintf(stderr, "short write\n"); return 1; }
    fprintf(stderr, "bb31_ops %s: %u records\n", form, n);
    return 0;
}
