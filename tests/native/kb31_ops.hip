// tests/native/kb31_ops.hip — every operation of sp1_amd/csrc/kb31.hpp (included unchanged) on operand records, in one of
// two forms: `host` (the KB_HD code compiled for the CPU; never opens a GPU) and `device` (a gfx950 kernel, one lane per
// record). tests/test_kb31_arith.py writes the operands and checks every result word against Python integers.
//
//   kb31_ops FORM IN OUT          ("-" for IN reads stdin, "-" for OUT writes stdout)
//   IN:  u32 n, then n records of 16 u32: op, n, a[4], b[4], c[4], x_lo, x_hi   (little-endian words)
//   OUT: n results of 4 u32 (a base-field result in word 0; an unknown op: all words 0xffffffff)
//
// The accumulator operations run `n` terms inside one record. Term r of `dot` is e = rot^r(a), v = b[r & 3]; term r of `edot`
// is a = rot^r(a), a3 = rot^r(c), b = rot^r(b), where rot^r rotates the four words by (r & 3) places when the record's x_lo
// is 1 and is the identity when it is 0. c carries 3a: it is an operand, so this file never forms it with the header's code.
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc ...
// The host form alone also builds with a plain C++ compiler: g++ -x c++ -D__HIP_PLATFORM_AMD__ -I<rocm>/include ...
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "kb31.hpp"

using kb::Ext;

enum Op : uint32_t {
    OP_ADD, OP_SUB, OP_NEG, OP_DBL, OP_MUL, OP_SQR, OP_TO_MONTY, OP_FROM_MONTY, OP_REDUCE_LAZY, OP_REDUCE, OP_REDUCE_WIDE,
    OP_POW, OP_INV, OP_GEN, OP_REVBITS, OP_EXT_ADD, OP_EXT_SUB, OP_EXT_MUL_BASE, OP_EXT_MUL, OP_EXT_INV, OP_DOT, OP_EDOT,
    OP_DOT_REDUCE64, OP_COUNT
};
constexpr int REC = 16, RES = 4;
constexpr uint32_t MAX_TERMS = 1u << 16;

KB_HD Ext rot(const Ext& e, uint32_t k) { return Ext{{e.c[k & 3], e.c[(k + 1) & 3], e.c[(k + 2) & 3], e.c[(k + 3) & 3]}}; }

KB_HD Ext eval(const uint32_t* rec) {
    const uint32_t n = rec[1];
    Ext a, b, c;
    for (int i = 0; i < 4; i++) {
        a.c[i] = rec[2 + i];
        b.c[i] = rec[6 + i];
        c.c[i] = rec[10 + i];
    }
    const uint64_t x = (uint64_t)rec[14] | ((uint64_t)rec[15] << 32);
    switch (rec[0]) {
    case OP_ADD: return kb::ext_from_base(kb::add(a.c[0], b.c[0]));
    case OP_SUB: return kb::ext_from_base(kb::sub(a.c[0], b.c[0]));
    case OP_NEG: return kb::ext_from_base(kb::neg(a.c[0]));
    case OP_DBL: return kb::ext_from_base(kb::dbl(a.c[0]));
    case OP_MUL: return kb::ext_from_base(kb::mul(a.c[0], b.c[0]));
    case OP_SQR: return kb::ext_from_base(kb::sqr(a.c[0]));
    case OP_TO_MONTY: return kb::ext_from_base(kb::to_monty(a.c[0]));
    case OP_FROM_MONTY: return kb::ext_from_base(kb::from_monty(a.c[0]));
    case OP_REDUCE_LAZY: return kb::ext_from_base(kb::monty_reduce_lazy(x));
    case OP_REDUCE: return kb::ext_from_base(kb::monty_reduce(x));
    case OP_REDUCE_WIDE: return kb::ext_from_base(kb::monty_reduce_wide(x));
    case OP_POW: return kb::ext_from_base(kb::pow(a.c[0], x));
    case OP_INV: return kb::ext_from_base(kb::inv(a.c[0]));
    case OP_GEN: return kb::ext_from_base(n <= (uint32_t)kb::TWO_ADICITY ? kb::two_adic_generator((int)n) : 0xffffffffu);
    case OP_REVBITS: return kb::ext_from_base(n <= 32u ? kb::reverse_bits_len(a.c[0], (int)n) : 0xffffffffu);
    case OP_EXT_ADD: return kb::ext_add(a, b);
    case OP_EXT_SUB: return kb::ext_sub(a, b);
    case OP_EXT_MUL_BASE: return kb::ext_mul_base(a, b.c[0]);
    case OP_EXT_MUL: return kb::ext_mul(a, b);
    case OP_EXT_INV: return kb::ext_inv(a);
    case OP_DOT: {
        kb::DotAcc acc;
        kb::dot_init(acc);
        const uint32_t terms = n <= MAX_TERMS ? n : 0u, vary = rec[14] & 1u;
        for (uint32_t r = 0; r < terms; r++) kb::dot_add(acc, rot(a, vary * r), b.c[(vary * r) & 3]);
        return kb::dot_finish(acc);
    }
    case OP_EDOT: {
        kb::DotAcc acc;
        kb::dot_init(acc);
        const uint32_t terms = n <= (MAX_TERMS >> 2) ? n : 0u, vary = rec[14] & 1u;
        for (uint32_t r = 0; r < terms; r++) kb::edot_add(acc, rot(a, vary * r), rot(c, vary * r), rot(b, vary * r));
        return kb::dot_finish(acc);
    }
    case OP_DOT_REDUCE64: return kb::ext_from_base(kb::dot_reduce64(x));
    default: return Ext{{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}};
    }
}

#if defined(__HIPCC__)
__global__ __launch_bounds__(256) void ops_kernel(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const Ext r = eval(in + (size_t)i * REC);
    for (int k = 0; k < RES; k++) out[(size_t)i * RES + k] = r.c[k];
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

static int run_device(const std::vector<uint32_t>& in, uint32_t n, std::vector<uint32_t>& out) {
    uint32_t *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc(&d_in, in.size() * 4 + 4));
    CHECK(hipMalloc(&d_out, (size_t)n * RES * 4 + 4));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0, (size_t)n * RES * 4 + 4));
    hipLaunchKernelGGL(ops_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d_in, n, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, (size_t)n * RES * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));
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
    if (!strcmp(form, "host")) {
        for (uint32_t i = 0; i < n; i++) {
            const Ext r = eval(in.data() + (size_t)i * REC);
            memcpy(out.data() + (size_t)i * RES, r.c, RES * 4);
        }
    } else if (!strcmp(form, "device")) {
#if defined(__HIPCC__)
        const int st = run_device(in, n, out);
        if (st) return st;
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
    fprintf(stderr, "kb31_ops %s: %u records\n", form, n);
    return 0;
}
