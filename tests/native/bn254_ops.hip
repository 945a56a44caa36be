// tests/native/bn254_ops.hip — every operation of sp1_amd/csrc/bn254.hpp (included unchanged) on operands read from a file,
// in one of three forms: `host` (the BN_HD code compiled for the CPU; never opens a GPU), `mad` and `lohi` (a gfx950 kernel,
// one lane per record, with the Montgomery product in MulForm::Mad or MulForm::LoHi). tests/test_outer_arith.py writes the
// operands and checks every result against Python integers.
//
//   bn254_ops FORM IN OUT
//   IN:  u32 n, then n records of 17 u32: op, a[8], b[8] (little-endian words)
//   OUT: n results of 8 u32 (cmp: the int result in word 0; an unknown op: all words 0xffffffff)
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc -Iinclude ...
// The host form alone also builds with a plain C++ compiler: g++ -x c++ -D__HIP_PLATFORM_AMD__ -I<rocm>/include ...
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "bn254.hpp"

using bn254::Fr;
using bn254::MulForm;

enum Op : uint32_t {
    OP_MUL, OP_SQR, OP_ADD, OP_DBL, OP_SUB, OP_TO_MONTY, OP_FROM_MONTY, OP_ADD_LAZY, OP_REDUCE_2P, OP_REDUCE_4P, OP_REDUCE_5P,
    OP_COND_SUB, OP_CMP, OP_PACK31, OP_COUNT
};
constexpr int REC = 17;

template <MulForm F> BN_HD Fr eval(const uint32_t* rec) {
    Fr a, b;
    uint32_t v[8];
    for (int i = 0; i < 8; i++) {
        a.w[i] = rec[1 + i];
        b.w[i] = rec[9 + i];
        v[i] = rec[1 + i];
    }
    switch (rec[0]) {
    case OP_MUL: return bn254::mul<F>(a, b);
    case OP_SQR: return bn254::sqr<F>(a);
    case OP_ADD: return bn254::add(a, b);
    case OP_DBL: return bn254::dbl(a);
    case OP_SUB: return bn254::sub(a, b);
    case OP_TO_MONTY: return bn254::to_monty<F>(a);
    case OP_FROM_MONTY: return bn254::from_monty<F>(a);
    case OP_ADD_LAZY: return bn254::add_lazy(a, b);
    case OP_REDUCE_2P: return bn254::reduce_2p(a);
    case OP_REDUCE_4P: return bn254::reduce_4p(a);
    case OP_REDUCE_5P: return bn254::reduce_5p(a);
    case OP_COND_SUB: return bn254::cond_sub(a, b);
    case OP_CMP: {
        Fr r = bn254::zero();
        r.w[0] = (uint32_t)bn254::cmp(a, b);
        return r;
    }
    case OP_PACK31: return bn254::pack31(v);
    default: {
        Fr r;
        for (int i = 0; i < 8; i++) r.w[i] = 0xffffffffu;
        return r;
    }
    }
}

#if defined(__HIPCC__)
template <MulForm F>
__global__ __launch_bounds__(256) void ops_kernel(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const Fr r = eval<F>(in + (size_t)i * REC);
    for (int k = 0; k < 8; k++) out[(size_t)i * 8 + k] = r.w[k];
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

static int run_device(bool lohi, const std::vector<uint32_t>& in, uint32_t n, std::vector<uint32_t>& out) {
    uint32_t *d_in = nullptr, *d_out = nullptr;
    CHECK(hipMalloc(&d_in, in.size() * 4 + 4));
    CHECK(hipMalloc(&d_out, (size_t)n * 32 + 4));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0, (size_t)n * 32 + 4));
    if (lohi)
        hipLaunchKernelGGL(ops_kernel<MulForm::LoHi>, dim3((n + 255) / 256), dim3(256), 0, 0, d_in, n, d_out);
    else
        hipLaunchKernelGGL(ops_kernel<MulForm::Mad>, dim3((n + 255) / 256), dim3(256), 0, 0, d_in, n, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, (size_t)n * 32, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in));
    CHECK(hipFree(d_out));
    return 0;
}
#endif

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: %s host|mad|lohi IN OUT\n", argv[0]);
        return 1;
    }
    const char* form = argv[1];
    FILE* f = fopen(argv[2], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    uint32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n == 0 || n > (1u << 24)) { fprintf(stderr, "bad record count\n"); fclose(f); return 1; }
    std::vector<uint32_t> in((size_t)n * REC);
    const size_t got = fread(in.data(), 4, in.size(), f);
    fclose(f);
    if (got != in.size()) { fprintf(stderr, "short input: %zu of %zu words\n", got, in.size()); return 1; }
    std::vector<uint32_t> out((size_t)n * 8);
    if (!strcmp(form, "host")) {
        for (uint32_t i = 0; i < n; i++) {
            const Fr r = eval<MulForm::Mad>(in.data() + (size_t)i * REC);
            memcpy(out.data() + (size_t)i * 8, r.w, 32);
        }
    } else if (!strcmp(form, "mad") || !strcmp(form, "lohi")) {
#if defined(__HIPCC__)
        const int st = run_device(!strcmp(form, "lohi"), in, n, out);
        if (st) return st;
#else
        fprintf(stderr, "built without a device compiler: only the host form\n");
        return 1;
#endif
    } else {
        fprintf(stderr, "unknown form %s\n", form);
        return 1;
    }
    FILE* g = fopen(argv[3], "wb");
    if (!g) { fprintf(stderr, "cannot open %s\n", argv[3]); return 1; }
    const size_t put = fwrite(out.data(), 4, out.size(), g);
    fclose(g);
    if (put != out.size()) { fprintf(stderr, "short write\n"); return 1; }
    printf("bn254_ops %s: %u records\n", form, n);
    return 0;
}
