// tests/native/septic_ops.hip — the septic field, the curve addition, the root choice and the row function of
// sp1_amd/csrc/septic.hpp (included unchanged) behind a file interface, in one of two forms: `host` (the KB_HD code compiled for
// the CPU; never opens a GPU) and `device` (a gfx950 kernel, one lane per record or per row). tests/test_septic_arith.py and
// tests/test_tracegen_global_host.py write the inputs and check every result word against the Python integers of
// tests/septic_model.py.
//
//   septic_ops FORM ops IN OUT
//       IN:  u32 n, then n records of 32 u32: op, k, a[7], b[7], c[7], d[7], 2 unused      (little-endian, Montgomery words)
//       OUT: n results of 16 u32 (unused words 0; an unknown op: all words 0xffffffff)
//         mul a b -> a b            frob k a -> a^(p^k), k = 1..6       norm_parts a -> a^(r - 1) [7], N(a)
//         inv a -> 1 / a            fp_sqrt a[0] -> root                sqrt a -> flag, root [7] (zeros without the flag)
//         curve_rhs a -> a^3 + 45 a + 41 z^3                            ec_add (a, b) (c, d) -> x [7], y [7]
//         pick_root a, k = is_receive -> accepted, y [7], range-check value (zeros when rejected)
//         frob_table k | i << 8 -> row i of make_frob_tables()'s map k
//   septic_ops FORM rows IN HEIGHT OUT
//       IN:  n events of 9 u32 (message[8], is_receive | kind << 8), n = file size / 36, n <= HEIGHT <= 2^20
//       OUT: 213 x HEIGHT u32, column-major: the Global chip's non-accumulation columns, rows >= n the padding row
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc -Iinclude ...
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "septic.hpp"

using namespace sp1hip::septic;

enum Op : uint32_t { OP_MUL, OP_FROB, OP_NORM_PARTS, OP_INV, OP_FP_SQRT, OP_SQRT, OP_CURVE_RHS, OP_EC_ADD, OP_PICK_ROOT, OP_FROB_TABLE, OP_COUNT };
constexpr int REC = 32, RES = 16;
constexpr int ROW_COLS = G_INIT_X;                                    // 213

KB_HD void eval(const uint32_t* rec, const FrobTables& ft, uint32_t* out) {
    const uint32_t k = rec[1];
    S7 a, b, c, d;
    for (int i = 0; i < 7; i++) { a.c[i] = rec[2 + i]; b.c[i] = rec[9 + i]; c.c[i] = rec[16 + i]; d.c[i] = rec[23 + i]; }
    for (int i = 0; i < RES; i++) out[i] = 0;
    auto put7 = [&](int at, const S7& v) { for (int i = 0; i < 7; i++) out[at + i] = v.c[i]; };
    switch (rec[0]) {
    case OP_MUL: put7(0, s7_mul(a, b)); return;
    case OP_FROB: if (k >= 1 && k <= 6) { put7(0, s7_frob(ft, a, (int)k)); return; } break;
    case OP_NORM_PARTS: { S7 t; uint32_t n; s7_norm_parts(ft, a, &t, &n); put7(0, t); out[7] = n; return; }
    case OP_INV: put7(0, s7_inv(ft, a)); return;
    case OP_FP_SQRT: out[0] = fp_sqrt(a.c[0]); return;
    case OP_SQRT: { S7 root; if (s7_sqrt(ft, a, &root)) { out[0] = 1; put7(1, root); } return; }
    case OP_CURVE_RHS: put7(0, s7_curve_rhs(a)); return;
    case OP_EC_ADD: { const Pt r = ec_add(ft, Pt{a, b}, Pt{c, d}); put7(0, r.x); put7(7, r.y); return; }
    case OP_PICK_ROOT: { S7 y; uint32_t v; if (global_pick_root(a, k != 0, &y, &v)) { out[0] = 1; put7(1, y); out[8] = v; } return; }
    case OP_FROB_TABLE: if ((k & 0xffu) >= 1 && (k & 0xffu) <= 6 && (k >> 8) < 7) { put7(0, ft.f[(k & 0xffu) - 1][k >> 8]); return; } break;
    default: break;
    }
    for (int i = 0; i < RES; i++) out[i] = 0xffffffffu;
}

// row r of the table: out[column * height + r]; false when the event has no point
KB_HD bool eval_row(const uint32_t* events, uint32_t n, uint32_t height, uint32_t r, const p2::RoundConstants* rc, const FrobTables& ft,
                    const Pt& dummy, uint32_t* out) {
    Pt point;
    return global_row(r < n ? events + (size_t)r * G_EVENT_WORDS : nullptr, r, rc, ft, dummy,
                      [&](int col, uint32_t v) { out[(size_t)col * height + r] = v; }, &point);
}

__global__ __launch_bounds__(256) void ops_kernel(const uint32_t* __restrict__ in, uint32_t n, const FrobTables* __restrict__ ft, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    eval(in + (size_t)i * REC, *ft, out + (size_t)i * RES);
}

__global__ __launch_bounds__(256) void rows_kernel(const uint32_t* __restrict__ events, uint32_t n, uint32_t height, const p2::RoundConstants* __restrict__ rc,
                                                   const FrobTables* __restrict__ ft, Pt dummy, uint32_t* __restrict__ out, uint32_t* __restrict__ failed) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= height) return;
    if (!eval_row(events, n, height, r, rc, *ft, dummy, out)) atomicAdd(failed, 1u);
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

static int device_ops(const std::vector<uint32_t>& in, uint32_t n, const FrobTables& ft, std::vector<uint32_t>& out) {
    uint32_t *d_in = nullptr, *d_out = nullptr;
    FrobTables* d_ft = nullptr;
    CHECK(hipMalloc(&d_in, in.size() * 4));
    CHECK(hipMalloc(&d_out, out.size() * 4));
    CHECK(hipMalloc(&d_ft, sizeof ft));
    CHECK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_ft, &ft, sizeof ft, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0, out.size() * 4));
    hipLaunchKernelGGL(ops_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d_in, n, d_ft, d_out);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_in)); CHECK(hipFree(d_out)); CHECK(hipFree(d_ft));
    return 0;
}

static int device_rows(const std::vector<uint32_t>& events, uint32_t n, uint32_t height, const p2::RoundConstants& rc, const FrobTables& ft,
                       const Pt& dummy, std::vector<uint32_t>& out, uint32_t* failed) {
    uint32_t *d_ev = nullptr, *d_out = nullptr, *d_failed = nullptr;
    FrobTables* d_ft = nullptr;
    p2::RoundConstants* d_rc = nullptr;
    CHECK(hipMalloc(&d_ev, events.size() * 4 + 4));
    CHECK(hipMalloc(&d_out, out.size() * 4));
    CHECK(hipMalloc(&d_failed, 4));
    CHECK(hipMalloc(&d_ft, sizeof ft));
    CHECK(hipMalloc(&d_rc, sizeof rc));
    if (n) CHECK(hipMemcpy(d_ev, events.data(), events.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_ft, &ft, sizeof ft, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_rc, &rc, sizeof rc, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xee, out.size() * 4));
    CHECK(hipMemset(d_failed, 0, 4));
    hipLaunchKernelGGL(rows_kernel, dim3((height + 255) / 256), dim3(256), 0, 0, d_ev, n, height, d_rc, d_ft, dummy, d_out, d_failed);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(failed, d_failed, 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_ev)); CHECK(hipFree(d_out)); CHECK(hipFree(d_failed)); CHECK(hipFree(d_ft)); CHECK(hipFree(d_rc));
    return 0;
}

static bool read_words(const char* path, std::vector<uint32_t>& words) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return false; }
    uint32_t buf[4096];
    size_t got;
    bool whole = true;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) {
        if (got % 4) { whole = false; break; }
        words.insert(words.end(), buf, buf + got / 4);
    }
    fclose(f);
    if (!whole) fprintf(stderr, "%s is not a whole number of words\n", path);
    return whole;
}

static int write_out(const char* path, const std::vector<uint32_t>& words) {
    FILE* g = fopen(path, "wb");
    if (!g) { fprintf(stderr, "cannot open %s\n", path); return 1; }
    const size_t wrote = words.empty() ? 0 : fwrite(words.data(), 4, words.size(), g);
    if (fclose(g) != 0 || wrote != words.size()) { fprintf(stderr, "short write\n"); return 1; }
    return 0;
}

static int usage(const char* me) {
    fprintf(stderr, "usage: %s host|device ops IN OUT\n       %s host|device rows IN HEIGHT OUT\n", me, me);
    return 1;
}

int main(int argc, char** argv) {
    if (argc < 5) return usage(argv[0]);
    const bool host = !strcmp(argv[1], "host");
    if (!host && strcmp(argv[1], "device")) { fprintf(stderr, "unknown form %s\n", argv[1]); return 1; }
    const FrobTables ft = make_frob_tables();
    std::vector<uint32_t> in;
    if (!strcmp(argv[2], "ops") && argc == 5) {
        if (!read_words(argv[3], in)) return 1;
        if (in.empty() || in[0] == 0 || in[0] > (1u << 22) || in.size() != 1 + (size_t)in[0] * REC) { fprintf(stderr, "bad record count\n"); return 1; }
        const uint32_t n = in[0];
        in.erase(in.begin());
        std::vector<uint32_t> out((size_t)n * RES);
        if (host) {
            for (uint32_t i = 0; i < n; i++) eval(in.data() + (size_t)i * REC, ft, out.data() + (size_t)i * RES);
        } else {
            const int st = device_ops(in, n, ft, out);
            if (st) return st;
        }
        if (write_out(argv[4], out)) return 1;
        fprintf(stderr, "septic_ops %s ops: %u records\n", argv[1], n);
        return 0;
    }
    if (strcmp(argv[2], "rows") || argc != 6) return usage(argv[0]);
    char* end = nullptr;
    const long height_arg = strtol(argv[4], &end, 10);
    if (*end || end == argv[4] || height_arg < 0 || height_arg > (1l << 20)) { fprintf(stderr, "bad height %s: need 0 <= height <= 2^20\n", argv[4]); return 1; }
    const uint32_t height = (uint32_t)height_arg;
    if (!read_words(argv[3], in)) return 1;
    if (in.size() % G_EVENT_WORDS) { fprintf(stderr, "%s is not a whole number of %d-word events\n", argv[3], G_EVENT_WORDS); return 1; }
    const size_t n = in.size() / G_EVENT_WORDS;
    if (n > height) { fprintf(stderr, "more than height = %u events\n", height); return 1; }
    const p2::RoundConstants rc = p2::make_round_constants();
    const Pt dummy = global_dummy_point();
    std::vector<uint32_t> out((size_t)ROW_COLS * height, 0xeeeeeeeeu);
    uint32_t failed = 0;
    if (host) {
        for (uint32_t r = 0; r < height; r++) failed += !eval_row(in.data(), (uint32_t)n, height, r, &rc, ft, dummy, out.data());
    } else if (height) {
        const int st = device_rows(in, (uint32_t)n, height, rc, ft, dummy, out, &failed);
        if (st) return st;
    }
    if (failed) { fprintf(stderr, "%u events have no curve point within 256 offsets\n", failed); return 3; }
    if (write_out(argv[5], out)) return 1;
    fprintf(stderr, "septic_ops %s rows: %d x %u words, %zu events\n", argv[1], ROW_COLS, height, n);
    return 0;
}
