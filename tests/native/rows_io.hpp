// tests/native/rows_io.hpp — the file interface the trace-row programs (riscv_rows, riscv_mem_rows, riscv_core_rows, riscv_sys_rows,
// riscv_memglobal_rows) share: record files in, the HEIGHT argument, tables and event lists out. Everything reports on stderr.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

// the whole file as u64 words; false when it is not a whole number of `record_words`-word records
static bool read_records(const char* path, size_t record_words, std::vector<uint64_t>& words) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return false; }
    uint64_t buf[1024];
    size_t got, bytes = 0;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) {
        if (got % 8) { bytes = 1; break; }
        words.insert(words.end(), buf, buf + got / 8);
    }
    fclose(f);
    if (bytes || words.size() % record_words) { fprintf(stderr, "%s is not a whole number of %zu-byte records\n", path, record_words * 8); return false; }
    return true;
}

static int write_out(const char* path, const void* data, size_t bytes) {
    FILE* g = fopen(path, "wb");
    if (!g) { fprintf(stderr, "cannot open %s\n", path); return 1; }
    const size_t wrote = bytes ? fwrite(data, 1, bytes, g) : 0;
    if (fclose(g) != 0 || wrote != bytes) { fprintf(stderr, "short write\n"); return 1; }
    return 0;
}

// HEIGHT (0 .. 2^20) and the n <= HEIGHT records of IN: what every `rows` command starts from
static bool read_rows_input(const char* height_arg, const char* path, size_t record_words, uint32_t& height, std::vector<uint64_t>& words, uint32_t& n) {
    char* end = nullptr;
    const long h = strtol(height_arg, &end, 10);
    if (*end || end == height_arg || h < 0 || h > (1l << 20)) { fprintf(stderr, "bad height %s: need 0 <= height <= 2^20\n", height_arg); return false; }
    height = (uint32_t)h;
    if (!read_records(path, record_words, words)) return false;
    if (words.size() / record_words > height) { fprintf(stderr, "more than height = %u records\n", height); return false; }
    n = (uint32_t)(words.size() / record_words);
    return true;
}

#if defined(__HIPCC__)
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <unistd.h>

#include "sp1hip.h"

// the library of the tree this program stands in: tests/native/PROGRAM -> sp1_amd/lib/libsp1hip.so
static std::string library_path() {
    char exe[4096];
    const ssize_t len = readlink("/proc/self/exe", exe, sizeof exe - 1);
    if (len <= 0) return "";
    std::string p(exe, (size_t)len);
    for (int up = 0; up < 3; up++) {
        const size_t cut = p.rfind('/');
        if (cut == std::string::npos) return "";
        p.resize(cut);
    }
    return p + "/sp1_amd/lib/libsp1hip.so";
}

// The `device` form of a chip-numbered family: the table of chip `chip` from the real kernels, through the library's entry point
// `entry` (sp1hip_tracegen_riscv_alu, _mem: int chip, table, height, records, n, stream), loaded at run time
static int device_rows(const char* entry, int chip, std::vector<uint32_t>& out, uint32_t height, const std::vector<uint64_t>& words, uint32_t n) {
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)
    const std::string path = library_path();
    void* lib = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!lib) { fprintf(stderr, "cannot load %s: %s\n", path.c_str(), dlerror()); return 2; }
    using Fn = int (*)(int, uint32_t*, uint32_t, const void*, uint32_t, sp1hip_stream_t);
    using Err = const char* (*)();
    const Fn run = (Fn)dlsym(lib, entry);
    const Err last_error = (Err)dlsym(lib, "sp1hip_last_error");
    if (!run) { fprintf(stderr, "%s has no %s\n", path.c_str(), entry); return 2; }
    void* d_ev = nullptr;
    uint32_t* d_out = nullptr;
    CHECK(hipMalloc(&d_ev, words.size() * 8 + 8));
    CHECK(hipMalloc(&d_out, out.size() * 4 + 8));
    CHECK(hipMemcpy(d_ev, words.data(), words.size() * 8, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0xee, out.size() * 4 + 8));
    const int st = run(chip, d_out, height, d_ev, n, nullptr);
    if (st != 0) { fprintf(stderr, "%s: %d %s\n", entry, st, last_error ? last_error() : ""); return 2; }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_ev));
    CHECK(hipFree(d_out));
    return 0;
#undef CHECK
}
#endif
