// tests/native/lookup_counts.hip — the byte-lookup count of sp1_amd/csrc/tg_lookup_counts.hpp (included unchanged) behind a file
// interface, in one of two forms: `host` (the __host__ __device__ row function in a serial loop with plain adds; never opens a GPU,
// never loads the library) and `device` (the real kernel: sp1hip_lookup_count_sends of sp1_amd/lib/libsp1hip.so, loaded at run time
// from beside this program's tree). tests/test_lookup_counts_host.py (CPU) and tests/test_gpu_lookup_counts.py write the inputs
// and check every word.
//
//   lookup_counts FORM DESC MAIN_WIDTH PREP_WIDTH ROWS MAIN PREP OUT
//       DESC:  the chip's interaction words (air.InteractionProgram.to_array), u32 little-endian
//       MAIN:  MAIN_WIDTH x ROWS u32, column-major [width][rows], Montgomery words; PREP the same with PREP_WIDTH, or `-` for none
//       OUT:   393216 byte counts, 131072 range counts, 8 status words (sp1hip.h: sp1hip_lookup_count_sends), u32, raw counts
//   exit status: 0 counted (bad messages are in the status words), 3 the description was rejected (the reason on stderr), 1 usage or
//   file trouble, 2 the device or the library failed
//
// Build (done by __graft_entry__.build()): hipcc --offload-arch=gfx950 -O3 -std=c++17 -Isp1_amd/csrc -Iinclude ...
#include <dlfcn.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

#include "sp1hip.h"
#include "tg_lookup_counts.hpp"

namespace tg = sp1hip::tg;

constexpr size_t OUT_WORDS = (size_t)tg::LC_BYTE_CELLS + tg::LC_RANGE_CELLS + tg::LC_STATUS_WORDS;

// what lookup_count_sends_kernel does, serially: every compiled send on every row, plain adds, the first bad message recorded
static int host_counts(const std::vector<uint32_t>& desc, uint32_t main_width, uint32_t prep_width, const uint32_t* main, const uint32_t* prep,
                       uint32_t rows, uint32_t* out) {
    std::vector<uint32_t> prog;
    const char* why = tg::lc_compile(desc.data(), desc.size(), main_width, prep_width, prog);
    if (why) { fprintf(stderr, "rejected: %s\n", why); return 3; }
    uint32_t *byte_counts = out, *range_counts = out + tg::LC_BYTE_CELLS, *status = range_counts + tg::LC_RANGE_CELLS;
    for (uint32_t row = 0; row < rows; row++) {
        const uint32_t* send = prog.data() + 1;
        for (uint32_t s = 0; s < prog[0]; s++, send += send[1]) {
            const tg::LcMsg msg = tg::lc_message(send, main, prep, rows, row);
            if (msg.where == tg::LC_BYTE) byte_counts[msg.cell] += msg.m;
            else if (msg.where == tg::LC_RANGE) range_counts[msg.cell] += msg.m;
            else if (msg.where == tg::LC_BAD && status[0]++ == 0) { status[1] = tg::LC_WHAT_MESSAGE; status[2] = send[0]; status[3] = row; }
        }
    }
    return 0;
}

#if defined(__HIPCC__)
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); return 2; } } while (0)

// the library of the tree this program stands in: tests/native/lookup_counts -> sp1_amd/lib/libsp1hip.so
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

static int device_counts(const std::vector<uint32_t>& desc, uint32_t main_width, uint32_t prep_width, const std::vector<uint32_t>& main,
                         const std::vector<uint32_t>& prep, uint32_t rows, uint32_t* out) {
    const std::string path = library_path();
    void* lib = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!lib) { fprintf(stderr, "cannot load %s: %s\n", path.c_str(), dlerror()); return 2; }
    using Fn = int (*)(const uint32_t*, uint64_t, uint32_t, uint32_t, const uint32_t*, const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t*, uint32_t,
                       sp1hip_stream_t);
    using Err = const char* (*)();
    const Fn run = (Fn)dlsym(lib, "sp1hip_lookup_count_sends");
    const Err last_error = (Err)dlsym(lib, "sp1hip_last_error");
    if (!run) { fprintf(stderr, "%s has no sp1hip_lookup_count_sends\n", path.c_str()); return 2; }
    uint32_t *d_main = nullptr, *d_prep = nullptr, *d_out = nullptr;
    CHECK(hipMalloc(&d_main, main.size() * 4 + 8));
    CHECK(hipMalloc(&d_prep, prep.size() * 4 + 8));
    CHECK(hipMalloc(&d_out, OUT_WORDS * 4));
    CHECK(hipMemcpy(d_main, main.data(), main.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(d_prep, prep.data(), prep.size() * 4, hipMemcpyHostToDevice));
    CHECK(hipMemset(d_out, 0, OUT_WORDS * 4));
    const int st = run(desc.data(), desc.size(), main_width, prep_width, main_width ? d_main : nullptr, prep_width ? d_prep : nullptr, rows, d_out,
                       d_out + tg::LC_BYTE_CELLS, d_out + tg::LC_BYTE_CELLS + tg::LC_RANGE_CELLS, 0u, nullptr);
    if (st != 0) { fprintf(stderr, "sp1hip_lookup_count_sends: %d %s\n", st, last_error ? last_error() : ""); return st == -1 ? 3 : 2; }
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(out, d_out, OUT_WORDS * 4, hipMemcpyDeviceToHost));
    CHECK(hipFree(d_main));
    CHECK(hipFree(d_prep));
    CHECK(hipFree(d_out));
    return 0;
}
#endif

static bool read_words(const char* path, std::vector<uint32_t>& out, size_t want, bool exact) {
    FILE* f = fopen(path, "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", path); return false; }
    fseek(f, 0, SEEK_END);
    const long bytes = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (bytes < 0 || bytes % 4 || (exact && (size_t)bytes != want * 4)) {
        fprintf(stderr, "%s: %ld bytes where %zu words are expected\n", path, bytes, want);
        fclose(f);
        return false;
    }
    out.resize((size_t)bytes / 4);
    const size_t got = out.empty() ? 0 : fread(out.data(), 4, out.size(), f);
    fclose(f);
    return got == out.size();
}

static bool number(const char* s, long max, uint32_t& v) {
    char* end = nullptr;
    const long x = strtol(s, &end, 10);
    if (*end || end == s || x < 0 || x > max) { fprintf(stderr, "bad number %s: need 0 <= n <= %ld\n", s, max); return false; }
    v = (uint32_t)x;
    return true;
}

int main(int argc, char** argv) {
    if (argc != 9) { fprintf(stderr, "usage: %s host|device DESC MAIN_WIDTH PREP_WIDTH ROWS MAIN PREP|- OUT\n", argv[0]); return 1; }
    const bool host = !strcmp(argv[1], "host"), device = !strcmp(argv[1], "device");
    if (!host && !device) { fprintf(stderr, "unknown form %s\n", argv[1]); return 1; }
#if !defined(__HIPCC__)
    if (device) { fprintf(stderr, "built without a device compiler: only the host form\n"); return 1; }
#endif
    uint32_t main_width, prep_width, rows;
    if (!number(argv[3], 1 << 16, main_width) || !number(argv[4], 1 << 16, prep_width) || !number(argv[5], 1 << 22, rows)) return 1;
    std::vector<uint32_t> desc, main_table, prep_table;
    if (!read_words(argv[2], desc, 0, false)) return 1;
    if (!read_words(argv[6], main_table, (size_t)main_width * rows, true)) return 1;
    const bool has_prep = strcmp(argv[7], "-") != 0;
    if (has_prep ? !read_words(argv[7], prep_table, (size_t)prep_width * rows, true) : prep_width != 0) {
        if (!has_prep) fprintf(stderr, "a preprocessed width without a preprocessed table\n");
        return 1;
    }
    std::vector<uint32_t> out(OUT_WORDS, 0u);
    int st = 0;
    if (host) st = host_counts(desc, main_width, prep_width, main_table.data(), prep_table.data(), rows, out.data());
#if defined(__HIPCC__)
    else st = device_counts(desc, main_width, prep_width, main_table, prep_table, rows, out.data());
#endif
    if (st) return st;
    FILE* g = fopen(argv[8], "wb");
    if (!g) { fprintf(stderr, "cannot open %s\n", argv[8]); return 1; }
    const size_t wrote = fwrite(out.data(), 4, out.size(), g);
    if (fclose(g) != 0 || wrote != out.size()) { fprintf(stderr, "short write\n"); return 1; }
    fprintf(stderr, "lookup_counts %s: %u rows x %u (+%u) columns, %u bad messages\n", argv[1], rows, main_width, prep_width,
            out[tg::LC_BYTE_CELLS + tg::LC_RANGE_CELLS]);
    return 0;
}
