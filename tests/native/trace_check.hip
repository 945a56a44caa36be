// tests/native/trace_check.hip — the host form of the trace checker: the row function of sp1_amd/csrc/tc_rows.hpp (included
// unchanged, the same __host__ __device__ code the kernel of trace_check.hip runs one row per lane) in a plain loop over a
// ROW-major table on the CPU. The program is compiled by the library of the tree this program stands in
// (sp1hip_trace_check_compile of sp1_amd/lib/libsp1hip.so: host code, no device is opened), checked by tc_check_words, and every
// piece is run on every row. tests/test_trace_check_host.py writes the inputs and compares every value with numpy.
//
//   trace_check constraints PROG MAIN_WIDTH PREP_WIDTH NUM_CONSTRAINTS ROWS MAIN PREP|- PUBLICS MAX_REGS OUT
//       PROG:     the chip's constraint program (air.AirProgram.to_array), [n][3] u32 little-endian
//       MAIN:     ROWS x MAIN_WIDTH u32, row-major, Montgomery words; PREP the same with PREP_WIDTH, or `-` for none
//       PUBLICS:  the public values, Montgomery words (an empty file for none)
//       MAX_REGS: the register budget the program is cut for; 0 = the library's
//       OUT:      4 words [pieces, registers, lanes, constraints], then ROWS x NUM_CONSTRAINTS Montgomery words, row-major: the value
//                 of every constraint on every row
//   trace_check messages DESC MAIN_WIDTH PREP_WIDTH ROWS MAIN PREP|- OUT
//       the bus side (tc_rows.hpp: ia_message, what both passes of sp1hip_check_interactions run per lane): DESC the chip's interaction
//       words (air.InteractionProgram.to_array), MAIN / PREP COLUMN-major [width][rows] Montgomery words; the description is compiled
//       by lc_compile_interactions (no library). OUT: 8 words per message with a non-zero multiplicity, rows outermost:
//       [interaction, row, canonical multiplicity, is_send, hash A low, high, hash B low, high]
//   exit status: 0 evaluated, 3 the program was rejected (the reason on stderr), 1 usage or file trouble, 2 the library failed
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
#include "tc_rows.hpp"

namespace tc = sp1hip::tc;

// the library of the tree this program stands in: tests/native/trace_check -> sp1_amd/lib/libsp1hip.so
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

static int messages(char** argv) {
    uint32_t main_width, prep_width, rows;
    if (!number(argv[1], 1 << 16, main_width) || !number(argv[2], 1 << 16, prep_width) || !number(argv[3], 1 << 22, rows)) return 1;
    std::vector<uint32_t> desc, main_table, prep_table, prog, out;
    if (!read_words(argv[0], desc, 0, false)) return 1;
    if (!read_words(argv[4], main_table, (size_t)main_width * rows, true)) return 1;
    const bool has_prep = strcmp(argv[5], "-") != 0;
    if (has_prep ? !read_words(argv[5], prep_table, (size_t)prep_width * rows, true) : prep_width != 0) {
        if (!has_prep) fprintf(stderr, "a preprocessed width without a preprocessed table\n");
        return 1;
    }
    const char* why = sp1hip::tg::lc_compile_interactions(desc.data(), desc.size(), main_width, prep_width, true, prog);
    if (why) { fprintf(stderr, "rejected: %s\n", why); return 3; }
    for (uint32_t row = 0; row < rows; row++) {
        const uint32_t* rec = prog.data() + 1;
        for (uint32_t k = 0; k < prog[0]; k++, rec += rec[1]) {
            const tc::IaMsg msg = tc::ia_message(rec, main_table.data(), prep_table.data(), rows, row);
            if (msg.m == 0) continue;
            out.insert(out.end(), {rec[0], row, msg.m, rec[2], (uint32_t)msg.ha, (uint32_t)(msg.ha >> 32), (uint32_t)msg.hb, (uint32_t)(msg.hb >> 32)});
        }
    }
    FILE* g = fopen(argv[6], "wb");
    if (!g) { fprintf(stderr, "cannot open %s\n", argv[6]); return 1; }
    const size_t wrote = out.empty() ? 0 : fwrite(out.data(), 4, out.size(), g);
    if (fclose(g) != 0 || wrote != out.size()) { fprintf(stderr, "short write\n"); return 1; }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 9 && !strcmp(argv[1], "messages")) return messages(argv + 2);
    if (argc != 12 || strcmp(argv[1], "constraints")) {
        fprintf(stderr, "usage: %s constraints PROG MAIN_WIDTH PREP_WIDTH NUM_CONSTRAINTS ROWS MAIN PREP|- PUBLICS MAX_REGS OUT\n"
                        "       %s messages DESC MAIN_WIDTH PREP_WIDTH ROWS MAIN PREP|- OUT\n", argv[0], argv[0]);
        return 1;
    }
    argv++;
    uint32_t main_width, prep_width, n_constraints, rows, max_regs;
    if (!number(argv[2], 1 << 16, main_width) || !number(argv[3], 1 << 16, prep_width) || !number(argv[4], 1 << 24, n_constraints) ||
        !number(argv[5], 1 << 22, rows) || !number(argv[9], 1 << 16, max_regs))
        return 1;
    std::vector<uint32_t> prog, main_table, prep_table, publics;
    if (!read_words(argv[1], prog, 0, false) || prog.size() % 3) { fprintf(stderr, "%s is no [n][3] program\n", argv[1]); return 1; }
    if (!read_words(argv[6], main_table, (size_t)main_width * rows, true)) return 1;
    const bool has_prep = strcmp(argv[7], "-") != 0;
    if (has_prep ? !read_words(argv[7], prep_table, (size_t)prep_width * rows, true) : prep_width != 0) {
        if (!has_prep) fprintf(stderr, "a preprocessed width without a preprocessed table\n");
        return 1;
    }
    if (!read_words(argv[8], publics, 0, false)) return 1;

    const std::string path = library_path();
    void* lib = dlopen(path.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!lib) { fprintf(stderr, "cannot load %s: %s\n", path.c_str(), dlerror()); return 2; }
    using Fn = int (*)(const uint32_t*, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t*, size_t*);
    using Err = const char* (*)();
    const Fn compile = (Fn)dlsym(lib, "sp1hip_trace_check_compile");
    const Err last_error = (Err)dlsym(lib, "sp1hip_last_error");
    if (!compile) { fprintf(stderr, "%s has no sp1hip_trace_check_compile\n", path.c_str()); return 2; }
    size_t n_words = 0;
    int st = compile(prog.data(), (uint32_t)(prog.size() / 3), main_width, prep_width, n_constraints, max_regs, nullptr, &n_words);
    if (st != SP1HIP_ERROR_BUFFER_TOO_SMALL) { fprintf(stderr, "rejected: %d %s\n", st, last_error ? last_error() : ""); return st == SP1HIP_ERROR_INVALID_ARGUMENT ? 3 : 2; }
    std::vector<uint32_t> words(n_words);
    st = compile(prog.data(), (uint32_t)(prog.size() / 3), main_width, prep_width, n_constraints, max_regs, words.data(), &n_words);
    if (st != 0) { fprintf(stderr, "sp1hip_trace_check_compile: %d %s\n", st, last_error ? last_error() : ""); return 2; }
    // what the kernel is launched on passed this very check inside the library; the host loop asks it again of what it was handed
    const char* why = tc::tc_check_words(words.data(), words.size(), main_width, prep_width, (uint32_t)publics.size(), max_regs ? max_regs : tc::TC_MAX_REGS);
    if (why) { fprintf(stderr, "rejected: %s\n", why); return 3; }

    std::vector<uint32_t> out(4 + (size_t)rows * n_constraints, 0u), file(words[1] + 4u, 0u);
    out[0] = words[0]; out[1] = words[1]; out[2] = words[2]; out[3] = words[3];
    std::vector<uint32_t> seen(n_constraints, 0u);
    for (uint32_t row = 0; row < rows; row++) {
        uint32_t* values = out.data() + 4 + (size_t)row * n_constraints;
        const uint32_t* p = words.data() + tc::TC_HEADER;
        for (uint32_t piece = 0; piece < words[0]; piece++) {
            tc::tc_run_piece(p + tc::TC_PIECE_HEADER, p[0], file.data(), 1u, main_table.data() + (size_t)row * main_width, (size_t)1,
                             prep_table.data() + (size_t)row * prep_width, (size_t)1, publics.data(),
                             [&](uint32_t index, uint32_t value) { values[index] = value; seen[index]++; });
            p += tc::TC_PIECE_HEADER + 4 * (size_t)p[0];
        }
    }
    for (uint32_t k = 0; k < n_constraints; k++)
        if (seen[k] != rows) { fprintf(stderr, "constraint %u was evaluated %u times on %u rows\n", k, seen[k], rows); return 2; }
    FILE* g = fopen(argv[10], "wb");
    if (!g) { fprintf(stderr, "cannot open %s\n", argv[10]); return 1; }
    const size_t wrote = fwrite(out.data(), 4, out.size(), g);
    if (fclose(g) != 0 || wrote != out.size()) { fprintf(stderr, "short write\n"); return 1; }
    fprintf(stderr, "trace_check: %u rows x %u (+%u) columns, %u constraints in %u pieces of at most %u registers, %u lanes\n", rows, main_width, prep_width,
            n_constraints, words[0], words[1], words[2]);
    return 0;
}
