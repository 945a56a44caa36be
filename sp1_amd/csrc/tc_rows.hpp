// sp1_amd/csrc/tc_rows.hpp — the row functions of the trace checker (trace_check.hip): one compiled piece of a chip's constraint
// program evaluated on ONE row in the base field, every ASSERT_ZERO handed to a sink with its index in the whole program. The
// function compiles for the host and the device alike: the kernel runs it one row per lane with the register file in LDS, the
// entry point runs it on the first failing row it fetched, and tests/native/trace_check.hip runs it over a row-major table in a
// plain loop on the CPU.
//
// Compiled form (u32 words, what sp1hip_trace_check_compile returns and the kernel reads):
//   [0] pieces  [1] registers (the largest piece's)  [2] lanes per workgroup  [3] constraints of the whole program  [4] words in all
//   then per piece: [instructions, registers], instructions x [op | flags, dst, a, b]
// The instruction words are those of the zerocheck's register allocator (zc_compile.cpp: allocate_registers; zc_device.hpp for
// the opcodes and flags): operand forwarding through `prev`, immediates and constants in Montgomery form, runs of up to 4 loads of
// consecutive columns in one word. What is NOT shared with the zerocheck: its instruction order, its hinted sub-AIRs and every
// fused piece of zc_*.hpp — a piece here is the caller's plain SSA (zc_plain_pieces).
#pragma once

#include <stdint.h>

#include <vector>

#include "kb31.hpp"
#include "tg_lookup_counts.hpp"
#include "zc_device.hpp"

#ifndef TG_HD
#define TG_HD __host__ __device__ __forceinline__
#endif

namespace sp1hip {
namespace tc {

constexpr uint32_t TC_HEADER = 5, TC_PIECE_HEADER = 2;
// The register budget. A lane's file is 4 bytes per register in LDS and a compute unit has 160 KB: 512 registers are 128 KB for
// one wave, which leaves the CU to that wave alone. Every RISC-V chip but KeccakPermute fits (the largest plain program,
// Bls12381DoubleAssign, needs 453 by air.allocate_registers); KeccakPermute (2,285) is cut.
constexpr uint32_t TC_MAX_REGS = 512;
constexpr uint32_t TC_LDS_CU = 160 * 1024;
constexpr uint32_t TC_MAX_FIRST = 64;              // constraint indices reported for the first failing row

// Rows per workgroup: 256, unless the register file forces fewer — the widest of 256 / 128 / 64 whose file fits a compute unit's
// LDS (up to 160 registers: 256; up to 320: 128; up to 640: 64). 0: even one wave's file does not fit.
inline uint32_t tc_lanes_for(uint32_t n_regs) {
    for (uint32_t wg = 256; wg >= 64; wg >>= 1)
        if ((uint64_t)n_regs * 4 * wg <= TC_LDS_CU) return wg;
    return 0;
}

// One piece on one row. `rf`: this lane's register 0, register r at rf[r * rf_stride] (LDS on the device, lane-interleaved; a plain
// array with stride 1 on the host). `main` / `prep`: column 0 of the row, column c at main[c * main_cs] (column-major device
// tables: the height; a row-major row: 1). Montgomery words throughout. on_assert(constraint index, value).
template <class Sink>
TG_HD void tc_run_piece(const uint32_t* words, uint32_t n_instr, uint32_t* rf, uint32_t rf_stride, const uint32_t* main, size_t main_cs,
                        const uint32_t* prep, size_t prep_cs, const uint32_t* publics, Sink&& on_assert) {
    uint32_t prev = 0;
    for (uint32_t k = 0; k < n_instr; k++) {
        const uint32_t opw = words[4 * k], op = opw & 0xffu, dst = words[4 * k + 1], x = words[4 * k + 2], y = words[4 * k + 3];
        if (op == ZC_LOAD_MAIN || op == ZC_LOAD_PREP) {
            const uint32_t* col = op == ZC_LOAD_MAIN ? main + (size_t)x * main_cs : prep + (size_t)x * prep_cs;
            const size_t cs = op == ZC_LOAD_MAIN ? main_cs : prep_cs;
            const uint32_t cnt = ((opw >> 16) & 3u) + 1;
            for (uint32_t j = 0; j < cnt; j++) {
                prev = col[j * cs];
                if (!(opw & ZC_DST_TEMP)) rf[(size_t)(dst + j) * rf_stride] = prev;
            }
            continue;
        }
        const bool bin = (op >= ZC_ADD && op <= ZC_MUL) || op == ZC_RSUB;
        const bool reads_a = op >= ZC_ADD && op != ZC_TOUCH;
        const uint32_t A = (opw & ZC_A_PREV) ? prev : (reads_a ? rf[(size_t)x * rf_stride] : 0u);
        const uint32_t B = bin ? ((opw & ZC_B_PREV) ? prev : rf[(size_t)y * rf_stride]) : 0u;
        uint32_t res;
        switch (op) {
            case ZC_CONST: res = x; break;
            case ZC_PUBLIC: res = publics[x]; break;
            case ZC_ADD: res = kb::add(A, B); break;
            case ZC_SUB: res = kb::sub(A, B); break;
            case ZC_MUL: res = kb::mul(A, B); break;
            case ZC_RSUB: res = kb::sub(B, A); break;
            case ZC_NEG: res = kb::neg(A); break;
            case ZC_ADDC: res = kb::add(A, y); break;
            case ZC_SUBC: res = kb::sub(A, y); break;
            case ZC_CSUB: res = kb::sub(y, A); break;
            case ZC_MULC: res = kb::mul(A, y); break;
            case ZC_MADC: res = kb::add((opw & ZC_B_PREV) ? prev : rf[(size_t)(dst >> 16) * rf_stride], kb::mul(A, y)); break;
            case ZC_MAD: res = kb::add((opw & ZC_B_PREV) ? prev : rf[(size_t)(dst >> 16) * rf_stride], kb::mul(A, rf[(size_t)y * rf_stride])); break;
            case ZC_MSB: res = kb::sub((opw & ZC_B_PREV) ? prev : rf[(size_t)(dst >> 16) * rf_stride], kb::mul(A, rf[(size_t)y * rf_stride])); break;
            case ZC_ASSERT_ZERO: on_assert(y, A); continue;
            default: continue;                     // tc_check_words admits no other opcode
        }
        prev = res;
        if (!(opw & ZC_DST_TEMP)) rf[(size_t)(dst & 0xffffu) * rf_stride] = res;
    }
}

// Host: is every index a compiled program holds inside what it indexes? Registers below the piece's count (which is at most
// `max_regs`), columns inside the tables' widths, public values below n_publics, constraint indices below the count, every
// constraint in exactly one piece, and the word list exactly as long as its header says. nullptr, or what is wrong. The kernel
// and the host loop read nothing through an index that did not pass here.
inline const char* tc_check_words(const uint32_t* w, size_t n_words, uint32_t main_width, uint32_t prep_width, uint32_t n_publics, uint32_t max_regs) {
    if (n_words < TC_HEADER || w[4] != n_words) return "compiled program: the header does not match the word count";
    const uint32_t n_pieces = w[0], n_constraints = w[3];
    if (w[1] > max_regs) return "compiled program: more registers than the budget";
    std::vector<uint8_t> seen(n_constraints, 0);
    size_t at = TC_HEADER;
    for (uint32_t p = 0; p < n_pieces; p++) {
        if (n_words - at < TC_PIECE_HEADER) return "compiled program: the word list ends inside a piece";
        const uint32_t n = w[at], regs = w[at + 1];
        at += TC_PIECE_HEADER;
        if ((n_words - at) / 4 < n) return "compiled program: the word list ends inside a piece";
        if (regs > w[1]) return "compiled program: a piece with more registers than the header says";
        for (uint32_t k = 0; k < n; k++, at += 4) {
            const uint32_t opw = w[at], op = opw & 0xffu, dst = w[at + 1], x = w[at + 2], y = w[at + 3];
            const bool temp = opw & ZC_DST_TEMP;
            auto reg_ok = [&](uint32_t r) { return r < regs; };
            if (op == ZC_LOAD_MAIN || op == ZC_LOAD_PREP) {
                const uint32_t cnt = ((opw >> 16) & 3u) + 1, width = op == ZC_LOAD_MAIN ? main_width : prep_width;
                if ((uint64_t)x + cnt > width) return "compiled program: a column outside its table's width";
                if (!temp && (uint64_t)dst + cnt > regs) return "compiled program: a register outside the file";
                continue;
            }
            const bool bin = (op >= ZC_ADD && op <= ZC_MUL) || op == ZC_RSUB, fma = op == ZC_MADC || op == ZC_MAD || op == ZC_MSB;
            const bool unary = op == ZC_NEG || (op >= ZC_ADDC && op <= ZC_MULC) || op == ZC_ASSERT_ZERO;
            if (op == ZC_CONST) { /* x: the constant */ }
            else if (op == ZC_PUBLIC) { if (x >= n_publics) return "compiled program: a public value outside the public values"; }
            else if (bin || fma || unary) {
                if (!(opw & ZC_A_PREV) && !reg_ok(x)) return "compiled program: a register outside the file";
                if ((bin || op == ZC_MAD || op == ZC_MSB) && !(bin && (opw & ZC_B_PREV)) && !reg_ok(y)) return "compiled program: a register outside the file";
                if (fma && !(opw & ZC_B_PREV) && !reg_ok(dst >> 16)) return "compiled program: a register outside the file";
            } else return "compiled program: an unknown opcode";
            if (op == ZC_ASSERT_ZERO) {
                if (y >= n_constraints || seen[y]++) return "compiled program: a constraint outside the program, or evaluated twice";
            } else if (!temp && !reg_ok(dst & 0xffffu)) return "compiled program: a register outside the file";
        }
    }
    if (at != n_words) return "compiled program: words after the last piece";
    for (uint32_t k = 0; k < n_constraints; k++) if (!seen[k]) return "compiled program: a constraint that no piece evaluates";
    return nullptr;
}

// ---- buses: one message of one compiled interaction on one row -------------------------------------------------------------------
// The compiled form is lc_compile_interactions(every = true) of tg_lookup_counts.hpp: [n, then per interaction: index, words in
// this record, is_send, kind, n_values, form(m), form(value 0), ...]; the forms are evaluated by lc_form, the function the byte
// lookup counter runs. A message is (kind, n_values, canonical values); it is folded, value by value as the forms are evaluated (no
// per-lane array), into TWO 64-bit hashes that share nothing but their input: chain A steps with the splitmix64 finaliser from one
// seed, chain B with the murmur3 finaliser from another, and the value enters A by addition and B by exclusive or. Each hash picks
// one bucket (its top log_buckets bits) of its own table.
constexpr uint32_t IA_RECORD_HEADER = 5, IA_RECORD_WORDS = 4;      // a pass-2 record: chip, interaction, row, canonical multiplicity

TG_HD uint64_t ia_step_a(uint64_t h, uint64_t v) {
    uint64_t x = h + v + 0x9E3779B97F4A7C15ull;
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull; x ^= x >> 27; x *= 0x94D049BB133111EBull; x ^= x >> 31;
    return x;
}
TG_HD uint64_t ia_step_b(uint64_t h, uint64_t v) {
    uint64_t x = (h ^ v) * 0x2545F4914F6CDD1Dull + 0xD6E8FEB86659FD93ull;
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
    return x;
}

struct IaMsg {
    uint32_t m;            // canonical multiplicity; 0: no message (nothing else is set)
    int64_t add;           // what the message adds to its buckets: m, or m - p when m > p / 2, negated for a receive
    uint64_t ha, hb;       // the two hashes
};

// `rec` points at the interaction's record. Column-major Montgomery tables of `rows` rows.
TG_HD IaMsg ia_message(const uint32_t* rec, const uint32_t* main, const uint32_t* prep, uint32_t rows, uint32_t row) {
    IaMsg r{0u, 0, 0ull, 0ull};
    const uint32_t is_send = rec[2], kind = rec[3], n_values = rec[4];
    const uint32_t* p = rec + IA_RECORD_HEADER;
    r.m = tg::lc_form(p, main, prep, rows, row);
    if (r.m == 0) return r;
    const int64_t s = r.m > kb::P / 2 ? (int64_t)r.m - (int64_t)kb::P : (int64_t)r.m;
    r.add = is_send ? s : -s;
    r.ha = ia_step_a(ia_step_a(0x243F6A8885A308D3ull, kind), n_values);
    r.hb = ia_step_b(ia_step_b(0x13198A2E03707344ull, kind), n_values);
    for (uint32_t v = 0; v < n_values; v++) {
        const uint32_t x = tg::lc_form(p, main, prep, rows, row);
        r.ha = ia_step_a(r.ha, x);
        r.hb = ia_step_b(r.hb, x);
    }
    return r;
}

TG_HD uint32_t ia_bucket(uint64_t h, uint32_t log_buckets) { return (uint32_t)(h >> (64 - log_buckets)); }

}  // namespace tc
}  // namespace sp1hip
