// sp1_amd/csrc/tg_lookup_counts.hpp — the receive side of the byte lookup argument, counted from the tables that send: what the
// reference's Byte and Range chips get from every other chip's `generate_dependencies` (crates/core/machine/src/bytes/trace.rs:L50-L66,
// range/trace.rs:L54-L95). A chip is DATA here: its interaction description (air.InteractionProgram.to_array, the words
// `sp1hip_gkr_chip_t.interactions` takes) is compiled on the host into the sends of kind BYTE, and one function evaluates one such
// send on one row of the chip's column-major Montgomery table and says which cell of which count array it goes to. The function
// compiles for the host and the device alike (tests/native/lookup_counts.hip runs it on the CPU); tracegen_lookup.hip is the
// kernels around it.
//
// A BYTE message is [opcode, a, b, c] with a multiplicity m, each an affine form of the row's columns:
//   opcode 6 (Range): `a` has `b` bits                 -> range cell (1 << b) + a            (Range's main table [1][131072])
//   opcode 0..5 (AND, OR, XOR, U8Range, LTU, MSB)      -> byte cell opcode * 65536 + b * 256 + c   (Byte's main table [6][65536],
//                                                         column-major: column = opcode, row = b * 256 + c)
// A message with m == 0 is no message (padding rows may hold anything). A message with m != 0 is checked to BE a row of the table it
// addresses before its cell is formed (the assertions of riscv_trace.Tracer.byte_range_tables); one that is not is never an index.
//
// Compiled form (u32 words): [n_sends, then per send: interaction index, words in this record, form(m), form(opcode), form(a),
// form(b), form(c)], form = [n_terms, constant, n_terms x (column reference, weight)], constants and weights in Montgomery form, a
// column reference = column, + LC_PREP for a preprocessed column. Every column reference is below its table's width: lc_compile
// rejects a description where one is not, so the row function reads inside the tables whatever the words are.
#pragma once

#include <stdint.h>

#include <vector>

#include "kb31.hpp"

#ifndef TG_HD
#define TG_HD __host__ __device__ __forceinline__
#endif

namespace sp1hip {
namespace tg {

constexpr uint32_t LC_KIND_BYTE = 5;                   // riscv.BYTE: the InteractionKind of the byte lookups
constexpr uint32_t LC_OP_RANGE = 6, LC_OP_U8RANGE = 3, LC_OP_LTU = 4, LC_OP_MSB = 5;
constexpr uint32_t LC_BYTE_CELLS = 6u << 16, LC_RANGE_CELLS = 1u << 17;
constexpr uint32_t LC_PREP = 0x80000000u;
constexpr uint32_t LC_STATUS_WORDS = 8;                // [0] bad messages, [1] what, [2] send, [3] row, [4] tag of the call
enum { LC_SKIP = 0, LC_BYTE = 1, LC_RANGE = 2, LC_BAD = 3 };
enum { LC_WHAT_MESSAGE = 1, LC_WHAT_PC = 2, LC_WHAT_COUNT = 3 };

struct LcMsg {
    uint32_t m;        // canonical multiplicity
    uint32_t cell;     // index into the byte (LC_BYTE) or range (LC_RANGE) count array; 0 otherwise
    uint32_t where;    // LC_SKIP (m == 0), LC_BYTE, LC_RANGE, or LC_BAD: m != 0 and the message is no row of its table
};

// One affine form at `row`, canonical; `p` moves past the form.
TG_HD uint32_t lc_form(const uint32_t*& p, const uint32_t* main, const uint32_t* prep, uint32_t rows, uint32_t row) {
    const uint32_t n_terms = p[0];
    uint32_t acc = p[1];
    p += 2;
    for (uint32_t t = 0; t < n_terms; t++, p += 2) {
        const uint32_t ref = p[0];
        const uint32_t* table = (ref & LC_PREP) ? prep : main;
        acc = kb::add(acc, kb::mul(table[(size_t)(ref & ~LC_PREP) * rows + row], p[1]));
    }
    return kb::from_monty(acc);
}

// Where a message [opcode, a, b, c] with multiplicity m != 0 goes.
TG_HD LcMsg lc_classify(uint32_t m, uint32_t opcode, uint32_t a, uint32_t b, uint32_t c) {
    LcMsg r{m, 0u, (uint32_t)LC_BAD};
    if (m >= (1u << 16)) return r;                     // a "negative" multiplicity arrives as p - k
    if (opcode == LC_OP_RANGE) {
        if (b > 16 || a >= (1u << b) || c != 0) return r;
        r.cell = (1u << b) + a;
        r.where = LC_RANGE;
        return r;
    }
    if (opcode > LC_OP_MSB || b > 255 || c > 255) return r;
    const uint32_t want = opcode == 0 ? (b & c) : opcode == 1 ? (b | c) : opcode == 2 ? (b ^ c) : opcode == LC_OP_U8RANGE ? 0u
                        : opcode == LC_OP_LTU ? (uint32_t)(b < c) : (b >> 7);
    if (a != want || (opcode == LC_OP_MSB && c != 0)) return r;
    r.cell = (opcode << 16) + (b << 8) + c;
    r.where = LC_BYTE;
    return r;
}

// One compiled send (`send` points at its record) on one row.
TG_HD LcMsg lc_message(const uint32_t* send, const uint32_t* main, const uint32_t* prep, uint32_t rows, uint32_t row) {
    const uint32_t* p = send + 2;
    const uint32_t m = lc_form(p, main, prep, rows, row);
    if (m == 0) return LcMsg{0u, 0u, (uint32_t)LC_SKIP};
    const uint32_t opcode = lc_form(p, main, prep, rows, row), a = lc_form(p, main, prep, rows, row);
    const uint32_t b = lc_form(p, main, prep, rows, row), c = lc_form(p, main, prep, rows, row);
    return lc_classify(m, opcode, a, b, c);
}

// The Program table's row of an executed pc; false for a pc below the text, off the 4-byte grid or past the last instruction.
TG_HD bool lc_program_cell(uint64_t pc, uint64_t pc_base, uint32_t n_instructions, uint32_t& cell) {
    const uint64_t off = pc - pc_base;
    const bool good = pc >= pc_base && (off & 3) == 0 && (off >> 2) < n_instructions;
    cell = good ? (uint32_t)(off >> 2) : 0u;
    return good;
}

// Host: interaction words -> compiled form. Returns nullptr, or what is wrong with the description (nothing is appended to a
// meaningful `out` then). every == false (lc_compile): sends of kind BYTE are kept; receives and other kinds are parsed, checked and
// skipped. every == true (the trace checker's bus tally, tc_rows.hpp): EVERY interaction is kept, with three more words in front of
// its forms — [interaction index, words in this record, is_send, kind, n_values, form(m), form(value 0), ...] — and any number of
// values up to LC_MAX_VALUES. One parser, so both refuse the same descriptions.
constexpr uint32_t LC_MAX_VALUES = 4096;
inline const char* lc_compile_interactions(const uint32_t* words, size_t n_words, uint32_t main_width, uint32_t prep_width, bool every,
                                           std::vector<uint32_t>& out) {
    out.assign(1, 0u);
    if (!words || n_words < 1) return "the description has no interaction count";
    size_t at = 1;
    const uint32_t n = words[0];
    if (main_width >= LC_PREP || prep_width >= LC_PREP) return "a table width of 2^31 or more";
    for (uint32_t k = 0; k < n; k++) {
        if (n_words - at < 3) return "the word list ends inside an interaction";
        const uint32_t is_send = words[at], kind = words[at + 1], n_values = words[at + 2];
        at += 3;
        if (is_send > 1) return "an interaction is neither a send nor a receive";
        const bool keep = every || (is_send == 1 && kind == LC_KIND_BYTE);
        if (keep && !every && n_values != 4) return "a byte message with other than 4 values";
        if (every && n_values > LC_MAX_VALUES) return "a message with more than 4096 values";
        const size_t head = out.size();
        if (keep) { out.push_back(k); out.push_back(0u); }
        if (every) { out.push_back(is_send); out.push_back(kind); out.push_back(n_values); }
        for (uint64_t f = 0; f < (uint64_t)n_values + 1; f++) {
            if (n_words - at < 2) return "the word list ends inside an affine form";
            const uint32_t n_terms = words[at], constant = words[at + 1];
            at += 2;
            if (constant >= kb::P) return "a constant outside the field";
            if ((n_words - at) / 3 < n_terms) return "the word list ends inside an affine form";
            if (keep) { out.push_back(n_terms); out.push_back(kb::to_monty(constant)); }
            for (uint32_t t = 0; t < n_terms; t++, at += 3) {
                const uint32_t is_main = words[at], column = words[at + 1], weight = words[at + 2];
                if (is_main > 1) return "a column that is neither main nor preprocessed";
                if (column >= (is_main ? main_width : prep_width)) return "a column index outside its table's width";
                if (weight >= kb::P) return "a weight outside the field";
                if (keep) { out.push_back(column | (is_main ? 0u : LC_PREP)); out.push_back(kb::to_monty(weight)); }
            }
        }
        if (keep) { out[head + 1] = (uint32_t)(out.size() - head); out[0]++; }
    }
    if (at != n_words) return "words after the last interaction";
    return nullptr;
}

inline const char* lc_compile(const uint32_t* words, size_t n_words, uint32_t main_width, uint32_t prep_width, std::vector<uint32_t>& out) {
    return lc_compile_interactions(words, n_words, main_width, prep_width, false, out);
}

}  // namespace tg
}  // namespace sp1hip
