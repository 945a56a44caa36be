// sp1_amd/csrc/tg_poseidon2_rows.hpp — the row of the Poseidon2 precompile chip (POSEIDON2: eight u64 words at ptr, sixteen KoalaBear
// elements low half first, rewritten in place by one permutation), for host and device code alike, on the memory columns of
// tg_field_op.hpp and the permutation walk of septic.hpp (perm_rows: the Global chip's 179 columns). The definition followed is
//   Poseidon2Chip::generate_trace_into       crates/core/machine/src/syscall/precompiles/poseidon2/air.rs:L107-L290
// as sp1_amd/machines/riscv_more_trace.py restates it (poseidon2_shard_from), which the tests compare every word with. The column
// offsets are the #[repr(C)] order that riscv_more.poseidon2_chip transcribes.
//
// One lane owns one row; the sixteen state words are indexed by constants only; the permutation's columns go to memory as perm_rows
// makes them, from the words READ (a wrong word written fails the chip's output constraints, as on the host).
#pragma once
#include "septic.hpp"
#include "tg_field_op.hpp"

namespace sp1hip {
namespace tgp {

using tgf::Cursor;
constexpr int EVENT_WORDS = 26;                                    // clk, ptr, 8 x (previous timestamp, word read), 8 words written
constexpr int WORDS = 8, MEMORY_ACCESS_COLS = 9, PERMUTATION_COLS = 179;
constexpr int CLK_HIGH = 0, CLK_LOW = 1, PTR = 2, ADDRS = PTR + tgf::SYSCALL_ADDR_COLS, MEMORY = ADDRS + 3 * WORDS,
              HASH_RESULT = MEMORY + MEMORY_ACCESS_COLS * WORDS, HASH_RESULT_RANGE_CHECKERS = HASH_RESULT + 4 * WORDS,
              INPUT_RANGE_CHECKERS = HASH_RESULT_RANGE_CHECKERS + 2 * WORDS, PERMUTATION = INPUT_RANGE_CHECKERS + 2 * WORDS,
              IS_REAL = PERMUTATION + PERMUTATION_COLS, WIDTH = IS_REAL + 1;
static_assert(WIDTH == 348 && MEMORY == 32 && HASH_RESULT == 104 && PERMUTATION == 168, "Poseidon2 layout");
constexpr uint32_t TOP_LIMB = (kb::P - 1) >> 16;                   // SP1FieldWordRangeChecker: the upper limb of a half is below this, or not

// The two SP1FieldWordRangeChecker bits of a word: limb 1 below TOP_LIMB for the low half, limb 3 for the high half
TG_HD void range_checker_bits(Cursor& w, uint64_t word) {
    w.bit(((uint32_t)(word >> 16) & 0xffffu) < TOP_LIMB);
    w.bit((uint32_t)(word >> 48) < TOP_LIMB);
}

// One row of the Poseidon2 chip. `ev` = the event's words, or null for a padding row: zero but for the permutation columns, which
// are those of the zero state. `rc`: the permutation's round constants (device memory on the device).
TG_HD void poseidon2_row(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* ev, const p2::RoundConstants* rc) {
    Cursor w{out, row, height};
    uint32_t s[2 * WORDS];
    if (ev != nullptr) {
        const uint64_t clk = tgf::event_word(ev, 0), ptr = tgf::event_word(ev, 1);
        uint64_t pre[WORDS];
#pragma unroll
        for (int i = 0; i < WORDS; i++) pre[i] = tgf::event_word(ev, 3 + 2 * i);
        w.val((uint32_t)(clk >> 24));
        w.val((uint32_t)clk & 0xffffffu);
        tgf::syscall_addr(w, ptr);
        for (uint32_t i = 0; i < (uint32_t)WORDS; i++) tgf::addr_add(w, ptr + 8u * i);
#pragma unroll
        for (int i = 0; i < WORDS; i++) tgf::memory_access(w, pre[i], tgf::event_word(ev, 2 + 2 * i), clk);
        for (int i = 0; i < WORDS; i++) w.limbs(tgf::event_word(ev, 2 + 2 * WORDS + i));
        for (int i = 0; i < WORDS; i++) range_checker_bits(w, tgf::event_word(ev, 2 + 2 * WORDS + i));
#pragma unroll
        for (int i = 0; i < WORDS; i++) {
            range_checker_bits(w, pre[i]);
            s[2 * i] = kb::to_monty((uint32_t)pre[i] % kb::P);
            s[2 * i + 1] = kb::to_monty((uint32_t)(pre[i] >> 32) % kb::P);
        }
    } else {
        w.zeros(PERMUTATION);
#pragma unroll
        for (int i = 0; i < 2 * WORDS; i++) s[i] = 0;
    }
    septic::perm_rows(s, rc, [&](int col, uint32_t v) {
        w.seek((uint32_t)(PERMUTATION + col), row);
        w.word(v);
    }, true);
    w.seek(IS_REAL, row);
    w.bit(ev != nullptr);
}

}  // namespace tgp
}  // namespace sp1hip
