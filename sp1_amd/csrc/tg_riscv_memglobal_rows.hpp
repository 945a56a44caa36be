// sp1_amd/csrc/tg_riscv_memglobal_rows.hpp — the rows of the chips that close a memory shard and a precompile shard:
// MemoryGlobalInit / MemoryGlobalFinalize, SyscallPrecompile, the Global event each of their rows stands for, and the step from a
// precompile's event record to the MemoryLocal records of the words it touched — for host and device code alike (as
// tg_riscv_sys_rows.hpp is for the small chips of a core shard, whose Row, inverse and kind constants it takes).
// tracegen_riscv_memglobal.hip calls them one lane per row; tests/native/riscv_memglobal_rows.hip runs the same functions on the
// CPU, so every word can be compared with the host tracer (sp1_amd/machines/riscv_more_trace.py memory_shard_from,
// _close_precompile_shard) without a GPU.
//
//   MemoryGlobalInit / Finalize  crates/core/machine/src/memory/global.rs (generate_trace_into; eval L307-L474): both kinds share one
//                                layout, the kind only decides the Global message
//   SyscallPrecompile            crates/core/machine/src/syscall/chip.rs (generate_trace_into; its Global receive L299-L420)
//   MemoryLocal records          crates/core/machine/src/memory/local.rs: a precompile shard has one row per word of each call
#pragma once
#include "tg_riscv_sys_rows.hpp"

namespace sp1hip {
namespace tg {

constexpr int MEMORY_GLOBAL_WIDTH = 30, SYSCALL_PRECOMPILE_WIDTH = 10;
constexpr int MEMORY_GLOBAL_RECORD_WORDS = 3;                 // { addr, value, timestamp }
constexpr int PRECOMPILE_MAX_SEGMENTS = 4;
constexpr uint32_t PRECOMPILE_NO_WORD = 0xffffffffu;          // a segment whose words are only read has no final_word
constexpr uint32_t PRECOMPILE_QUAD_WORDS = 0xfffffffeu;       // final_word of a segment in the quad form: four record words per word

namespace col {
constexpr int MG_CLK_HIGH = 0, MG_CLK_LOW = 1, MG_INDEX = 2, MG_PREV_ADDR = 3, MG_ADDR = 6, MG_LT_BIT = 9, MG_LT_U16_FLAGS = 10,
              MG_LT_NOT_EQ_INV = 14, MG_LT_COMPARISON_LIMBS = 15, MG_VALUE = 17, MG_VALUE_LOWER = 21, MG_VALUE_UPPER = 22, MG_IS_REAL = 23,
              MG_IS_COMP = 24, MG_PREV_VALID = 25, MG_IS_PREV_ADDR_ZERO = 26, MG_IS_INDEX_ZERO = 28;
constexpr int SP_CLK_HIGH = 0, SP_CLK_LOW = 1, SP_SYSCALL_ID = 2, SP_ARG1 = 3, SP_ARG2 = 6, SP_IS_REAL = 9;
}  // namespace col

// MemoryGlobalInit / MemoryGlobalFinalize from record `index` = { addr, value, timestamp } and the address before it (record
// index - 1's, the call's previous_addr for index 0); padding rows are zero. Three field inversions: of the sum of prev_addr's
// limbs, of the index, of the difference of the compared limbs.
TG_HD void fill_memory_global(Row<MEMORY_GLOBAL_WIDTH>& r, const uint64_t* rec, uint64_t prev, uint32_t index) {
    namespace c = col;
    const uint64_t addr = rec[0], v = rec[1], t = rec[2];
    r.c[c::MG_CLK_HIGH] = (uint32_t)(t >> 24); r.c[c::MG_CLK_LOW] = (uint32_t)t & 0xffffffu;
    r.c[c::MG_INDEX] = index;
    r.limbs3(c::MG_PREV_ADDR, prev); r.limbs3(c::MG_ADDR, addr); r.limbs4(c::MG_VALUE, v);
    r.c[c::MG_VALUE_LOWER] = (uint32_t)(v >> 32) & 0xff; r.c[c::MG_VALUE_UPPER] = (uint32_t)(v >> 40) & 0xff;
    r.c[c::MG_IS_REAL] = 1;
    const bool comp = prev != 0 || index != 0;
    r.c[c::MG_IS_COMP] = comp;
    r.c[c::MG_PREV_VALID] = !(prev == 0 && index != 0);
    const uint32_t sum = r.c[c::MG_PREV_ADDR] + r.c[c::MG_PREV_ADDR + 1] + r.c[c::MG_PREV_ADDR + 2];
    r.c[c::MG_IS_PREV_ADDR_ZERO] = inv_canonical(sum); r.c[c::MG_IS_PREV_ADDR_ZERO + 1] = sum == 0;
    r.c[c::MG_IS_INDEX_ZERO] = inv_canonical(index); r.c[c::MG_IS_INDEX_ZERO + 1] = index == 0;
    // lt_cols: prev < addr through the most significant of the four 16-bit limbs that differ (limb 3 when none does); every
    // column times is_comp, so the uncompared row (address 0 opening the first shard) keeps its eight zeros
    if (comp) {
        const uint64_t diff = prev ^ addr;
        const int j = diff >> 48 ? 3 : diff >> 32 ? 2 : diff >> 16 ? 1 : diff ? 0 : 3;
        const uint32_t x = (uint32_t)(prev >> (16 * j)) & M16, y = (uint32_t)(addr >> (16 * j)) & M16;
#pragma unroll
        for (int i = 0; i < 4; i++) r.c[c::MG_LT_U16_FLAGS + i] = j == i;
        r.c[c::MG_LT_COMPARISON_LIMBS] = x; r.c[c::MG_LT_COMPARISON_LIMBS + 1] = y;
        r.c[c::MG_LT_NOT_EQ_INV] = inv_canonical(x >= y ? x - y : kb::P - (y - x));
        r.c[c::MG_LT_BIT] = x < y;
    }
}

// The row's Global event as sp1hip_tracegen_riscv_global reads it, 9 words: message = clk_high, clk_low (both zero for Init, whatever
// its clk columns hold), addr[3], value[0] + lower * 2^16, value[1] + upper * 2^16, value[3]; then is_receive | kind << 8. Init sends,
// Finalize receives; kind Memory
TG_HD void memory_global_event(int32_t* o, const uint64_t* rec, bool finalize) {
    const uint64_t addr = rec[0], v = rec[1], t = rec[2];
    o[0] = finalize ? (int32_t)(t >> 24) : 0; o[1] = finalize ? (int32_t)((uint32_t)t & 0xffffffu) : 0;
    o[2] = (int32_t)(addr & M16); o[3] = (int32_t)((addr >> 16) & M16); o[4] = (int32_t)((addr >> 32) & M16);
    o[5] = (int32_t)((v & M16) + (((v >> 32) & 0xff) << 16));
    o[6] = (int32_t)(((v >> 16) & M16) + (((v >> 40) & 0xff) << 16));
    o[7] = (int32_t)((v >> 48) & M16);
    o[8] = (int32_t)((finalize ? 1u : 0u) | KIND_MEMORY << 8);
}

// SyscallPrecompile from a precompile's event record as the executor leaves it: word 0 the clk, word 1 the first pointer, word
// arg2_word the second (arg2_word < 0: none); padding rows are zero
TG_HD void fill_syscall_precompile(Row<SYSCALL_PRECOMPILE_WIDTH>& r, const uint64_t* ev, uint32_t syscall_id, int arg2_word) {
    namespace c = col;
    r.c[c::SP_CLK_HIGH] = (uint32_t)(ev[0] >> 24); r.c[c::SP_CLK_LOW] = (uint32_t)ev[0] & 0xffffffu;
    r.c[c::SP_SYSCALL_ID] = syscall_id;
    r.limbs3(c::SP_ARG1, ev[1]); r.limbs3(c::SP_ARG2, arg2_word >= 0 ? ev[arg2_word] : 0ull);
    r.c[c::SP_IS_REAL] = 1;
}

// Its Global event, what syscall_core_global_event sends received: message = clk_high, clk_low, syscall_id + arg1[0] * 2^8, arg1[1],
// arg1[2], arg2[3]; then 1 | kind Syscall << 8
TG_HD void syscall_precompile_global_event(int32_t* o, const uint64_t* ev, uint32_t syscall_id, int arg2_word) {
    const uint64_t a1 = ev[1], a2 = arg2_word >= 0 ? ev[arg2_word] : 0ull;
    o[0] = (int32_t)(ev[0] >> 24); o[1] = (int32_t)((uint32_t)ev[0] & 0xffffffu);
    o[2] = (int32_t)(syscall_id + (((uint32_t)a1 & M16) << 8));
    o[3] = (int32_t)((a1 >> 16) & M16); o[4] = (int32_t)((a1 >> 32) & M16);
    o[5] = (int32_t)(a2 & M16); o[6] = (int32_t)((a2 >> 16) & M16); o[7] = (int32_t)((a2 >> 32) & M16);
    o[8] = (int32_t)(1u | KIND_SYSCALL << 8);
}

// The chips of row_kernel / host_rows (tg_row_kernel.hpp). `global_events` (may be null): [n][9] words, row i's event at row i.
// MemoryGlobal's row i reads record i and the ADDRESS of record i - 1 (the call's previous_addr for row 0): the one neighbour read
// among the chips. On the device it is a second load of a word the lane before loads as its own, not an exchange between lanes, so
// it is the same at a wave's and a workgroup's first lane as anywhere else.
struct MemoryGlobal : ZeroPaddedChip<MEMORY_GLOBAL_WIDTH, uint64_t> {
    static TG_HD void live(Row<WIDTH>& r, const uint64_t* __restrict__ records, uint32_t row, uint64_t previous_addr, int finalize,
                           int32_t* __restrict__ global_events) {
        uint64_t rec[MEMORY_GLOBAL_RECORD_WORDS];
        load_record<MEMORY_GLOBAL_RECORD_WORDS>(rec, records, row);
        const uint64_t prev = row ? records[(size_t)(row - 1) * MEMORY_GLOBAL_RECORD_WORDS] : previous_addr;
        fill_memory_global(r, rec, prev, row);
        if (global_events) {
            int32_t ev[GLOBAL_EVENT_WORDS];
            memory_global_event(ev, rec, finalize != 0);
            store_global_events<1>(global_events, row, ev);
        }
    }
};
struct SyscallPrecompile : ZeroPaddedChip<SYSCALL_PRECOMPILE_WIDTH, uint64_t> {
    static TG_HD void live(Row<WIDTH>& r, const uint64_t* __restrict__ events, uint32_t row, uint32_t words_per_event, uint32_t syscall_id, int arg2_word,
                           int32_t* __restrict__ global_events) {
        const uint64_t* e = events + (size_t)row * words_per_event;
        fill_syscall_precompile(r, e, syscall_id, arg2_word);
        if (global_events) {
            int32_t ev[GLOBAL_EVENT_WORDS];
            syscall_precompile_global_event(ev, e, syscall_id, arg2_word);
            store_global_events<1>(global_events, row, ev);
        }
    }
};
// The same for a shard that mixes system calls (FpOpAssign: ADD, SUB, MUL; Fp2AddSubAssign: ADD, SUB): the id is the low byte of
// the event's own word `code_word`
struct SyscallPrecompileCoded : ZeroPaddedChip<SYSCALL_PRECOMPILE_WIDTH, uint64_t> {
    static TG_HD void live(Row<WIDTH>& r, const uint64_t* __restrict__ events, uint32_t row, uint32_t words_per_event, uint32_t code_word, int arg2_word,
                           int32_t* __restrict__ global_events) {
        const uint64_t* e = events + (size_t)row * words_per_event;
        const uint32_t syscall_id = (uint32_t)e[code_word] & 0xffu;
        fill_syscall_precompile(r, e, syscall_id, arg2_word);
        if (global_events) {
            int32_t ev[GLOBAL_EVENT_WORDS];
            syscall_precompile_global_event(ev, e, syscall_id, arg2_word);
            store_global_events<1>(global_events, row, ev);
        }
    }
};

// One run of consecutive words a precompile touches through one pointer: event word ptr_word holds the pointer, `count` words
// follow it in memory; event words pairs_word + 2 i, + 2 i + 1 hold word i's previous timestamp and value, event word final_word + i
// the value the call leaves (PRECOMPILE_NO_WORD: the words are only read and keep theirs); the call's last access to them is at
// clk + final_clk_delta. The quad form (final_word = PRECOMPILE_QUAD_WORDS) is for a call whose words end at different timestamps
// (SHA_EXTEND): event words pairs_word + 4 i .. + 4 i + 3 hold word i's initial timestamp, initial value, final timestamp and final
// value, and final_clk_delta is not read
struct LocalSegment { uint32_t ptr_word, count, pairs_word, final_word, final_clk_delta; };
struct LocalSegments { LocalSegment s[PRECOMPILE_MAX_SEGMENTS]; uint32_t n; };

// The MemoryLocal record { addr, initial clk, initial value, final clk, final value } of word i of event `ev` in segment `s`
TG_HD void precompile_local_record(uint64_t* rec, const uint64_t* ev, const LocalSegment& s, uint32_t i) {
    const bool quad = s.final_word == PRECOMPILE_QUAD_WORDS;
    const uint32_t at = s.pairs_word + (quad ? 4 : 2) * i;
    rec[0] = ev[s.ptr_word] + 8ull * i;
    rec[1] = ev[at];
    rec[2] = ev[at + 1];
    rec[3] = quad ? ev[at + 2] : ev[0] + s.final_clk_delta;
    rec[4] = quad ? ev[at + 3] : s.final_word == PRECOMPILE_NO_WORD ? rec[2] : ev[s.final_word + i];
}

// Where record `q` of a shard of n_events events comes from: the segments lie one after the other, segment s holding n_events *
// count_s records, event by event. False when q lies behind the last segment. (The loop is unrolled over constant indices: the
// segments are kernel arguments, and a lane-dependent index into them would move them to scratch.)
TG_HD bool precompile_local_locate(const LocalSegments& segs, uint32_t n_events, uint64_t q, LocalSegment& seg, uint32_t& event, uint32_t& word) {
    bool found = false;
#pragma unroll
    for (int k = 0; k < PRECOMPILE_MAX_SEGMENTS; k++) {
        if (found || (uint32_t)k >= segs.n) continue;
        const uint64_t size = (uint64_t)n_events * segs.s[k].count;
        if (q < size) { seg = segs.s[k]; event = (uint32_t)(q / segs.s[k].count); word = (uint32_t)(q % segs.s[k].count); found = true; }
        else q -= size;
    }
    return found;
}

}  // namespace tg
}  // namespace sp1hip
