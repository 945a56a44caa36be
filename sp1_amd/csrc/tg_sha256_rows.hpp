// sp1_amd/csrc/tg_sha256_rows.hpp — the rows of the four chips of the two SHA-256 precompile shards, for host and device code alike:
// ShaExtend (128 columns, 48 rows per SHA_EXTEND call), ShaExtendControl (18, one row per call), ShaCompress (206, 80 rows per
// SHA_COMPRESS call: 8 initialise, 64 compress, 8 finalise) and ShaCompressControl (53, one row per call), from the executor's event
// records (sp1hip_rv64_sha_extend_events: 786 u64, _sha_compress_events: 155 u64). The definitions followed are
//   ShaExtendChip::event_to_rows              crates/core/machine/src/syscall/precompiles/sha256/extend/trace.rs:L82-L190
//   ShaExtendControlChip                      .../sha256/extend/controller.rs:L172-L311
//   ShaCompressChip::event_to_rows, padding   .../sha256/compress/trace.rs:L78-L104, L120-L360
//   ShaCompressControlChip                    .../sha256/compress/controller.rs:L205-L345
//   FixedRotateRightOperation / FixedShiftRightOperation, XorU32Operation / AndU32Operation, Add4 / Add5 / AddU32 ::populate
// as sp1_amd/machines/riscv_more_trace.py restates them (sha_extend_shard_from, sha_compress_shard_from, _set_fixed, _set_byte_op,
// _set_sum, _mem_access_t, _syscall_addr_t), which the tests compare every word with. The column order is the one
// sp1_amd/machines/riscv_more.py transcribes (sha_extend_chip, sha_extend_control_chip, sha_compress_chip, sha_compress_control_chip).
//
// One lane (or one host loop iteration) owns one row and stores each value through tgf::Cursor as it is made, in table order: a row
// is never held. The eight working variables are eight named registers, never an array; the lane that owns a ShaCompress row
// recomputes the state entering its round from the event's h and w words (at most 64 rounds) and reads no other lane's row.
#pragma once
#include "tg_field_op.hpp"

namespace sp1hip {
namespace tgs {

using tgf::Cursor;
using tgf::event_word;

constexpr int EXTEND_EVENT_WORDS = 786, COMPRESS_EVENT_WORDS = 155;  // SP1HIP_RV64_SHA_EXTEND_WORDS, SP1HIP_RV64_SHA_COMPRESS_WORDS
constexpr int EXTEND_ROWS = 48, COMPRESS_ROWS = 80;                  // rows per call
constexpr int MEM_ACCESS = 9, FIXED_ROT = 4, BYTE_OP = 8, HALF_WORD = 2, ADDR = 3;

// the event records: clk, w_ptr, 48 steps x 11 words (4 x (previous timestamp, word read) for w[i-15], w[i-2], w[i-16], w[i-7], then
// w[i]'s previous timestamp, previous value and new value), then 64 x (initial timestamp, initial value, final timestamp, final value)
namespace ext {
constexpr int CLK = 0, W_PTR = 1, STEPS = 2, STEP_WORDS = 11, AROUND = STEPS + EXTEND_ROWS * STEP_WORDS;
constexpr int CLK_HIGH = 0, CLK_LOW = 1, NEXT_CLK = 2, W_PTR_COL = 5, W_I_MINUS_15_PTR = 8, W_I_MINUS_2_PTR = 11, W_I_MINUS_16_PTR = 14,
              W_I_MINUS_7_PTR = 17, W_I_PTR = 20, I = 23, W_I_MINUS_15 = 24, W_I_MINUS_15_RR_7 = W_I_MINUS_15 + MEM_ACCESS,
              S0_INTERMEDIATE = W_I_MINUS_15_RR_7 + 3 * FIXED_ROT, S0 = S0_INTERMEDIATE + BYTE_OP, W_I_MINUS_2 = S0 + BYTE_OP,
              W_I_MINUS_2_RR_17 = W_I_MINUS_2 + MEM_ACCESS, S1_INTERMEDIATE = W_I_MINUS_2_RR_17 + 3 * FIXED_ROT, S1 = S1_INTERMEDIATE + BYTE_OP,
              W_I_MINUS_16 = S1 + BYTE_OP, W_I_MINUS_7 = W_I_MINUS_16 + MEM_ACCESS, S2 = W_I_MINUS_7 + MEM_ACCESS, W_I = S2 + HALF_WORD,
              IS_REAL = W_I + MEM_ACCESS, WIDTH = IS_REAL + 1;
constexpr int CONTROL_WIDTH = 2 + tgf::SYSCALL_ADDR_COLS + 3 * ADDR + 1;
static_assert(AROUND == 530 && AROUND + 4 * 64 == EXTEND_EVENT_WORDS && WIDTH == 128 && CONTROL_WIDTH == 18, "ShaExtend layouts");
}  // namespace ext

// clk, w_ptr, h_ptr, 8 x (previous timestamp, h word), 64 x (previous timestamp, w word), the 8 h words written
namespace cmp {
constexpr int CLK = 0, W_PTR = 1, H_PTR = 2, H_READS = 3, W_READS = 19, H_WRITES = 147;
constexpr int CLK_HIGH = 0, CLK_LOW = 1, W_PTR_COL = 2, H_PTR_COL = 5, INDEX = 8, OCTET = 9, OCTET_NUM = 17, MEM = 27, MEM_VALUE = MEM + MEM_ACCESS,
              MEM_ADDR = MEM_VALUE + 2, MEM_ADDR_INIT = MEM_ADDR + ADDR, MEM_ADDR_COMPRESS = MEM_ADDR_INIT + ADDR,
              MEM_ADDR_FINALIZE = MEM_ADDR_COMPRESS + ADDR, A = MEM_ADDR_FINALIZE + ADDR, K = A + 16, E_RR_6 = K + 2,
              S1_INTERMEDIATE = E_RR_6 + 3 * FIXED_ROT, S1 = S1_INTERMEDIATE + BYTE_OP, E_AND_F = S1 + BYTE_OP, E_NOT = E_AND_F + BYTE_OP,
              E_NOT_AND_G = E_NOT + HALF_WORD, CH = E_NOT_AND_G + BYTE_OP, TEMP1 = CH + BYTE_OP, A_RR_2 = TEMP1 + HALF_WORD,
              S0_INTERMEDIATE = A_RR_2 + 3 * FIXED_ROT, S0 = S0_INTERMEDIATE + BYTE_OP, A_AND_B = S0 + BYTE_OP, A_AND_C = A_AND_B + BYTE_OP,
              B_AND_C = A_AND_C + BYTE_OP, MAJ_INTERMEDIATE = B_AND_C + BYTE_OP, MAJ = MAJ_INTERMEDIATE + BYTE_OP, TEMP2 = MAJ + BYTE_OP,
              D_ADD_TEMP1 = TEMP2 + HALF_WORD, TEMP1_ADD_TEMP2 = D_ADD_TEMP1 + HALF_WORD, FINALIZED_OPERAND = TEMP1_ADD_TEMP2 + HALF_WORD,
              FINALIZE_ADD = FINALIZED_OPERAND + 2, IS_INITIALIZE = FINALIZE_ADD + HALF_WORD, IS_COMPRESSION = IS_INITIALIZE + 1,
              IS_FINALIZE = IS_COMPRESSION + 1, IS_REAL = IS_FINALIZE + 1, WIDTH = IS_REAL + 1;
constexpr int COMPRESSION_COLS = FINALIZED_OPERAND - E_RR_6;    // the column groups that are zero off the compression rows
constexpr int CONTROL_WIDTH = 2 + 2 * tgf::SYSCALL_ADDR_COLS + 2 * ADDR + 1 + 16 + 16;
static_assert(H_WRITES + 8 == COMPRESS_EVENT_WORDS && WIDTH == 206 && COMPRESSION_COLS == 130 && CONTROL_WIDTH == 53, "ShaCompress layouts");
}  // namespace cmp

// the round constants (FIPS 180-4 §4.2.2): read-only data on the device, indexed by the round
TG_HD uint32_t round_constant(uint32_t i) {
    static constexpr uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
        0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
        0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
        0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
        0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
        0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    return K[i];
}

template <int R> TG_HD uint32_t rotr(uint32_t x) { return (x >> R) | (x << (32 - R)); }

// a u32 as two 16-bit limbs
TG_HD void half(Cursor& w, uint32_t v) {
    w.val(v & 0xffffu);
    w.val(v >> 16);
}
// FixedRotateRightOperation (SHIFT false) / FixedShiftRightOperation (true) by the constant R: value[2], higher_limb[2] — the limbs
// the result's limbs start from, shifted right by R mod 16
template <int R, bool SHIFT> TG_HD uint32_t fixed(Cursor& w, uint32_t x) {
    constexpr int NL = R / 16, NB = R % 16;
    const uint32_t lo = x & 0xffffu, hi = x >> 16;
    const uint32_t out = SHIFT ? x >> R : rotr<R>(x);
    const uint32_t first = NL ? hi : lo, second = SHIFT ? (NL ? 0u : hi) : (NL ? lo : hi);
    half(w, out);
    w.val(first >> NB);
    w.val(second >> NB);
    return out;
}
// XorU32Operation / AndU32Operation: the low bytes of both operands' limbs, the result's four bytes
TG_HD uint32_t byte_op(Cursor& w, uint32_t x, uint32_t y, bool is_xor) {
    const uint32_t out = is_xor ? x ^ y : x & y;
    w.val(x & 0xffu);
    w.val((x >> 16) & 0xffu);
    w.val(y & 0xffu);
    w.val((y >> 16) & 0xffu);
#pragma unroll
    for (int i = 0; i < 4; i++) w.val((out >> (8 * i)) & 0xffu);
    return out;
}
TG_HD uint32_t xor_op(Cursor& w, uint32_t x, uint32_t y) { return byte_op(w, x, y, true); }
TG_HD uint32_t and_op(Cursor& w, uint32_t x, uint32_t y) { return byte_op(w, x, y, false); }
// Add4 / Add5 / AddU32: the sum modulo 2^32
TG_HD uint32_t sum(Cursor& w, uint32_t v) {
    half(w, v);
    return v;
}

// Row 48 e + r of ShaExtend: step i = 16 + r of event e, at clk + 1 + r; rows behind the events' are zero
TG_HD void sha_extend_row(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* events, uint32_t n_events) {
    Cursor w{out, row, height};
    const uint32_t e = row / EXTEND_ROWS, r = row - e * EXTEND_ROWS;
    if (e >= n_events) {
        w.zeros(ext::WIDTH);
        return;
    }
    const uint64_t* ev = events + (size_t)e * EXTEND_EVENT_WORDS;
    const int st = ext::STEPS + ext::STEP_WORDS * (int)r;
    const uint64_t clk = event_word(ev, ext::CLK), w_ptr = event_word(ev, ext::W_PTR);
    const uint32_t i = 16 + r;
    const uint32_t row_low = ((uint32_t)clk & 0xffffffu) + 1;                                   // the controller hands over (clk_high, clk_low + 1)
    const uint32_t next = row_low + r;
    const uint64_t ts = clk + 1 + r;
    w.val((uint32_t)(clk >> 24));
    w.val(row_low);
    w.val((next >> 16) & 0xffu);                                                                 // next_clk: next_clk_16_24, next_clk_0_16, is_overflow
    w.val(next & 0xffffu);
    w.bit((next >> 24) & 1);
    w.limbs(w_ptr, 3);
    tgf::addr_add(w, w_ptr + 8ull * (i - 15));
    tgf::addr_add(w, w_ptr + 8ull * (i - 2));
    tgf::addr_add(w, w_ptr + 8ull * (i - 16));
    tgf::addr_add(w, w_ptr + 8ull * (i - 7));
    tgf::addr_add(w, w_ptr + 8ull * i);
    w.val(i);
    const uint64_t w15 = event_word(ev, st + 1), w2 = event_word(ev, st + 3), w16 = event_word(ev, st + 5), w7 = event_word(ev, st + 7);
    tgf::memory_access(w, w15, event_word(ev, st + 0), ts);
    uint32_t x = (uint32_t)w15;
    const uint32_t a7 = fixed<7, false>(w, x), a18 = fixed<18, false>(w, x), a3 = fixed<3, true>(w, x);
    const uint32_t s0 = xor_op(w, xor_op(w, a7, a18), a3);
    tgf::memory_access(w, w2, event_word(ev, st + 2), ts);
    x = (uint32_t)w2;
    const uint32_t b17 = fixed<17, false>(w, x), b19 = fixed<19, false>(w, x), b10 = fixed<10, true>(w, x);
    const uint32_t s1 = xor_op(w, xor_op(w, b17, b19), b10);
    tgf::memory_access(w, w16, event_word(ev, st + 4), ts);
    tgf::memory_access(w, w7, event_word(ev, st + 6), ts);
    sum(w, (uint32_t)w16 + s0 + (uint32_t)w7 + s1);
    tgf::memory_access(w, event_word(ev, st + 9), event_word(ev, st + 8), ts);                  // the write of w[i] against its previous access
    w.bit(true);
}

// Row e of ShaExtendControl
TG_HD void sha_extend_control_row(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* events, uint32_t n_events) {
    Cursor w{out, row, height};
    if (row >= n_events) {
        w.zeros(ext::CONTROL_WIDTH);
        return;
    }
    const uint64_t* ev = events + (size_t)row * EXTEND_EVENT_WORDS;
    const uint64_t clk = event_word(ev, ext::CLK), w_ptr = event_word(ev, ext::W_PTR);
    w.val((uint32_t)(clk >> 24));
    w.val((uint32_t)clk & 0xffffffu);
    tgf::syscall_addr(w, w_ptr);
    tgf::addr_add(w, w_ptr + 8ull * 15);
    tgf::addr_add(w, w_ptr + 8ull * 16);
    tgf::addr_add(w, w_ptr + 8ull * 63);
    w.bit(true);
}

// The eight working variables, and one compression round on them
struct State { uint32_t a, b, c, d, e, f, g, h; };
TG_HD State initial_state(const uint64_t* ev) {
    return {(uint32_t)event_word(ev, cmp::H_READS + 1), (uint32_t)event_word(ev, cmp::H_READS + 3), (uint32_t)event_word(ev, cmp::H_READS + 5),
            (uint32_t)event_word(ev, cmp::H_READS + 7), (uint32_t)event_word(ev, cmp::H_READS + 9), (uint32_t)event_word(ev, cmp::H_READS + 11),
            (uint32_t)event_word(ev, cmp::H_READS + 13), (uint32_t)event_word(ev, cmp::H_READS + 15)};
}
TG_HD void round_in_place(State& s, uint32_t k, uint32_t wv) {
    const uint32_t s1 = rotr<6>(s.e) ^ rotr<11>(s.e) ^ rotr<25>(s.e), ch = (s.e & s.f) ^ (~s.e & s.g);
    const uint32_t t1 = s.h + s1 + ch + k + wv;
    const uint32_t s0 = rotr<2>(s.a) ^ rotr<13>(s.a) ^ rotr<22>(s.a), mj = (s.a & s.b) ^ (s.a & s.c) ^ (s.b & s.c);
    s = {t1 + s0 + mj, s.a, s.b, s.c, s.d + t1, s.e, s.f, s.g};
}
// the state after `rounds` rounds of the event's compression
TG_HD State state_after(const uint64_t* ev, uint32_t rounds) {
    State s = initial_state(ev);
    for (uint32_t t = 0; t < rounds; t++) round_in_place(s, round_constant(t), (uint32_t)event_word(ev, cmp::W_READS + 2 * (int)t + 1));
    return s;
}
// working variable q of a state, by selects
TG_HD uint32_t variable(const State& s, uint32_t q) {
    return q == 0 ? s.a : q == 1 ? s.b : q == 2 ? s.c : q == 3 ? s.d : q == 4 ? s.e : q == 5 ? s.f : q == 6 ? s.g : s.h;
}

// Row 80 e + j of ShaCompress: j < 8 reads h[j] at clk, 8 <= j < 72 is round j - 8 and reads w[j - 8] at clk + 1, j >= 72 writes
// h[j - 72] at clk + 2. octet, octet_num, index and k cycle by row mod 80 on EVERY row of the table; a row behind the events' rows
// holds nothing else.
TG_HD void sha_compress_row(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* events, uint32_t n_events) {
    Cursor w{out, row, height};
    const uint32_t e = row / COMPRESS_ROWS, j = row - e * COMPRESS_ROWS;
    const uint32_t octet = j & 7u, octet_num = j >> 3;
    const uint32_t phase = j < 8 ? 0u : j < 72 ? 1u : 2u;
    const uint32_t k = phase == 1 ? round_constant(j - 8) : 0u;
    const bool real = e < n_events;
    if (!real) {
        w.zeros(cmp::INDEX);
        w.val(j);
        for (uint32_t i = 0; i < 8; i++) w.bit(i == octet);
        for (uint32_t i = 0; i < 10; i++) w.bit(i == octet_num);
        w.zeros(cmp::K - cmp::MEM);
        half(w, k);
        w.zeros(cmp::WIDTH - cmp::E_RR_6);
        return;
    }
    const uint64_t* ev = events + (size_t)e * COMPRESS_EVENT_WORDS;
    const uint64_t clk = event_word(ev, cmp::CLK), w_ptr = event_word(ev, cmp::W_PTR), h_ptr = event_word(ev, cmp::H_PTR);
    const uint32_t wq = phase == 0 ? 0u : phase == 1 ? j - 8 : 63u;
    const State s = state_after(ev, phase == 0 ? 0u : phase == 1 ? j - 8 : 64u);
    w.val((uint32_t)(clk >> 24));
    w.val((uint32_t)clk & 0xffffffu);
    w.limbs(w_ptr, 3);
    w.limbs(h_ptr, 3);
    w.val(j);
    for (uint32_t i = 0; i < 8; i++) w.bit(i == octet);
    for (uint32_t i = 0; i < 10; i++) w.bit(i == octet_num);
    // the row's memory access
    const int read = phase == 1 ? cmp::W_READS + 2 * (int)wq : cmp::H_READS + 2 * (int)octet;
    const uint64_t addr = phase == 1 ? w_ptr + 8ull * wq : h_ptr + 8ull * octet;
    const uint64_t prev_value = event_word(ev, read + 1);
    const uint64_t t_prev = phase == 2 ? clk : event_word(ev, read);
    const uint32_t value = phase == 2 ? (uint32_t)event_word(ev, cmp::H_WRITES + (int)octet) : (uint32_t)prev_value;
    tgf::memory_access(w, prev_value, t_prev, clk + phase);
    half(w, value);
    w.limbs(addr, 3);
    for (uint32_t p = 0; p < 3; p++) w.limbs(p == phase ? addr : 0ull, 3);                       // mem_addr_init, _compress, _finalize
    half(w, s.a); half(w, s.b); half(w, s.c); half(w, s.d); half(w, s.e); half(w, s.f); half(w, s.g); half(w, s.h);
    half(w, k);
    if (phase == 1) {
        const uint32_t e6 = fixed<6, false>(w, s.e), e11 = fixed<11, false>(w, s.e), e25 = fixed<25, false>(w, s.e);
        const uint32_t s1 = xor_op(w, xor_op(w, e6, e11), e25);
        const uint32_t e_and_f = and_op(w, s.e, s.f);
        const uint32_t e_not = sum(w, ~s.e);
        const uint32_t e_not_and_g = and_op(w, e_not, s.g);
        const uint32_t ch = xor_op(w, e_and_f, e_not_and_g);
        const uint32_t t1 = sum(w, s.h + s1 + ch + k + (uint32_t)prev_value);
        const uint32_t a2 = fixed<2, false>(w, s.a), a13 = fixed<13, false>(w, s.a), a22 = fixed<22, false>(w, s.a);
        const uint32_t s0 = xor_op(w, xor_op(w, a2, a13), a22);
        const uint32_t a_and_b = and_op(w, s.a, s.b), a_and_c = and_op(w, s.a, s.c), b_and_c = and_op(w, s.b, s.c);
        const uint32_t mj = xor_op(w, xor_op(w, a_and_b, a_and_c), b_and_c);
        const uint32_t t2 = sum(w, s0 + mj);
        sum(w, s.d + t1);
        sum(w, t1 + t2);
    } else {
        w.zeros(cmp::COMPRESSION_COLS);
    }
    const uint32_t operand = phase == 2 ? variable(s, octet) : 0u;
    half(w, operand);
    half(w, phase == 2 ? (uint32_t)prev_value + operand : 0u);
    w.bit(phase == 0);
    w.bit(phase == 1);
    w.bit(phase == 2);
    w.bit(true);
}

// Row e of ShaCompressControl: the state read and the state after the 64 rounds (the digest words written are their sums)
TG_HD void sha_compress_control_row(uint32_t* out, uint32_t height, uint32_t row, const uint64_t* events, uint32_t n_events) {
    Cursor w{out, row, height};
    if (row >= n_events) {
        w.zeros(cmp::CONTROL_WIDTH);
        return;
    }
    const uint64_t* ev = events + (size_t)row * COMPRESS_EVENT_WORDS;
    const uint64_t clk = event_word(ev, cmp::CLK), w_ptr = event_word(ev, cmp::W_PTR), h_ptr = event_word(ev, cmp::H_PTR);
    w.val((uint32_t)(clk >> 24));
    w.val((uint32_t)clk & 0xffffffu);
    tgf::syscall_addr(w, w_ptr);
    tgf::syscall_addr(w, h_ptr);
    tgf::addr_add(w, w_ptr + 8ull * 63);
    tgf::addr_add(w, h_ptr + 8ull * 7);
    w.bit(true);
    const State s0 = initial_state(ev), s = state_after(ev, 64);
    half(w, s0.a); half(w, s0.b); half(w, s0.c); half(w, s0.d); half(w, s0.e); half(w, s0.f); half(w, s0.g); half(w, s0.h);
    half(w, s.a); half(w, s.b); half(w, s.c); half(w, s.d); half(w, s.e); half(w, s.f); half(w, s.g); half(w, s.h);
}

}  // namespace tgs
}  // namespace sp1hip
