// sp1_amd/csrc/jagged_kernels.hpp — the device side of the jagged evaluation proof: the descriptors the host fills (JgSeg .. JgTab,
// JeCols, JeV), the round kernels of the jagged sumcheck (round 0 and the first folds in their generic and table-major forms, the
// factored folds, the later folds) and the kernels of the jagged-eval sumcheck (branching-program suffixes, the two round halves).
// Included by jagged.hip only (the prover and its launches; the shape of the stage is described there).
#pragma once
#include "device_ctx.hpp"
#include "round_sync.hpp"

namespace sp1hip {

using Ext = kb::Ext;

struct JgSeg { const uint32_t* ptr; uint32_t start, len; };
struct JgSegs { JgSeg s[8]; int n; uint32_t total; };

struct JgJ {                       // what J(x) needs
    const uint32_t* prefix;        // [ncols + 1]
    uint32_t ncols;
    const Ext* col_eq;             // [>= ncols] AoS
    const uint32_t* row_eq;        // SoA, 4 planes of row_len
    uint32_t row_len;
};

__device__ __forceinline__ Ext ld_ext(const Ext* p, uint32_t i) {
    const uint4 v = reinterpret_cast<const uint4*>(p)[i];
    return Ext{{v.x, v.y, v.z, v.w}};
}
__device__ __forceinline__ void st_ext(Ext* p, uint32_t i, const Ext& e) {
    reinterpret_cast<uint4*>(p)[i] = make_uint4(e.c[0], e.c[1], e.c[2], e.c[3]);
}

__device__ __forceinline__ uint32_t jg_q(const JgSegs& S, uint32_t x) {
#pragma unroll 1
    for (int k = 0; k < S.n; k++)
        if (x - S.s[k].start < S.s[k].len) return S.s[k].ptr[x - S.s[k].start];
    return 0u;
}

// last column c with prefix[c] <= x  (then prefix[c + 1] > x because x < prefix[ncols])
__device__ __forceinline__ uint32_t jg_find_col(const JgJ& J, uint32_t x) {
    uint32_t lo = 0, hi = J.ncols;   // invariant: prefix[lo] <= x < prefix[hi]
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (J.prefix[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ Ext jg_j_at(const JgJ& J, uint32_t c, uint32_t row) {
    const Ext r{{J.row_eq[row], J.row_eq[J.row_len + row], J.row_eq[2 * J.row_len + row], J.row_eq[3 * J.row_len + row]}};
    return kb::ext_mul(ld_ext(J.col_eq, c), r);
}

// q and J for NV consecutive dense indices x0 .. x0 + NV - 1 (zero past `total`)
template <int NV>
__device__ __forceinline__ void jg_load_base(const JgSegs& S, const JgJ& J, uint32_t x0, uint32_t (&q)[NV], Ext (&j)[NV]) {
    uint32_t c = 0;
    bool have = false;
#pragma unroll
    for (int v = 0; v < NV; v++) {
        const uint32_t x = x0 + v;
        if (x >= S.total) { q[v] = 0u; j[v] = kb::ext_zero(); continue; }
        q[v] = jg_q(S, x);
        if (!have) { c = jg_find_col(J, x); have = true; }
        else while (J.prefix[c + 1] <= x) c++;
        j[v] = jg_j_at(J, c, x - J.prefix[c]);
    }
}

// The end of every round kernel of this file: the two extension sums of the round go through the last-workgroup hand-over
// of round_sync.hpp (rs_finish: coherent partial stores, ticket, the last workgroup totals and publishes to mapped host
// memory) — the one-workgroup reduce kernel that used to follow each of the ~120 round launches of a proof is gone.
struct JgTail { uint32_t* partials; RoundSync rs; uint32_t seq; };
__device__ __forceinline__ void jg_finish(const Ext& a, const Ext& b, const JgTail& t) {
    const Ext acc[2] = {a, b};
    rs_finish<2>(acc, t.partials, blockIdx.x, gridDim.x, t.rs, t.seq);
}
__device__ __forceinline__ void jg_finish8(const Ext (&acc)[8], const JgTail& t) {      // the two-round pass: eight sums
    rs_finish<8>(acc, t.partials, blockIdx.x, gridDim.x, t.rs, t.seq);
}

// ---- round 0: y(0) = sum J[2i] q[2i], H = sum (J[2i] + J[2i+1]) (q[2i] + q[2i+1])   (hadamard.rs:L100-L135)
// J(x) = eq_col[c] * eq_row[row] and a column is a long run of consecutive x, so eq_col[c] is factored out of
// the run: per element only ext x base products (4 multiplies) remain, and the column search is done once per
// thread. A thread owns RUN consecutive dense indices; when its run crosses into another column the partial
// sums are flushed through that column's eq_col. A pair that straddles two columns takes the unfactored formula.
constexpr int JG_ITERS = 16;     // pairs per thread; a workgroup covers 256 * JG_ITERS consecutive pairs
__device__ __forceinline__ Ext jg_row_eq(const JgJ& J, uint32_t row) {
    return Ext{{J.row_eq[row], J.row_eq[J.row_len + row], J.row_eq[2 * J.row_len + row], J.row_eq[3 * J.row_len + row]}};
}
// Lanes take CONSECUTIVE pairs (coalesced 8 B of q and 2 x 4 planes of eq_row per lane) and step by 256 pairs,
// so a lane stays inside one column for many steps and keeps that column's sums un-multiplied.
__global__ __launch_bounds__(256) void jg_round0_sum(JgSegs S, JgJ J, uint32_t n_pairs, JgTail tail) {
    Ext e0 = kb::ext_zero(), eh = kb::ext_zero();
    for (uint32_t chunk = blockIdx.x; (uint64_t)chunk * 256 * JG_ITERS < n_pairs; chunk += gridDim.x) {
        uint32_t c = 0, col_end = 0;
        bool have = false;
        Ext a0 = kb::ext_zero(), ah = kb::ext_zero();     // sums of the current column, without eq_col[c]
#pragma unroll 1
        for (int it = 0; it < JG_ITERS; it++) {
            const uint32_t pair = chunk * 256 * JG_ITERS + it * 256 + threadIdx.x;
            if (pair >= n_pairs) break;
            const uint32_t x = 2 * pair;
            if (!have) { c = jg_find_col(J, x); col_end = J.prefix[c + 1]; have = true; }
            else if (x >= col_end) {                      // entered a later column: flush
                const Ext w = ld_ext(J.col_eq, c);
                e0 = kb::ext_add(e0, kb::ext_mul(w, a0));
                eh = kb::ext_add(eh, kb::ext_mul(w, ah));
                a0 = ah = kb::ext_zero();
                while (J.prefix[c + 1] <= x) c++;
                col_end = J.prefix[c + 1];
            }
            const uint32_t q0 = jg_q(S, x), q1 = jg_q(S, x + 1);
            const uint32_t row = x - J.prefix[c];
            const Ext r0 = jg_row_eq(J, row);
            a0 = kb::ext_add(a0, kb::ext_mul_base(r0, q0));
            if (x + 1 < col_end) {
                ah = kb::ext_add(ah, kb::ext_mul_base(kb::ext_add(r0, jg_row_eq(J, row + 1)), kb::add(q0, q1)));
            } else {                                      // x + 1 opens the next non-empty column (at its row 0)
                uint32_t c1 = c + 1;
                while (J.prefix[c1 + 1] <= x + 1) c1++;
                const Ext j0 = kb::ext_mul(ld_ext(J.col_eq, c), r0), j1 = kb::ext_mul(ld_ext(J.col_eq, c1), jg_row_eq(J, x + 1 - J.prefix[c1]));
                eh = kb::ext_add(eh, kb::ext_mul_base(kb::ext_add(j0, j1), kb::add(q0, q1)));
            }
        }
        if (have) {
            const Ext w = ld_ext(J.col_eq, c);
            e0 = kb::ext_add(e0, kb::ext_mul(w, a0));
            eh = kb::ext_add(eh, kb::ext_mul(w, ah));
        }
    }
    jg_finish(e0, eh, tail);
}

// ---- round 0, table-major form (every table height even, so dense pairs are row pairs (2k, 2k+1) of one column).
// sum_x J(x) q(x) = sum_tables sum_rows eq_row[r] * (sum_c eq_col[c] q[c, r]): a lane owns one row pair of a table
// and walks the table's columns — consecutive lanes read consecutive 8-byte pairs of a column — accumulating
// sum_c eq_col[c] q unreduced (kb::DotAcc, wave-uniform coefficients), and multiplies by eq_row ONCE per row pair.
// The generic kernel above re-reads the 16 B/row eq_row table for every column (6.4 GB at core scale against the
// 1.6 GB of q) and spends an ext x base product plus a table walk per element.
struct JgTab { const uint32_t* q; uint32_t height, col0, ncols, tile0, x0, tile1, tile2; };   // q: the table's first column in the dense buffer; x0: its dense index; tile0/1/2: first tile in the round-0 / one-level / two-level fold launches
constexpr uint32_t JG_TAB_PAIRS = 256;                                       // row pairs per tile
constexpr uint32_t JG_COL_SLICE = 64;                                        // columns per table descriptor (see where the tables are listed)
static_assert(JG_COL_SLICE <= 0x3fffu, "jg_round01_tables accumulates a descriptor's columns in one kb::DotAcc window");
__global__ __launch_bounds__(256) void jg_round0_tables(const JgTab* __restrict__ tabs, uint32_t n_tabs, uint32_t n_tiles,
                                                        JgJ J, JgTail tail) {
    Ext e0 = kb::ext_zero(), eh = kb::ext_zero();
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t lo = 0, hi = n_tabs;                     // last table with tile0 <= tile
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (__builtin_amdgcn_readfirstlane(tabs[mid].tile0) <= tile) lo = mid; else hi = mid;
        }
        const JgTab t = tabs[lo];
        const uint32_t k = (tile - t.tile0) * JG_TAB_PAIRS + threadIdx.x;     // row pair of this lane
        if (2 * k >= t.height) continue;
        kb::DotAcc u0, us;
        kb::dot_init(u0);
        kb::dot_init(us);
        const uint32_t* col = t.q + 2 * (size_t)k;
        for (uint32_t c = 0; c < t.ncols; c++, col += t.height) {
            if ((c & 0x3fffu) == 0x3fffu) {               // 2^14 columns per accumulator window (never in practice)
                const Ext r0 = jg_row_eq(J, 2 * k), r1 = jg_row_eq(J, 2 * k + 1);
                e0 = kb::ext_add(e0, kb::ext_mul(r0, kb::dot_finish(u0)));
                eh = kb::ext_add(eh, kb::ext_mul(kb::ext_add(r0, r1), kb::dot_finish(us)));
                kb::dot_init(u0);
                kb::dot_init(us);
            }
            const uint2 v = *reinterpret_cast<const uint2*>(col);
            const Ext w = ld_ext(J.col_eq, t.col0 + c);   // wave-uniform
            kb::dot_add(u0, w, v.x);
            kb::dot_add(us, w, kb::add(v.x, v.y));
        }
        const Ext r0 = jg_row_eq(J, 2 * k), r1 = jg_row_eq(J, 2 * k + 1);
        e0 = kb::ext_add(e0, kb::ext_mul(r0, kb::dot_finish(u0)));
        eh = kb::ext_add(eh, kb::ext_mul(kb::ext_add(r0, r1), kb::dot_finish(us)));
    }
    jg_finish(e0, eh, tail);
}

// ---- rounds 0 AND 1 from one pass over the base words (table heights % 4 == 0; the look-ahead of the reference's
// /root/reference/sp1-gpu/crates/sys/lib/experimental/look_ahead.cu:L98 on this file's table-major form). A lane owns base
// rows 4k .. 4k+3 of a table — the values of q and J at (X, Y) = (bit 0, bit 1) in {0,1}^2 — and walks the columns once,
// accumulating U_l = sum_c eq_col[c] q[c, 4k + l] unreduced like round 0 does (the same four multiply-adds per element as
// the two accumulators of jg_round0_tables on a row pair). J(x) = eq_col[c] r_l with r_l = eq_row[4k + l], and everything
// the two rounds need is bilinear in (r, U):
//   round 0:  y(0) = sum r_0 U_0 + r_2 U_2,   H = sum (r_0 + r_1)(U_0 + U_1) + (r_2 + r_3)(U_2 + U_3)
//   round 1 (after alpha_0, with r'(Y) = r_0Y + alpha_0 (r_1Y - r_0Y) and U' likewise):
//             y'(0) = sum r'(0) U'(0):  a quadratic in alpha_0 through P0 = r_0 U_0, P1 = r_1 U_1, leading coefficient
//                     (r_1 - r_0)(U_1 - U_0) = 2 (P0 + P1) - (r_0 + r_1)(U_0 + U_1)
//             H'    = sum (r'(0) + r'(1))(U'(0) + U'(1)):  through Q0 = (r_0 + r_2)(U_0 + U_2), Q1 = (r_1 + r_3)(U_1 + U_3),
//                     leading coefficient Qinf = ((r_1 + r_3) - (r_0 + r_2))((U_1 + U_3) - (U_0 + U_2))
// Eight sums: [P0, r_2 U_2, Ha, Hb, P1, Q0, Q1, Qinf] — eight extension products per lane and table, not per element. The
// second pass over the 1.6 GB of base words that round 1 used to be (jg_fold_tables<1, false>, sums only) is gone.
__global__ __launch_bounds__(256) void jg_round01_tables(const JgTab* __restrict__ tabs, uint32_t n_tabs, uint32_t n_tiles,
                                                         JgJ J, JgTail tail) {
    Ext acc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = kb::ext_zero();
    auto flush = [&](const kb::DotAcc (&u)[4], uint32_t k) {
        Ext U[4], r[4];
#pragma unroll
        for (int l = 0; l < 4; l++) { U[l] = kb::dot_finish(u[l]); r[l] = jg_row_eq(J, 4 * k + l); }
        acc[0] = kb::ext_add(acc[0], kb::ext_mul(r[0], U[0]));
        acc[1] = kb::ext_add(acc[1], kb::ext_mul(r[2], U[2]));
        acc[2] = kb::ext_add(acc[2], kb::ext_mul(kb::ext_add(r[0], r[1]), kb::ext_add(U[0], U[1])));
        acc[3] = kb::ext_add(acc[3], kb::ext_mul(kb::ext_add(r[2], r[3]), kb::ext_add(U[2], U[3])));
        acc[4] = kb::ext_add(acc[4], kb::ext_mul(r[1], U[1]));
        const Ext sr0 = kb::ext_add(r[0], r[2]), sr1 = kb::ext_add(r[1], r[3]), sU0 = kb::ext_add(U[0], U[2]), sU1 = kb::ext_add(U[1], U[3]);
        acc[5] = kb::ext_add(acc[5], kb::ext_mul(sr0, sU0));
        acc[6] = kb::ext_add(acc[6], kb::ext_mul(sr1, sU1));
        acc[7] = kb::ext_add(acc[7], kb::ext_mul(kb::ext_sub(sr1, sr0), kb::ext_sub(sU1, sU0)));
    };
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t lo = 0, hi = n_tabs;                     // last table with tile1 <= tile
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (__builtin_amdgcn_readfirstlane(tabs[mid].tile1) <= tile) lo = mid; else hi = mid;
        }
        const JgTab t = tabs[lo];
        const uint32_t k = (tile - t.tile1) * JG_TAB_PAIRS + threadIdx.x;     // row quad of this lane
        if (4 * k >= t.height) continue;
        kb::DotAcc u[4];
#pragma unroll
        for (int l = 0; l < 4; l++) kb::dot_init(u[l]);
        // a descriptor is at most JG_COL_SLICE columns (<= 2^16 terms per accumulator); four columns per step, the four 16-byte
        // loads of a step issued before its first multiply-add
        const uint32_t* col = t.q + 4 * (size_t)k;
        auto add = [&](uint32_t c, const uint4& v) {
            const Ext w = ld_ext(J.col_eq, t.col0 + c);   // wave-uniform
            kb::dot_add(u[0], w, v.x);
            kb::dot_add(u[1], w, v.y);
            kb::dot_add(u[2], w, v.z);
            kb::dot_add(u[3], w, v.w);
        };
        uint32_t c = 0;
        for (; c + 4 <= t.ncols; c += 4, col += 4 * (size_t)t.height) {
            uint4 v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = *reinterpret_cast<const uint4*>(col + i * (size_t)t.height);
#pragma unroll
            for (int i = 0; i < 4; i++) add(c + i, v[i]);
        }
        for (; c < t.ncols; c++, col += t.height) add(c, *reinterpret_cast<const uint4*>(col));
        flush(u, k);
    }
    jg_finish8(acc, tail);
}

__device__ __forceinline__ Ext fold_ext(const Ext& a, const Ext& b, const Ext& alpha) {   // a + alpha (b - a)
    return kb::ext_add(a, kb::ext_mul(kb::ext_sub(b, a), alpha));      // alpha: wave-uniform, second
}

// ---- first fold(s), table-major form (J stays factored). LEVELS = 1 (heights % 4 == 0): a lane owns the level-1 row
// pair (2k, 2k+1) of a table = base rows 4k .. 4k+3 of every column; q1 = lerp of the base pairs with alpha0.
// LEVELS = 2 (heights % 8 == 0): the level-2 row pair = base rows 8k .. 8k+7; level 1 is recomputed in registers and
// folded again with alpha1, so the level-1 table (16 B per entry written, then read) never exists: round 1 runs
// with STORE = false (sums only, 4 B/element read), round 2 reads the base words again and writes level 2.
// The next round's sums use sum_c eq_col[c] q[c, r] accumulated unreduced (kb::edot_add with the (eq_col, 3 eq_col)
// pairs), times the level's eq_row once per row.
template <int LEVELS, bool STORE>
__global__ __launch_bounds__(256) void jg_fold_tables(const JgTab* __restrict__ tabs, uint32_t n_tabs, uint32_t n_tiles, JgJ Jl,
                                                      const Ext* __restrict__ col_eq3, Ext alpha0, Ext alpha1, Ext* __restrict__ q_out,
                                                      JgTail tail) {
    constexpr uint32_t SPAN = 2u << LEVELS;               // base rows per lane and column
    Ext e0 = kb::ext_zero(), eh = kb::ext_zero();
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        uint32_t lo = 0, hi = n_tabs;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            const uint32_t t0 = __builtin_amdgcn_readfirstlane(LEVELS == 1 ? tabs[mid].tile1 : tabs[mid].tile2);
            if (t0 <= tile) lo = mid; else hi = mid;
        }
        const JgTab t = tabs[lo];
        const uint32_t k = (tile - (LEVELS == 1 ? t.tile1 : t.tile2)) * JG_TAB_PAIRS + threadIdx.x;   // row pair of this lane
        if (SPAN * k >= t.height) continue;
        kb::DotAcc u0, us;
        kb::dot_init(u0);
        kb::dot_init(us);
        const uint32_t* col = t.q + SPAN * (size_t)k;
        const uint32_t hl = t.height >> LEVELS;
        Ext* out = q_out + (t.x0 >> LEVELS) + 2 * (size_t)k;
        for (uint32_t c = 0; c < t.ncols; c++, col += t.height, out += hl) {
            if ((c & 0xfffu) == 0xfffu) {                 // 2^12 columns per accumulator window (never in practice)
                const Ext r0 = jg_row_eq(Jl, 2 * k), r1 = jg_row_eq(Jl, 2 * k + 1);
                e0 = kb::ext_add(e0, kb::ext_mul(r0, kb::dot_finish(u0)));
                eh = kb::ext_add(eh, kb::ext_mul(kb::ext_add(r0, r1), kb::dot_finish(us)));
                kb::dot_init(u0);
                kb::dot_init(us);
            }
            Ext qa, qb;
            const uint4 v = *reinterpret_cast<const uint4*>(col);
            const Ext l0 = kb::ext_add(kb::ext_from_base(v.x), kb::ext_mul_base(alpha0, kb::sub(v.y, v.x)));
            const Ext l1 = kb::ext_add(kb::ext_from_base(v.z), kb::ext_mul_base(alpha0, kb::sub(v.w, v.z)));
            if (LEVELS == 1) { qa = l0; qb = l1; }
            else {
                const uint4 v2 = *reinterpret_cast<const uint4*>(col + 4);
                const Ext l2 = kb::ext_add(kb::ext_from_base(v2.x), kb::ext_mul_base(alpha0, kb::sub(v2.y, v2.x)));
                const Ext l3 = kb::ext_add(kb::ext_from_base(v2.z), kb::ext_mul_base(alpha0, kb::sub(v2.w, v2.z)));
                qa = kb::ext_add(l0, kb::ext_mul(kb::ext_sub(l1, l0), alpha1));
                qb = kb::ext_add(l2, kb::ext_mul(kb::ext_sub(l3, l2), alpha1));
            }
            if (STORE) { st_ext(out, 0, qa); st_ext(out, 1, qb); }
            const Ext w = ld_ext(Jl.col_eq, t.col0 + c), w3 = ld_ext(col_eq3, t.col0 + c);     // wave-uniform
            kb::edot_add(u0, w, w3, qa);
            kb::edot_add(us, w, w3, kb::ext_add(qa, qb));
        }
        const Ext r0 = jg_row_eq(Jl, 2 * k), r1 = jg_row_eq(Jl, 2 * k + 1);
        e0 = kb::ext_add(e0, kb::ext_mul(r0, kb::dot_finish(u0)));
        eh = kb::ext_add(eh, kb::ext_mul(kb::ext_add(r0, r1), kb::dot_finish(us)));
    }
    jg_finish(e0, eh, tail);
}

// ---- first fold (base q, recomputed J) fused with the next round's sums. One step of a thread: inputs 4k..4k+3,
// outputs 2k, 2k+1 of the round-1 tables (n_out entries). Lanes take consecutive k (16 B of q per lane) and step by
// 256, tracking their column like jg_round0_sum; inside one column J folds as eq_col[c] * lerp(eq_row[r], eq_row[r+1]).
// Always writes the j table: when the next level keeps J factored the first fold is table-major (jg_fold_tables), never this one.
__global__ __launch_bounds__(256) void jg_fold0_sum(JgSegs S, JgJ J, Ext alpha, uint32_t n_out, Ext* __restrict__ q_out,
                                                    Ext* __restrict__ j_out, JgTail tail) {
    Ext e0 = kb::ext_zero(), eh = kb::ext_zero();
    const uint32_t n_thr = (n_out + 1) / 2;
    for (uint32_t chunk = blockIdx.x; (uint64_t)chunk * 256 * JG_ITERS < n_thr; chunk += gridDim.x) {
        uint32_t c = 0, col_end = 0;
        bool have = false;
#pragma unroll 1
        for (int it = 0; it < JG_ITERS; it++) {
            const uint32_t k = chunk * 256 * JG_ITERS + it * 256 + threadIdx.x;
            if (k >= n_thr) break;
            const uint32_t x0 = 4 * k;
            Ext qo[2], jo[2];
            if (x0 + 3 < S.total) {
                if (!have) { c = jg_find_col(J, x0); col_end = J.prefix[c + 1]; have = true; }
                else if (x0 >= col_end) { while (J.prefix[c + 1] <= x0) c++; col_end = J.prefix[c + 1]; }
            }
            if (x0 + 3 < S.total && x0 + 3 < col_end) {       // all four inputs in column c
                const uint32_t row = x0 - J.prefix[c];
                const Ext w = ld_ext(J.col_eq, c);
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const uint32_t qa = jg_q(S, x0 + 2 * h), qb = jg_q(S, x0 + 2 * h + 1);
                    qo[h] = kb::ext_add(kb::ext_from_base(qa), kb::ext_mul_base(alpha, kb::sub(qb, qa)));
                    const Ext ra = jg_row_eq(J, row + 2 * h), rb = jg_row_eq(J, row + 2 * h + 1);
                    jo[h] = kb::ext_mul(w, kb::ext_add(ra, kb::ext_mul(kb::ext_sub(rb, ra), alpha)));
                }
            } else {                                          // column boundary or the zero tail: element by element
                uint32_t q[4];
                Ext j[4];
                jg_load_base<4>(S, J, x0, q, j);
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    qo[h] = kb::ext_add(kb::ext_from_base(q[2 * h]), kb::ext_mul_base(alpha, kb::sub(q[2 * h + 1], q[2 * h])));
                    jo[h] = fold_ext(j[2 * h], j[2 * h + 1], alpha);
                }
                have = false;                                 // re-search next time (cheap: boundaries are rare)
            }
#pragma unroll
            for (int h = 0; h < 2; h++)
                if (2 * k + h < n_out) { st_ext(q_out, 2 * k + h, qo[h]); st_ext(j_out, 2 * k + h, jo[h]); }
            e0 = kb::ext_add(e0, kb::ext_mul(jo[0], qo[0]));
            eh = kb::ext_add(eh, kb::ext_mul(kb::ext_add(jo[0], jo[1]), kb::ext_add(qo[0], qo[1])));
        }
    }
    jg_finish(e0, eh, tail);
}

// ---- folds that keep J factored. While every column starts at a multiple of 2^r in the dense order (chip heights
// are multiples of 32 in the reference's shards, powers of two in the synthetic ones), folding the r lowest dense
// variables never mixes two columns, so J_r(x) = eq_col[c] * eq_row_r[x - (prefix[c] >> r)] with eq_row_r the row
// table folded r times (a 2^(L-r)-entry table that lives in L2 / MALL). The j tables of these levels — 32 B/entry
// written and read back, 12 GB over levels 1..5 at core scale — are never materialised: a fold reads q_{r-1}, writes
// q_r and sums against the factored J_r, with eq_col[c] pulled out of each column run as in round 0.
__global__ __launch_bounds__(256) void jg_fold_row_eq(const uint32_t* __restrict__ in, uint32_t len_in, Ext alpha,
                                                      uint32_t* __restrict__ out) {
    const uint32_t len_out = len_in >> 1;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= len_out) return;
    const Ext a{{in[2 * i], in[len_in + 2 * i], in[2 * len_in + 2 * i], in[3 * len_in + 2 * i]}};
    const Ext b{{in[2 * i + 1], in[len_in + 2 * i + 1], in[2 * len_in + 2 * i + 1], in[3 * len_in + 2 * i + 1]}};
    const Ext r = fold_ext(a, b, alpha);
#pragma unroll
    for (int k = 0; k < 4; k++) out[(size_t)k * len_out + i] = r.c[k];
}

// q_in: level r-1 (n_in live entries); J: level r (prefix >> r, eq_row_r); writes q_out = level r (n_out entries)
__global__ __launch_bounds__(256) void jg_foldf_sum(const Ext* __restrict__ q_in, uint32_t n_in, JgJ J, Ext alpha, uint32_t n_out,
                                                    Ext* __restrict__ q_out, JgTail tail) {
    Ext e0 = kb::ext_zero(), eh = kb::ext_zero();
    const uint32_t n_pairs = (n_out + 1) / 2;
    for (uint32_t chunk = blockIdx.x; (uint64_t)chunk * 256 * JG_ITERS < n_pairs; chunk += gridDim.x) {
        uint32_t c = 0, col_end = 0;
        bool have = false;
        Ext a0 = kb::ext_zero(), ah = kb::ext_zero();     // sums of the current column, without eq_col[c]
#pragma unroll 1
        for (int it = 0; it < JG_ITERS; it++) {
            const uint32_t pair = chunk * 256 * JG_ITERS + it * 256 + threadIdx.x;
            if (pair >= n_pairs) break;
            const uint32_t x = 2 * pair;                  // level-r index of the first output
            Ext q[4];
#pragma unroll
            for (int v = 0; v < 4; v++) q[v] = 2 * x + v < n_in ? ld_ext(q_in, 2 * x + v) : kb::ext_zero();
            const Ext q0 = fold_ext(q[0], q[1], alpha), q1 = fold_ext(q[2], q[3], alpha);
            st_ext(q_out, x, q0);
            if (x + 1 < n_out) st_ext(q_out, x + 1, q1);
            if (!have) { c = jg_find_col(J, x); col_end = J.prefix[c + 1]; have = true; }
            else if (x >= col_end) {                      // entered a later column: flush
                const Ext w = ld_ext(J.col_eq, c);
                e0 = kb::ext_add(e0, kb::ext_mul(w, a0));
                eh = kb::ext_add(eh, kb::ext_mul(w, ah));
                a0 = ah = kb::ext_zero();
                while (J.prefix[c + 1] <= x) c++;
                col_end = J.prefix[c + 1];
            }
            const Ext r0 = jg_row_eq(J, x - J.prefix[c]);
            a0 = kb::ext_add(a0, kb::ext_mul(r0, q0));
            if (x + 1 < col_end) {
                ah = kb::ext_add(ah, kb::ext_mul(kb::ext_add(r0, jg_row_eq(J, x + 1 - J.prefix[c])), kb::ext_add(q0, q1)));
            } else {
                Ext jsum = kb::ext_mul(ld_ext(J.col_eq, c), r0);
                if (x + 1 < n_out) {                      // x + 1 opens a later non-empty column
                    uint32_t c1 = c + 1;
                    while (J.prefix[c1 + 1] <= x + 1) c1++;
                    jsum = kb::ext_add(jsum, kb::ext_mul(ld_ext(J.col_eq, c1), jg_row_eq(J, x + 1 - J.prefix[c1])));
                }
                eh = kb::ext_add(eh, kb::ext_mul(jsum, kb::ext_add(q0, q1)));
            }
        }
        if (have) {
            const Ext w = ld_ext(J.col_eq, c);
            e0 = kb::ext_add(e0, kb::ext_mul(w, a0));
            eh = kb::ext_add(eh, kb::ext_mul(w, ah));
        }
    }
    jg_finish(e0, eh, tail);
}

// ---- later folds: ext tables with n_in live entries -> n_out = ceil(n_in / 2), fused with the sums
__global__ __launch_bounds__(256) void jg_fold_sum(const Ext* __restrict__ q_in, const Ext* __restrict__ j_in, uint32_t n_in,
                                                   Ext alpha, uint32_t n_out, Ext* __restrict__ q_out, Ext* __restrict__ j_out,
                                                   JgTail tail) {
    Ext e0 = kb::ext_zero(), eh = kb::ext_zero();
    const uint32_t n_thr = (n_out + 1) / 2;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n_thr; k += gridDim.x * blockDim.x) {
        Ext q[4], j[4];
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const uint32_t x = 4 * k + v;
            q[v] = x < n_in ? ld_ext(q_in, x) : kb::ext_zero();
            j[v] = x < n_in ? ld_ext(j_in, x) : kb::ext_zero();
        }
        Ext qo[2], jo[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            qo[h] = fold_ext(q[2 * h], q[2 * h + 1], alpha);
            jo[h] = fold_ext(j[2 * h], j[2 * h + 1], alpha);
            if (2 * k + h < n_out) { st_ext(q_out, 2 * k + h, qo[h]); st_ext(j_out, 2 * k + h, jo[h]); }
        }
        e0 = kb::ext_add(e0, kb::ext_mul(jo[0], qo[0]));
        eh = kb::ext_add(eh, kb::ext_mul(kb::ext_add(jo[0], jo[1]), kb::ext_add(qo[0], qo[1])));
    }
    jg_finish(e0, eh, tail);
}

// The same fold with J still FACTORED on the way in (the first round after the factored levels): a lane computes the j of its
// four entries from eq_col x eq_row (one column search, then a walk) instead of reading a table that a launch of its own would
// have had to write at full size first — 16 B written and 16 B read per entry of the largest generic level saved.
__global__ __launch_bounds__(256) void jg_fold_sum_fj(const Ext* __restrict__ q_in, JgJ J, uint32_t n_in, Ext alpha, uint32_t n_out,
                                                      Ext* __restrict__ q_out, Ext* __restrict__ j_out, JgTail tail) {
    Ext e0 = kb::ext_zero(), eh = kb::ext_zero();
    const uint32_t n_thr = (n_out + 1) / 2;
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n_thr; k += gridDim.x * blockDim.x) {
        Ext q[4], j[4];
        uint32_t c = 0;
        bool have = false;
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const uint32_t x = 4 * k + v;
            if (x >= n_in) { q[v] = kb::ext_zero(); j[v] = kb::ext_zero(); continue; }
            q[v] = ld_ext(q_in, x);
            if (!have) { c = jg_find_col(J, x); have = true; }
            else while (J.prefix[c + 1] <= x) c++;
            j[v] = jg_j_at(J, c, x - J.prefix[c]);
        }
        Ext qo[2], jo[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            qo[h] = fold_ext(q[2 * h], q[2 * h + 1], alpha);
            jo[h] = fold_ext(j[2 * h], j[2 * h + 1], alpha);
            if (2 * k + h < n_out) { st_ext(q_out, 2 * k + h, qo[h]); st_ext(j_out, 2 * k + h, jo[h]); }
        }
        e0 = kb::ext_add(e0, kb::ext_mul(jo[0], qo[0]));
        eh = kb::ext_add(eh, kb::ext_mul(kb::ext_add(jo[0], jo[1]), kb::ext_add(qo[0], qo[1])));
    }
    jg_finish(e0, eh, tail);
}

// ================================================================ jagged-eval sumcheck
// Transfer matrices of the branching program. A layer reads (row bit, index bit, curr-prefix bit,
// next-prefix bit); with the first two bound to z_row / z_trace values the layer acts on the 4 memory
// states as a 4x4 matrix that is multilinear in (curr, next): mats[layer][2 cb + nb][m][m'].
struct JeCols {                     // condensed columns (runs of equal (t_c, t_{c+1}) merged)
    const uint32_t* t;              // t_c
    const uint32_t* u;              // t_{c+1}
    const Ext* zcol;                // summed eq(z_col, c) of the run
    uint32_t n;
};

__device__ __forceinline__ void matvec(const Ext* __restrict__ A, const Ext (&s)[4], Ext (&out)[4]) {   // out = A s
#pragma unroll
    for (int m = 0; m < 4; m++) {
        Ext acc = kb::ext_mul(ld_ext(A, 4 * m), s[0]);
#pragma unroll
        for (int k = 1; k < 4; k++) acc = kb::ext_add(acc, kb::ext_mul(ld_ext(A, 4 * m + k), s[k]));
        out[m] = acc;
    }
}
__device__ __forceinline__ void vecmat(const Ext (&w)[4], const Ext* __restrict__ A, Ext (&out)[4]) {   // out = w^T A
#pragma unroll
    for (int k = 0; k < 4; k++) {
        Ext acc = kb::ext_mul(w[0], ld_ext(A, k));
#pragma unroll
        for (int m = 1; m < 4; m++) acc = kb::ext_add(acc, kb::ext_mul(w[m], ld_ext(A, 4 * m + k)));
        out[k] = acc;
    }
}
__device__ __forceinline__ Ext dot4(const Ext (&a)[4], const Ext (&b)[4]) {
    Ext acc = kb::ext_mul(a[0], b[0]);
#pragma unroll
    for (int k = 1; k < 4; k++) acc = kb::ext_add(acc, kb::ext_mul(a[k], b[k]));
    return acc;
}

// suffix[layer][k] = prod_{l >= layer} M_l(column k) e_success, for layer = D-1 .. 0.
// PAIR = true: matrices indexed by (t bit, u bit) (mats has 4 per layer); false: by the t bit only (2 per layer).
// Also accumulates sum_k zcol[k] * suffix[0][k][initial state] into out8[0..3] (full J evaluation).
template <bool PAIR>
__global__ __launch_bounds__(256) void je_suffix_kernel(JeCols C, const Ext* __restrict__ mats, int D, Ext* __restrict__ suffix,
                                                        JgTail tail) {
    Ext total = kb::ext_zero();
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < C.n; k += gridDim.x * blockDim.x) {
        const uint32_t t = C.t[k], u = C.u[k];
        Ext s[4] = {kb::ext_zero(), kb::ext_zero(), kb::ext_one(), kb::ext_zero()};   // success = {carry 0, comparison 1}
        for (int layer = D - 1; layer >= 0; layer--) {
            const uint32_t cb = (t >> layer) & 1u, nb = (u >> layer) & 1u;
            const Ext* A = PAIR ? mats + ((size_t)layer * 4 + cb * 2 + nb) * 16 : mats + ((size_t)layer * 2 + cb) * 16;
            Ext o[4];
            matvec(A, s, o);
#pragma unroll
            for (int m = 0; m < 4; m++) { s[m] = o[m]; st_ext(suffix, ((uint32_t)layer * C.n + k) * 4 + m, o[m]); }
        }
        total = kb::ext_add(total, kb::ext_mul(ld_ext(C.zcol, k), s[0]));
    }
    jg_finish(total, kb::ext_zero(), tail);
}

// One round of the first half (variable = bit r of t_{c+1}). state[k] = {v0[4], v1[4]} of the previous
// round, inter[k] = eq accumulator. first: r == 0.
__global__ __launch_bounds__(256) void je_phase1_round(JeCols C, const Ext* __restrict__ mats, const Ext* __restrict__ suffix, int D,
                                                       int r, Ext alpha_prev, Ext half, Ext* __restrict__ state,
                                                       Ext* __restrict__ inter, JgTail tail) {
    Ext y0 = kb::ext_zero(), yh = kb::ext_zero();
    const Ext one = kb::ext_one();
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < C.n; k += gridDim.x * blockDim.x) {
        const uint32_t t = C.t[k], u = C.u[k];
        Ext w[4], it;
        if (r == 0) {
            w[0] = one; w[1] = w[2] = w[3] = kb::ext_zero();     // initial state = {carry 0, comparison 0}
            it = one;
        } else {
#pragma unroll
            for (int m = 0; m < 4; m++) w[m] = fold_ext(ld_ext(state, 8 * k + m), ld_ext(state, 8 * k + 4 + m), alpha_prev);
            const bool x = (u >> (r - 1)) & 1u;
            it = kb::ext_mul(ld_ext(inter, k), x ? alpha_prev : kb::ext_sub(one, alpha_prev));
        }
        st_ext(inter, k, it);
        const uint32_t cb = (t >> r) & 1u;
        Ext v0[4], v1[4], s[4];
        vecmat(w, mats + ((size_t)r * 4 + cb * 2 + 0) * 16, v0);
        vecmat(w, mats + ((size_t)r * 4 + cb * 2 + 1) * 16, v1);
#pragma unroll
        for (int m = 0; m < 4; m++) { st_ext(state, 8 * k + m, v0[m]); st_ext(state, 8 * k + 4 + m, v1[m]); }
        if (r + 1 < D)
#pragma unroll
            for (int m = 0; m < 4; m++) s[m] = ld_ext(suffix, ((uint32_t)(r + 1) * C.n + k) * 4 + m);
        else { s[0] = s[1] = s[3] = kb::ext_zero(); s[2] = one; }
        const Ext bp0 = dot4(v0, s), bp1 = dot4(v1, s);
        const Ext f = kb::ext_mul(ld_ext(C.zcol, k), it);
        if (!((u >> r) & 1u)) y0 = kb::ext_add(y0, kb::ext_mul(f, bp0));
        yh = kb::ext_add(yh, kb::ext_mul(kb::ext_mul(f, half), kb::ext_mul(kb::ext_add(bp0, bp1), half)));
    }
    jg_finish(y0, yh, tail);
}

// One round of the second half (variable = bit rp of t_c; every bit of t_{c+1} is bound). V0 / V1: the
// column-independent bound part times the two lambda-endpoint matrices (host). prev_bit_of_u: the
// previously bound variable was bit D-1 of u (rp == 0) or bit rp-1 of t.
struct JeV { Ext v[8]; };          // the two prefix row vectors of a phase-2 round, passed by value (128 B of kernarg)
__global__ __launch_bounds__(256) void je_phase2_round(JeCols C, const Ext* __restrict__ suffix2, int D, int rp, Ext alpha_prev,
                                                       Ext half, JeV V, Ext* __restrict__ inter,
                                                       JgTail tail) {
    Ext y0 = kb::ext_zero(), yh = kb::ext_zero();
    const Ext one = kb::ext_one();
    Ext v0[4], v1[4];
#pragma unroll
    for (int m = 0; m < 4; m++) { v0[m] = V.v[m]; v1[m] = V.v[4 + m]; }
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < C.n; k += gridDim.x * blockDim.x) {
        const uint32_t t = C.t[k], u = C.u[k];
        const bool x = rp == 0 ? ((u >> (D - 1)) & 1u) : ((t >> (rp - 1)) & 1u);
        const Ext it = kb::ext_mul(ld_ext(inter, k), x ? alpha_prev : kb::ext_sub(one, alpha_prev));
        st_ext(inter, k, it);
        Ext s[4];
        if (rp + 1 < D)
#pragma unroll
            for (int m = 0; m < 4; m++) s[m] = ld_ext(suffix2, ((uint32_t)(rp + 1) * C.n + k) * 4 + m);
        else { s[0] = s[1] = s[3] = kb::ext_zero(); s[2] = one; }
        const Ext bp0 = dot4(v0, s), bp1 = dot4(v1, s);
        const Ext f = kb::ext_mul(ld_ext(C.zcol, k), it);
        if (!((t >> rp) & 1u)) y0 = kb::ext_add(y0, kb::ext_mul(f, bp0));
        yh = kb::ext_add(yh, kb::ext_mul(kb::ext_mul(f, half), kb::ext_mul(kb::ext_add(bp0, bp1), half)));
    }
    jg_finish(y0, yh, tail);
}

}  // namespace sp1hip
