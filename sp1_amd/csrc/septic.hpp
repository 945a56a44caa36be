// sp1_amd/csrc/septic.hpp — the septic extension F_p^7 = F_p[z] / (z^7 - 3 z - 5) over KoalaBear, the curve
// y^2 = x^3 + 45 x + 41 z^3 over it, and the row of the RISC-V Global chip that lifts a Poseidon2 digest onto that curve
// (hypercube/src/septic_{extension,curve,digest}.rs, operations/global_interaction.rs:L33-L103, global/mod.rs:L131-L260).
//
// Everything is KB_HD: tracegen_global.hip's kernels call it on the device, tests/native/septic_ops.hip calls the same code on
// the host (tests/test_septic_arith.py, tests/test_tracegen_global_host.py check it against Python integers). Words are
// Montgomery words throughout. Square roots take the norm route (n^((r+1)/2) / sqrt_p(N(n)), r = 1 + p + ... + p^6), with the
// Frobenius maps from a table computed on the host (make_frob_tables) and Tonelli-Shanks in F_p.
#pragma once

#include "kb31.hpp"
#include "poseidon2.hpp"

namespace sp1hip {
namespace septic {

struct S7 { uint32_t c[7]; };                       // an element of F_p^7, Montgomery words

KB_HD S7 s7_zero() { S7 r; for (int i = 0; i < 7; i++) r.c[i] = 0; return r; }
KB_HD S7 s7_add(const S7& a, const S7& b) { S7 r; for (int i = 0; i < 7; i++) r.c[i] = kb::add(a.c[i], b.c[i]); return r; }
KB_HD S7 s7_sub(const S7& a, const S7& b) { S7 r; for (int i = 0; i < 7; i++) r.c[i] = kb::sub(a.c[i], b.c[i]); return r; }
KB_HD S7 s7_neg(const S7& a) { S7 r; for (int i = 0; i < 7; i++) r.c[i] = kb::neg(a.c[i]); return r; }
KB_HD S7 s7_scale(const S7& a, uint32_t k) { S7 r; for (int i = 0; i < 7; i++) r.c[i] = kb::mul(a.c[i], k); return r; }
// a b mod z^7 - 3 z - 5 (septic_extension.rs:L307-L325)
KB_HD S7 s7_mul(const S7& a, const S7& b) {
    uint32_t t[13];
    for (int s = 0; s < 13; s++) t[s] = 0;
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) t[i + j] = kb::add(t[i + j], kb::mul(a.c[i], b.c[j]));
    const uint32_t c5 = kb::to_monty(5), c3 = kb::to_monty(3);
    S7 r;
    for (int i = 0; i < 7; i++) r.c[i] = t[i];
    for (int s = 7; s < 13; s++) {
        r.c[s - 7] = kb::add(r.c[s - 7], kb::mul(t[s], c5));
        r.c[s - 6] = kb::add(r.c[s - 6], kb::mul(t[s], c3));
    }
    return r;
}
KB_HD uint32_t fp_pow(uint32_t x, uint32_t e) {
    uint32_t r = kb::R1;
    for (; e; e >>= 1) { if (e & 1) r = kb::mul(r, x); x = kb::mul(x, x); }
    return r;
}
KB_HD uint32_t fp_inv(uint32_t x) { return fp_pow(x, kb::P - 2); }

// frob[k - 1][i] = (z^i)^(p^k), k = 1..6 (computed on the host: z^p by square-and-multiply)
struct FrobTables { S7 f[6][7]; };
KB_HD S7 s7_frob(const FrobTables& ft, const S7& a, int k) {
    S7 r = s7_zero();
    for (int i = 0; i < 7; i++)
        for (int j = 0; j < 7; j++) r.c[j] = kb::add(r.c[j], kb::mul(a.c[i], ft.f[k - 1][i].c[j]));
    return r;
}
// (a^(r - 1), N(a)) with r = 1 + p + ... + p^6
KB_HD void s7_norm_parts(const FrobTables& ft, const S7& a, S7* t_out, uint32_t* n_out) {
    S7 t = s7_mul(s7_frob(ft, a, 1), s7_frob(ft, a, 2));            // a^(p + p^2)
    t = s7_mul(s7_mul(t, s7_frob(ft, t, 2)), s7_frob(ft, t, 4));     // ^(1 + p^2 + p^4)
    *t_out = t;
    *n_out = s7_mul(t, a).c[0];
}
KB_HD S7 s7_inv(const FrobTables& ft, const S7& a) {
    S7 t; uint32_t n;
    s7_norm_parts(ft, a, &t, &n);
    return s7_scale(t, fp_inv(n));
}
// Tonelli-Shanks in F_p, p - 1 = 2^24 127 (a root for quadratic residues)
KB_HD uint32_t fp_sqrt(uint32_t a) {
    const int S = 24;
    const uint32_t Q = 127;
    uint32_t c = fp_pow(kb::to_monty(3), Q), t = fp_pow(a, Q), r = fp_pow(a, (Q + 1) / 2);
    for (int i = 1; i < S; i++) {
        uint32_t b = t;
        for (int k = 0; k < S - 1 - i; k++) b = kb::mul(b, b);
        const bool m = b != kb::R1;
        if (m) r = kb::mul(r, c);
        c = kb::mul(c, c);
        if (m) t = kb::mul(t, c);
    }
    return r;
}
// a square root of n if it has one (ok): n^((r + 1) / 2) / sqrt_p(N(n)), (r + 1) / 2 = 1 + p ((p + 1) / 2) (1 + p^2 + p^4)
KB_HD bool s7_sqrt(const FrobTables& ft, const S7& n, S7* root) {
    S7 t; uint32_t nn;
    s7_norm_parts(ft, n, &t, &nn);
    if (fp_pow(nn, (kb::P - 1) / 2) != kb::R1) return false;
    S7 w = n, sq = n;
    for (int i = 1; i < 30; i++) {                                    // w = n^((p + 1) / 2) = n^(1 + 2^23 + ... + 2^29)
        sq = s7_mul(sq, sq);
        if (i >= 23) w = s7_mul(w, sq);
    }
    const S7 cand = s7_mul(s7_mul(s7_mul(s7_frob(ft, w, 1), s7_frob(ft, w, 3)), s7_frob(ft, w, 5)), n);
    *root = s7_scale(cand, fp_inv(fp_sqrt(nn)));
    return true;
}
KB_HD S7 s7_curve_rhs(const S7& x) {                                  // x^3 + 45 x + 41 z^3 (septic_curve.rs:L101-L113)
    S7 r = s7_add(s7_mul(s7_mul(x, x), x), s7_scale(x, kb::to_monty(45)));
    r.c[3] = kb::add(r.c[3], kb::to_monty(41));
    return r;
}
struct Pt { S7 x, y; };
KB_HD Pt ec_add(const FrobTables& ft, const Pt& p1, const Pt& p2) {  // add_incomplete (septic_curve.rs:L58-L63)
    const S7 slope = s7_mul(s7_sub(p2.y, p1.y), s7_inv(ft, s7_sub(p2.x, p1.x)));
    Pt r;
    r.x = s7_sub(s7_sub(s7_mul(slope, slope), p1.x), p2.x);
    r.y = s7_sub(s7_mul(slope, s7_sub(p1.x, r.x)), p1.y);
    return r;
}

// z^p, then row i of the k-th Frobenius power = (z^i)^(p^k): the linear map composed k times
inline FrobTables make_frob_tables() {
    FrobTables ft;
    S7 z = s7_zero(), zp = s7_zero();
    z.c[1] = kb::R1;
    zp.c[0] = kb::R1;
    {
        S7 b = z;
        for (uint32_t e = kb::P; e; e >>= 1) { if (e & 1) zp = s7_mul(zp, b); b = s7_mul(b, b); }
    }
    S7 pw = s7_zero();
    pw.c[0] = kb::R1;
    for (int i = 0; i < 7; i++) { ft.f[0][i] = pw; pw = s7_mul(pw, zp); }
    for (int k = 1; k < 6; k++)
        for (int i = 0; i < 7; i++) {                              // frob^(k+1)(z^i) = frob(frob^k(z^i)): apply the k = 1 map to the previous row
            S7 r = s7_zero();
            for (int a = 0; a < 7; a++)
                for (int j = 0; j < 7; j++) r.c[j] = kb::add(r.c[j], kb::mul(ft.f[k - 1][i].c[a], ft.f[0][a].c[j]));
            ft.f[k][i] = r;
        }
    return ft;
}

// column offsets of the Global chip (riscv.py::global_chip)
constexpr int G_MESSAGE = 0, G_KIND = 8, G_M0_16 = 9, G_M0_8 = 10, G_X = 11, G_Y = 18, G_PERM = 25, G_OFFSET = 204, G_Y6 = 205,
              G_IS_REAL = 209, G_IS_RECV = 210, G_IS_SEND = 211, G_INDEX = 212, G_INIT_X = 213, G_INIT_Y = 220, G_CUM_X = 227,
              G_CUM_Y = 234, G_WIDTH = 241;
constexpr int G_EVENT_WORDS = 9;                                      // message[8], is_receive | kind << 8
constexpr uint32_t Y6_LIMIT = 63u << 24;
// CURVE_CUMULATIVE_SUM_START / CURVE_WITNESS_DUMMY_POINT (hypercube/src/septic_curve.rs:L170-L196), canonical
constexpr uint32_t START_X[7] = {21053971, 90322736, 156256384, 23627556, 34171264, 126183783, 25645942};
constexpr uint32_t START_Y[7] = {2020310104, 1513506566, 1843922297, 2003644209, 805967281, 1882435203, 1623804682};
constexpr uint32_t DUMMY_X[7] = {57770625, 136856976, 72496438, 2651249, 55731748, 158816036, 118044313};
constexpr uint32_t DUMMY_Y[7] = {1250555984, 1592495468, 656721246, 420301347, 2125819749, 819876460, 17687681};

inline Pt monty_point(const uint32_t (&x)[7], const uint32_t (&y)[7]) {
    Pt p;
    for (int i = 0; i < 7; i++) { p.x.c[i] = kb::to_monty(x[i]); p.y.c[i] = kb::to_monty(y[i]); }
    return p;
}
inline Pt global_start_point() { return monty_point(START_X, START_Y); }
inline Pt global_dummy_point() { return monty_point(DUMMY_X, DUMMY_Y); }

// Which of +-root the row carries, and the value its four y6 bytes decompose. A receive takes the root whose last coordinate
// lies in [1, 63 2^24], a send its negative (last coordinate in [p - 63 2^24, p - 1]); the value is y6 - 1 for a receive and
// p - y6 - 1 for a send, so it is below 63 2^24 either way. False — the exception — when neither root's last coordinate is in range.
KB_HD bool global_pick_root(const S7& root, bool is_recv, S7* y_out, uint32_t* range_check_value) {
    const uint32_t y6 = kb::from_monty(root.c[6]);
    const uint32_t neg6 = y6 ? kb::P - y6 : 0u;
    const bool pos_ok = y6 >= 1 && y6 <= Y6_LIMIT, neg_ok = neg6 >= 1 && neg6 <= Y6_LIMIT;
    if (!pos_ok && !neg_ok) return false;
    S7 y = pos_ok ? root : s7_neg(root);                          // the "receive" root
    if (!is_recv) y = s7_neg(y);                                  // a send carries the negated point
    const uint32_t yc6 = kb::from_monty(y.c[6]);
    *range_check_value = is_recv ? yc6 - 1 : kb::P - yc6 - 1;
    *y_out = y;
    return true;
}

// `populate_perm` into the 179 permutation columns (operations/poseidon2/trace.rs:L29-L152; the same walk as tracegen.hip's
// Poseidon2Wide kernel) through put(column, word), columns counted from 0; returns the output state in s
template <class Put>
__host__ __device__ void perm_rows(uint32_t (&s)[16], const p2::RoundConstants* rc, Put put_col, bool store) {
    auto put = [&](int col, uint32_t v) { if (store) put_col(col, v); };
    int col = 0;
#pragma unroll 1
    for (int round = 0; round < 8; round++) {
        for (int i = 0; i < 16; i++) put(col + i, s[i]);
        col += 16;
        if (round == 0) p2::external_linear(s);
        for (int i = 0; i < 16; i++) s[i] = p2::sbox(s[i], rc->ext[round][i]);
        p2::external_linear(s);
        if (round == 3) {
            for (int i = 0; i < 16; i++) put(128 + i, s[i]);
#pragma unroll 1
            for (int k = 0; k < 20; k++) {
                s[0] = p2::sbox(s[0], rc->internal[k]);
                p2::internal_linear_lazy(s);
                if (k < 19) put(144 + k, s[0]);
            }
            for (int i = 1; i < 16; i++) s[i] = kb::umin(s[i], s[i] - kb::P);
        }
    }
    for (int i = 0; i < 16; i++) put(163 + i, s[i]);
}

// The padding row's 213 non-accumulation columns (global/mod.rs:L213-L236): zeros, the permutation of the zero state, the dummy point
template <class Put>
KB_HD void global_padding_row(const p2::RoundConstants* rc, const Pt& dummy, Put put) {
    for (int c = 0; c < G_INIT_X; c++) put(c, 0u);
    uint32_t s[16];
    for (int i = 0; i < 16; i++) s[i] = 0;
    perm_rows(s, rc, [&](int col, uint32_t v) { put(G_PERM + col, v); }, true);
    for (int i = 0; i < 7; i++) { put(G_X + i, dummy.x.c[i]); put(G_Y + i, dummy.y.c[i]); }
}

// The 213 non-accumulation columns of event `ev`'s row, index `row`, through put(column, word), and its point: for offset = 0,
// 1, ...: m = message (kind folded into word 0, offset into word 7), x = Poseidon2(m)[0..7]; the first offset whose
// x^3 + 45 x + 41 z^3 has a root that global_pick_root accepts. False (and nothing stored) when no offset below 256 has one.
template <class Put>
KB_HD bool global_event_row(const uint32_t* ev, uint32_t row, const p2::RoundConstants* rc, const FrobTables& ft, Put put, Pt* point) {
    auto put_perm = [&](int col, uint32_t v) { put(G_PERM + col, v); };
    const bool is_recv = (ev[8] & 0xffu) != 0;
    const uint32_t kind = (ev[8] >> 8) & 0xffu;
    uint32_t m[16];
    for (int i = 0; i < 8; i++) m[i] = kb::to_monty(ev[i] % kb::P);
    for (int i = 8; i < 16; i++) m[i] = 0;
    m[0] = kb::add(m[0], kb::to_monty((kind << 24) % kb::P));
    uint32_t offset = 0, rcv = 0;
    uint32_t s_in[16];
    S7 x, y;
    bool found = false;
    for (; offset < 256; offset++) {
        uint32_t s[16];
        for (int i = 0; i < 16; i++) s[i] = m[i];
        s[7] = kb::add(s[7], kb::to_monty(offset << 16));
        for (int i = 0; i < 16; i++) s_in[i] = s[i];
        perm_rows(s, rc, put_perm, false);
        for (int i = 0; i < 7; i++) x.c[i] = s[i];
        S7 root;
        if (!s7_sqrt(ft, s7_curve_rhs(x), &root)) continue;
        if (global_pick_root(root, is_recv, &y, &rcv)) { found = true; break; }
    }
    if (!found) return false;
    for (int c = 0; c < 8; c++) put(G_MESSAGE + c, kb::to_monty(ev[c] % kb::P));
    put(G_KIND, kb::to_monty(kind));
    put(G_M0_16, kb::to_monty(ev[0] & 0xffffu));
    put(G_M0_8, kb::to_monty((ev[0] >> 16) & 0xffu));
    for (int i = 0; i < 7; i++) { put(G_X + i, x.c[i]); put(G_Y + i, y.c[i]); }
    perm_rows(s_in, rc, put_perm, true);
    put(G_OFFSET, kb::to_monty(offset));
    for (int k = 0; k < 4; k++) put(G_Y6 + k, kb::to_monty((rcv >> (8 * k)) & 0xffu));
    put(G_IS_REAL, kb::R1);
    put(G_IS_RECV, is_recv ? kb::R1 : 0u);
    put(G_IS_SEND, is_recv ? 0u : kb::R1);
    put(G_INDEX, kb::to_monty(row));
    *point = Pt{x, y};
    return true;
}

// Row `row` of a table with n_events real rows: the event's row, or the padding row for ev == nullptr
template <class Put>
KB_HD bool global_row(const uint32_t* ev, uint32_t row, const p2::RoundConstants* rc, const FrobTables& ft, const Pt& dummy, Put put, Pt* point) {
    if (!ev) { global_padding_row(rc, dummy, put); return true; }
    return global_event_row(ev, row, rc, ft, put, point);
}

}  // namespace septic
}  // namespace sp1hip
