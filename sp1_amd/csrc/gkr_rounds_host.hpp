// sp1_amd/csrc/gkr_rounds_host.hpp — the row rounds of a LogUp-GKR layer in closed form, from the grid sums of one pass
// (gkr_kernels.hpp, above gkr_pass). Host code only, and nothing but the field: gkr.hip runs it between two hand-overs, and
// tests/native/gkr_rounds.hip checks it against the definition of the round polynomials without a GPU.
//
// A pass that sums k rounds hands over G on the grid {0, 1, inf}^k and the eq mass of its real cells. `finish` is the end of a
// round: finish(poly, pt, PA) puts the cubic into the proof and the transcript, multiplies PA (the eq factor of the variables
// bound so far) by eq(pt, challenge) and returns the challenge (LayerRounds::finish_round in gkr.hip).
#pragma once
#include <array>

#include "kb31.hpp"

namespace sp1hip {
namespace gkr_rounds {

using Ext = kb::Ext;
using Poly4 = std::array<Ext, 4>;

inline Ext add(const Ext& a, const Ext& b) { return kb::ext_add(a, b); }
inline Ext sub(const Ext& a, const Ext& b) { return kb::ext_sub(a, b); }
inline Ext mul(const Ext& a, const Ext& b) { return kb::ext_mul(a, b); }

// the cubic  scale (1 - pt + (2 pt - 1) X) (q0 + q1 X + q2 X^2)
inline Poly4 eq_times_quadratic(const Ext& scale, const Ext& pt, const Ext (&q)[3]) {
    const Ext e0 = mul(scale, sub(kb::ext_one(), pt)), e1 = mul(scale, sub(add(pt, pt), kb::ext_one()));
    return Poly4{mul(e0, q[0]), add(mul(e0, q[1]), mul(e1, q[0])), add(mul(e0, q[2]), mul(e1, q[1])), mul(e1, q[2])};
}
// the quadratic with values g0, g1 at 0, 1 and leading coefficient gi
inline void quadratic(const Ext& g0, const Ext& g1, const Ext& gi, Ext (&q)[3]) { q[0] = g0; q[1] = sub(sub(g1, g0), gi); q[2] = gi; }
inline Ext eval_quadratic(const Ext (&q)[3], const Ext& x) { return add(mul(add(mul(q[2], x), q[1]), x), q[0]); }

// The sv <= 2 rounds of a two-round pass from its sums S. t = row variables still unbound: the pass summed over
// row_point[t - 1] (the last unbound variable) and, sv == 2, row_point[t - 2]. PA = eq factor of the row variables bound so far.
// a[0], a[1] come back as the challenges the next pass folds with.
template <class Finish>
void row_rounds_closed_form(int sv, const Ext* S, const Ext* row_point, int t, Ext& PA, Finish&& finish, Ext* a) {
    const Ext one = kb::ext_one(), pt_a = row_point[t - 1];
    if (sv == 2) {
        // S: G00 G10 G01 G11 | Gi0 Gi1 | G0i G1i | Gii | Seq (first index: the last variable). The padding cells carry
        // F = 1, i.e. their eq mass on the constant coefficient: on the four finite grid points
        const Ext pt_b = row_point[t - 2];
        const Ext corr = sub(one, S[9]);
        Ext c0[3], c1[3], ci[3];
        quadratic(add(S[0], corr), add(S[1], corr), S[4], c0);     // G(X, 0)
        quadratic(add(S[2], corr), add(S[3], corr), S[5], c1);     // G(X, 1)
        quadratic(S[6], S[7], S[8], ci);                           // leading coefficient in Y
        Ext h[3];
        for (int k = 0; k < 3; k++) h[k] = add(c0[k], mul(pt_b, sub(c1[k], c0[k])));
        a[0] = finish(eq_times_quadratic(PA, pt_a, h), pt_a, PA);
        const Ext g0 = eval_quadratic(c0, a[0]), g1 = eval_quadratic(c1, a[0]), gi = eval_quadratic(ci, a[0]);
        Ext gy[3];
        quadratic(g0, g1, gi, gy);                                 // G(a0, Y)
        a[1] = finish(eq_times_quadratic(PA, pt_b, gy), pt_b, PA);
    } else {
        // S: G0 G1 | Gi | Seq
        const Ext corr = sub(one, S[3]);
        Ext h[3];
        quadratic(add(S[0], corr), add(S[1], corr), S[2], h);
        a[0] = finish(eq_times_quadratic(PA, pt_a, h), pt_a, PA);
        a[1] = kb::ext_zero();
    }
}

// The same for k <= GRID_MAX_K rounds from the 3^k + 1 sums of a deep pass. Axis j of the grid is the variable round j binds,
// row_point[t - 1 - j]; grid point (g_0 .. g_(k-1)), g_j in {0, 1, 2 = inf}, is S[sum g_j 3^j]; S[3^k] is the eq mass of the real
// cells. Round j's cubic is PA eq(pt_j, X) times the quadratic in X that is left of G when the axes before j sit at their
// challenges and the axes behind it are weighed with eq(pt, .) over their finite points: the triple (value at 0, value at 1,
// leading coefficient) of that quadratic is the weighted sum of the grid's triples, because a quadratic is linear in its triple.
// Then axis j is bound — every triple along it collapses to its quadratic's value at the challenge, the inf points of the
// later axes included: G is multi-quadratic, so a leading coefficient in Y is itself a quadratic in X with the triple
// (G(0, inf), G(1, inf), G(inf, inf)). The padding cells carry F = 1: their eq mass 1 - Seq goes on the finite points only.
constexpr int GRID_MAX_K = 4;
constexpr int grid_points(int k) { int n = 1; for (int j = 0; j < k; j++) n *= 3; return n; }
constexpr int grid_sums(int k) { return grid_points(k) + 1; }

template <class Finish>
void row_rounds_from_grid(int k, const Ext* S, const Ext* row_point, int t, Ext& PA, Finish&& finish, Ext* a) {
    const Ext one = kb::ext_one();
    int n = grid_points(k);
    Ext cur[grid_points(GRID_MAX_K)];
    const Ext corr = sub(one, S[n]);
    for (int g = 0; g < n; g++) {
        bool finite = true;
        for (int x = g, j = 0; j < k; j++, x /= 3) finite = finite && x % 3 != 2;
        cur[g] = finite ? add(S[g], corr) : S[g];
    }
    for (int j = 0; j < k; j++) {                            // cur: the axes j .. k - 1, axis j fastest
        const Ext pt = row_point[t - 1 - j];
        const int later = k - 1 - j;
        Ext h[3] = {kb::ext_zero(), kb::ext_zero(), kb::ext_zero()};
        for (int b = 0; b < (1 << later); b++) {             // the finite points of the later axes
            Ext wgt = one;
            int idx = 0;
            for (int m = 0, p3 = 1; m < later; m++, p3 *= 3) {
                const Ext& pm = row_point[t - 2 - j - m];
                const bool bit = (b >> m) & 1;
                wgt = later == 0 ? wgt : mul(wgt, bit ? pm : sub(one, pm));
                idx += bit ? p3 : 0;
            }
            for (int d = 0; d < 3; d++) h[d] = add(h[d], later == 0 ? cur[d] : mul(wgt, cur[3 * idx + d]));
        }
        Ext q[3];
        quadratic(h[0], h[1], h[2], q);
        a[j] = finish(eq_times_quadratic(PA, pt, q), pt, PA);
        n /= 3;
        for (int m = 0; m < n; m++) {
            Ext qm[3];
            quadratic(cur[3 * m], cur[3 * m + 1], cur[3 * m + 2], qm);
            cur[m] = eval_quadratic(qm, a[j]);
        }
    }
    for (int j = k; j < GRID_MAX_K; j++) a[j] = kb::ext_zero();
}

}  // namespace gkr_rounds
}  // namespace sp1hip
