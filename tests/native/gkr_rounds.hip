// tests/native/gkr_rounds.hip — host driver for sp1_amd/csrc/gkr_rounds_host.hpp (the header unchanged): the k round polynomials
// that the closed form makes of a pass's 3^k + 1 grid sums against the DEFINITION of a sumcheck round, on small random layers
// whose interactions end inside a cell, are shorter than one cell, or have no rows. Host code only: no kernel, no device call.
//
//   gkr_rounds SEED      every k = 1 .. 4 with 0 .. 2 further unbound variables; prints one line per case, "OK n" at the end
//
// A layer here: W = 8 interaction slots with the weights eq(int_point, i), of which the first K hold tables n0, d0, n1, d1 of
// rows_i <= 2^t real rows (the rest of every table, and every slot >= K, is the padding fraction (0, 1)); t unbound row
// variables, row index bit 0 = the last variable. The claim is  PA sum_i sum_x eq_int[i] eq(row_point, x) F_i(x).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "gkr_rounds_host.hpp"

using namespace sp1hip;
using namespace sp1hip::gkr_rounds;

static uint64_t g_state;
static uint64_t next_u64() {
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static Ext rand_ext() { Ext e; for (int k = 0; k < 4; k++) e.c[k] = (uint32_t)(next_u64() % kb::P); return e; }
static Ext eq1(const Ext& pt, const Ext& x) { const Ext one = kb::ext_one(); return add(mul(pt, x), mul(sub(one, pt), sub(one, x))); }
static Ext lerp(const Ext& a, const Ext& b, const Ext& x) { return add(a, mul(sub(b, a), x)); }
static std::vector<Ext> eq_table(const std::vector<Ext>& pt) {        // first coordinate = most significant index bit
    std::vector<Ext> ev{kb::ext_one()};
    for (const Ext& x : pt) {
        std::vector<Ext> nx(ev.size() * 2);
        for (size_t i = 0; i < ev.size(); i++) { const Ext pr = mul(ev[i], x); nx[2 * i] = sub(ev[i], pr); nx[2 * i + 1] = pr; }
        ev.swap(nx);
    }
    return ev;
}

struct Row { Ext n0, d0, n1, d1; };
static Row padding_row() { return Row{kb::ext_zero(), kb::ext_one(), kb::ext_zero(), kb::ext_one()}; }
static Row lerp_row(const Row& a, const Row& b, const Ext& x) { return Row{lerp(a.n0, b.n0, x), lerp(a.d0, b.d0, x), lerp(a.n1, b.n1, x), lerp(a.d1, b.d1, x)}; }
static Row sub_row(const Row& a, const Row& b) { return Row{sub(a.n0, b.n0), sub(a.d0, b.d0), sub(a.n1, b.n1), sub(a.d1, b.d1)}; }
static Ext F(const Row& r, const Ext& lambda) { return add(mul(lambda, add(mul(r.n0, r.d1), mul(r.n1, r.d0))), mul(r.d0, r.d1)); }

struct Recorder {                                            // the end of a round: keeps the cubic, draws the challenge
    std::vector<Poly4> polys;
    std::vector<Ext> alphas;
    Ext operator()(const Poly4& poly, const Ext& pt, Ext& eq_factor) {
        polys.push_back(poly);
        const Ext a = rand_ext();
        alphas.push_back(a);
        eq_factor = mul(eq_factor, eq1(pt, a));
        return a;
    }
};
static Ext poly_eval(const Poly4& c, const Ext& x) { return add(mul(add(mul(add(mul(c[3], x), c[2]), x), c[1]), x), c[0]); }
static Ext small(uint32_t v) { return kb::ext_from_base(kb::to_monty(v)); }

static int g_fail = 0, g_checks = 0;
static void expect(bool ok, const char* what, int k, int extra, int j) {
    g_checks++;
    if (!ok) { g_fail++; printf("FAIL %s: k = %d, extra = %d, round %d\n", what, k, extra, j); }
}

// tables[i]: 2^t rows, padding filled in
static void run_case(int k, int extra) {
    const int t = k + extra, W = 8, niv = 3;
    const uint32_t full = 1u << t, cell = 1u << k;
    // heights: a full table; one that ends one row short, inside its last cell; one shorter than a cell (its other cells are whole
    // padding); one cell and a row; a single row; none; and one that ends on a cell boundary short of the table
    std::vector<uint32_t> rows = {full, full - 1, cell > 1 ? cell - 1 : 1, std::min(full, cell + 1), 1, 0, extra ? full - cell : full};
    const int K = (int)rows.size();
    std::vector<Ext> int_point(niv), row_point(t);
    for (auto& x : int_point) x = rand_ext();
    for (auto& x : row_point) x = rand_ext();
    const Ext lambda = rand_ext(), PA0 = rand_ext();
    const std::vector<Ext> eq_int = eq_table(int_point);
    std::vector<std::vector<Row>> tab(W, std::vector<Row>(full, padding_row()));
    for (int i = 0; i < K; i++)
        for (uint32_t r = 0; r < rows[i]; r++) tab[i][r] = Row{rand_ext(), rand_ext(), rand_ext(), rand_ext()};

    // ---- the grid sums, straight from the definition: per real cell, every table on {0, 1, inf}^k axis by axis
    const int NP = grid_points(k);
    std::vector<Ext> S(NP + 1, kb::ext_zero());
    const std::vector<Ext> T = eq_table(std::vector<Ext>(row_point.begin(), row_point.begin() + extra));
    for (int i = 0; i < K; i++) {
        const uint32_t cells = (rows[i] + cell - 1) / cell;
        for (uint32_t c = 0; c < cells; c++) {
            const Ext w = mul(T[c], eq_int[i]);
            std::vector<Row> g(tab[i].begin() + c * cell, tab[i].begin() + (c + 1) * cell);
            // axis a (row bit a): entries ordered with the axes already transformed fastest
            size_t lo = 1;                                   // 3^a
            for (int a = 0; a < k; a++, lo *= 3) {
                const size_t hi = (size_t)1 << (k - 1 - a);  // row bits still untransformed above this axis
                std::vector<Row> nx(lo * 3 * hi, padding_row());
                for (size_t h = 0; h < hi; h++)
                    for (size_t l = 0; l < lo; l++) {
                        const Row &v0 = g[(2 * h) * lo + l], &v1 = g[(2 * h + 1) * lo + l];
                        nx[(3 * h) * lo + l] = v0; nx[(3 * h + 1) * lo + l] = v1; nx[(3 * h + 2) * lo + l] = sub_row(v1, v0);
                    }
                g.swap(nx);
            }
            for (int p = 0; p < NP; p++) S[p] = add(S[p], mul(w, F(g[p], lambda)));
            S[NP] = add(S[NP], w);
        }
    }

    // ---- the closed form
    const uint64_t rng_at_rounds = g_state;
    Recorder rec;
    Ext PA = PA0, a[GRID_MAX_K];
    row_rounds_from_grid(k, S.data(), row_point.data(), t, PA, rec, a);
    expect((int)rec.polys.size() == k, "round count", k, extra, -1);

    // ---- the definition, round by round: fold the bound variables, lay X on the next one, sum the rest of the hypercube
    Ext claim = kb::ext_zero();
    {
        const std::vector<Ext> eq_rows = eq_table(row_point);
        for (int i = 0; i < W; i++)
            for (uint32_t r = 0; r < full; r++) claim = add(claim, mul(mul(eq_int[i], eq_rows[r]), F(tab[i][r], lambda)));
        claim = mul(claim, PA0);
    }
    std::vector<std::vector<Row>> cur = tab;
    Ext bound = PA0;                                         // PA0 x eq factor of the variables bound so far
    for (int j = 0; j < k; j++) {
        const Ext pt = row_point[t - 1 - j];
        const std::vector<Ext> eq_rest = eq_table(std::vector<Ext>(row_point.begin(), row_point.begin() + (t - 1 - j)));
        const size_t half = cur[0].size() / 2;
        Ext sum01 = kb::ext_zero();
        for (uint32_t xv = 0; xv < 4; xv++) {
            const Ext X = small(xv);
            Ext acc = kb::ext_zero();
            for (int i = 0; i < W; i++)
                for (size_t q = 0; q < half; q++) acc = add(acc, mul(mul(eq_int[i], eq_rest[q]), F(lerp_row(cur[i][2 * q], cur[i][2 * q + 1], X), lambda)));
            const Ext want = mul(mul(bound, eq1(pt, X)), acc);
            expect(kb::ext_eq(poly_eval(rec.polys[j], X), want), "round polynomial against the definition", k, extra, j);
            if (xv < 2) sum01 = add(sum01, poly_eval(rec.polys[j], X));
        }
        expect(kb::ext_eq(sum01, claim), "the running claim chains", k, extra, j);
        expect(kb::ext_eq(a[j], rec.alphas[j]), "challenge returned", k, extra, j);
        claim = poly_eval(rec.polys[j], rec.alphas[j]);
        bound = mul(bound, eq1(pt, rec.alphas[j]));
        for (int i = 0; i < W; i++) {
            std::vector<Row> nx(half);
            for (size_t q = 0; q < half; q++) nx[q] = lerp_row(cur[i][2 * q], cur[i][2 * q + 1], rec.alphas[j]);
            cur[i].swap(nx);
        }
    }
    expect(kb::ext_eq(PA, bound), "eq factor of the bound variables", k, extra, k);

    // ---- k <= 2: the two-round pass's own function, from the same sums in its order, draws the same challenges and must give
    // the same words
    if (k <= 2) {
        static const int order2[10] = {0, 1, 3, 4, 2, 5, 6, 7, 8, 9}, order1[4] = {0, 1, 2, 3};   // G00 G10 G01 G11 | Gi0 Gi1 | G0i G1i | Gii | Seq
        Ext S2[10];
        for (int q = 0; q < (k == 2 ? 10 : 4); q++) S2[q] = S[k == 2 ? order2[q] : order1[q]];
        g_state = rng_at_rounds;
        Recorder rec2;
        Ext PA2 = PA0, a2[2];
        row_rounds_closed_form(k, S2, row_point.data(), t, PA2, rec2, a2);
        bool same = rec2.polys.size() == rec.polys.size() && kb::ext_eq(PA2, PA);
        for (size_t j = 0; same && j < rec.polys.size(); j++) {
            for (int c = 0; c < 4; c++) same = same && kb::ext_eq(rec2.polys[j][c], rec.polys[j][c]);
            same = same && kb::ext_eq(a2[j], a[j]);
        }
        expect(same, "k <= 2 equals the two-round closed form word for word", k, extra, -1);
    }
    printf("case k = %d, t = %d: done\n", k, t);
}

int main(int argc, char** argv) {
    g_state = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;
    for (int k = 1; k <= GRID_MAX_K; k++)
        for (int extra = 0; extra <= 2; extra++) run_case(k, extra);
    if (g_fail) { printf("FAILED %d of %d\n", g_fail, g_checks); return 1; }
    printf("OK %d\n", g_checks);
    return 0;
}
