// sp1_amd/csrc/gkr.hip — LogUp-GKR on the device: the lookup argument that sits between
// `commit_traces` and zerocheck in a shard proof.
//
//   sp1hip_logup_gkr_prove  `GkrProverImpl::prove_logup_gkr`   /root/reference/crates/hypercube/src/logup_gkr/prover.rs:L70-L215
//     first layer           `generate_interaction_vals` / `generate_first_layer`   execution.rs:L13-L36, L112-L252
//     circuit               `layer_transition`, `extract_outputs`                 execution.rs:L38-L110, L254-L382
//     per-layer sumcheck    `prove_gkr_round` + `LogupRoundPolynomial`            cpu.rs:L146-L226, logup_poly.rs:L70-L553
//                           driven as `reduce_sumcheck_to_evaluation`             /root/reference/slop/crates/sumcheck/src/prover.rs:L13-L96
//   Output: bincode(LogupGkrProof) (/root/reference/crates/hypercube/src/logup_gkr/proof.rs:L32-L62).
//
// File map
//   gkr_kernels.hpp   every kernel and the descriptors the host fills for them (IntDesc .. OpenDesc)
//   gkr_host.cpp      the interaction-variable rounds in AVX-512 (tables as coefficient planes)
//   gkr_rounds_host.hpp   the closed forms of the row rounds from a pass's sums (host only; tests/native/gkr_rounds.hip)
//   ext_host.hpp      the host field helpers shared with jagged.hip (Ext operators, eq tables, DeviceBuf, upload)
//   gkr.hip (here)    the cubic interpolation and the proof's byte writer; Levels (the fraction tree's storage); plan_passes (pure host:
//                     every pass's shape and descriptors); the two forms of the host
//                     interaction rounds; GkrProver: one proof, a phase per member function, run in order by GkrProver::prove
//
// MI355X shape
//  * Layout: every (chip, interaction) owns contiguous per-row vectors `N[level][i][row]`, `D[level][i][row]`
//    over the chip's REAL rows only (padding rows are the constants (0, 1) and are never stored): a wave
//    walks consecutive rows of one interaction, so all loads are unit-stride (4 B lanes for the base-field
//    first-layer numerators, 16 B lanes for ext), and the interaction's program / eq weight are wave-uniform.
//  * The fraction tree (level L -> 1) is built once and kept: level l has ceil(h / 2^(L-l)) rows per chip.
//    The GKR layer with v row variables reads level v+1 in place (numerator_0/1 = even/odd rows).
//  * One fused kernel per sumcheck round over a row variable: fold the previous round's four tables with
//    alpha and accumulate the next round's three sums (y(0), 8 y(1/2), eq mass of the real entries) from
//    the folded values in registers. The padding rows enter in closed form on the host, exactly as the
//    reference does it (`eq_correction_term`, logup_poly.rs:L521-L530).
//  * eq over the row variables is never folded: the per-round tables are the partial-Lagrange tables of
//    the remaining prefix of the point, built for all prefix lengths by one launch per layer; the factor
//    of the already-bound variables is a host scalar.
//  * Once the row variables are bound, a layer is 2^niv x 4 values: the interaction-variable rounds run on
//    the host (a few hundred ext products).
#include <algorithm>
#include <array>
#include <chrono>
#include <cstring>
#include <optional>
#include <string>
#include <vector>

#include "device_ctx.hpp"
#include "host_par.hpp"

namespace sp1hip {      // gkr_host.cpp: the interaction-variable rounds in AVX-512 (tables as coefficient planes)
bool gkr_host_simd_available();
void gkr_host_round_sums(const uint32_t* tab, size_t stride, const uint32_t* eq, size_t eq_stride, size_t real_pairs, uint32_t out[6][4]);
void gkr_host_round_fold(const uint32_t* tab, uint32_t* out, size_t stride, size_t real_pairs, const uint32_t alpha[4]);
}
#include "round_sync.hpp"
#include "tensor_table.hpp"
#include "ext_host.hpp"
#include "gkr_kernels.hpp"
#include "gkr_rounds_host.hpp"

namespace sp1hip {

void challenger_observe(sp1hip_challenger_t* ch, uint32_t x);
kb::Ext challenger_sample_ext(sp1hip_challenger_t* ch);
void challenger_restore(sp1hip_challenger_t* dst, const sp1hip_challenger_t* src);

namespace gkr {

// ================================================================ host side
using namespace ext_host;   // DeviceBuf, the Ext operators, ext_c, log2_ceil, partial_lagrange_host, eval_mle_host, upload

using gkr_rounds::Poly4;
Ext poly_eval(const Poly4& c, const Ext& x) { return ((c[3] * x + c[2]) * x + c[1]) * x + c[0]; }

// the cubic through (0, y0), (1, y1), (1/2, yh), (b, 0): Lagrange interpolation as the reference's
// interpolate_univariate_polynomial (univariate.rs:L85-L97) — any exact method gives the same coefficients
Poly4 interpolate4(const Ext (&xs)[4], const Ext (&ys)[4]) {
    Poly4 res{kb::ext_zero(), kb::ext_zero(), kb::ext_zero(), kb::ext_zero()};
    // a node whose value is zero contributes nothing (every caller's fourth value is the root of the eq factor), and
    // the remaining denominators are inverted together (one inversion + 3 products per extra denominator): this runs
    // once per sumcheck round on the host, between two device hand-overs
    Ext num[4][4], den[4];
    bool live[4];
    for (int i = 0; i < 4; i++) {
        live[i] = !kb::ext_eq(ys[i], kb::ext_zero());
        if (!live[i]) continue;
        den[i] = kb::ext_one();
        Ext cur[4] = {ys[i], kb::ext_zero(), kb::ext_zero(), kb::ext_zero()};
        int deg = 0;
        for (int j = 0; j < 4; j++) {
            if (j == i) continue;
            den[i] = den[i] * (xs[i] - xs[j]);
            Ext nxt[4] = {kb::ext_zero(), kb::ext_zero(), kb::ext_zero(), kb::ext_zero()};
            for (int k = 0; k <= deg; k++) { nxt[k + 1] = nxt[k + 1] + cur[k]; nxt[k] = nxt[k] - cur[k] * xs[j]; }
            deg++;
            for (int k = 0; k < 4; k++) cur[k] = nxt[k];
        }
        for (int k = 0; k < 4; k++) num[i][k] = cur[k];
    }
    // batch inversion of the live denominators
    Ext prefix[4], running = kb::ext_one();
    for (int i = 0; i < 4; i++) if (live[i]) { prefix[i] = running; running = running * den[i]; }
    Ext inv_all = kb::ext_inv(running);
    for (int i = 3; i >= 0; i--) {
        if (!live[i]) continue;
        const Ext inv = inv_all * prefix[i];
        inv_all = inv_all * den[i];
        for (int k = 0; k < 4; k++) res[k] = res[k] + num[i][k] * inv;
    }
    return res;
}

struct Bytes {
    std::vector<uint8_t> b;
    void u64(uint64_t v) { for (int i = 0; i < 8; i++) b.push_back((uint8_t)(v >> (8 * i))); }
    void felt(uint32_t m) { const uint32_t v = kb::from_monty(m); for (int i = 0; i < 4; i++) b.push_back((uint8_t)(v >> (8 * i))); }
    void ext(const Ext& e) { for (int k = 0; k < 4; k++) felt(e.c[k]); }
};

void observe_ext(sp1hip_challenger_t* ch, const Ext& e) { for (int k = 0; k < 4; k++) challenger_observe(ch, e.c[k]); }

struct ChipInfo {
    std::string name;
    uint32_t rows, k, main_w, prep_w, int0;                 // k interactions, int0 = first global interaction index
    const uint32_t* d_main;
    const uint32_t* d_prep;
};

constexpr uint32_t MAX_TILES = 512;
constexpr uint64_t GKR_LOOKAHEAD_DEFAULT = 4;                // rounds per flat pass (SP1HIP_GKR_LOOKAHEAD; HISTORY: the A/B runs of 2, 3 and 4)
uint32_t tiles_for(uint64_t threads) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((threads + 255) / 256, 1), MAX_TILES); }

// per global interaction: is_send, kind (canonical), multiplicity and values as (constant flag, words) — words = the vcol in
// device form [n_terms, constant (Montgomery), n_terms x (is_main, column, weight (Montgomery))]
struct ParsedInt { uint32_t is_send, kind; std::vector<uint32_t> mult; std::vector<std::vector<uint32_t>> values; };
struct RoundOut { Ext n0, n1, d0, d1; std::vector<Poly4> polys; Ext claimed_sum, eval; std::vector<Ext> point; };
// The passes of a layer with v row variables: (fold 0, sum s0), then (fold what was just summed, sum what the planner takes of
// what remains) until nothing remains; the last pass only folds. A pass sums two rounds (gkr_pass) — or up to `depth` rounds
// where that keeps it a FLAT launch (gkr_pass_deep; choose_pass).
struct PassShape { int fv, sv; bool first; uint32_t tiles, tile_size, total_slots; size_t flat_off; bool flat; };

// ---- SP1HIP_GKR_DEBUG=1: host-side phase times on stderr (where a stage's non-kernel time goes). Off: a branch per call.
struct GkrTimer {
    enum Part { ROWS, INT, LAYER_HEAD, WAIT, HOST, LAUNCH, SKIP };     // two clocks: a layer's halves | a pass's parts; *_HEAD / SKIP count nowhere
    using Clock = std::chrono::steady_clock;
    bool on = false;
    Clock::time_point last, clk[2];
    double part_ms[7] = {};
    int waits = 0;                                           // hand-overs inside the layers
    static double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
    void start() { static const bool env = env_flag("SP1HIP_GKR_DEBUG", false); on = env; last = Clock::now(); }
    void mark(const char* what) {                            // the time since the previous mark
        if (!on) return;
        const auto now = Clock::now();
        fprintf(stderr, "[sp1hip gkr] %-28s %8.3f ms\n", what, ms(last, now));
        last = now;
    }
    void lap(Part p) {                                       // the time since the previous lap of p's clock goes to part p
        if (!on) return;
        const auto now = Clock::now();
        part_ms[p] += ms(clk[p >= WAIT], now);
        clk[p >= WAIT] = now;
        waits += p == WAIT;
    }
    void report_layers() {
        if (!on) return;
        fprintf(stderr, "[sp1hip gkr]   of which row-variable rounds %.3f ms, interaction-variable rounds (host) %.3f ms\n", part_ms[ROWS], part_ms[INT]);
        fprintf(stderr, "[sp1hip gkr]   %d hand-overs inside the layers: waiting for the sums %.3f ms, closed forms + transcript %.3f ms, launch calls %.3f ms\n",
                waits, part_ms[WAIT], part_ms[HOST], part_ms[LAUNCH]);
    }
};

// ---- device storage: levels L .. 1 of the fraction tree, per interaction. Rows at level l of a chip of h real rows: ceil(h / 2^(L - l))
struct Levels {
    int L = 0;
    uint32_t K = 0;
    std::vector<uint32_t> h;                                 // real rows of interaction i's chip
    std::vector<size_t> entries;                             // total entries of level l over all interactions
    std::vector<std::vector<size_t>> off;                    // offsets of interaction i inside level l
    std::vector<DeviceBuf> N, D;                             // (level L's numerators are base-field words)
    uint32_t rows_at(uint32_t i, int l) const { return (uint32_t)(((uint64_t)h[i] + (((uint64_t)1 << (L - l)) - 1)) >> (L - l)); }
    void* n_ptr(int l, uint32_t i) const { return (char*)N[l].p + off[l][i] * (l == L ? 4 : 16); }
    Ext* d_ptr(int l, uint32_t i) const { return D[l].ext() + off[l][i]; }
    int alloc(int L_, std::vector<uint32_t> rows_of_interaction, hipStream_t s) {
        L = L_; h = std::move(rows_of_interaction); K = (uint32_t)h.size();
        entries.assign(L + 2, 0);
        off.assign(L + 1, std::vector<size_t>(K + 1, 0));
        for (int l = 1; l <= L; l++) {
            for (uint32_t i = 0; i < K; i++) off[l][i + 1] = off[l][i] + rows_at(i, l);
            entries[l] = off[l][K];
        }
        N = std::vector<DeviceBuf>(L + 1); D = std::vector<DeviceBuf>(L + 1);
        for (int l = 1; l <= L; l++) {
            SP1HIP_TRY(N[l].alloc(std::max<size_t>(entries[l], 1) * (l == L ? 4 : 16), s));
            SP1HIP_TRY(D[l].alloc(std::max<size_t>(entries[l], 1) * 16, s));
        }
        return SP1HIP_SUCCESS;
    }
};

// ---- the descriptors of every pass of every layer: pure host work on shapes, launches nothing and touches no stream
struct PassPlan {
    std::vector<PassShape> shapes;
    std::vector<PassDesc> all_descs;                         // K per pass, in launch order
    std::vector<uint16_t> flat_index;                        // FLAT launches: slot -> descriptor, all launches back to back
};
// What the next pass of a layer sums. rows_in: every interaction's rows before the pass folds fv variables; left: the variables
// unbound after that fold. The look-ahead `depth` (SP1HIP_GKR_LOOKAHEAD: 2, 3 or 4) is taken where the pass is FLAT at that depth
// — its slots, rows rounded up to whole cells of 2^sv per interaction, fit one flat launch —, otherwise the pass sums two rounds as
// it always did: the large passes are bound by their products, a deeper grid costs them more than a launch, and only the flat
// passes (latency, not work) gain from running fewer of them. depth = 2 is the two-round plan, launch for launch.
struct PassChoice { int sv; bool flat; uint64_t total_slots; };
PassChoice choose_pass(const std::vector<uint32_t>& rows_in, int fv, int left, int depth, uint32_t flat_max_slots) {
    auto total_slots = [&](int sv) {
        uint64_t n = 0;
        for (uint32_t rin : rows_in) { const uint32_t ro = (rin + (1u << fv) - 1) >> fv; n += ((ro + (1u << sv) - 1) >> sv) << sv; }
        return n;
    };
    const bool index_fits = rows_in.size() <= 65536;         // flat_index entries are 16-bit
    if (depth > 2 && left > 2) {
        const int sv = std::min(depth, left);
        const uint64_t n = total_slots(sv);
        if (n <= flat_max_slots && index_fits) return PassChoice{sv, true, n};
    }
    const int sv = std::min(2, left);
    const uint64_t n = total_slots(sv);
    return PassChoice{sv, n <= flat_max_slots && index_fits, n};
}
// passes of layers 1 .. L - 1 (depth 2: (0, .), the folds in pairs, the last fold = v + 1 / 2 + 1 per layer): the walk of plan_passes
// over the shapes alone, for the buffers that are taken before the plan is made
size_t count_passes(const Levels& lv, uint32_t flat_max_slots, int depth) {
    size_t n = 0;
    std::vector<uint32_t> rows_in(lv.K);
    for (int v = 1; v <= lv.L - 1; v++) {
        for (uint32_t i = 0; i < lv.K; i++) rows_in[i] = (lv.rows_at(i, v + 1) + 1) / 2;
        for (int t = v, fv = 0;;) {
            const int sv = choose_pass(rows_in, fv, t - fv, depth, flat_max_slots).sv;
            for (uint32_t& r : rows_in) r = (r + (1u << fv) - 1) >> fv;
            t -= fv;
            n++;
            if (sv == 0) break;
            fv = sv;
        }
    }
    return n;
}

// scratch[b]: the folded tables (4 vectors per interaction, ping-pong); host_rows: where a layer's last fold (one row per
// interaction) goes when it is published straight to the host (null: it stays in scratch)
void plan_passes(const Levels& lv, uint32_t flat_max_slots, int depth, size_t n_passes, Ext* const (&scratch)[2], Ext* host_rows, PassPlan& plan) {
    const uint32_t K = lv.K;
    auto scratch_ptr = [&](int b, uint32_t i, int which, const std::vector<size_t>& so) -> Ext* { return scratch[b] + 4 * so[i] + (size_t)which * (so[i + 1] - so[i]); };
    // workgroups of a large pass. While every workgroup paid an L2 write-back and a serialised ticket in its tail
    // (round_sync.hpp) one resident set — 256 CUs x 4 workgroups — was the optimum; without them finer tiles balance the
    // tail better (sweep of round 2 on the one-round kernels: 4096 best, flat between 2048 and 8192). Round 4, two-round passes on
    // the real-chip shard (alternating runs on three boxes): 1024-3072 tiles are within 0.3 ms of each other, 4096 is 0.7-1.0 ms
    // slower over the stage, 8192 / 16384 1.4 / 3.2 ms slower — a pass carries more state per workgroup than a round kernel did.
    constexpr uint32_t TARGET_TILES = 2048;
    plan.all_descs.reserve(n_passes * K);                    // ~10 MB at 730 interactions: no regrowth copies while planning
    std::vector<uint32_t> rows_in(K);
    std::vector<size_t> so_prev, so_next;
    for (int v = 1; v <= lv.L - 1; v++) {
        for (uint32_t i = 0; i < K; i++) rows_in[i] = (lv.rows_at(i, v + 1) + 1) / 2;
        int cur = 0, t = v, fv = 0, pass = 0;
        for (;;) {
            const PassChoice choice = choose_pass(rows_in, fv, t - fv, depth, flat_max_slots);   // variables left after this pass's fold: t - fv
            const int sv = choice.sv;
            const bool first = pass <= 1;                    // pass 0 only sums, so pass 1 still reads the level
            if (fv > 0) { so_next.assign(K + 1, 0); for (uint32_t i = 0; i < K; i++) so_next[i + 1] = so_next[i] + ((rows_in[i] + (1u << fv) - 1) >> fv); }
            auto slots_of = [&](uint32_t rin) -> uint32_t { const uint32_t ro = (rin + (1u << fv) - 1) >> fv; return ((ro + (1u << sv) - 1) >> sv) << sv; };
            const uint64_t total_slots = choice.total_slots;
            const bool flat = choice.flat;
            const uint32_t tile_size = flat ? 1u : (uint32_t)std::max<uint64_t>(256, ((total_slots + TARGET_TILES - 1) / TARGET_TILES + 255) / 256 * 256);
            const size_t flat_off = plan.flat_index.size();
            plan.all_descs.resize(plan.all_descs.size() + K);
            PassDesc* out = plan.all_descs.data() + plan.all_descs.size() - K;
            uint32_t tile0 = 0;
            for (uint32_t i = 0; i < K; i++) {
                PassDesc& d = out[i];
                d = PassDesc{};
                d.rows_in = rows_in[i]; d.eq_int_index = i;
                if (first) { d.src[0] = lv.n_ptr(v + 1, i); d.src[1] = lv.d_ptr(v + 1, i); d.rows_x = lv.rows_at(i, v + 1); }
                else for (int w = 0; w < 4; w++) d.src[w] = scratch_ptr(cur ^ 1, i, w, so_prev);
                if (fv > 0) for (int w = 0; w < 4; w++)
                    d.dst[w] = (sv == 0 && host_rows) ? host_rows + 4 * so_next[i] + (size_t)w * (so_next[i + 1] - so_next[i]) : scratch_ptr(cur, i, w, so_next);
                d.tile0 = tile0;
                const uint32_t n_tiles = (slots_of(rows_in[i]) + tile_size - 1) / tile_size;
                if (flat) plan.flat_index.insert(plan.flat_index.end(), n_tiles, (uint16_t)i);
                tile0 += n_tiles;
            }
            // slots per workgroup of a flat launch: 256, one lane per output row; a deep fold (gkr_pass_deep_fold) 64, four lanes per row
            const uint32_t wg_slots = fv > 2 ? 64 : 256;
            if (flat) plan.shapes.push_back(PassShape{fv, sv, first, std::max<uint32_t>((tile0 + wg_slots - 1) / wg_slots, 1), tile_size, tile0, flat_off, true});
            else plan.shapes.push_back(PassShape{fv, sv, first, std::max<uint32_t>(tile0, 1), tile_size, tile0, 0, false});
            if (fv > 0) { for (uint32_t i = 0; i < K; i++) rows_in[i] = (rows_in[i] + (1u << fv) - 1) >> fv; so_prev = so_next; cur ^= 1; }
            t -= fv;
            pass++;
            if (sv == 0) break;
            fv = sv;
        }
    }
    if (plan.flat_index.empty()) plan.flat_index.push_back(0);
    plan.flat_index.resize((plan.flat_index.size() + 1) / 2 * 2);
}

// ================================================================ a layer's sumcheck rounds on the host
struct Consts { const Ext one = kb::ext_one(), zero = kb::ext_zero(), inv8 = kb::ext_inv(ext_c(8)), inv2 = kb::ext_inv(ext_c(2)), four = ext_c(4); };

// what the rounds of one layer accumulate: the layer's part of the proof, the challenges, the running claim
struct LayerRounds {
    sp1hip_challenger_t* ch;
    RoundOut ro;
    std::vector<Ext> alphas;
    Ext claim;
    // the end of a round: the polynomial goes into the proof and the transcript and the challenge comes back; the claim moves on,
    // and eq_factor (of the variables bound so far) takes the factor eq(pt, challenge) of the variable this round binds
    Ext finish_round(const Poly4& poly, const Ext& pt, Ext& eq_factor) {
        ro.polys.push_back(poly);
        for (auto& c : poly) observe_ext(ch, c);
        const Ext a = challenger_sample_ext(ch), one = kb::ext_one();
        alphas.push_back(a);
        claim = poly_eval(poly, a);
        eq_factor = eq_factor * (pt * a + (one - pt) * (one - a));
        return a;
    }
};

constexpr size_t plane_stride(size_t n) { return ((n + 15) / 16) * 16 + 16; }     // words of one coefficient plane of an n-entry table (gkr_host.cpp)

// Lagrange tables of every prefix of the interaction point (tabs[m]: the first m coordinates, 2^m entries) for the
// HOST rounds at the end of the layer
struct EqTabs {
    std::vector<std::vector<Ext>> tabs;
    std::vector<std::vector<uint32_t>> soa;                  // simd: the same tables as coefficient planes (gkr_host.cpp)
    void build(const std::vector<Ext>& int_point, bool simd) {
        const int niv = (int)int_point.size();
        tabs.assign(niv + 1, {}); soa.assign(niv + 1, {});
        tabs[0] = {kb::ext_one()};
        for (int m = 0; m < niv; m++) {
            const std::vector<Ext>& ev = tabs[m];
            std::vector<Ext>& nx = tabs[m + 1];
            nx.resize(ev.size() * 2);
            const Ext x = int_point[m];
            for (size_t i = 0; i < ev.size(); i++) { const Ext pr = ev[i] * x; nx[2 * i] = ev[i] - pr; nx[2 * i + 1] = pr; }
        }
        if (!simd) return;
        for (int m = 1; m <= niv; m++) {
            const size_t es = plane_stride((size_t)1 << m);
            soa[m].assign(4 * es, 0u);
            for (size_t i = 0; i < tabs[m].size(); i++)
                for (int k = 0; k < 4; k++) soa[m][(size_t)k * es + i] = tabs[m][i].c[k];
        }
    }
};

// A layer whose row variables are bound is four tables (n0, d0, n1, d1) dense over 2^niv, entries >= real being the padding
// fraction (0, 1). Two forms of them with the same interface: sums(m, real_pairs) = a round's six sums against the eq table
// of the first m coordinates, fold(real_pairs, half, alpha) = bind the last variable, first_row = what is left at the end.
struct alignas(64) RoundSums { Ext x0, y0, xh, yh, e0, es; };

// AVX-512, one thread, the helpers stay asleep: coefficient planes, table w, plane k at (4 w + k) stride (gkr_host.cpp)
struct PlaneTables {
    const EqTabs& eq;
    const size_t stride;
    std::vector<uint32_t> soa[2];
    int side = 0;
    PlaneTables(const EqTabs& eq_, uint32_t W) : eq(eq_), stride(plane_stride(W)) {
        for (int b = 0; b < 2; b++) {                        // all (0, 1) first
            soa[b].assign(16 * stride, 0u);
            for (int w = 1; w < 4; w += 2) std::fill_n(soa[b].begin() + (size_t)(4 * w) * stride, stride, kb::R1);
        }
    }
    void set_row(uint32_t i, const Ext* row) { for (int q = 0; q < 16; q++) soa[0][(size_t)q * stride + i] = row[q / 4].c[q % 4]; }
    RoundSums sums(int m, size_t real_pairs) const {
        uint32_t o6[6][4];
        gkr_host_round_sums(soa[side].data(), stride, eq.soa[m].data(), plane_stride((size_t)1 << m), real_pairs, o6);
        RoundSums t;
        Ext* dstp[6] = {&t.x0, &t.y0, &t.xh, &t.yh, &t.e0, &t.es};
        for (int q = 0; q < 6; q++) memcpy(dstp[q]->c, o6[q], 16);
        return t;
    }
    void fold(size_t real_pairs, size_t half, const Ext& alpha) {
        gkr_host_round_fold(soa[side].data(), soa[side ^ 1].data(), stride, real_pairs, alpha.c);
        if (real_pairs < half)                               // the entry behind the last real one is the padding fraction (0, 1) again
            for (int w = 0; w < 4; w++)
                for (int k = 0; k < 4; k++) soa[side ^ 1][(size_t)(4 * w + k) * stride + real_pairs] = (w & 1) && k == 0 ? kb::R1 : 0u;
        side ^= 1;
    }
    void first_row(Ext (&f)[4]) const { for (int q = 0; q < 16; q++) f[q / 4].c[q % 4] = soa[side][(size_t)q * stride]; }
};

// Portable: the sums and the folds of a round run on the helper threads (host_par.hpp); the tables ping-pong because a
// parallel fold cannot be in place.
struct ScalarTables {
    const EqTabs& eq;
    HostPar::Scope& par;
    std::vector<Ext> tab[2][4];
    int side = 0;
    ScalarTables(const EqTabs& eq_, HostPar::Scope& par_, uint32_t W) : eq(eq_), par(par_) {
        for (int w = 0; w < 4; w++) { tab[0][w].assign(W, (w & 1) ? kb::ext_one() : kb::ext_zero()); tab[1][w].resize(W / 2 + 1); }
    }
    void set_row(uint32_t i, const Ext* row) { for (int w = 0; w < 4; w++) tab[0][w][i] = row[w]; }
    RoundSums sums(int m, size_t real_pairs) const {
        const std::vector<Ext>& eqi = eq.tabs[m];
        const Ext *n0 = tab[side][0].data(), *d0 = tab[side][1].data(), *n1 = tab[side][2].data(), *d1 = tab[side][3].data();
        RoundSums parts[HostPar::Scope::MAX_THREADS];
        const int nparts = par.threads();
        for (int q = 0; q < nparts; q++) parts[q] = RoundSums{kb::ext_zero(), kb::ext_zero(), kb::ext_zero(), kb::ext_zero(), kb::ext_zero(), kb::ext_zero()};
        par.run(real_pairs, 24, [&](int part, size_t kb0, size_t ke) {
            RoundSums acc = parts[part];
            for (size_t k = kb0; k < ke; k++) {
                const size_t a = 2 * k, b = 2 * k + 1;
                // lambda is factored out of the sums: sum eq (lambda X + Y) = lambda sum eq X + sum eq Y
                acc.x0 = acc.x0 + eqi[a] * (d0[a] * n1[a] + d1[a] * n0[a]);
                acc.y0 = acc.y0 + eqi[a] * (d0[a] * d1[a]);
                const Ext sn0 = n0[a] + n0[b], sn1 = n1[a] + n1[b], sd0 = d0[a] + d0[b], sd1 = d1[a] + d1[b];
                const Ext es = eqi[a] + eqi[b];
                acc.xh = acc.xh + es * (sd0 * sn1 + sd1 * sn0);
                acc.yh = acc.yh + es * (sd0 * sd1);
                acc.e0 = acc.e0 + eqi[a];
                acc.es = acc.es + es;
            }
            parts[part] = acc;
        });
        RoundSums t = parts[0];
        for (int q = 1; q < nparts; q++) {
            t.x0 = t.x0 + parts[q].x0; t.y0 = t.y0 + parts[q].y0; t.xh = t.xh + parts[q].xh; t.yh = t.yh + parts[q].yh;
            t.e0 = t.e0 + parts[q].e0; t.es = t.es + parts[q].es;
        }
        return t;
    }
    void fold(size_t real_pairs, size_t half, const Ext& alpha) {
        const Ext *n0 = tab[side][0].data(), *d0 = tab[side][1].data(), *n1 = tab[side][2].data(), *d1 = tab[side][3].data();
        Ext *o0 = tab[side ^ 1][0].data(), *o1 = tab[side ^ 1][1].data(), *o2 = tab[side ^ 1][2].data(), *o3 = tab[side ^ 1][3].data();
        par.run(real_pairs, 48, [&](int, size_t kb0, size_t ke) {
            for (size_t k = kb0; k < ke; k++) {
                o0[k] = n0[2 * k] + alpha * (n0[2 * k + 1] - n0[2 * k]); o1[k] = d0[2 * k] + alpha * (d0[2 * k + 1] - d0[2 * k]);
                o2[k] = n1[2 * k] + alpha * (n1[2 * k + 1] - n1[2 * k]); o3[k] = d1[2 * k] + alpha * (d1[2 * k + 1] - d1[2 * k]);
            }
        });
        if (real_pairs < half) { o0[real_pairs] = kb::ext_zero(); o1[real_pairs] = kb::ext_one(); o2[real_pairs] = kb::ext_zero(); o3[real_pairs] = kb::ext_one(); }
        side ^= 1;
    }
    void first_row(Ext (&f)[4]) const { for (int w = 0; w < 4; w++) f[w] = tab[side][w][0]; }
};

// interaction-variable rounds on the host (InteractionLayer, logup_poly.rs:L240-L316); eq_adjustment = PA.
// The eq table is never folded: after binding the last j variables it is eq_scale x the Lagrange table of the
// first niv - j coordinates (an intermediate table of EqTabs::build), and a Lagrange table sums to one,
// which gives the padding entries' share of both sums without visiting them.
template <class Tables>
void interaction_rounds(Tables& tb, size_t real, const std::vector<Ext>& int_point, const Ext& lambda, const Ext& PA, const Consts& k, LayerRounds& lr) {
    const int niv = (int)int_point.size();
    Ext eq_scale = k.one;
    for (int j = 0; j < niv; j++) {                          // entries >= real are the padding fraction (0, 1) in all four tables
        const size_t half = ((size_t)1 << (niv - j)) / 2, real_pairs = (real + 1) / 2;
        const RoundSums t = tb.sums(niv - j, real_pairs);
        const Ext pt = int_point[niv - 1 - j];
        // a pair of padding entries contributes eq[a] * 1 to the first sum and (eq[a] + eq[b]) * (1 + 1)(1 + 1) to the
        // second; over ALL pairs sum eq[a] = 1 - pt and sum (eq[a] + eq[b]) = 1
        const Ext s0 = lambda * t.x0 + t.y0 + ((k.one - pt) - t.e0);
        const Ext sh = lambda * t.xh + t.yh + (k.one - t.es) * k.four;
        const Ext PAe = PA * eq_scale;
        const Ext p0 = PAe * s0, ph = PAe * sh * k.inv8;
        const Ext xs[4] = {k.zero, k.one, k.inv2, (k.one - pt) * kb::ext_inv(k.one - (pt + pt))};
        const Ext ys[4] = {p0, lr.claim - p0, ph, k.zero};
        tb.fold(real_pairs, half, lr.finish_round(interpolate4(xs, ys), pt, eq_scale));
        real = real_pairs;
    }
    Ext f[4];
    tb.first_row(f);
    lr.ro.n0 = f[0]; lr.ro.d0 = f[1]; lr.ro.n1 = f[2]; lr.ro.d1 = f[3];
}

// rows: the layer's last fold, one row (n0, d0, n1, d1) per interaction that has rows, at 4 so[i]; the others stay (0, 1)
void interaction_rounds_host(bool simd, HostPar::Scope& par, const EqTabs& eq, uint32_t W, const std::vector<size_t>& so, const Ext* rows,
                             const std::vector<Ext>& int_point, const Ext& lambda, const Ext& PA, const Consts& k, LayerRounds& lr, GkrTimer& timer) {
    auto run = [&](auto tb) {
        const uint32_t K = (uint32_t)so.size() - 1;
        for (uint32_t i = 0; i < K; i++) if (so[i + 1] != so[i]) tb.set_row(i, rows + 4 * so[i]);
        timer.lap(GkrTimer::ROWS);
        interaction_rounds(tb, K, int_point, lambda, PA, k, lr);
        timer.lap(GkrTimer::INT);
    };
    if (simd) run(PlaneTables(eq, W)); else run(ScalarTables(eq, par, W));
}

// SP1HIP_REQUIRE names the enclosing function; a caller keeps reading the entry point's name from whichever phase refuses
#define SP1HIP_GKR_REQUIRE(cond, msg) \
    do { if (!(cond)) { sp1hip::set_error("sp1hip_logup_gkr_prove: %s", msg); return SP1HIP_ERROR_INVALID_ARGUMENT; } } while (0)

// ================================================================ one proof
// Members are declared in the order the call creates them and are released in reverse. That order matters: RoundSyncHost and
// Mailbox drain the stream (when a publishing kernel may still be in flight after an early error return) BEFORE any DeviceBuf
// declared ahead of them returns its block to the arena and before the PinnedStages hand their blocks on; the cloned challenger
// goes last.
struct GkrProver {
    // the call's arguments (the struct is an aggregate: the entry point fills these, everything else starts empty)
    const sp1hip_gkr_chip_t* const chips;
    const int n_chips, L;
    sp1hip_challenger_t* const challenger;
    uint8_t* const h_proof;
    size_t* const proof_len;
    const sp1hip_stream_t stream;
    const hipStream_t s;

    GkrTimer timer;
    const Consts k;
    std::vector<ChipInfo> info;                              // parse_programs
    std::vector<ParsedInt> progs;
    size_t max_arity = 0, total_cols = 0, need = 0;          // need: bytes of the proof
    uint32_t K = 0, W = 0;                                   // interactions; 2^niv
    int niv = 0;
    struct Cloned { sp1hip_challenger_t* c = nullptr; ~Cloned() { sp1hip_challenger_free(c); } } clone;   // freed on every path
    sp1hip_challenger_t* ch = nullptr;                       // = clone.c: the transcript of this call
    uint32_t witness = 0, flat_max_slots = 0;
    int lookahead = 2;                                       // rounds a flat pass may sum (SP1HIP_GKR_LOOKAHEAD)
    Ext alpha;
    std::vector<Ext> betas;
    std::vector<uint32_t> int_chip;                          // global interaction -> chip
    Levels lv;
    size_t n_passes_total = 0;
    hipStream_t side = nullptr;
    hipEvent_t* side_ev = nullptr;
    DeviceBuf d_all, d_flat;                                 // every pass's descriptors and FLAT slot index (plan.all_descs, plan.flat_index)
    PinnedStage side_stage, stage;                           // small uploads (round_sync.hpp) on `side` and on `s`
    DeviceBuf d_progs, d_betas, d_descs;
    std::vector<uint32_t> flat;                              // upload sources live to the end of the call
    std::vector<IntDesc> descs;
    DeviceBuf d_trans, d_trans2;
    Mailbox mb;                                              // device -> host hand-overs outside the sumcheck rounds
    DeviceBuf d_eq_int, d_T, d_TL, d_partials, scratch[2];
    bool direct_final = false, simd = false;                 // a layer's last fold goes straight to the mailbox slot | AVX-512 host rounds
    PassPlan plan;
    std::vector<Ext> out_n, out_d, eval_point;               // circuit output; the point of the current claims (num_eval, den_eval)
    Ext num_eval, den_eval;
    size_t launch_idx = 0;                                   // next pass: plan.shapes[launch_idx], K descriptors of d_all
    RoundSyncHost rsync;
    std::optional<HostPar::Scope> par;                       // helper threads for the host loops between hand-overs (made when the layers start)
    std::vector<RoundOut> rounds;
    std::vector<Ext> trace_point, openings;

    // ---- parse the interaction programs (host words -> Montgomery device words), gather shapes
    int parse_programs() {
        info.resize(n_chips);
        for (int c = 0; c < n_chips; c++) {
            const sp1hip_gkr_chip_t& ci = chips[c];
            SP1HIP_GKR_REQUIRE(ci.name && ci.interactions, "null chip field");
            SP1HIP_GKR_REQUIRE(ci.real_rows <= ((uint64_t)1 << L), "chip taller than 2^max_log_row_count");
            SP1HIP_GKR_REQUIRE(ci.real_rows == 0 || ci.main_width == 0 || ci.d_main, "null main trace");
            SP1HIP_GKR_REQUIRE(ci.real_rows == 0 || ci.prep_width == 0 || ci.d_prep, "null preprocessed trace");
            if (c) SP1HIP_GKR_REQUIRE(strcmp(chips[c - 1].name, ci.name) < 0, "chips must be sorted by name (BTreeSet order)");
            info[c] = ChipInfo{ci.name, (uint32_t)ci.real_rows, 0, ci.main_width, ci.prep_width, (uint32_t)progs.size(), ci.d_main, ci.d_prep};
            const uint32_t* p = ci.interactions;
            const uint32_t* end = p + ci.n_words;
            SP1HIP_GKR_REQUIRE(ci.n_words >= 1, "empty interaction program");
            const uint32_t ni = *p++;
            info[c].k = ni;
            auto vcol = [&](std::vector<uint32_t>& out) -> bool {
                if (p + 2 > end) return false;
                const uint32_t nt = p[0];
                if (p[1] >= kb::P || p + 2 + 3 * (size_t)nt > end) return false;
                out.push_back(nt);
                out.push_back(kb::to_monty(p[1]));
                p += 2;
                for (uint32_t t = 0; t < nt; t++, p += 3) {
                    if (p[0] > 1 || p[2] >= kb::P) return false;
                    if (p[1] >= (p[0] ? ci.main_width : ci.prep_width)) return false;
                    out.push_back(p[0]); out.push_back(p[1]); out.push_back(kb::to_monty(p[2]));
                }
                return true;
            };
            for (uint32_t i = 0; i < ni; i++) {
                SP1HIP_GKR_REQUIRE(p + 3 <= end, "truncated interaction program");
                const uint32_t nv = p[2];
                SP1HIP_GKR_REQUIRE(p[0] <= 1 && p[1] < kb::P && nv < 4096, "bad interaction header");      // (the Keccak bus carries 106 values per message)
                ParsedInt pi{p[0], p[1], {}, std::vector<std::vector<uint32_t>>(nv)};
                p += 3;
                SP1HIP_GKR_REQUIRE(vcol(pi.mult), "bad multiplicity column");
                for (uint32_t j = 0; j < nv; j++) SP1HIP_GKR_REQUIRE(vcol(pi.values[j]), "bad value column (index or weight out of range)");
                max_arity = std::max<size_t>(max_arity, nv + 1);
                progs.push_back(std::move(pi));
            }
            SP1HIP_GKR_REQUIRE(p == end, "trailing words in interaction program");
            total_cols += (size_t)ci.main_width + ci.prep_width;
        }
        K = (uint32_t)progs.size();
        SP1HIP_GKR_REQUIRE(K >= 1, "no interactions in the shard");
        niv = log2_ceil(K);
        W = 1u << niv;
        return SP1HIP_SUCCESS;
    }

    // ---- proof size (everything is determined by the shapes)
    size_t proof_size() const {
        size_t n = 2 * (8 + (size_t)2 * W * 16 + 24) + 8;
        for (int v = 1; v <= L - 1; v++) n += 64 + 8 + (size_t)(niv + v) * (8 + 64) + 16 + 8 + (size_t)(niv + v) * 16 + 16;
        n += 8 + (size_t)L * 16 + 8;
        for (int c = 0; c < n_chips; c++) {
            n += 8 + info[c].name.size() + 8 + (size_t)info[c].main_w * 16 + 16 + 1;
            if (info[c].prep_w) n += 8 + (size_t)info[c].prep_w * 16 + 16;
        }
        return n + 4;
    }

    // ---- transcript head (prover.rs:L86-L95), on a clone: the caller's challenger only moves when the proof is produced
    int transcript_head() {
        SP1HIP_TRY(sp1hip_challenger_clone(challenger, &clone.c));
        ch = clone.c;
        SP1HIP_TRY(sp1hip_challenger_grind(ch, 12, &witness, stream));
        alpha = challenger_sample_ext(ch);
        std::vector<Ext> beta_seed(log2_ceil(max_arity));
        for (auto& b : beta_seed) b = challenger_sample_ext(ch);
        (void)challenger_sample_ext(ch);                     // _pv_challenge
        betas = partial_lagrange_host(beta_seed);
        return SP1HIP_SUCCESS;
    }

    // ---- device storage: the tree's levels; the buffers of the pass descriptors
    int alloc_levels_and_plan_buffers() {
        int_chip.resize(K);
        std::vector<uint32_t> rows(K);
        for (int c = 0; c < n_chips; c++) for (uint32_t i = 0; i < info[c].k; i++) { int_chip[info[c].int0 + i] = c; rows[info[c].int0 + i] = info[c].rows; }
        SP1HIP_TRY(lv.alloc(L, std::move(rows), s));
        timer.mark("parse + level buffers");
        // The pass descriptors (~10 MB at 730 interactions) go up on the caller's SIDE stream while the first layer and the
        // fraction tree run: on `s` the copy sat between the last tree kernel and the first hand-over (0.2 ms of an idle GPU).
        // Their buffer is taken from the arena HERE, before anything of this call is enqueued, and the side stream waits for
        // this point of `s` — a recycled block's previous user is then out of the way (the arena orders reuse by stream).
        flat_max_slots = (uint32_t)env_uint("SP1HIP_GKR_FLAT_SLOTS", 65536);   // read per call (tests)
        // rounds per flat pass: 2 = the two-round plan; 3 / 4 = fewer, deeper passes in the latency-bound tails (choose_pass)
        lookahead = (int)std::min<uint64_t>(std::max<uint64_t>(env_uint("SP1HIP_GKR_LOOKAHEAD", GKR_LOOKAHEAD_DEFAULT), 2), 4);   // read per call (tests)
        n_passes_total = count_passes(lv, flat_max_slots, lookahead);
        SP1HIP_TRY(aux_stream_for(s, 2, &side, &side_ev));
        // (their buffers come from the SIDE stream's share of the arena: a recycled block's previous user ran on that stream,
        // so the copies need not wait for anything on `s`; the blocks go back when this call has seen its last result)
        SP1HIP_TRY(d_all.alloc(std::max<size_t>(n_passes_total * K, 1) * sizeof(PassDesc), side));
        SP1HIP_TRY(d_flat.alloc((n_passes_total * (size_t)flat_max_slots + 4) * sizeof(uint16_t), side));    // a flat pass indexes <= flat_max_slots slots
        SP1HIP_TRY(side_stage.init(side));
        return stage.init(s);
    }

    // ---- first layer and fraction tree: every launch enqueued back to back
    int build_first_layer_and_tree() {
        // device programs (see first_layer_kernel): the row-independent part of every denominator is folded into `head` here
        std::vector<size_t> poff(K);
        for (uint32_t i = 0; i < K; i++) {
            poff[i] = flat.size();
            const ParsedInt& pi = progs[i];
            Ext head = alpha + kb::ext_mul_base(betas[0], kb::to_monty(pi.kind));
            uint32_t live = 0;
            for (size_t j = 0; j < pi.values.size(); j++) {
                if (pi.values[j][0] == 0) head = head + kb::ext_mul_base(betas[1 + j], pi.values[j][1]);   // no terms: the constant
                else live++;
            }
            flat.insert(flat.end(), {pi.is_send, live, head.c[0], head.c[1], head.c[2], head.c[3]});
            flat.insert(flat.end(), pi.mult.begin(), pi.mult.end());
            for (size_t j = 0; j < pi.values.size(); j++) {
                if (pi.values[j][0] == 0) continue;
                flat.push_back((uint32_t)(1 + j));
                flat.insert(flat.end(), pi.values[j].begin(), pi.values[j].end());
            }
        }
        SP1HIP_TRY(upload(d_progs, flat.data(), flat.size() * 4, s, stage));
        SP1HIP_TRY(upload(d_betas, betas.data(), betas.size() * 16, s, stage));
        uint32_t max_rows = 0;
        descs.resize(K);
        for (uint32_t i = 0; i < K; i++) {
            const ChipInfo& c = info[int_chip[i]];
            descs[i] = IntDesc{d_progs.u32() + poff[i], c.d_main, c.d_prep, c.rows, (uint32_t*)lv.n_ptr(L, i), lv.d_ptr(L, i)};
            max_rows = std::max(max_rows, c.rows);
        }
        // L >= 3: the first layer and the two levels below it come out of ONE pass over the traces (first_layers_kernel), the
        // rest of the tree two levels per launch (transition2_kernel; a last single level by transition_kernel). SP1HIP_GKR_FUSED=0:
        // the separate kernels (first_layer_kernel, one transition launch per level) — same words in every level (tests)
        const bool fused_tree = L >= 3 && env_flag("SP1HIP_GKR_FUSED", true);
        if (fused_tree) {
            std::vector<FirstDesc> fdescs(K);
            for (uint32_t i = 0; i < K; i++)
                fdescs[i] = FirstDesc{descs[i].prog, descs[i].main, descs[i].prep, descs[i].rows, descs[i].n_out, descs[i].d_out,
                                      (Ext*)lv.n_ptr(L - 1, i), lv.d_ptr(L - 1, i), (Ext*)lv.n_ptr(L - 2, i), lv.d_ptr(L - 2, i)};
            SP1HIP_TRY(upload(d_descs, fdescs.data(), fdescs.size() * sizeof(FirstDesc), s, stage));
            if (max_rows) {
                ScopedTimer t("gkr_first_layer", s);
                hipLaunchKernelGGL(first_layers_kernel, dim3(tiles_for((max_rows + 3) / 4), K), dim3(256), 0, s, (const FirstDesc*)d_descs.p,
                                   (const Ext*)d_betas.p);
                SP1HIP_LAUNCH_CHECK();
            }
        } else {
            SP1HIP_TRY(upload(d_descs, descs.data(), descs.size() * sizeof(IntDesc), s, stage));
            if (max_rows) {
                ScopedTimer t("gkr_first_layer", s);
                hipLaunchKernelGGL(first_layer_kernel, dim3(tiles_for(max_rows), K), dim3(256), 0, s, (const IntDesc*)d_descs.p,
                                   (const Ext*)d_betas.p);
                SP1HIP_LAUNCH_CHECK();
            }
        }
        timer.mark("first layer enqueued");
        // every level's descriptors are planned and uploaded once: the tree is built by back-to-back launches
        const int top = fused_tree ? L - 2 : L;              // the highest level that still has to be combined downwards
        std::vector<Trans2Desc> t2;                          // launches (top -> top - 2), (top - 2 -> top - 4), ...
        std::vector<TransDesc> t1;                           // then at most one single level (or, unfused, every level)
        std::vector<uint32_t> t2_mr, t1_mr;
        std::vector<int> t1_level;
        int l = top;
        if (fused_tree)
            for (; l >= 3; l -= 2) {
                uint32_t mr = 0;
                for (uint32_t i = 0; i < K; i++) {
                    const uint32_t rin = lv.rows_at(i, l);
                    t2.push_back(Trans2Desc{(const Ext*)lv.n_ptr(l, i), lv.d_ptr(l, i), (Ext*)lv.n_ptr(l - 1, i), lv.d_ptr(l - 1, i), (Ext*)lv.n_ptr(l - 2, i), lv.d_ptr(l - 2, i), rin});
                    mr = std::max(mr, (rin + 3) / 4);
                }
                t2_mr.push_back(mr);
            }
        for (; l >= 2; l--) {
            uint32_t mr = 0;
            for (uint32_t i = 0; i < K; i++) {
                const uint32_t rin = lv.rows_at(i, l);
                t1.push_back(TransDesc{lv.n_ptr(l, i), lv.d_ptr(l, i), (Ext*)lv.n_ptr(l - 1, i), lv.d_ptr(l - 1, i), rin});
                mr = std::max(mr, (rin + 1) / 2);
            }
            t1_mr.push_back(mr);
            t1_level.push_back(l);
        }
        if (!t2.empty()) SP1HIP_TRY(upload(d_trans2, t2.data(), t2.size() * sizeof(Trans2Desc), s, stage));
        if (!t1.empty()) SP1HIP_TRY(upload(d_trans, t1.data(), t1.size() * sizeof(TransDesc), s, stage));
        for (size_t j = 0; j < t2_mr.size(); j++) {
            if (!t2_mr[j]) continue;
            ScopedTimer t("gkr_transition", s);
            hipLaunchKernelGGL(transition2_kernel, dim3(tiles_for(t2_mr[j]), K), dim3(256), 0, s, (const Trans2Desc*)d_trans2.p + j * K);
            SP1HIP_LAUNCH_CHECK();
        }
        for (size_t j = 0; j < t1_mr.size(); j++) {
            if (!t1_mr[j]) continue;
            const TransDesc* d_t = (const TransDesc*)d_trans.p + j * K;
            ScopedTimer t("gkr_transition", s);
            if (t1_level[j] == L) hipLaunchKernelGGL(transition_kernel<true>, dim3(tiles_for(t1_mr[j]), K), dim3(256), 0, s, d_t);
            else hipLaunchKernelGGL(transition_kernel<false>, dim3(tiles_for(t1_mr[j]), K), dim3(256), 0, s, d_t);
            SP1HIP_LAUNCH_CHECK();
        }
        timer.mark("tree enqueued");
        return SP1HIP_SUCCESS;
    }

    // ---- the layers' buffers, then the descriptors of every pass. They depend on shapes only: they are planned and uploaded WHILE
    // the GPU builds the first layer and the fraction tree, i.e. after the tree has been enqueued and before the first hand-over —
    // milliseconds of host work at 730 interactions x ~130 passes that would otherwise sit on the critical path behind it
    int plan_and_upload_passes() {
        SP1HIP_TRY(mb.init(s));
        SP1HIP_TRY(d_eq_int.alloc((size_t)W * 16, s));
        SP1HIP_TRY(d_T.alloc(((size_t)2 << std::max(L - 1, 1)) * 16, s));
        SP1HIP_TRY(d_TL.alloc(((size_t)2 << std::max(L - 1, 1)) * 16, s));
        // folded tables: 4 vectors per interaction, at most ceil(rows(level v+1) / 4) entries each after the first fold
        size_t scratch_entries = 0;
        for (uint32_t i = 0; i < K; i++) scratch_entries += (lv.rows_at(i, L) + 3) / 4 + 1;
        for (int b = 0; b < 2; b++) SP1HIP_TRY(scratch[b].alloc(std::max<size_t>(scratch_entries, 1) * 64, s));
        // a layer's last fold (one row per interaction) goes straight to the mailbox slot, 16-byte aligned behind word 0
        direct_final = (size_t)K * 16 + 4 <= MAILBOX_WORDS;
        Ext* const scratch_ext[2] = {scratch[0].ext(), scratch[1].ext()};
        plan_passes(lv, flat_max_slots, lookahead, n_passes_total, scratch_ext, direct_final ? reinterpret_cast<Ext*>(mb.h_slot + 4) : nullptr, plan);
        {   // partial sums: one slot per workgroup of a launch, 16 bytes per sum it hands over
            size_t bytes = 160;
            for (auto& sh : plan.shapes) {
                bytes = std::max(bytes, (size_t)sh.tiles * 16 * pass_sums(sh.sv));
                SP1HIP_GKR_REQUIRE(sh.flat || (sh.fv <= 2 && sh.sv <= 2), "internal error: a deep pass that is not flat");
            }
            SP1HIP_TRY(d_partials.alloc(bytes, s));
        }
        timer.mark("pass descriptors planned");
        if (timer.on) {
            size_t deep = 0;
            for (auto& sh : plan.shapes) deep += sh.fv > 2 || sh.sv > 2;
            fprintf(stderr, "[sp1hip gkr] %zu passes at look-ahead %d, of which %zu deep\n", plan.shapes.size(), lookahead, deep);
        }
        SP1HIP_GKR_REQUIRE(plan.all_descs.size() == n_passes_total * K, "internal error: pass count");
        SP1HIP_TRY(side_stage.upload(d_all.p, plan.all_descs.data(), plan.all_descs.size() * sizeof(PassDesc)));
        SP1HIP_GKR_REQUIRE(plan.flat_index.size() * sizeof(uint16_t) <= d_flat.n, "internal error: flat index size");
        SP1HIP_TRY(side_stage.upload(d_flat.p, plan.flat_index.data(), plan.flat_index.size() * sizeof(uint16_t)));
        SP1HIP_HIP(hipEventRecord(side_ev[1], side));
        SP1HIP_HIP(hipStreamWaitEvent(s, side_ev[1], 0));    // (enqueued behind the tree: the copies have long finished by then)
        timer.mark("pass descriptors uploaded");
        return SP1HIP_SUCCESS;
    }

    // ---- circuit output = level 1 (<= 2 rows per interaction): index 2 i + r, padding (0, 1); the first evaluation claims
    int fetch_circuit_output() {
        out_n.assign(2 * (size_t)W, kb::ext_zero()); out_d.assign(2 * (size_t)W, kb::ext_one());
        std::vector<Ext> hn(std::max<size_t>(lv.entries[1], 1)), hd(std::max<size_t>(lv.entries[1], 1));
        if (L >= 2) {
            SP1HIP_TRY(mb.fetch(lv.N[1].p, lv.entries[1] * 4, hn.data()));
        } else {                                             // L == 1: level 1 is the first layer itself (base numerators)
            std::vector<uint32_t> hb(std::max<size_t>(lv.entries[1], 1));
            SP1HIP_TRY(mb.fetch(lv.N[1].p, lv.entries[1], hb.data()));
            for (size_t e = 0; e < lv.entries[1]; e++) hn[e] = kb::ext_from_base(hb[e]);
        }
        SP1HIP_TRY(mb.fetch(lv.D[1].p, lv.entries[1] * 4, hd.data()));
        for (uint32_t i = 0; i < K; i++)
            for (uint32_t r = 0; r < lv.rows_at(i, 1); r++) { out_n[2 * i + r] = hn[lv.off[1][i] + r]; out_d[2 * i + r] = hd[lv.off[1][i] + r]; }
        timer.mark("circuit output fetched");
        challenger_observe(ch, kb::to_monty(2 * W));
        for (auto& e : out_n) observe_ext(ch, e);
        challenger_observe(ch, kb::to_monty(2 * W));
        for (auto& e : out_d) observe_ext(ch, e);
        eval_point.resize(niv + 1);
        for (auto& z : eval_point) z = challenger_sample_ext(ch);
        num_eval = eval_mle_host(out_n, eval_point); den_eval = eval_mle_host(out_d, eval_point);
        return SP1HIP_SUCCESS;
    }

    // ---- one pass of layer v: plan.shapes[idx], t_after = row variables left once it has folded; c0, c1 = the challenges it folds with
#define SP1HIP_GKR_PASS(FV, SV, F, NB, FL) hipLaunchKernelGGL((gkr_pass<FV, SV, F, NB, FL>), dim3(shape.tiles), dim3(256), 0, s, d_descs, (const Ext*)d_eq_int.p, Tp, TLp, c0, c1, d_partials.u32(), rs, publish_rows ? mb.seq + 1 : rsync.seq, K, shape.tile_size, fa)
#define SP1HIP_GKR_PASS_FL(FV, SV, F, NB) do { if (shape.flat) SP1HIP_GKR_PASS(FV, SV, F, NB, true); else SP1HIP_GKR_PASS(FV, SV, F, NB, false); } while (0)
#define SP1HIP_GKR_PASS_SRC(FV, SV) do { if (nbase) SP1HIP_GKR_PASS_FL(FV, SV, true, true); else if (shape.first) SP1HIP_GKR_PASS_FL(FV, SV, true, false); else SP1HIP_GKR_PASS_FL(FV, SV, false, false); } while (0)
#define SP1HIP_GKR_DEEP_K(FV, SV, F, NB) hipLaunchKernelGGL((SP1HIP_GKR_DEEP_NAME(FV)<FV, SV, F, NB>), dim3(shape.tiles), dim3(256), 0, s, d_descs, (const Ext*)d_eq_int.p, Tp, TLp, ch, d_partials.u32(), rs, seq, fa)
#define SP1HIP_GKR_DEEP_NAME(FV) SP1HIP_GKR_DEEP_NAME_##FV
#define SP1HIP_GKR_DEEP_NAME_0 gkr_pass_deep
#define SP1HIP_GKR_DEEP_NAME_2 gkr_pass_deep
#define SP1HIP_GKR_DEEP_NAME_3 gkr_pass_deep_fold
#define SP1HIP_GKR_DEEP_NAME_4 gkr_pass_deep_fold
#define SP1HIP_GKR_DEEP_FIRST(FV, SV) else if (fv == FV && sv == SV) { if (nbase) SP1HIP_GKR_DEEP_K(FV, SV, true, true); else SP1HIP_GKR_DEEP_K(FV, SV, true, false); }
#define SP1HIP_GKR_DEEP(FV, SV) else if (fv == FV && sv == SV) { if (nbase) SP1HIP_GKR_DEEP_K(FV, SV, true, true); else if (shape.first) SP1HIP_GKR_DEEP_K(FV, SV, true, false); else SP1HIP_GKR_DEEP_K(FV, SV, false, false); }
    int launch_pass(size_t idx, int v, int t_after, const Ext (&a)[4]) {
        const Ext &c0 = a[0], &c1 = a[1];
        const PassShape shape = plan.shapes[idx];
        const PassDesc* d_descs = (const PassDesc*)d_all.p + idx * K;
        const int fv = shape.fv, sv = shape.sv;
        const FlatArgs fa{(const uint16_t*)d_flat.p + shape.flat_off, shape.total_slots};
        const bool nbase = shape.first && v + 1 == L;
        const bool publish_rows = sv == 0 && direct_final;
        if (publish_rows) { rsync.pending = true; mb.pending = true; }       // (an early error return must drain the stream first)
        const RoundSync rs = sv > 0 ? rsync.next() : publish_rows ? RoundSync{rsync.d_counter, (volatile uint32_t*)mb.h_slot} : RoundSync{};
        // table t of d_T / d_TL (eq_layer_tables_kernel) starts at 2^t - 1
        const Ext* Tp = sv > 0 ? d_T.ext() + (((size_t)1 << (t_after - sv)) - 1) : (const Ext*)nullptr;
        const Ext* TLp = sv > 0 ? d_TL.ext() + (((size_t)1 << (t_after - sv)) - 1) : (const Ext*)nullptr;
        ScopedTimer tm(fv == 0 ? "gkr_pass_sum" : sv == 0 ? "gkr_pass_fold" : "gkr_pass_fold_sum", s);
        if (fv > 2 || sv > 2) {                              // up to four rounds per pass: flat launches only (choose_pass)
            const DeepChallenges ch{{a[0], a[1], a[2], a[3]}};
            const uint32_t seq = publish_rows ? mb.seq + 1 : rsync.seq;
            if (false) {}
            SP1HIP_GKR_DEEP_FIRST(0, 3) SP1HIP_GKR_DEEP_FIRST(0, 4)
            SP1HIP_GKR_DEEP(2, 3) SP1HIP_GKR_DEEP(2, 4)
            SP1HIP_GKR_DEEP(3, 0) SP1HIP_GKR_DEEP(3, 1) SP1HIP_GKR_DEEP(3, 2) SP1HIP_GKR_DEEP(3, 3)
            SP1HIP_GKR_DEEP(4, 0) SP1HIP_GKR_DEEP(4, 1) SP1HIP_GKR_DEEP(4, 2) SP1HIP_GKR_DEEP(4, 3) SP1HIP_GKR_DEEP(4, 4)
            else { set_error("internal error: GKR pass shape (%d, %d)", fv, sv); return SP1HIP_ERROR_RUNTIME; }
            SP1HIP_LAUNCH_CHECK();
            return SP1HIP_SUCCESS;
        }
        if (fv == 0 && sv == 2) { if (nbase) SP1HIP_GKR_PASS_FL(0, 2, true, true); else SP1HIP_GKR_PASS_FL(0, 2, true, false); }
        else if (fv == 0 && sv == 1) { if (nbase) SP1HIP_GKR_PASS_FL(0, 1, true, true); else SP1HIP_GKR_PASS_FL(0, 1, true, false); }
        else if (fv == 2 && sv == 2) SP1HIP_GKR_PASS_SRC(2, 2);
        else if (fv == 2 && sv == 1) SP1HIP_GKR_PASS_SRC(2, 1);
        else if (fv == 2 && sv == 0) SP1HIP_GKR_PASS_SRC(2, 0);
        else if (fv == 1 && sv == 0) SP1HIP_GKR_PASS_SRC(1, 0);
        else { set_error("internal error: GKR pass shape (%d, %d)", fv, sv); return SP1HIP_ERROR_RUNTIME; }
        SP1HIP_LAUNCH_CHECK();
        return SP1HIP_SUCCESS;
    }
#undef SP1HIP_GKR_DEEP
#undef SP1HIP_GKR_DEEP_FIRST
#undef SP1HIP_GKR_DEEP_K
#undef SP1HIP_GKR_DEEP_NAME
#undef SP1HIP_GKR_DEEP_NAME_0
#undef SP1HIP_GKR_DEEP_NAME_2
#undef SP1HIP_GKR_DEEP_NAME_3
#undef SP1HIP_GKR_DEEP_NAME_4
#undef SP1HIP_GKR_PASS_SRC
#undef SP1HIP_GKR_PASS_FL
#undef SP1HIP_GKR_PASS

    // ---- GKR layer v (reads level v + 1): the row rounds on the device, two per pass, then the interaction rounds on the host
    int prove_layer(int v) {
        timer.lap(GkrTimer::LAYER_HEAD);
        const Ext lambda = challenger_sample_ext(ch);
        LayerRounds lr{ch, {}, {}, num_eval * lambda + den_eval};
        lr.ro.claimed_sum = lr.claim;
        const std::vector<Ext> int_point(eval_point.begin(), eval_point.begin() + niv), row_point(eval_point.begin() + niv, eval_point.end());
        // the device builds its own tables: eq over the interaction point, and over every prefix of the row point (x 1 and x lambda)
        SP1HIP_GKR_REQUIRE(niv <= 32 && v <= 32, "point too long");
        {
            PointArg pi{}, pa{};
            for (int j = 0; j < niv; j++) pi.c[j] = int_point[j];
            for (int j = 0; j < v; j++) pa.c[j] = row_point[j];
            const uint32_t full_blocks = (W + 255) / 256, prefix_blocks = ((2u << v) + 255) / 256;
            hipLaunchKernelGGL(eq_layer_tables_kernel, dim3(full_blocks + prefix_blocks), dim3(256), 0, s, pi, niv, d_eq_int.ext(), full_blocks, pa, v,
                               lambda, d_T.ext(), d_TL.ext());
            SP1HIP_LAUNCH_CHECK();
        }
        EqTabs eq_tabs;                                      // built lazily, after the first pass of the layer has been launched
        Ext PA = k.one;                                      // eq factor of the row variables bound so far
        Ext a[4] = {k.zero, k.zero, k.zero, k.zero};         // the challenges the next pass folds with
        int folds = 0;                                       // folding passes so far: they alternate scratch[0], [1], ...
        auto finish = [&lr](const Poly4& poly, const Ext& pt, Ext& eq_factor) { return lr.finish_round(poly, pt, eq_factor); };
        int t = v;                                           // row variables not yet bound by a FOLD
        for (bool first_pass = true;; first_pass = false) {  // the passes of the layer (two rounds each; up to four where flat)
            const size_t idx = launch_idx++;
            const int fv = plan.shapes[idx].fv, sv = plan.shapes[idx].sv;
            t -= fv;                                         // variables left once this pass has folded
            folds += fv > 0;
            if (!simd && t == sv) par->wake();               // the helpers' wake-up hides behind the layer's last two passes
            timer.lap(first_pass ? GkrTimer::SKIP : GkrTimer::HOST);   // closed forms + transcript since the last hand-over
            SP1HIP_TRY(launch_pass(idx, v, t, a));
            timer.lap(GkrTimer::LAUNCH);
            if (first_pass) eq_tabs.build(int_point, simd);  // host work behind a running kernel
            if (sv == 0) break;
            const int ns = pass_sums(sv);
            uint32_t h_sums[4 * pass_sums(gkr_rounds::GRID_MAX_K)];
            timer.lap(GkrTimer::SKIP);
            SP1HIP_TRY(rsync.wait(h_sums, 4 * ns));
            timer.lap(GkrTimer::WAIT);
            Ext S[pass_sums(gkr_rounds::GRID_MAX_K)];
            memcpy(S, h_sums, 16 * (size_t)ns);
            if (fv <= 2 && sv <= 2) gkr_rounds::row_rounds_closed_form(sv, S, row_point.data(), t, PA, finish, a);
            else gkr_rounds::row_rounds_from_grid(sv, S, row_point.data(), t, PA, finish, a);
        }
        // the layer's last fold left one row per interaction: dense over 2^niv on the host
        std::vector<size_t> so(K + 1, 0);
        for (uint32_t i = 0; i < K; i++) so[i + 1] = so[i] + (lv.rows_at(i, v + 1) ? 1 : 0);     // (a chip without rows stays (0, 1))
        const size_t final_rows_total = so[K];
        const int cur = (folds - 1) & 1;                     // where the last fold wrote
        std::vector<Ext> host(std::max<size_t>(final_rows_total, 1) * 4);
        if (direct_final) { SP1HIP_TRY(mb.wait_next(host.data(), final_rows_total * 16, 4)); rsync.pending = false; }
        else SP1HIP_TRY(mb.fetch(scratch[cur].p, final_rows_total * 16, host.data()));
        interaction_rounds_host(simd, *par, eq_tabs, W, so, host.data(), int_point, lambda, PA, k, lr, timer);
        RoundOut& ro = lr.ro;
        ro.eval = lr.claim;
        ro.point.assign(lr.alphas.rbegin(), lr.alphas.rend());
        observe_ext(ch, ro.n0); observe_ext(ch, ro.n1); observe_ext(ch, ro.d0); observe_ext(ch, ro.d1);
        eval_point = ro.point;
        const Ext lc = challenger_sample_ext(ch);
        num_eval = ro.n0 + (ro.n1 - ro.n0) * lc;
        den_eval = ro.d0 + (ro.d1 - ro.d0) * lc;
        eval_point.push_back(lc);
        rounds.push_back(std::move(ro));
        par->park();
        return SP1HIP_SUCCESS;
    }

    // ---- GKR rounds, layer v = 1 .. L-1
    int prove_layers() {
        SP1HIP_TRY(rsync.init(s));
        simd = gkr_host_simd_available();
        par.emplace();
        par->park();                                         // asleep through the device rounds; woken ahead of each layer's host rounds
        for (int v = 1; v <= L - 1; v++) SP1HIP_TRY(prove_layer(v));
        timer.report_layers();
        timer.mark("all layers");
        return SP1HIP_SUCCESS;
    }

    // ---- trace openings at the last L coordinates
    int open_traces() {
        trace_point.assign(eval_point.end() - L, eval_point.end());
        openings.assign(std::max<size_t>(total_cols, 1), kb::ext_zero());
        if (!total_cols) return SP1HIP_SUCCESS;
        DeviceBuf d_eq, d_od, d_part, d_res;
        SP1HIP_TRY(d_eq.alloc(((size_t)16) << L, s));
        SP1HIP_TRY(sp1hip_partial_lagrange(reinterpret_cast<const sp1hip_ext_t*>(trace_point.data()), L, d_eq.u32(), stream));
        std::vector<OpenDesc> od;
        uint32_t out0 = 0, max_rows_open = 0;
        for (int c = 0; c < n_chips; c++) {
            // proof order per chip: main evaluations, then preprocessed; opening slots: [main | prep]
            for (uint32_t g = 0; g < info[c].main_w; g += OPEN_COLS) od.push_back(OpenDesc{info[c].d_main, info[c].rows, info[c].main_w, g, out0 + g});
            out0 += info[c].main_w;
            for (uint32_t g = 0; g < info[c].prep_w; g += OPEN_COLS) od.push_back(OpenDesc{info[c].d_prep, info[c].rows, info[c].prep_w, g, out0 + g});
            out0 += info[c].prep_w;
            max_rows_open = std::max(max_rows_open, info[c].rows);
        }
        const uint32_t chunks = std::max<uint32_t>((max_rows_open + OPEN_ROWS - 1) / OPEN_ROWS, 1);
        SP1HIP_TRY(upload(d_od, od.data(), od.size() * sizeof(OpenDesc), s, stage));
        SP1HIP_TRY(d_part.alloc((size_t)chunks * total_cols * 16, s));
        SP1HIP_TRY(d_res.alloc(total_cols * 16, s));
        SP1HIP_HIP(hipMemsetAsync(d_part.p, 0, (size_t)chunks * total_cols * 16, s));
        ScopedTimer t("gkr_openings", s);
        hipLaunchKernelGGL(open_columns_kernel, dim3((uint32_t)od.size(), chunks), dim3(256), 0, s, (const OpenDesc*)d_od.p, d_eq.u32(),
                           1u << L, d_part.u32(), (uint32_t)total_cols);
        SP1HIP_LAUNCH_CHECK();
        hipLaunchKernelGGL(open_sum_kernel, dim3(((uint32_t)total_cols * 4 + 63) / 64), dim3(256), 0, s, d_part.u32(), chunks,
                           (uint32_t)total_cols * 4, d_res.u32());
        SP1HIP_LAUNCH_CHECK();
        return mb.fetch(d_res.p, total_cols * 4, openings.data());
    }

    void observe_openings() {
        challenger_observe(ch, kb::to_monty((uint32_t)n_chips));
        size_t o = 0;
        for (int c = 0; c < n_chips; c++) {
            const Ext* main = openings.data() + o;
            const Ext* prep = main + info[c].main_w;
            if (info[c].prep_w) {
                challenger_observe(ch, kb::to_monty(info[c].prep_w));
                for (uint32_t j = 0; j < info[c].prep_w; j++) observe_ext(ch, prep[j]);
            }
            challenger_observe(ch, kb::to_monty(info[c].main_w));
            for (uint32_t j = 0; j < info[c].main_w; j++) observe_ext(ch, main[j]);
            o += info[c].main_w + info[c].prep_w;
        }
        timer.mark("openings");
    }

    // ---- bincode(LogupGkrProof)
    int write_proof() {
        Bytes w;
        for (const std::vector<Ext>* vv : {&out_n, &out_d}) {
            w.u64(vv->size());
            for (auto& e : *vv) w.ext(e);
            w.u64(2); w.u64(vv->size()); w.u64(1);
        }
        w.u64(rounds.size());
        for (auto& r : rounds) {
            w.ext(r.n0); w.ext(r.n1); w.ext(r.d0); w.ext(r.d1);
            w.u64(r.polys.size());
            for (auto& p : r.polys) { w.u64(4); for (auto& c : p) w.ext(c); }
            w.ext(r.claimed_sum);
            w.u64(r.point.size());
            for (auto& x : r.point) w.ext(x);
            w.ext(r.eval);
        }
        w.u64(trace_point.size());
        for (auto& x : trace_point) w.ext(x);
        w.u64(n_chips);
        size_t o = 0;
        for (int c = 0; c < n_chips; c++) {
            w.u64(info[c].name.size());
            for (char chr : info[c].name) w.b.push_back((uint8_t)chr);
            w.u64(info[c].main_w);
            for (uint32_t j = 0; j < info[c].main_w; j++) w.ext(openings[o + j]);
            w.u64(1); w.u64(info[c].main_w);
            w.b.push_back(info[c].prep_w ? 1 : 0);
            if (info[c].prep_w) {
                w.u64(info[c].prep_w);
                for (uint32_t j = 0; j < info[c].prep_w; j++) w.ext(openings[o + info[c].main_w + j]);
                w.u64(1); w.u64(info[c].prep_w);
            }
            o += info[c].main_w + info[c].prep_w;
        }
        w.felt(witness);
        if (w.b.size() != need) {
            set_error("internal error: GKR proof size %zu != expected %zu", w.b.size(), need);
            return SP1HIP_ERROR_RUNTIME;
        }
        memcpy(h_proof, w.b.data(), w.b.size());
        *proof_len = w.b.size();
        return SP1HIP_SUCCESS;
    }

    int prove() {
        timer.start();
        SP1HIP_TRY(parse_programs());
        need = proof_size();
        if (!h_proof || *proof_len < need) {
            *proof_len = need;
            set_error("sp1hip_logup_gkr_prove: proof buffer too small, need %zu bytes", need);
            return SP1HIP_ERROR_BUFFER_TOO_SMALL;
        }
        const DeviceCtx* ctx;                                // (validation and the size query above need no device)
        SP1HIP_TRY(get_device_ctx(&ctx));
        SP1HIP_TRY(transcript_head());
        SP1HIP_TRY(alloc_levels_and_plan_buffers());
        SP1HIP_TRY(build_first_layer_and_tree());
        SP1HIP_TRY(plan_and_upload_passes());
        SP1HIP_TRY(fetch_circuit_output());
        SP1HIP_TRY(prove_layers());
        SP1HIP_TRY(open_traces());
        observe_openings();
        SP1HIP_TRY(write_proof());
        challenger_restore(challenger, ch);                  // the caller's transcript moves on success only
        return SP1HIP_SUCCESS;
    }
};
#undef SP1HIP_GKR_REQUIRE
}  // namespace gkr
}  // namespace sp1hip

using namespace sp1hip;

extern "C" int sp1hip_logup_gkr_prove(const sp1hip_gkr_chip_t* chips, int n_chips, int max_log_row_count, sp1hip_challenger_t* challenger,
                                      uint8_t* h_proof, size_t* proof_len, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(chips && n_chips > 0 && challenger && proof_len, "bad argument");
    SP1HIP_REQUIRE(max_log_row_count >= 1 && max_log_row_count <= 30, "max_log_row_count out of range");
    gkr::GkrProver p{chips, n_chips, max_log_row_count, challenger, h_proof, proof_len, stream, S(stream)};
    return p.prove();
}
