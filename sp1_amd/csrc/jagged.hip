// sp1_amd/csrc/jagged.hip — the jagged PCS evaluation proof: everything between the
// zerocheck point and the BaseFold opening, on the device.
//
//   sp1hip_jagged_prove   `JaggedProver::prove_trusted_evaluations`  /root/reference/slop/crates/jagged/src/prover.rs:L162-L328
//     jagged sumcheck     `jagged_sumcheck_poly` + `HadamardProduct`  sumcheck.rs:L13-L39, hadamard.rs:L52-L146
//                         driven as `reduce_sumcheck_to_evaluation`   /root/reference/slop/crates/sumcheck/src/prover.rs:L13-L96
//     J table             `partial_jagged_little_polynomial_evaluation` poly.rs:L258-L318
//     jagged-eval proof   `JaggedEvalSumcheckProver::prove_jagged_evaluation` jagged_eval/sumcheck_eval.rs:L185-L243,
//                         sumcheck_poly.rs, sumcheck_sum_as_poly.rs, eval_sumcheck_prover.rs; branching program poly.rs:L120-L160,L385-L460
//     dense opening       `StackedPcsProver::prove_trusted_evaluation` /root/reference/slop/crates/stacked/src/prover.rs:L107-L152
//                         + `prove_untrusted_evaluation(s)` (multilinear/src/pcs.rs:L128-L139, basefold-prover/src/prover.rs:L245-L270)
//   Output: bincode(JaggedPcsProof) (/root/reference/slop/crates/jagged/src/verifier.rs:L17-L26).
//
// File map
//   jagged_kernels.hpp  every kernel and the descriptors the host fills for them (JgSeg .. JgTab, JeCols, JeV)
//   ext_host.hpp        the host field helpers shared with gkr.hip (Ext operators, eq tables, DeviceBuf, upload)
//   jagged_host.hpp     JaggedBackend: what differs between the inner and the outer (BN254) configuration
//   jagged.hip (here)   the proof's byte writer; RoundTranscript (one sumcheck's transcript side: finish_round); Scratch (the round
//                       hand-over); plan_first_rounds (pure host: which kernels prove rounds 0-2); JeProver (the jagged-eval
//                       sumcheck); JgProver: one proof, a phase per member function, run in order by JgProver::prove;
//                       jagged_prove_with = argument checks + JgProver::prove; the inner JaggedBackend and the C entry point
//
// MI355X shape
//  * The dense vector q of the sumcheck is the commit-time dense buffer itself (column-major stacked
//    batches ARE the long vector the reference re-stacks), read in place, one segment per round.
//  * J(x) = eq(z_col, col(x)) eq(z_row, row(x)) is never materialised at full length: round 0 and the
//    first fold recompute it from the two small eq tables (row table: 2^max_log_row_count ext, SoA,
//    coalesced along a column; column table + prefix sums: L2 resident; column of x by binary search).
//  * One fused kernel per round: fold the previous round's tables with alpha AND accumulate the next
//    round's y(0), 4 y(1/2) sums from the folded values while they are in registers (read 32 B, write
//    16 B per surviving element). Everything past the real area T is zero and is neither stored nor read.
//  * The jagged-eval sumcheck does NOT re-run the branching program per column, round and evaluation
//    point (the reference's CPU path: ~2(log m + 1) layers x 31 ext products each time). The program
//    is a product of 4x4 transfer matrices, one per bit layer, multilinear in the layer's two prefix
//    bits: per column we keep a running row vector (layers already bound to challenges) and
//    precomputed suffix vectors (layers still boolean), so a round costs two 4x4 vector-matrix
//    products and two dot products per column; in the second half of the rounds the bound part is
//    column-independent and is advanced on the host. Same field elements, ~30x less work.
#include <algorithm>
#include <array>
#include <chrono>
#include <cstring>
#include <vector>

#include "device_ctx.hpp"
#include "jagged_host.hpp"
#include "round_sync.hpp"
#include "stacked_data.hpp"
#include "tensor_table.hpp"
#include "ext_host.hpp"
#include "jagged_kernels.hpp"

namespace sp1hip {

void challenger_observe(sp1hip_challenger_t* ch, uint32_t x);
kb::Ext challenger_sample_ext(sp1hip_challenger_t* ch);
void challenger_restore(sp1hip_challenger_t* dst, const sp1hip_challenger_t* src);

// ================================================================ host driver
namespace {

using namespace ext_host;   // DeviceBuf, the Ext operators, ext_c, log2_ceil, partial_lagrange_host, eval_mle_host, upload

struct Bytes {                     // bincode writer over the caller's proof buffer
    uint8_t* p = nullptr;
    size_t cap = 0, n = 0;
    bool overflow = false;
    void raw(const void* src, size_t k) { if (n + k > cap) { overflow = true; return; } memcpy(p + n, src, k); n += k; }
    void u64(uint64_t v) { raw(&v, 8); }               // little-endian host
    void felt(uint32_t m) { const uint32_t v = kb::from_monty(m); raw(&v, 4); }
    void ext(const Ext& e) { for (int k = 0; k < 4; k++) felt(e.c[k]); }
};

struct Sumcheck {                  // PartialSumcheckProof<EF> (sumcheck/src/proof.rs:L10-L14)
    std::vector<std::array<Ext, 3>> polys;
    Ext claimed_sum, eval;
    std::vector<Ext> point;
    void write(Bytes& w) const {
        w.u64(polys.size());
        for (auto& p : polys) { w.u64(3); for (auto& c : p) w.ext(c); }
        w.ext(claimed_sum);
        w.u64(point.size());
        for (auto& x : point) w.ext(x);
        w.ext(eval);
    }
};

Ext poly_eval(const std::array<Ext, 3>& c, const Ext& x) { return (c[2] * x + c[1]) * x + c[0]; }

// degree-2 interpolation through y(0), y(1/2), y(1) given y0, H = 4 y(1/2), y1: c2 = 2 (y0 + y1) - H
std::array<Ext, 3> interpolate(const Ext& y0, const Ext& h4, const Ext& y1) {
    const Ext s = y0 + y1;
    const Ext c2 = s + s - h4;
    return {y0, y1 - y0 - c2, c2};
}

void observe_ext(JaggedBackend& ch, const Ext& e) { for (int k = 0; k < 4; k++) ch.observe(e.c[k]); }

// The transcript side of one sumcheck (reduce_sumcheck_to_evaluation): the running claim, the challenges and the proof under
// construction. Touches no device object: a round hands it the two sums its kernel produced.
struct RoundTranscript {
    JaggedBackend& ch;
    Sumcheck proof;
    Ext claim = kb::ext_zero(), alpha = kb::ext_zero();      // alpha: the latest challenge (zero before the first round)
    std::vector<Ext> alphas;                                 // sampling order
    void begin(const Ext& claimed_sum) { proof.claimed_sum = claim = claimed_sum; }
    // y0 = y(0), h4 = 4 y(1/2) of the round's polynomial; y(1) = claim - y(0)
    void finish_round(const Ext& y0, const Ext& h4) {
        const std::array<Ext, 3> poly = interpolate(y0, h4, claim - y0);
        proof.polys.push_back(poly);
        for (auto& c : poly) observe_ext(ch, c);
        alpha = ch.sample_ext();
        alphas.push_back(alpha);
        claim = poly_eval(poly, alpha);
    }
    void end() { proof.point.assign(alphas.rbegin(), alphas.rend()); proof.eval = claim; }
};

struct Scratch {                    // device scratch shared by all rounds of one proof
    DeviceBuf partials;
    RoundSyncHost rsync;
    Mailbox mb;
    PinnedStage stage;
    uint32_t h_out[8];
    hipStream_t s;
    static constexpr uint32_t MAX_BLOCKS = 2048;
    int init(hipStream_t stream) {
        s = stream;
        SP1HIP_TRY(partials.alloc((size_t)MAX_BLOCKS * 128, s));      // 8 extension sums per workgroup at most (jg_round01_tables)
        SP1HIP_TRY(stage.init(s));
        SP1HIP_TRY(rsync.init(s));
        return mb.init(s);
    }
    // argument of the round kernel about to be launched (one per launch: it advances the sequence number finish() waits for)
    JgTail tail() { const RoundSync rs = rsync.next(); return JgTail{partials.u32(), rs, rsync.seq}; }
    static uint32_t blocks_for(uint64_t threads) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((threads + 255) / 256, 1), MAX_BLOCKS); }
    // wait for the round kernel's last workgroup and take its eight / two ext sums from the slot
    int finish8(Ext (&out)[8]) {
        uint32_t h[32];
        SP1HIP_TRY(rsync.wait(h, 32));
        memcpy(out, h, 128);
        return SP1HIP_SUCCESS;
    }
    int finish(Ext* a, Ext* b) {
        SP1HIP_TRY(rsync.wait(h_out, 8));
        memcpy(a, h_out, 16);
        memcpy(b, h_out + 4, 16);
        return SP1HIP_SUCCESS;
    }
};

// ---- SP1HIP_JG_TIMING=1: host wall time of the call's parts on stderr. lap(p): the time since the previous lap goes to part p.
struct JgTimer {
    enum Part { SETUP, SUMCHECK, EVAL, COLUMNS, BASEFOLD, BYTES, N_PARTS };
    using Clock = std::chrono::steady_clock;
    bool on = false;
    Clock::time_point last;
    double part_ms[N_PARTS] = {};
    void start() { on = env_flag("SP1HIP_JG_TIMING", false); last = Clock::now(); }
    void lap(Part p) {
        if (!on) return;
        const auto now = Clock::now();
        part_ms[p] += std::chrono::duration<double, std::milli>(now - last).count();
        last = now;
    }
    void report(int log_m) const {
        if (!on) return;
        fprintf(stderr, "[sp1hip jagged] set-up %.3f ms | %d sumcheck rounds %.3f | jagged-eval %.3f | column evaluations %.3f | BaseFold %.3f | proof bytes %.3f\n",
                part_ms[SETUP], log_m, part_ms[SUMCHECK], part_ms[EVAL], part_ms[COLUMNS], part_ms[BASEFOLD], part_ms[BYTES]);
    }
};

struct StageMarks {                 // roctx sub-ranges of the evaluation proof (rocprofv3 --marker-trace)
    bool open = false;
    void next(const char* name) { if (open) roctx_pop(); roctx_push(name); open = true; }
    ~StageMarks() { if (open) roctx_pop(); }
};

// ================================================================ which kernels prove rounds 0, 1 and 2
// Everything follows from g, the OR of the dense area and of every column start: 2^ctz(g) divides every table height.
//   g odd, or the factored switch off
//                         generic kernels (jg_round0_sum, jg_fold0_sum, then jg_fold_sum), J materialised from level 1 on
//   g even                round 0 table-major (jg_round0_tables); g = 2 mod 4 still folds generically (rf = 0)
//   g = 0 mod 4           rf >= 2 (area and row count permitting): levels 1 .. rf keep J factored, the first fold is
//                         table-major (jg_fold_tables<1, true>), later factored levels jg_foldf_sum
//   g = 0 mod 8           level 1 is never stored: round 1 takes sums only, round 2 folds two levels from the base words
//                         (jg_fold_tables<2, true>); with the look-ahead switch rounds 0 and 1 are ONE pass (jg_round01_tables)
// A factored level implies the table-major form: rf >= 2 needs g = 0 mod 4 with the factored switch on, and a round that can be
// opened has a real table (area > 0), so a slice is listed and tables_mult4 holds. The generic first fold therefore always
// materialises j (there is no jg_fold0_sum without the j table).
struct FirstRoundsPlan {
    int rf = 0;                     // levels 1 .. rf keep J factored (see jg_foldf_sum): 0 or >= 2
    std::vector<JgTab> tabs0;       // table-major descriptors (only when every column start is even, i.e. dense pairs never straddle columns)
    uint32_t n_tiles0 = 0, n_tiles1 = 0, n_tiles2 = 0;     // tiles of the round-0 / one-level / two-level table-major launches
    bool tables_mult4 = false;      // every table height a multiple of 4: the first fold can go table-major too
    bool skip_level1 = false;       // ... of 8: rounds 1 and 2 both fold from the base words, level 1 is never stored
    bool lookahead01 = false;       // rounds 0 and 1 from one pass over the base words
    std::vector<std::pair<uint64_t, uint64_t>> zero_tails;      // dense index ranges holding only padding zeros
    bool table_major() const { return !tabs0.empty(); }
};

// Pure host: no device call, no allocation on the device (the JgTab slices only carry addresses inside the rounds' dense buffers).
// factored / lookahead: the SP1HIP_JAGGED_FACTORED and SP1HIP_JAGGED_LOOKAHEAD switches.
FirstRoundsPlan plan_first_rounds(const std::vector<uint32_t>& prefix, uint32_t T, int log_m, int max_log_row_count,
                                  StackedCore* const* rounds, int n_rounds, bool factored, bool lookahead) {
    FirstRoundsPlan pl;
    uint32_t g = T;
    for (uint32_t pfx : prefix) g |= pfx;
    // every column must start at a multiple of 2^level
    pl.rf = g ? __builtin_ctz(g) : 0;
    pl.rf = std::min(pl.rf, std::min(log_m - 2, max_log_row_count - 1));
    if (!factored) pl.rf = 0;
    if (pl.rf < 2) pl.rf = 0;          // a single factored level is not worth the extra table
    if ((g & 1u) != 0 || !factored) return pl;
    uint64_t seg_start = 0;
    uint32_t col = 0;
    for (int r = 0; r < n_rounds; r++) {
        const StackedCore* d = rounds[r];
        uint64_t off = 0;
        const size_t n_real = d->row_counts.size() - 2;           // the two padding tables hold zeros only
        for (size_t t = 0; t < d->row_counts.size(); t++) {
            const uint32_t h = (uint32_t)d->row_counts[t], w = (uint32_t)d->column_counts[t];
            if (t < n_real && h && w) {
                // a lane of the table-major kernels owns a few rows of a table and walks its columns one after the other, so a
                // wide, short table is a few waves with a long dependent loop: the 2,640 columns x 122k rows of a Keccak shard
                // made jg_fold_tables<2> one 3.3 ms launch on 60 workgroups (0.7 ms on a core shard of the same area). Every
                // quantity is a sum over columns, so a table enters as slices of at most JG_COL_SLICE columns — descriptors of
                // their own, the kernels see narrower tables.
                for (uint32_t c_lo = 0; c_lo < w; c_lo += JG_COL_SLICE) {
                    const uint32_t wc = std::min(JG_COL_SLICE, w - c_lo);
                    const uint64_t o = off + (uint64_t)c_lo * h;
                    pl.tabs0.push_back(JgTab{(const uint32_t*)d->d_dense + o, h, col + c_lo, wc, pl.n_tiles0, (uint32_t)(seg_start + o),
                                             pl.n_tiles1, pl.n_tiles2});
                    pl.n_tiles0 += (h / 2 + JG_TAB_PAIRS - 1) / JG_TAB_PAIRS;
                    pl.n_tiles1 += ((h + 3) / 4 + JG_TAB_PAIRS - 1) / JG_TAB_PAIRS;
                    pl.n_tiles2 += ((h + 7) / 8 + JG_TAB_PAIRS - 1) / JG_TAB_PAIRS;
                }
            }
            if (t == n_real) pl.zero_tails.push_back({seg_start + off, seg_start + d->padded});
            off += (uint64_t)h * w;
            col += w;
        }
        seg_start += d->padded;
    }
    if (pl.table_major()) {
        pl.tables_mult4 = (g & 3u) == 0;
        pl.skip_level1 = (g & 7u) == 0 && pl.rf >= 2 && log_m >= 4;
        pl.lookahead01 = pl.skip_level1 && lookahead;
    }
    return pl;
}

// ---- branching-program layer matrices (poly.rs:L120-L160): out[layer][2 cb + nb][m][m']
void build_layer_matrices(const std::vector<Ext>& z_row, const std::vector<Ext>& z_index, int D, std::vector<Ext>* out) {
    auto lsb = [](const std::vector<Ext>& p, size_t i) { return p.size() <= i ? kb::ext_zero() : p[p.size() - 1 - i]; };
    out->assign((size_t)D * 4 * 16, kb::ext_zero());
    const Ext one = kb::ext_one();
    for (int layer = 0; layer < D; layer++) {
        const Ext zr = lsb(z_row, layer), zi = lsb(z_index, layer);
        const Ext er[2] = {one - zr, zr}, ei[2] = {one - zi, zi};
        for (int cb = 0; cb < 2; cb++)
            for (int nb = 0; nb < 2; nb++)
                for (int m = 0; m < 4; m++) {
                    const int carry = m & 1, cmp = m >> 1;
                    for (int rb = 0; rb < 2; rb++)
                        for (int ib = 0; ib < 2; ib++) {
                            const int sum = rb + carry + cb;
                            if (ib != (sum & 1)) continue;                       // fail transition
                            const int new_cmp = ib == nb ? cmp : nb;
                            const int target = (sum >> 1) + 2 * new_cmp;
                            Ext& e = (*out)[(((size_t)layer * 4 + cb * 2 + nb) * 4 + m) * 4 + target];
                            e = e + er[rb] * ei[ib];
                        }
                }
    }
}

// ================================================================ the jagged-eval sumcheck
// JaggedEvalSumcheckProver::prove_jagged_evaluation. prefix: #columns + 1 dense prefix sums. The device buffers live as long as
// the struct: one JeProver per proof, made and dropped by JgProver::prove_jagged_eval.
struct JeProver {
    const std::vector<uint32_t>& prefix;
    const int D;                                             // log_m + 1 bit layers; 2 D rounds
    const std::vector<Ext>&z_row, &z_col, &z_trace;
    Scratch& sc;
    RoundTranscript& tr;

    const hipStream_t s = sc.s;
    const Ext half = kb::ext_inv(ext_c(2));
    uint32_t n = 0, nb = 0;                                  // condensed columns; workgroups of every launch
    std::vector<Ext> mats;                                   // build_layer_matrices
    DeviceBuf d_t, d_u, d_zc, d_mats, d_suffix, d_state, d_inter;
    JeCols C{};
    std::vector<Ext> B;                                      // phase 2: B[layer][cb] = A_layer(cb, alpha_layer)
    DeviceBuf d_B, d_suffix2;

    // condensed (t_c, t_{c+1}) runs with their summed eq(z_col, .) weights (sumcheck_poly.rs:L106-L121), the layer matrices
    int setup_columns() {
        const std::vector<Ext> col_eq = partial_lagrange_host(z_col);
        std::vector<uint32_t> ts, us;
        std::vector<Ext> zc;
        for (size_t c = 0; c + 1 < prefix.size(); c++) {
            if (!ts.empty() && ts.back() == prefix[c] && us.back() == prefix[c + 1]) zc.back() = zc.back() + col_eq[c];
            else { ts.push_back(prefix[c]); us.push_back(prefix[c + 1]); zc.push_back(col_eq[c]); }
        }
        n = (uint32_t)ts.size();
        SP1HIP_TRY(upload(d_t, ts.data(), n * 4, s, sc.stage));
        SP1HIP_TRY(upload(d_u, us.data(), n * 4, s, sc.stage));
        SP1HIP_TRY(upload(d_zc, zc.data(), (size_t)n * 16, s, sc.stage));
        build_layer_matrices(z_row, z_trace, D, &mats);
        SP1HIP_TRY(upload(d_mats, mats.data(), mats.size() * 16, s, sc.stage));
        SP1HIP_TRY(d_suffix.alloc((size_t)D * n * 64, s));
        SP1HIP_TRY(d_state.alloc((size_t)n * 128, s));
        SP1HIP_TRY(d_inter.alloc((size_t)n * 16, s));
        C = JeCols{d_t.u32(), d_u.u32(), d_zc.ext(), n};
        nb = Scratch::blocks_for(n);
        return SP1HIP_SUCCESS;
    }

    int finish_round() {
        SP1HIP_LAUNCH_CHECK();
        Ext y0, yh;
        SP1HIP_TRY(sc.finish(&y0, &yh));
        tr.finish_round(y0, yh + yh + yh + yh);
        return SP1HIP_SUCCESS;
    }

    // first half: the bits of t_{c+1}, after the claimed J(z_trace)
    int phase1() {
        // all-boolean suffixes; their layer-0 entry gives the claimed J(z_trace) (full_jagged_little_polynomial_evaluation)
        hipLaunchKernelGGL(je_suffix_kernel<true>, dim3(nb), dim3(256), 0, s, C, (const Ext*)d_mats.p, D, d_suffix.ext(), sc.tail());
        SP1HIP_LAUNCH_CHECK();
        Ext expected_sum, unused;
        SP1HIP_TRY(sc.finish(&expected_sum, &unused));
        observe_ext(tr.ch, expected_sum);
        tr.begin(expected_sum);
        for (int r = 0; r < D; r++) {
            hipLaunchKernelGGL(je_phase1_round, dim3(nb), dim3(256), 0, s, C, (const Ext*)d_mats.p, (const Ext*)d_suffix.p, D, r, tr.alpha,
                               half, d_state.ext(), d_inter.ext(), sc.tail());
            SP1HIP_TRY(finish_round());
        }
        return SP1HIP_SUCCESS;
    }

    // second half: every bit of t_{c+1} is bound to alphas[0..D); the bound part is column-independent and advanced here
    int phase2() {
        B.resize((size_t)D * 2 * 16);
        for (int layer = 0; layer < D; layer++)
            for (int cb = 0; cb < 2; cb++)
                for (int e = 0; e < 16; e++) {
                    const Ext a0 = mats[((size_t)layer * 4 + cb * 2 + 0) * 16 + e], a1 = mats[((size_t)layer * 4 + cb * 2 + 1) * 16 + e];
                    B[((size_t)layer * 2 + cb) * 16 + e] = a0 + tr.alphas[layer] * (a1 - a0);
                }
        SP1HIP_TRY(upload(d_B, B.data(), B.size() * 16, s, sc.stage));
        SP1HIP_TRY(d_suffix2.alloc((size_t)D * n * 64, s));
        hipLaunchKernelGGL(je_suffix_kernel<false>, dim3(nb), dim3(256), 0, s, C, (const Ext*)d_B.p, D, d_suffix2.ext(), sc.tail());
        SP1HIP_LAUNCH_CHECK();
        Ext W[4] = {kb::ext_one(), kb::ext_zero(), kb::ext_zero(), kb::ext_zero()};     // e_initial^T
        for (int rp = 0; rp < D; rp++) {
            Ext V[8];
            for (int b = 0; b < 2; b++)
                for (int k = 0; k < 4; k++) {
                    Ext acc = kb::ext_zero();
                    for (int m = 0; m < 4; m++) acc = acc + W[m] * B[((size_t)rp * 2 + b) * 16 + 4 * m + k];
                    V[4 * b + k] = acc;
                }
            JeV Varg;
            memcpy(Varg.v, V, sizeof V);
            hipLaunchKernelGGL(je_phase2_round, dim3(nb), dim3(256), 0, s, C, (const Ext*)d_suffix2.p, D, rp, tr.alpha, half,
                               Varg, d_inter.ext(), sc.tail());
            SP1HIP_TRY(finish_round());
            for (int k = 0; k < 4; k++) W[k] = V[k] + tr.alpha * (V[4 + k] - V[k]);
        }
        return SP1HIP_SUCCESS;
    }

    int prove() {
        SP1HIP_TRY(setup_columns());
        SP1HIP_TRY(phase1());
        SP1HIP_TRY(phase2());
        tr.end();
        return SP1HIP_SUCCESS;
    }
};

#define SP1HIP_JG_REQUIRE(cond, msg) \
    do { if (!(cond)) { sp1hip::set_error("jagged_prove_with: %s", msg); return SP1HIP_ERROR_INVALID_ARGUMENT; } } while (0)

// where the jagged sumcheck's tables are between two rounds
struct FoldState {
    int cur = 0;                       // tabs[cur] (and tabs[cur + 1] once materialised) hold (q, j) of the current level
    uint32_t n_live = 0;               // live entries of the current round's tables
    bool j_materialised = false;       // does tabs[cur + 1] hold the j table of the current level?
    const uint32_t* row_eq = nullptr;  // the row-eq table folded once per level so far (level_J): what a factored J reads
    uint32_t row_len = 0;              // ... and its entries per plane
};

// ================================================================ one proof
// The members are declared in the order the phases create them: the device buffers are destroyed in reverse order, every one
// after the work that uses it has been enqueued (the arena is stream-ordered), and Scratch — whose RoundSyncHost / Mailbox drain
// the stream when a publishing kernel may still be in flight after an early error return — after all of them.
struct JgProver {
    // the call's arguments (the struct is an aggregate: jagged_prove_with fills these, everything else starts empty)
    JaggedBackend& be;                                       // the transcript (a clone; committed by accept()), the dense PCS, the commitments
    const sp1hip_ext_t* const h_z_row;
    const int max_log_row_count;
    StackedCore* const* const rounds;
    const int n_rounds;
    const sp1hip_ext_t* const h_claims;
    const size_t* const claims_per_round;
    const sp1hip_fri_config_t config;
    uint8_t* const h_proof;
    size_t* const proof_len;
    const sp1hip_stream_t stream;
    const hipStream_t s;

    JgTimer timer;
    StageMarks marks;
    int lsh = 0, log_m = 0, num_col_variables = 0;           // check_and_size
    uint64_t total_cols = 0, total_area = 0, n_claims = 0;
    std::vector<uint32_t> round_widths;
    std::vector<size_t> tables_per_round;
    size_t need = 0;                                         // bytes of the proof
    std::vector<Ext> z_row, z_col;                           // transcript_head
    Ext sumcheck_claim;
    std::vector<uint32_t> prefix;                            // upload_point_tables: dense prefix sums, one entry per column + the area
    uint32_t ncols = 0, T = 0;                               // columns; the dense area of all rounds
    std::vector<Ext> col_eq;
    Scratch sc;
    DeviceBuf d_prefix, d_col_eq, d_row_eq;
    JgSegs segs{};
    JgJ J{};
    FirstRoundsPlan plan;                                    // plan_first_rounds
    DeviceBuf tabs[4];                                       // q/j ping-pong: q of odd levels in tabs[0], of even levels in tabs[2]; j behind each
    DeviceBuf row_eq_lv[2], d_prefix_lv;                     // folded row tables (ping-pong) and the shifted prefix sums of every level
    DeviceBuf d_tabs0, d_col_eq3;                            // plan.tabs0; 3 eq_col (kb::edot_add)
    FoldState st;
    RoundTranscript jt{be}, et{be};                          // the jagged sumcheck's transcript, the jagged-eval sumcheck's
    Ext q_eval = kb::ext_zero();
    std::vector<Ext> stack_point, flat_claims;               // open_dense
    std::vector<std::vector<Ext>> batch_evals;
    DeviceBuf d_eq, d_evals;
    size_t bf_len = 0;                                       // bytes of the BaseFold proof at the head of h_proof

    // ---- the rounds' shapes against the arguments, the proof's size (everything is determined by the shapes)
    int check_and_size() {
        SP1HIP_JG_REQUIRE(rounds[0], "null round");
        lsh = rounds[0]->log_stacking_height;
        SP1HIP_JG_REQUIRE(lsh >= 1, "log_stacking_height must be at least 1");
        for (int r = 0; r < n_rounds; r++) {
            const StackedCore* d = rounds[r];
            SP1HIP_JG_REQUIRE(d && d->jagged, "round data did not come from a jagged commit");
            if (d->stream != s) rounds[r]->foreign_use = true;
            SP1HIP_JG_REQUIRE(d->log_stacking_height == lsh && d->max_log_row_count == max_log_row_count, "rounds disagree on parameters");
            SP1HIP_JG_REQUIRE(d->area > 0, "a commitment round without any table data cannot be opened");
            uint64_t expect = 0;
            for (size_t t = 0; t + 2 < d->column_counts.size(); t++) expect += d->column_counts[t];
            SP1HIP_JG_REQUIRE(claims_per_round[r] == expect, "claims_per_round does not match the committed tables");
            for (uint64_t c : d->column_counts) total_cols += c;
            total_area += d->padded;
            n_claims += claims_per_round[r];
            round_widths.push_back((uint32_t)(d->padded >> lsh));
        }
        SP1HIP_JG_REQUIRE(h_claims || n_claims == 0, "null claims");
        SP1HIP_JG_REQUIRE(total_area < ((uint64_t)1 << 30), "dense area must stay below 2^30 (jagged verifier bound)");
        log_m = log2_ceil(total_area);
        SP1HIP_JG_REQUIRE(log_m >= lsh, "internal: area smaller than one stacked column");
        num_col_variables = log2_ceil(total_cols);
        for (int r = 0; r < n_rounds; r++) tables_per_round.push_back(rounds[r]->row_counts.size());
        need = jagged_proof_size_with(be.opening_size(lsh, round_widths.data(), n_rounds, config), be.commitment_bytes(), round_widths,
                                      tables_per_round, total_area);
        if (!h_proof || *proof_len < need) {
            *proof_len = need;
            set_error("%s: proof buffer too small, need %zu bytes", be.entry_point(), need);
            return SP1HIP_ERROR_BUFFER_TOO_SMALL;
        }
        return SP1HIP_SUCCESS;
    }

    // ---- transcript head, on a copy of the transcript (committed only on success): z_col, the claim of the jagged sumcheck
    int transcript_head() {
        SP1HIP_TRY(be.begin());
        z_row.resize(max_log_row_count);
        z_col.resize(num_col_variables);
        memcpy(z_row.data(), h_z_row, (size_t)max_log_row_count * 16);
        for (auto& z : z_col) z = be.sample_ext();
        // column claims with the zero claims of the padding columns, padded to a power of two (prover.rs:L187-L212, L268-L271)
        std::vector<Ext> column_claims;
        size_t off = 0;
        for (int r = 0; r < n_rounds; r++) {
            for (size_t i = 0; i < claims_per_round[r]; i++) { Ext e; memcpy(&e, &h_claims[off + i], 16); column_claims.push_back(e); }
            off += claims_per_round[r];
            column_claims.insert(column_claims.end(), rounds[r]->padding_column_count, kb::ext_zero());
        }
        SP1HIP_JG_REQUIRE(column_claims.size() == total_cols, "internal: column claim count");
        sumcheck_claim = eval_mle_host(column_claims, z_col);
        return SP1HIP_SUCCESS;
    }

    // ---- what J(x) and q(x) are read from: the prefix sums, eq(z_col, .), eq(z_row, .), the rounds' dense segments
    int upload_point_tables() {
        // dense prefix sums, one entry per column (JaggedLittlePolynomialProverParams::new)
        uint64_t acc = 0;
        for (int r = 0; r < n_rounds; r++)
            for (size_t t = 0; t < rounds[r]->row_counts.size(); t++)
                for (uint64_t c = 0; c < rounds[r]->column_counts[t]; c++) { prefix.push_back((uint32_t)acc); acc += rounds[r]->row_counts[t]; }
        prefix.push_back((uint32_t)acc);
        SP1HIP_JG_REQUIRE(acc == total_area, "internal: prefix sums do not cover the dense area");
        ncols = (uint32_t)prefix.size() - 1;
        col_eq = partial_lagrange_host(z_col);

        SP1HIP_TRY(sc.init(s));
        SP1HIP_TRY(upload(d_prefix, prefix.data(), prefix.size() * 4, s, sc.stage));
        SP1HIP_TRY(upload(d_col_eq, col_eq.data(), col_eq.size() * 16, s, sc.stage));
        SP1HIP_TRY(d_row_eq.alloc(((size_t)16) << max_log_row_count, s));
        SP1HIP_TRY(sp1hip_partial_lagrange(h_z_row, max_log_row_count, d_row_eq.u32(), stream));
        segs.n = n_rounds;
        uint64_t start = 0;
        for (int r = 0; r < n_rounds; r++) {
            segs.s[r] = JgSeg{(const uint32_t*)rounds[r]->d_dense, (uint32_t)start, (uint32_t)rounds[r]->padded};
            start += rounds[r]->padded;
        }
        segs.total = T = (uint32_t)start;
        J = JgJ{d_prefix.u32(), ncols, d_col_eq.ext(), d_row_eq.u32(), 1u << max_log_row_count};
        return SP1HIP_SUCCESS;
    }

    // ---- the q/j ping-pong, the factored levels' row tables and prefix sums, the table-major descriptors
    int alloc_tables() {
        SP1HIP_JG_REQUIRE(!plan.rf || plan.tables_mult4, "internal: factored levels without the table-major form");
        const uint32_t n1 = (T + 1) / 2;
        st.j_materialised = plan.rf == 0;
        if (plan.rf == 0) {
            SP1HIP_TRY(tabs[1].alloc((size_t)std::max<uint32_t>(n1, 1) * 16, s));
            SP1HIP_TRY(tabs[3].alloc((size_t)std::max<uint32_t>((n1 + 1) / 2, 1) * 16, s));
        } else {
            SP1HIP_TRY(row_eq_lv[0].alloc(((size_t)16) << (max_log_row_count - 1), s));
            SP1HIP_TRY(row_eq_lv[1].alloc(((size_t)16) << (max_log_row_count - 1), s));
            SP1HIP_TRY(d_prefix_lv.alloc(prefix.size() * 4 * (size_t)(plan.rf + 1), s));
            std::vector<uint32_t> all_lv(prefix.size() * (size_t)(plan.rf + 1));      // the shifted prefix sums of every level: one upload
            for (int lv = 0; lv <= plan.rf; lv++)
                for (size_t c = 0; c < prefix.size(); c++) all_lv[(size_t)lv * prefix.size() + c] = prefix[c] >> lv;
            SP1HIP_TRY(sc.stage.upload(d_prefix_lv.p, all_lv.data(), all_lv.size() * 4));
        }
        if (plan.table_major()) {
            SP1HIP_TRY(upload(d_tabs0, plan.tabs0.data(), plan.tabs0.size() * sizeof(JgTab), s, sc.stage));
            std::vector<Ext> col_eq3(col_eq.size());
            for (size_t c = 0; c < col_eq.size(); c++)
                for (int q = 0; q < 4; q++) col_eq3[c].c[q] = kb::add(kb::dbl(col_eq[c].c[q]), col_eq[c].c[q]);
            SP1HIP_TRY(upload(d_col_eq3, col_eq3.data(), col_eq3.size() * 16, s, sc.stage));
        }
        // q of odd levels lives in tabs[0]: level 1 (T/2 entries), or level 3 when level 1 is never stored
        SP1HIP_TRY(tabs[0].alloc((size_t)std::max<uint32_t>(plan.skip_level1 ? (T + 7) / 8 : n1, 1) * 16, s));
        SP1HIP_TRY(tabs[2].alloc((size_t)std::max<uint32_t>((n1 + 1) / 2, 1) * 16, s));
        st.n_live = T;
        st.row_eq = d_row_eq.u32();
        st.row_len = 1u << max_log_row_count;
        return SP1HIP_SUCCESS;
    }

    // J of level `lv` (1 <= lv <= rf): folds the row table once more with the challenge that produced the level
    int level_J(int lv, const Ext& a_prev, JgJ* out) {
        uint32_t* dst = row_eq_lv[lv & 1].u32();
        hipLaunchKernelGGL(jg_fold_row_eq, dim3((st.row_len / 2 + 255) / 256), dim3(256), 0, s, st.row_eq, st.row_len, a_prev, dst);
        SP1HIP_LAUNCH_CHECK();
        st.row_eq = dst;
        st.row_len >>= 1;
        *out = JgJ{d_prefix_lv.u32() + (size_t)lv * prefix.size(), ncols, d_col_eq.ext(), st.row_eq, st.row_len};
        return SP1HIP_SUCCESS;
    }

    // the zero tail of every commitment round (its padding tables), `shift` levels down: the table-major folds write the real
    // tables only, and the tail must read as zero in the next fold
    int zero_tails(Ext* q, int shift) {
        for (auto& z : plan.zero_tails)
            if (z.second > z.first)
                SP1HIP_HIP(hipMemsetAsync(q + (z.first >> shift), 0, (size_t)((z.second - z.first) >> shift) * 16, s));
        return SP1HIP_SUCCESS;
    }

    // the end of a round: the launch's status, its two sums from the device, the transcript
    int finish_round() {
        SP1HIP_LAUNCH_CHECK();
        Ext y0, h4;
        SP1HIP_TRY(sc.finish(&y0, &h4));
        jt.finish_round(y0, h4);
        return SP1HIP_SUCCESS;
    }

    // ---- rounds 0 and 1 from ONE pass (jg_round01_tables); round 2 then folds from the base words with both challenges
    int rounds_0_and_1_lookahead() {
        {
            ScopedTimer t("jagged_round0_sum", s);
            const uint32_t nb = Scratch::blocks_for((uint64_t)plan.n_tiles1 * 256);
            hipLaunchKernelGGL(jg_round01_tables, dim3(nb), dim3(256), 0, s, (const JgTab*)d_tabs0.p, (uint32_t)plan.tabs0.size(),
                               plan.n_tiles1, J, sc.tail());
            SP1HIP_LAUNCH_CHECK();
        }
        Ext S[8];
        SP1HIP_TRY(sc.finish8(S));
        jt.finish_round(S[0] + S[1], S[2] + S[3]);           // round 0
        // the row-eq table of level 1 (the state later levels fold from), as round 1 would have built it
        const Ext a0 = jt.alpha;
        JgJ J1;
        SP1HIP_TRY(level_J(1, a0, &J1));
        // round 1: y'(0) and H' are quadratics in alpha_0 through their values at 0, 1 and their leading coefficients
        const Ext c0 = S[0], c2 = (S[0] + S[4]) + (S[0] + S[4]) - S[2], c1 = S[4] - c0 - c2;
        const Ext d0 = S[5], d2 = S[7], d1 = S[6] - d0 - d2;
        jt.finish_round(c0 + (c1 + c2 * a0) * a0, d0 + (d1 + d2 * a0) * a0);
        st.n_live = (st.n_live + 1) / 2;
        return SP1HIP_SUCCESS;
    }

    int round_0() {
        {
            ScopedTimer t("jagged_round0_sum", s);
            if (plan.table_major()) {
                const uint32_t nb = Scratch::blocks_for((uint64_t)plan.n_tiles0 * 256);
                hipLaunchKernelGGL(jg_round0_tables, dim3(nb), dim3(256), 0, s, (const JgTab*)d_tabs0.p, (uint32_t)plan.tabs0.size(),
                                   plan.n_tiles0, J, sc.tail());
            } else {
                const uint32_t nb = Scratch::blocks_for((T / 2 + JG_ITERS - 1) / JG_ITERS);
                hipLaunchKernelGGL(jg_round0_sum, dim3(nb), dim3(256), 0, s, segs, J, T / 2, sc.tail());
            }
        }
        return finish_round();
    }

    // ---- the first fold, from the base words: level 1 into tabs[0] (not stored when level 1 is skipped)
    int round_1() {
        const Ext alpha = jt.alpha;
        const uint32_t n_out = (st.n_live + 1) / 2;
        {
            ScopedTimer t("jagged_fold0_sum", s);
            if (plan.rf) {
                JgJ J1;                                    // eq_row_1 for this round's sums and for level 2
                SP1HIP_TRY(level_J(1, alpha, &J1));
                const uint32_t nb = Scratch::blocks_for((uint64_t)plan.n_tiles1 * 256);
                if (plan.skip_level1) {                    // sums only; round 2 folds from the base words again
                    hipLaunchKernelGGL((jg_fold_tables<1, false>), dim3(nb), dim3(256), 0, s, (const JgTab*)d_tabs0.p,
                                       (uint32_t)plan.tabs0.size(), plan.n_tiles1, J1, (const Ext*)d_col_eq3.p, alpha, alpha, (Ext*)nullptr,
                                       sc.tail());
                } else {                                   // (rf != 0 implies tables_mult4: alloc_tables)
                    SP1HIP_TRY(zero_tails(tabs[0].ext(), 1));
                    hipLaunchKernelGGL((jg_fold_tables<1, true>), dim3(nb), dim3(256), 0, s, (const JgTab*)d_tabs0.p,
                                       (uint32_t)plan.tabs0.size(), plan.n_tiles1, J1, (const Ext*)d_col_eq3.p, alpha, alpha, tabs[0].ext(),
                                       sc.tail());
                }
            } else {
                const uint32_t nb = Scratch::blocks_for(((n_out + 1) / 2 + JG_ITERS - 1) / JG_ITERS);
                hipLaunchKernelGGL(jg_fold0_sum, dim3(nb), dim3(256), 0, s, segs, J, alpha, n_out, tabs[0].ext(), tabs[1].ext(), sc.tail());
            }
            st.n_live = n_out;
            st.cur = 0;
        }
        return finish_round();
    }

    // ---- round >= 2: level `round` into the other half of the ping-pong
    int round_n(int round) {
        const Ext alpha = jt.alpha;
        const uint32_t n_out = (st.n_live + 1) / 2;
        const int cur = st.cur, nxt = cur ^ 2;
        {
            ScopedTimer t("jagged_fold_sum", s);
            if (round == 2 && plan.skip_level1) {          // level 2 straight from the base words (alpha0, alpha1)
                JgJ Jl;
                SP1HIP_TRY(level_J(2, alpha, &Jl));
                SP1HIP_TRY(zero_tails(tabs[nxt].ext(), 2));
                const uint32_t nb = Scratch::blocks_for((uint64_t)plan.n_tiles2 * 256);
                hipLaunchKernelGGL((jg_fold_tables<2, true>), dim3(nb), dim3(256), 0, s, (const JgTab*)d_tabs0.p, (uint32_t)plan.tabs0.size(),
                                   plan.n_tiles2, Jl, (const Ext*)d_col_eq3.p, jt.alphas[0], alpha, tabs[nxt].ext(), sc.tail());
            } else if (round <= plan.rf) {                 // factored: level `round` from level `round - 1`
                JgJ Jl;
                SP1HIP_TRY(level_J(round, alpha, &Jl));
                const uint32_t nb = Scratch::blocks_for(((n_out + 1) / 2 + JG_ITERS - 1) / JG_ITERS);
                hipLaunchKernelGGL(jg_foldf_sum, dim3(nb), dim3(256), 0, s, (const Ext*)tabs[cur].p, st.n_live, Jl, alpha, n_out,
                                   tabs[nxt].ext(), sc.tail());
            } else if (!st.j_materialised) {               // leave the factored form: this round computes j of level round - 1 as it loads
                const uint32_t nb = Scratch::blocks_for((n_out + 1) / 2);
                const JgJ Jp{d_prefix_lv.u32() + (size_t)(round - 1) * prefix.size(), ncols, d_col_eq.ext(), st.row_eq, st.row_len};
                SP1HIP_TRY(tabs[cur + 1].alloc((size_t)std::max<uint32_t>((n_out + 1) / 2, 1) * 16, s));   // (written by the round after next)
                SP1HIP_TRY(tabs[nxt + 1].alloc((size_t)std::max<uint32_t>(n_out, 1) * 16, s));
                st.j_materialised = true;
                hipLaunchKernelGGL(jg_fold_sum_fj, dim3(nb), dim3(256), 0, s, (const Ext*)tabs[cur].p, Jp, st.n_live, alpha, n_out,
                                   tabs[nxt].ext(), tabs[nxt + 1].ext(), sc.tail());
            } else {
                const uint32_t nb = Scratch::blocks_for((n_out + 1) / 2);
                hipLaunchKernelGGL(jg_fold_sum, dim3(nb), dim3(256), 0, s, (const Ext*)tabs[cur].p, (const Ext*)tabs[cur + 1].p, st.n_live,
                                   alpha, n_out, tabs[nxt].ext(), tabs[nxt + 1].ext(), sc.tail());
            }
            st.n_live = n_out;
            st.cur = nxt;
        }
        return finish_round();
    }

    // ---- the jagged sumcheck: log_m rounds
    int prove_sumcheck() {
        jt.begin(sumcheck_claim);
        if (plan.lookahead01) SP1HIP_TRY(rounds_0_and_1_lookahead());
        for (int round = plan.lookahead01 ? 2 : 0; round < log_m; round++)
            SP1HIP_TRY(round == 0 ? round_0() : round == 1 ? round_1() : round_n(round));
        jt.end();
        return SP1HIP_SUCCESS;
    }

    // ---- q at the sumcheck's point: fold the last (<= 2 entries) q table on the host
    int final_q_eval() {
        SP1HIP_JG_REQUIRE(log_m != 0, "degenerate dense area");
        if (log_m == 1) {
            // tables were never materialised: T == 2, fold straight from the base data (cannot happen with lsh >= 1 and
            // two-padding-table rounds unless the area is exactly 2; handled for completeness)
            uint32_t hq[2];
            SP1HIP_TRY(sc.mb.fetch(rounds[0]->d_dense, 2, hq));
            q_eval = kb::ext_from_base(hq[0]) + kb::ext_mul_base(jt.alpha, kb::sub(hq[1], hq[0]));
        } else {
            Ext hq[2] = {kb::ext_zero(), kb::ext_zero()};
            SP1HIP_TRY(sc.mb.fetch(tabs[st.cur].p, (size_t)st.n_live * 4, hq));
            q_eval = hq[0] + jt.alpha * (hq[1] - hq[0]);
        }
        return SP1HIP_SUCCESS;
    }

    // ---- the jagged-eval proof: J at the sumcheck's point
    int prove_jagged_eval() {
        JeProver je{prefix, log_m + 1, z_row, z_col, jt.proof.point, sc, et};
        return je.prove();
    }

    // ---- dense PCS: observe the claim, evaluate every stacked column at the stack point, BaseFold-open
    int open_dense() {
        observe_ext(be, q_eval);
        stack_point.assign(jt.proof.point.end() - lsh, jt.proof.point.end());
        SP1HIP_TRY(d_eq.alloc(((size_t)16) << lsh, s));
        SP1HIP_TRY(sp1hip_partial_lagrange(reinterpret_cast<const sp1hip_ext_t*>(stack_point.data()), lsh, d_eq.u32(), stream));
        batch_evals.resize(n_rounds);
        SP1HIP_TRY(d_evals.alloc((size_t)(*std::max_element(round_widths.begin(), round_widths.end())) * 16, s));
        for (int r = 0; r < n_rounds; r++) {
            const uint32_t w = round_widths[r];
            batch_evals[r].resize(w);
            ScopedTimer t("jagged_batch_evals", s);
            SP1HIP_TRY(sp1hip_mle_eval_columns(rounds[r]->batches.data(), (int)rounds[r]->batches.size(), lsh, d_eq.u32(), d_evals.u32(), stream));
            SP1HIP_TRY(sc.mb.fetch(d_evals.p, (size_t)w * 4, batch_evals[r].data()));
            flat_claims.insert(flat_claims.end(), batch_evals[r].begin(), batch_evals[r].end());
        }
        for (auto& e : flat_claims) observe_ext(be, e);
        timer.lap(JgTimer::COLUMNS);
        // the BaseFold proof is the first field of JaggedPcsProof: it is written straight into the caller's buffer, the rest behind it
        bf_len = need;
        return be.open(reinterpret_cast<const sp1hip_ext_t*>(stack_point.data()), lsh, reinterpret_cast<const sp1hip_ext_t*>(flat_claims.data()),
                       flat_claims.size(), config, h_proof, &bf_len, stream);
    }

    // ---- bincode(JaggedPcsProof), behind the BaseFold proof
    int write_proof() {
        Bytes w;
        w.p = h_proof;
        w.cap = need;
        w.n = bf_len;
        w.u64(n_rounds);
        for (auto& ev : batch_evals) { w.u64(ev.size()); for (auto& e : ev) w.ext(e); w.u64(1); w.u64(ev.size()); }
        jt.proof.write(w);
        et.proof.write(w);
        w.u64(n_rounds);
        for (int r = 0; r < n_rounds; r++) {
            w.u64(rounds[r]->row_counts.size());
            for (size_t t = 0; t < rounds[r]->row_counts.size(); t++) { w.u64(rounds[r]->row_counts[t]); w.u64(rounds[r]->column_counts[t]); }
        }
        w.u64(n_rounds);
        for (int r = 0; r < n_rounds; r++) {
            uint8_t c[64];
            be.write_commitment(r, c);
            w.raw(c, be.commitment_bytes());
        }
        w.ext(q_eval);
        w.u64(max_log_row_count);
        w.u64(log_m);
        if (w.overflow || w.n != need) {
            set_error("internal error: jagged proof size %zu != expected %zu", w.n, need);
            return SP1HIP_ERROR_RUNTIME;
        }
        *proof_len = w.n;
        return SP1HIP_SUCCESS;
    }

    int prove() {
        timer.start();
        marks.next("jagged_setup");
        SP1HIP_TRY(check_and_size());
        const DeviceCtx* ctx;                                // (validation and the size query above need no device)
        SP1HIP_TRY(get_device_ctx(&ctx));
        SP1HIP_TRY(transcript_head());
        SP1HIP_TRY(upload_point_tables());
        marks.next("jagged_sumcheck");
        // the A/B switches (the GPU tests run both forms): SP1HIP_JAGGED_FACTORED=0 keeps every level generic,
        // SP1HIP_JAGGED_LOOKAHEAD=0 proves rounds 0 and 1 as two passes over the base words
        plan = plan_first_rounds(prefix, T, log_m, max_log_row_count, rounds, n_rounds, env_flag("SP1HIP_JAGGED_FACTORED", true),
                                 env_flag("SP1HIP_JAGGED_LOOKAHEAD", true));
        SP1HIP_TRY(alloc_tables());
        timer.lap(JgTimer::SETUP);
        SP1HIP_TRY(prove_sumcheck());
        SP1HIP_TRY(final_q_eval());
        timer.lap(JgTimer::SUMCHECK);
        marks.next("jagged_eval");
        SP1HIP_TRY(prove_jagged_eval());
        timer.lap(JgTimer::EVAL);
        marks.next("stacked_basefold_open");
        SP1HIP_TRY(open_dense());                            // (laps COLUMNS before the backend's open)
        timer.lap(JgTimer::BASEFOLD);
        SP1HIP_TRY(write_proof());
        be.accept();                                         // the caller's transcript moves on success only
        timer.lap(JgTimer::BYTES);
        timer.report(log_m);
        return SP1HIP_SUCCESS;
    }
};
#undef SP1HIP_JG_REQUIRE

}  // namespace

size_t jagged_proof_size_with(size_t opening_bytes, size_t commitment_bytes, const std::vector<uint32_t>& round_widths,
                              const std::vector<size_t>& tables_per_round, uint64_t total_area) {
    const int n_rounds = (int)round_widths.size();
    const int log_m = log2_ceil(total_area), D = log_m + 1;
    size_t need = opening_bytes;
    need += 8;
    for (uint32_t w : round_widths) need += 8 + (size_t)w * 16 + 16;
    need += 8 + (size_t)log_m * (8 + 48) + 16 + 8 + (size_t)log_m * 16 + 16;
    need += 8 + (size_t)2 * D * (8 + 48) + 16 + 8 + (size_t)2 * D * 16 + 16;
    need += 8;
    for (size_t t : tables_per_round) need += 8 + t * 16;
    need += 8 + (size_t)n_rounds * commitment_bytes + 16 + 8 + 8;
    return need;
}

// the inner configuration's size (also what shard.hip sizes a shard proof with)
size_t jagged_proof_size(int lsh, const std::vector<uint32_t>& round_widths, const std::vector<size_t>& tables_per_round,
                         uint64_t total_area, sp1hip_fri_config_t config) {
    return jagged_proof_size_with(sp1hip_basefold_proof_size(lsh, round_widths.data(), (int)round_widths.size(), config), 32, round_widths,
                                  tables_per_round, total_area);
}

int jagged_prove_with(JaggedBackend& be, const sp1hip_ext_t* h_z_row, int max_log_row_count, StackedCore* const* rounds, int n_rounds,
                      const sp1hip_ext_t* h_claims, const size_t* claims_per_round, sp1hip_fri_config_t config, uint8_t* h_proof,
                      size_t* proof_len, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(h_z_row && rounds && n_rounds > 0 && n_rounds <= 8 && claims_per_round && proof_len, "bad argument");
    SP1HIP_REQUIRE(max_log_row_count >= 0 && max_log_row_count <= 30, "max_log_row_count out of range");
    JgProver p{be, h_z_row, max_log_row_count, rounds, n_rounds, h_claims, claims_per_round, config, h_proof, proof_len, stream, S(stream)};
    return p.prove();
}

namespace {
// The inner configuration: the KoalaBear DuplexChallenger, sp1hip_basefold_prove, a commitment of 8 KoalaBear words.
struct InnerJaggedBackend final : JaggedBackend {
    sp1hip_challenger_t* caller;
    sp1hip_challenger_t* work = nullptr;
    sp1hip_stacked_data_t* const* rounds;
    int n_rounds;
    InnerJaggedBackend(sp1hip_challenger_t* c, sp1hip_stacked_data_t* const* r, int n) : caller(c), rounds(r), n_rounds(n) {}
    ~InnerJaggedBackend() override { sp1hip_challenger_free(work); }
    const char* entry_point() const override { return "sp1hip_jagged_prove"; }
    int begin() override { return sp1hip_challenger_clone(caller, &work); }
    void observe(uint32_t monty) override { challenger_observe(work, monty); }
    Ext sample_ext() override { return challenger_sample_ext(work); }
    void accept() override { challenger_restore(caller, work); }
    size_t opening_size(int dim, const uint32_t* widths, int n, sp1hip_fri_config_t config) const override {
        return sp1hip_basefold_proof_size(dim, widths, n, config);
    }
    int open(const sp1hip_ext_t* h_point, int dim, const sp1hip_ext_t* h_claims, size_t n_claims, sp1hip_fri_config_t config,
             uint8_t* h_proof, size_t* len, sp1hip_stream_t stream) override {
        std::vector<sp1hip_basefold_data_t*> bf;
        for (int r = 0; r < n_rounds; r++) bf.push_back(rounds[r]->basefold);
        return sp1hip_basefold_prove(h_point, dim, bf.data(), n_rounds, h_claims, n_claims, config, work, h_proof, len, stream);
    }
    size_t commitment_bytes() const override { return 32; }
    void write_commitment(int round, uint8_t* dst) const override {
        for (int k = 0; k < 8; k++) { const uint32_t v = kb::from_monty(rounds[round]->commit[k]); memcpy(dst + 4 * k, &v, 4); }
    }
};
}  // namespace
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

int sp1hip_jagged_prove(const sp1hip_ext_t* h_z_row, int max_log_row_count, sp1hip_stacked_data_t* const* rounds, int n_rounds,
                        const sp1hip_ext_t* h_claims, const size_t* claims_per_round, sp1hip_fri_config_t config,
                        sp1hip_challenger_t* challenger, uint8_t* h_proof, size_t* proof_len, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(rounds && n_rounds > 0 && n_rounds <= 8 && challenger, "bad argument");
    std::vector<StackedCore*> cores(rounds, rounds + n_rounds);
    InnerJaggedBackend be(challenger, rounds, n_rounds);
    return jagged_prove_with(be, h_z_row, max_log_row_count, cores.data(), n_rounds, h_claims, claims_per_round, config, h_proof,
                             proof_len, stream);
}

}  // extern "C"