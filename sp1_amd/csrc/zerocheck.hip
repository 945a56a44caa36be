// sp1_amd/csrc/zerocheck.hip — zerocheck sumcheck over AIR constraints on gfx950 (SURVEY §8 a9–a12): the prover.
//
// The zerocheck is three files:
//   zc_compile.hpp / .cpp    the constraint-program compiler, host code only: a chip's SSA program (include/sp1hip.h,
//                            sp1_amd/air.py) becomes register-allocated instruction words in three granularities plus the
//                            hinted sub-AIRs that fused pieces evaluate; plans are cached per process (zc_get_plan)
//   zc_kernels.hpp           every kernel: the LDS register file and the bytecode interpreter (zc_round_kernel), the fused
//                            pieces (zc_macro_kernel), the bivariate first two rounds (zc_biv_*), the polynomial identities,
//                            the reductions, the table updates (zc_fix_kernel, zc_fix2_kernel), the gather
//   zerocheck.hip            this file: the launches and the prover (ZcProver), one proof = zerocheck_prove_impl
//
//   zc_round_kernel & co.    `ZerocheckCpuProver::sum_as_poly_in_last_variable` + `increment_y_values`
//                            /root/reference/crates/hypercube/src/prover/zerocheck/sum_as_poly.rs:L53-L181,L355-L440
//                            with `ConstraintSumcheckFolder::assert_zero` (/root/reference/crates/hypercube/src/folder.rs:L276-L323)
//   zc_fix_kernel            `zerocheck_fix_last_variable` -> `mle_fix_last_variable`
//                            /root/reference/crates/hypercube/src/prover/zerocheck/fix_last_variable.rs:L8-L62,
//                            /root/reference/slop/crates/multilinear/src/restrict.rs:L11-L58
//   host driver              `ShardProver::zerocheck` (/root/reference/crates/hypercube/src/prover/shard.rs:L474-L646),
//                            `reduce_sumcheck_to_evaluation` (/root/reference/slop/crates/sumcheck/src/prover.rs:L13-L96),
//                            univariate assembly sum_as_poly.rs:L187-L287, `VirtualGeq`
//                            (/root/reference/slop/crates/multilinear/src/virtual_geq.rs:L12-L99)
//
// The kernel is a register machine per row pair — one lane = one pair of adjacent rows, evaluated at the interpolation
// nodes t = 0, 2, 4 (leaf = row0 + t (row1 - row0)), `acc += alpha_pow[k] * reg` per assert, plus the GKR-opening batching
// term, times eq(zeta', pair), block-reduced to three extension sums. Traces are column-major, so every leaf load of a
// wave is one coalesced 256 B run; the program, alpha/gkr powers and publics are wave-uniform
// scalar loads. Round 0 works on base-field words, later rounds on extension words (4 sub-columns
// per column). The register file lives in LDS (up to 160 extension registers per lane); hinted sub-AIRs (Poseidon2 permutation,
// septic curve, Keccak-f round) are evaluated by fused pieces with
// their state in VGPRs instead (zc_poseidon2.hpp). Per-chip compiled kernels were built in round 3,
// measured slower than this interpreter and removed in round 4.
#include <algorithm>
#include <array>
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include "zc_compile.hpp"
#include "zc_kernels.hpp"

namespace sp1hip {

constexpr uint32_t ZC_MONO_MIN_TERMS = 1024; // rounds with at least this many row pairs run a chip's program in ONE piece
// rounds with at most this many workgroups (x 3 nodes) launch their groups / fused pieces on fork streams; the default forks every round
// (the large rounds gain the overlap of one launch's tail with the next one's head).
constexpr uint32_t ZC_FORK_MAX_BLOCKS = 1u << 30;
// the interpreter's workgroups of one chunk cover at most this many row pairs (quads in the bivariate rounds) per pass: the blocks of a
// taller chip stride over the rest
constexpr uint32_t ZC_MAX_PAIRS = 131072;
// rounds with at most this many workgroups are "small": every launch is at its latency floor (the two septic kinds then share one launch)
constexpr uint32_t ZC_SMALL_ROUND_WGS = 16384;
// Side streams of a round's launches, besides the caller's own. ZC_FORK_STREAMS are requested (+ the caller's = the four hardware
// queues a process gets by default) and size the per-stream state; ZC_N_FORK of them are used. Two since the end of round 5: with
// three, the commit's side stream shares a queue with one of them; measured A/B/A/B on one box, whole proof: fibonacci shard
// 89.2 -> 86.4-86.8 ms, recorded-shape shard 76.8 -> 74.7 (one fork: 88.0 / —)
constexpr int ZC_FORK_STREAMS = 3, ZC_N_FORK = 2;

static Ext ext_c(uint32_t canonical) { return kb::ext_from_base(kb::to_monty(canonical)); }
using UniPoly = std::vector<Ext>;

struct VGeq {
    uint32_t threshold;
    Ext geq_c, eq_c;
    VGeq fix(const Ext& alpha) const {
        VGeq r;
        r.threshold = threshold >> 1;
        r.geq_c = geq_c;
        r.eq_c = (threshold & 1) == 0 ? (kb::ext_one() - alpha) * eq_c : alpha * (eq_c + geq_c) - geq_c;
        return r;
    }
    Ext at(size_t idx) const {
        if (idx < threshold) return kb::ext_zero();
        if (idx == threshold) return eq_c + geq_c;
        return geq_c;
    }
};

struct DevBuf {
    void* p = nullptr;
    hipStream_t s = nullptr;
    size_t n = 0;
    int alloc(size_t bytes, hipStream_t stream) {
        s = stream;
        n = bytes;
        return arena_alloc(&p, bytes, stream);
    }
    void release() { arena_free(p, n, s); p = nullptr; }
    ~DevBuf() { release(); }
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    uint32_t* u32() const { return (uint32_t*)p; }
};

// register-file bytes one lane needs in LDS
template <bool FIRST> static inline size_t zc_rf_lane_bytes(uint32_t n_regs) { return (size_t)n_regs * (FIRST ? 4 : 16); }
constexpr size_t ZC_LDS_CU = 160 * 1024;          // LDS of a gfx950 compute unit; one workgroup may declare all of it
constexpr size_t ZC_LDS_BUDGET = ZC_LDS_CU;

// The workgroup width (256 / 128 / 64 lanes) that keeps the most lanes resident per compute unit given what the LDS register
// file costs: a CU holds floor(160 KB / LDS per workgroup) workgroups, so a file of R extension registers (16 R bytes per lane)
// allows ~10240 / R lanes however they are grouped, and narrower workgroups pack the remainder better (R = 50: three 64-lane
// workgroups = 192 lanes against one 128-lane workgroup). Ties go to the wider workgroup. 0 if even one wave's file does not
// fit 160 KB (R > 160 in the extension rounds): the caller then runs the chip's finer chunks.
template <bool FIRST> static inline uint32_t zc_wg_for(uint32_t n_regs, size_t other_lds) {
    // Measured (end of round 5, two fork streams) against the widest workgroup whose file fits 64 KB, the rule of rounds 2-4:
    // fibonacci shard 86.4-86.8 either way, recorded-shape shard 74.7 -> 74.2-74.6 (a 15-register program runs 640 lanes per CU
    // instead of 512, a 7-register one 2,048 instead of 1,280)
    uint32_t best = 0, best_lanes = 0;
    for (uint32_t wg = 256; wg >= 64; wg >>= 1) {
        const size_t per_wg = other_lds + zc_rf_lane_bytes<FIRST>(n_regs) * wg;
        if (per_wg > ZC_LDS_CU) continue;
        const uint32_t lanes = (uint32_t)std::min<size_t>(ZC_LDS_CU / per_wg, 2048 / wg) * wg;      // also: 32 waves per CU
        if (lanes > best_lanes) { best_lanes = lanes; best = wg; }
    }
    return best;
}

// One launch of the interpreter = a group of descriptors with a contiguous block range [block_lo, block_lo + n_blocks): chips whose
// programs run the same way this round (plan_round)
struct Group { bool staged; uint32_t wg, resident, max_regs, max_instr, block_lo, n_blocks; std::vector<int> chips; };
// FIRST: the register file holds base words (4 B slots); wgs_per_block workgroups evaluate the nodes of one block of rows
template <bool FIRST, class Kernel>
static int launch_interpreter(Kernel kern_staged, Kernel kern_plain, uint32_t wgs_per_block, const Group& g, const ZcDesc* d_descs, int n_descs,
                              const uint32_t* eq, uint32_t eq_len, const uint32_t* publics, uint32_t* partial, hipStream_t s) {
    const size_t lds = 32 * 4 + (g.staged ? (size_t)g.max_instr * 16 : 0);
    const uint32_t wg = zc_wg_for<FIRST>(g.max_regs, lds);
    SP1HIP_REQUIRE(wg != 0, "internal: a register file that does not fit LDS reached the launch (plan_round cuts such programs finer)");
    const size_t total = lds + zc_rf_lane_bytes<FIRST>(g.max_regs) * wg;
    const Kernel kern = g.staged ? kern_staged : kern_plain;
    if (total > 48 * 1024) SP1HIP_TRY(ensure_dynamic_lds((const void*)kern, (int)ZC_LDS_BUDGET));
    hipLaunchKernelGGL(kern, dim3(g.n_blocks * wgs_per_block), dim3(wg), total, s, d_descs, n_descs, eq, eq_len, publics, partial, (uint32_t)(lds / 4), g.block_lo);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}
template <bool FIRST, class... Args> static int launch_round(const Group& g, Args... args) {      // workgroup 3 b + p = node p of block b
    return launch_interpreter<FIRST>(zc_round_kernel<FIRST, 0, true>, zc_round_kernel<FIRST, 0, false>, 3u, g, args...);
}
// the bivariate kernels: three node-group workgroups per block of row quads, 16-byte slots (four node values per register)
template <class... Args> static int launch_biv_round(const Group& g, Args... args) {
    return launch_interpreter<false>(zc_biv_round_kernel<0, true>, zc_biv_round_kernel<0, false>, (uint32_t)ZC_BIV_GROUPS, g, args...);
}

struct ByteOut {
    std::vector<uint8_t> b;
    void u64(uint64_t v) { for (int i = 0; i < 8; i++) b.push_back((uint8_t)(v >> (8 * i))); }
    void ext(const Ext& e) {
        for (int k = 0; k < 4; k++) { uint32_t c = kb::from_monty(e.c[k]); for (int i = 0; i < 4; i++) b.push_back((uint8_t)(c >> (8 * i))); }
    }
};

// transcript hooks implemented in prover.hip
void challenger_observe(sp1hip_challenger_t* ch, uint32_t x);
kb::Ext challenger_sample_ext(sp1hip_challenger_t* ch);
void challenger_restore(sp1hip_challenger_t* dst, const sp1hip_challenger_t* src);
// basefold.hip: every prefix table of eq over the first t coordinates of a point, t = 0..d, one launch
int eq_prefix_tables_soa_async(const kb::Ext* h_point, int d, uint32_t* d_out, hipStream_t s);

// ---- the device side of a chip: its plan, where its programs and power tables sit in the call's constant blob, its tables
struct ChipState {
    const sp1hip_zc_chip_t* in;
    std::vector<ZcMacro> macros;
    std::shared_ptr<const ZcPlan> plan;   // (the polynomial identities' forms live in the plan)
    std::vector<size_t> poly_off;   // per macro: word offset of its device table in the call's constant blob (kind 7 only)
    const uint32_t* p_blob = nullptr;
    std::vector<Ext> alpha_pows, gkr_pows;
    std::vector<Chunk> chunks;         // split at assert boundaries (parallel across constraints: the small rounds)
    std::vector<uint32_t> chunk_off;   // offset (in instructions) of each chunk inside d_prog
    std::vector<Chunk> mono;           // the undivided program (+ a TOUCH chunk): no recomputation (the large rounds)
    std::vector<uint32_t> mono_off;
    std::vector<Chunk> fine;           // short pieces for the last, latency-bound rounds
    std::vector<uint32_t> fine_off;
    size_t off_prog = 0, off_alpha = 0, off_gkr = 0;     // word offsets into the call's single constant blob
    const uint32_t* p_prog = nullptr;
    const uint32_t* p_alpha = nullptr;
    const uint32_t* p_gkr = nullptr;
    const uint32_t* d_main = nullptr;
    const uint32_t* d_prep = nullptr;
};

// ---- the transcript side of a round: one round's messages from the chips' values at 0, 2, 4 (sum_as_poly.rs:L187-L287), the
// challenger, the claims behind it. Host arithmetic only: nothing here touches a device object.
// hv[i][k]: chip i's round polynomial at X = 0, 2, 4 WITHOUT the eq factor of the variable being bound (`last` = its zeta
// coordinate); the value at 1 comes from the chip's running claim. sum_as_poly interpolates through {0, 1, 2, 4, b} with the
// value at b equal to zero. Closed form, no allocation: the Lagrange basis polynomial of node x_k in {0, 1, 2, 4} is
// C_k(X) (X - b) / (x_k - b), with C_k the basis polynomial of x_k among those four nodes alone — constants of the field:
//   C_0 = (X^3 - 7 X^2 + 14 X - 8) / -8, C_1 = (X^3 - 6 X^2 + 8 X) / 3, C_2 = (X^3 - 5 X^2 + 4 X) / -4, C_3 = (X^3 - 3 X^2 + 2 X) / 24
// so a chip's univariate is (X - b) sum_k z_k C_k(X) with z_k = y_k / (x_k - b); the four inverses come from one
// inversion (Montgomery's trick). Exact field arithmetic: the same polynomial as any other interpolation.
struct CubicBasis {
    uint32_t c[4][4];                                     // c[k][d]: coefficient of X^d in C_k (Montgomery base words)
    CubicBasis() {
        const int num[4][4] = {{-8, 14, -7, 1}, {0, 8, -6, 1}, {0, 4, -5, 1}, {0, 2, -3, 1}};
        const int den[4] = {-8, 3, -4, 24};
        for (int k = 0; k < 4; k++) {
            const uint32_t dm = kb::to_monty(den[k] < 0 ? kb::P - (uint32_t)(-den[k]) : (uint32_t)den[k]);
            const uint32_t dinv = kb::ext_inv(kb::ext_from_base(dm)).c[0];
            for (int d = 0; d < 4; d++) {
                const uint32_t nm = kb::to_monty(num[k][d] < 0 ? kb::P - (uint32_t)(-num[k][d]) : (uint32_t)num[k][d]);
                c[k][d] = kb::mul(nm, dinv);
            }
        }
    }
};
static const CubicBasis& cubic_basis() {
    static const CubicBasis cubic;
    return cubic;
}

struct ChipClaim {                  // what the transcript follows of a chip
    uint64_t rows = 0;              // its table's height in the current round
    Ext eq_adj, pad_adj;            // eq over the variables bound so far; the constraints' value on a padded row
    VGeq vgeq;
};

// The interpolation is the SAME linear map for every chip (its nodes and b depend on the round only), so the transcript's
// message — the lambda-combination of the chips' polynomials — is the interpolation of the lambda-combined node values: four
// products per chip and ONE interpolation stand between the round's sums and the challenge, instead of an interpolation per
// chip (34 chips: ~35 us of host arithmetic per round with the device idle behind it). A chip's next claim u_i(a_r) is again
// linear in its node values, sum_k y_k e_k with e_k = (a_r - b) C_k(a_r) / (x_k - b): four more products per chip, taken
// AFTER the table update of the round has been launched (update_claims).
struct RoundTranscript {
    sp1hip_challenger_t* challenger = nullptr;
    int n_chips = 0;
    Ext lambda;
    std::vector<ChipClaim> chip;
    std::vector<Ext> claims;                                 // the chips' claimed sums (the GKR openings, batched)
    std::vector<Ext> round_claims;
    std::vector<Ext> lam_pows;                               // chip i's weight lambda^(n_chips - 1 - i): rlc = (...(u_0 l + u_1) l + ...) + u_last
    std::vector<std::array<Ext, 4>> ys;                      // a chip's round polynomial at 0, 1, 2, 4 (with the bound variable's eq factor)
    Ext claim_w[4];                                          // e_k of the round whose claims are pending
    Ext pending_a = kb::ext_zero(), pending_last = kb::ext_zero();
    bool claims_pending = false;
    std::vector<UniPoly> msgs;
    std::vector<Ext> point;   // [alpha_last, ..., alpha_first]

    // (after `chip` and `claims` are filled) samples the chips' batching challenge
    void begin(sp1hip_challenger_t* ch) {
        challenger = ch;
        n_chips = (int)chip.size();
        lambda = challenger_sample_ext(challenger);
        round_claims = claims;
        lam_pows.resize(n_chips);
        { Ext cur = kb::ext_one(); for (int i = n_chips - 1; i >= 0; i--) { lam_pows[i] = cur; cur = cur * lambda; } }
        ys.resize(n_chips);
    }
    void update_claims() {
        if (!claims_pending) return;
        claims_pending = false;
        for (int i = 0; i < n_chips; i++) {
            ChipClaim& c = chip[i];
            // the variable is bound: the virtual geq polynomial and the eq factor of the bound variables follow (fix_last_variable.rs)
            c.vgeq = c.vgeq.fix(pending_a);
            if (c.rows == 0) { round_claims[i] = kb::ext_zero(); continue; }
            round_claims[i] = ys[i][0] * claim_w[0] + ys[i][1] * claim_w[1] + ys[i][2] * claim_w[2] + ys[i][3] * claim_w[3];
            c.eq_adj = c.eq_adj * (pending_a * pending_last + (kb::ext_one() - pending_a) * (kb::ext_one() - pending_last));
        }
    }
    Ext round_messages(const Ext& last, const std::vector<std::array<Ext, 3>>& hv) {
        const CubicBasis& cubic = cubic_basis();
        update_claims();                                          // (a caller that did not: the claims of the previous round)
        const Ext b_node = (kb::ext_one() - last) * kb::ext_inv(kb::ext_one() - (last + last));
        Ext inv_xb[4];                                            // 1 / (x_k - b), x = 0, 1, 2, 4
        {
            const Ext dx[4] = {kb::ext_zero() - b_node, kb::ext_one() - b_node, ext_c(2) - b_node, ext_c(4) - b_node};
            const Ext p01 = dx[0] * dx[1], p012 = p01 * dx[2], p0123 = p012 * dx[3];
            Ext run = kb::ext_inv(p0123);
            inv_xb[3] = run * p012; run = run * dx[3];
            inv_xb[2] = run * p01; run = run * dx[2];
            inv_xb[1] = run * dx[0];
            inv_xb[0] = run * dx[1];
        }
        const Ext three = ext_c(3), seven = ext_c(7);
        const Ext f0 = kb::ext_one() - last, f2 = last * three - kb::ext_one(), f4 = last * seven - three;
        Ext Y[4] = {kb::ext_zero(), kb::ext_zero(), kb::ext_zero(), kb::ext_zero()};
        for (int i = 0; i < n_chips; i++) {
            if (chip[i].rows == 0) continue;
            const Ext y0 = hv[i][0] * f0;
            ys[i] = {y0, round_claims[i] - y0, hv[i][1] * f2, hv[i][2] * f4};
            for (int k = 0; k < 4; k++) Y[k] = Y[k] + ys[i][k] * lam_pows[i];
        }
        // (X - b) sum_k z_k C_k(X), z_k = Y_k / (x_k - b): coefficient d of the sum is g[d]
        UniPoly rlc(n_chips ? 5 : 1, kb::ext_zero());
        if (n_chips) {
            const Ext z[4] = {Y[0] * inv_xb[0], Y[1] * inv_xb[1], Y[2] * inv_xb[2], Y[3] * inv_xb[3]};
            Ext g[4];
            for (int d = 0; d < 4; d++) {
                Ext acc = kb::ext_mul_base(z[0], cubic.c[0][d]);
                for (int k = 1; k < 4; k++) acc = acc + kb::ext_mul_base(z[k], cubic.c[k][d]);
                g[d] = acc;
            }
            rlc[0] = kb::ext_zero() - b_node * g[0];
            for (int d = 1; d < 4; d++) rlc[d] = g[d - 1] - b_node * g[d];
            rlc[4] = g[3];
        }
        for (auto& cf : rlc)
            for (int k = 0; k < 4; k++) challenger_observe(challenger, cf.c[k]);
        msgs.push_back(rlc);
        const Ext a_r = challenger_sample_ext(challenger);
        point.insert(point.begin(), a_r);
        // e_k = (a_r - b) C_k(a_r) / (x_k - b)
        {
            const Ext a2 = a_r * a_r, a3 = a2 * a_r, ab = a_r - b_node;
            for (int k = 0; k < 4; k++) {
                const Ext ck = kb::ext_from_base(cubic.c[k][0]) + kb::ext_mul_base(a_r, cubic.c[k][1]) + kb::ext_mul_base(a2, cubic.c[k][2]) + kb::ext_mul_base(a3, cubic.c[k][3]);
                claim_w[k] = ab * ck * inv_xb[k];
            }
        }
        pending_a = a_r; pending_last = last; claims_pending = true;
        return a_r;
    }
    // the node values of a round from its sums (three extension sums and the eq entry of the first padded pair, per chip): the
    // values of every chip's round polynomial at 0, 2, 4 without the eq factor of the variable being bound
    void node_values(const std::vector<std::array<uint32_t, 16>>& sums, std::vector<std::array<Ext, 3>>& hv) const {
        const Ext two = ext_c(2), four = ext_c(4);
        for (int i = 0; i < n_chips; i++) {
            const ChipClaim& c = chip[i];
            if (c.rows == 0) continue;
            const size_t th = (size_t)((c.rows + 1) / 2) - 1;
            const Ext eq_th{{sums[i][12], sums[i][13], sums[i][14], sums[i][15]}};
            const Ext msb = c.eq_adj * eq_th;
            const Ext y0s{{sums[i][0], sums[i][1], sums[i][2], sums[i][3]}}, y2s{{sums[i][4], sums[i][5], sums[i][6], sums[i][7]}},
                y4s{{sums[i][8], sums[i][9], sums[i][10], sums[i][11]}};
            const Ext v0 = c.vgeq.fix(kb::ext_zero()).at(th), v2 = c.vgeq.fix(two).at(th), v4 = c.vgeq.fix(four).at(th);
            const Ext pm = c.pad_adj * msb;
            hv[i] = {y0s * c.eq_adj - pm * v0, y2s * c.eq_adj - pm * v2, y4s * c.eq_adj - pm * v4};
        }
    }
    // the tables were folded: `unit` rows became one
    void fold_rows(uint64_t unit) {
        for (ChipClaim& c : chip)
            if (c.rows) c.rows = (c.rows + unit - 1) / unit;
    }
};

// ---- per chip: H(X, Y) on {0, 1, 2, 4}^2 from the sums of the bivariate kernels (bsums: ZC_BIV_SUM_WORDS words per reduction
// range, desc_chip: the chip of each range). Boolean corners: the GKR term's corner sums (constraints vanish on real rows, a
// padded row's constant cancels against geq). Elsewhere: A + (bilinear extension of the corner sums) - pad_adj eq[qb] geq_b(X, Y),
// qb = the quad of the first padded row, geq_b = the bilinear extension of [row >= rows] over that quad (zero when it
// holds no real row: such a quad is not summed and cancels by itself).
using BivNodes = std::array<std::array<Ext, 4>, 4>;          // H[x index][y index], the index of a coordinate in {0, 1, 2, 4}
static void assemble_biv_nodes(const std::vector<int>& desc_chip, const std::vector<uint32_t>& bsums, const std::vector<ChipClaim>& chip,
                               std::vector<BivNodes>& H) {
    static const int NODE_X[12] = {0, 0, 1, 1, 2, 2, 2, 2, 4, 4, 4, 4}, NODE_Y[12] = {2, 4, 2, 4, 0, 1, 2, 4, 0, 1, 2, 4};
    auto xi = [](int v) { return v == 4 ? 3 : v; };             // index of a coordinate in {0, 1, 2, 4}
    auto small = [](int64_t v) -> Ext { return ext_c((uint32_t)(((v % (int64_t)kb::P) + (int64_t)kb::P) % (int64_t)kb::P)); };
    const int n_chips = (int)chip.size();
    std::vector<std::array<Ext, 17>> cs(n_chips);           // merged sums of a chip's ranges: A_0..11, B_0..3, eq[qb]
    std::vector<char> have(n_chips, 0);
    for (size_t k = 0; k < desc_chip.size(); k++) {
        const int ci = desc_chip[k];
        const uint32_t* src = bsums.data() + k * ZC_BIV_SUM_WORDS;
        for (int e = 0; e < 17; e++) {
            const Ext v{{src[4 * e], src[4 * e + 1], src[4 * e + 2], src[4 * e + 3]}};
            if (!have[ci] || e == 16) cs[ci][e] = v; else cs[ci][e] = cs[ci][e] + v;
        }
        have[ci] = 1;
    }
    for (int i = 0; i < n_chips; i++) {
        const ChipClaim& c = chip[i];
        if (c.rows == 0) continue;
        const Ext* A = cs[i].data();
        const Ext G00 = cs[i][12], G01 = cs[i][13], G10 = cs[i][14], G11 = cs[i][15];   // B_e: corner (X, Y) = (e >> 1, e & 1)
        const Ext gx = G10 - G00, gy = G01 - G00, gxy = (G11 - G10) - gy;
        const int m = (int)(c.rows % 4);                    // rows of the boundary quad that are real
        const Ext pe = m ? c.pad_adj * cs[i][16] : kb::ext_zero();
        H[i][0][0] = G00; H[i][0][1] = G01; H[i][1][0] = G10; H[i][1][1] = G11;
        for (int e = 0; e < 12; e++) {
            const int x = NODE_X[e], y = NODE_Y[e];
            Ext h = A[e] + G00 + gx * small(x) + gy * small(y) + gxy * small(x * y);
            if (m) {
                const int i01 = 1 >= m, i10 = 2 >= m;           // [row 4 qb + k >= rows] for k = 1, 2 (k = 0: real, k = 3: padded)
                const int64_t gq = (int64_t)x * i10 + (int64_t)y * i01 + (int64_t)x * y * (1 - i10 - i01);
                h = h - pe * small(gq);
            }
            H[i][xi(x)][xi(y)] = h;
        }
    }
}

// ---- the plan of a round: which chips run in which form, the descriptors of every launch, the reduction ranges and the table
// update that ends the round. It depends on the tables' heights and addresses only — not on anything the transcript
// produces — so round r + 1 is planned and its descriptors uploaded while round r's kernels run (the host used to do
// this between the fix launch and the round's first launch, ~35 us per round with the device idle).
struct RoundPlan {
    std::vector<ZcDesc> descs;
    std::vector<ZcChipRange> ranges;
    std::vector<int> desc_chip;
    std::vector<Group> groups;
    uint32_t total_blocks = 0, macro_lo[ZC_MACRO_KINDS + 1] = {}, macro_n[ZC_MACRO_KINDS + 1] = {};
    bool poly_wave = false;                             // the polynomial identities run one wave per row pair this round (zc_poly_wave_kernel)
    std::vector<ZcFixDesc> fds;
    std::vector<uint32_t*> fresh;
    std::vector<std::pair<int, bool>> owner;
    uint32_t fix_blocks = 0;
    size_t off_ranges = 0, off_fds = 0, pack_bytes = 0;
    std::vector<uint8_t> pack;
    std::vector<uint64_t> rows_next;
    std::vector<const uint32_t*> main_next, prep_next;
    // launches of the round: one per interpreter group, one per kind of fused piece that has blocks
    int n_launches() const { return (int)groups.size() + (macro_n[1] ? 1 : 0) + (macro_n[2] ? 1 : 0) + (macro_n[3] ? 1 : 0) + (macro_n[5] ? 1 : 0) + (macro_n[7] ? 1 : 0); }
};
struct PlanViews { const ZcDesc* descs; const ZcChipRange* ranges; const ZcFixDesc* fds; };    // an uploaded plan on the device

// ---- the fork and join of a round's launches. They read the same tables and write disjoint slots of d_partial: nothing orders
// them but the stream. They go out on fork streams — a round then costs its LONGEST launch instead of their sum (five launches
// of 30-70 us each in the last fifteen rounds of a core shard; in the large rounds one launch's tail overlaps the next one's
// head). begin() records the fork event on the caller's stream (behind the descriptor upload and the previous round's fix), a
// side stream waits for it when it is first handed out, join() puts the caller's stream behind every side stream that was used.
struct RoundFork {
    hipStream_t s = nullptr;
    bool forked = false;
    hipStream_t* fork_s = nullptr;
    hipEvent_t* fork_ev = nullptr;
    bool used[ZC_FORK_STREAMS] = {};
    int begin(hipStream_t caller, bool fork) {
        s = caller;
        forked = fork;
        if (forked) {
            SP1HIP_TRY(fork_streams_for(s, ZC_FORK_STREAMS, &fork_s, &fork_ev));
            SP1HIP_HIP(hipEventRecord(fork_ev[0], s));
        }
        return SP1HIP_SUCCESS;
    }
    int stream_of(int slot, hipStream_t* out) {                 // slot 0: the caller's stream
        *out = s;
        if (!forked || slot == 0) return SP1HIP_SUCCESS;
        if (slot > ZC_N_FORK) slot = 1 + (slot - 1) % ZC_N_FORK;
        if (!used[slot - 1]) { used[slot - 1] = true; SP1HIP_HIP(hipStreamWaitEvent(fork_s[slot - 1], fork_ev[0], 0)); }
        *out = fork_s[slot - 1];
        return SP1HIP_SUCCESS;
    }
    int join() {                                                // the reduction (and everything after it) follows every launch
        if (forked)
            for (int k = 0; k < ZC_FORK_STREAMS; k++)
                if (used[k]) {
                    SP1HIP_HIP(hipEventRecord(fork_ev[1 + k], fork_s[k]));
                    SP1HIP_HIP(hipStreamWaitEvent(s, fork_ev[1 + k], 0));
                }
        return SP1HIP_SUCCESS;
    }
};

// ---- SP1HIP_ZC_TIMING=1: host wall time of the call's three parts on stderr (set-up before the first round | rounds | proof),
// the rounds split into what the host spends planning and launching, waiting for the sums, and on the univariates and the transcript
struct ZcTimer {
    enum Part { PLAN, WAIT, UNI };
    using Clock = std::chrono::steady_clock;
    bool on = false;
    Clock::time_point t0, t1, t2, iter;
    double part_ms[3] = {0, 0, 0};
    static double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }
    void start() { on = env_flag("SP1HIP_ZC_TIMING", false); t0 = t1 = t2 = iter = Clock::now(); }
    void setup_done() { t1 = iter = Clock::now(); }
    void lap(Part p) {                                          // the time since the previous lap goes to part p
        if (!on) return;
        const auto now = Clock::now();
        part_ms[p] += ms(iter, now);
        iter = now;
    }
    void rounds_done() { t2 = Clock::now(); }
    void report(int n_rounds) const {
        if (!on) return;
        fprintf(stderr, "[sp1hip zerocheck] set-up %.3f ms | %d rounds %.3f ms (planning + launches %.3f, waiting for the sums %.3f, univariates + transcript %.3f) | openings + proof %.3f ms\n",
                ms(t0, t1), n_rounds, ms(t1, t2), part_ms[PLAN], part_ms[WAIT], part_ms[UNI], ms(t2, Clock::now()));
    }
};

// ---- one proof. Members are declared in the order the call creates them: they are released in reverse.
struct ZcProver {
    // the call's arguments
    const sp1hip_zc_chip_t* chips;
    const int n_chips, L;
    const sp1hip_ext_t *h_zeta, *h_openings;
    const Ext alpha, gkr;
    const uint32_t* h_publics;
    const int n_publics;
    sp1hip_challenger_t* challenger;
    uint8_t* h_proof;
    size_t* proof_len;
    hipStream_t s;

    ActiveProver active;                                     // a stand-alone call counts as a prover too
    size_t need = 0;                                         // bytes of the proof
    const DeviceCtx* ctx = nullptr;
    ZcTimer timer;
    std::vector<uint32_t> publics;
    DevBuf d_publics;
    // Host staging vectors handed to hipMemcpyAsync live until the end of the call (`blob`, the ChipStates, the
    // RoundPlans): no synchronisation is needed just to keep a source buffer valid, and every
    // device->host hand-over goes through the mailbox (round_sync.hpp), so the stream is never drained mid-proof.
    Mailbox mb;
    RoundSyncHost rsync;                          // its counters carry the reduce kernel's last-workgroup ticket
    PinnedStage stage;                            // small uploads go through a pinned block (round_sync.hpp)
    std::vector<uint32_t> blob;                   // programs and power tables of every chip: one upload for the whole call
    std::vector<std::unique_ptr<ChipState>> st;
    DevBuf d_blob;
    std::vector<Ext> zeta;
    DevBuf d_eq_all;                              // eq(zeta[0 .. t), .) for every t < L
    RoundTranscript tr;
    std::vector<std::array<uint32_t, 16>> sums;
    std::vector<uint32_t> h_sums;                 // up to four reduction ranges per chip (interpreter + one per kind of fused piece)
    DevBuf d_partial, d_sums;
    size_t partial_cap = 0;
    DevBuf d_fold[2];                             // the folded extension tables of all chips, ping-pong
    // the descriptors of rounds r and r + 1 live in two buffers: round r + 1's go up while round r's launches read theirs
    DevBuf d_descs2[2];
    size_t descs_cap2[2] = {0, 0};
    // SP1HIP_ZC_BIVARIATE=0: the sequential first two rounds; SP1HIP_ZC_FORK=0: every launch of a round on the caller's stream
    // (A/B runs and the tests of those paths — read per call; the proof bytes are the same)
    bool fork_enabled = true, bivariate = true;
    std::vector<std::unique_ptr<RoundPlan>> plans;           // (kept until the call returns)

    ZcProver(const sp1hip_zc_chip_t* chips_, int n_chips_, int max_log_row_count, const sp1hip_ext_t* h_zeta_, const sp1hip_ext_t* h_openings_,
             sp1hip_ext_t alpha_c, sp1hip_ext_t gkr_c, const uint32_t* h_publics_, int n_publics_, sp1hip_challenger_t* challenger_,
             uint8_t* h_proof_, size_t* proof_len_, sp1hip_stream_t stream)
        : chips(chips_), n_chips(n_chips_), L(max_log_row_count), h_zeta(h_zeta_), h_openings(h_openings_),
          alpha{{alpha_c.c[0], alpha_c.c[1], alpha_c.c[2], alpha_c.c[3]}}, gkr{{gkr_c.c[0], gkr_c.c[1], gkr_c.c[2], gkr_c.c[3]}},
          h_publics(h_publics_), n_publics(n_publics_), challenger(challenger_), h_proof(h_proof_), proof_len(proof_len_), s(S(stream)) {}

    // ---- set-up, 1: the arguments; the size of the proof
    int check_arguments() {
        SP1HIP_REQUIRE(chips && n_chips > 0 && h_zeta && h_openings && challenger && proof_len, "null argument");
        SP1HIP_REQUIRE(L >= 1 && L <= 30, "max_log_row_count out of range");
        SP1HIP_REQUIRE(h_publics || n_publics == 0, "null publics");
        size_t total_w = 0;
        for (int i = 0; i < n_chips; i++) {
            // a chip may have no constraints at all (the reference's MemoryConst / MemoryVar only take part in lookups):
            // its columns still enter through the GKR-opening batching term (TOUCH pseudo-instructions, build_chunks)
            SP1HIP_REQUIRE(chips[i].program || chips[i].n_instr == 0, "null constraint program");
            SP1HIP_REQUIRE(chips[i].real_rows <= ((uint64_t)1 << L), "chip taller than 2^max_log_row_count");
            SP1HIP_REQUIRE(chips[i].real_rows == 0 || (chips[i].d_main || chips[i].main_width == 0), "null main trace");
            SP1HIP_REQUIRE(chips[i].real_rows == 0 || (chips[i].d_prep || chips[i].prep_width == 0), "null preprocessed trace");
            total_w += chips[i].main_width + chips[i].prep_width;
        }
        need = 8 + (size_t)L * (8 + 80) + 16 + 8 + (size_t)L * 16 + 16 + 8 + (size_t)n_chips * 8 + total_w * 16;
        if (!h_proof || *proof_len < need) {
            *proof_len = need;
            set_error("sp1hip_zerocheck_prove: proof buffer too small, need %zu bytes", need);
            return SP1HIP_ERROR_BUFFER_TOO_SMALL;
        }
        return SP1HIP_SUCCESS;
    }

    // ---- set-up, 2: the hand-over slots, every chip's plan and claim, the call's constant blob in one upload
    int setup_chips() {
        SP1HIP_TRY(get_device_ctx(&ctx));
        timer.start();
        publics.assign(h_publics, h_publics + n_publics);
        SP1HIP_TRY(d_publics.alloc((size_t)n_publics * 4, s));

        int max_constraints = 0;
        for (int i = 0; i < n_chips; i++) max_constraints = std::max<int>(max_constraints, chips[i].num_constraints);
        std::vector<Ext> pows(max_constraints);
        { Ext cur = kb::ext_one(); for (auto& x : pows) { x = cur; cur = cur * alpha; } }

        SP1HIP_TRY(mb.init(s));
        SP1HIP_TRY(rsync.init(s));
        SP1HIP_TRY(stage.init(s));
        if (n_publics) SP1HIP_TRY(stage.upload(d_publics.p, publics.data(), (size_t)n_publics * 4));
        Ext rho = kb::ext_zero();                     // 1 / alpha, once a chip needs it
        bool have_rho = false;
        std::vector<kb::Ext> poly_scratch[2];
        tr.chip.resize(n_chips);
        size_t oo = 0;
        for (int i = 0; i < n_chips; i++) {
            std::unique_ptr<ChipState> c(new ChipState());
            c->in = &chips[i];
            uint32_t asserts = 0;
            for (uint32_t k = 0; k < chips[i].n_instr; k++) {
                const uint32_t op = chips[i].program[3 * k], a = chips[i].program[3 * k + 1];
                SP1HIP_REQUIRE(op <= ZC_ASSERT_ZERO || op == ZC_HINT, "bad opcode in constraint program");
                if (op == ZC_ASSERT_ZERO) asserts++;
                if (op == ZC_LOAD_MAIN) SP1HIP_REQUIRE(a < chips[i].main_width, "main column out of range");
                if (op == ZC_LOAD_PREP) SP1HIP_REQUIRE(a < chips[i].prep_width, "preprocessed column out of range");
                if (op == ZC_PUBLIC) SP1HIP_REQUIRE((int)a < n_publics, "public value index out of range");
            }
            SP1HIP_REQUIRE(asserts == chips[i].num_constraints, "num_constraints does not match the program");
            {
                std::shared_ptr<const ZcPlan> plan;
                SP1HIP_TRY(zc_get_plan(chips[i].program, chips[i].n_instr, chips[i].main_width, chips[i].prep_width, i, &plan, chips[i].real_rows));
                c->chunks = plan->chunks; c->mono = plan->mono; c->fine = plan->fine;
                c->macros = plan->macros;
                c->plan = plan;
            }
            // [alpha^(n-1), ..., alpha, 1] so that the folder matches the verifier's Horner order
            c->alpha_pows.assign(pows.begin(), pows.begin() + chips[i].num_constraints);
            std::reverse(c->alpha_pows.begin(), c->alpha_pows.end());
            { Ext cur = gkr; for (uint32_t k = 0; k < chips[i].main_width + chips[i].prep_width; k++) { c->gkr_pows.push_back(cur); cur = cur * gkr; } }
            ChipClaim& cc = tr.chip[i];
            cc.pad_adj = zc_eval_zero_row(*c->plan, c->alpha_pows.data(), publics.data());
            Ext claim = kb::ext_zero();
            for (uint32_t k = 0; k < chips[i].main_width + chips[i].prep_width; k++, oo++) {
                const Ext o{{h_openings[oo].c[0], h_openings[oo].c[1], h_openings[oo].c[2], h_openings[oo].c[3]}};
                claim = claim + o * c->gkr_pows[k];
            }
            tr.claims.push_back(claim);
            cc.rows = chips[i].real_rows;
            cc.eq_adj = kb::ext_one();
            cc.vgeq = VGeq{(uint32_t)chips[i].real_rows, kb::ext_one(), kb::ext_zero()};
            c->d_main = chips[i].d_main;
            c->d_prep = chips[i].d_prep;
            // programs and power tables of every chip go into ONE blob: one upload for the whole call
            auto pad4 = [&]() { while (blob.size() & 3) blob.push_back(0); };
            pad4();
            c->off_prog = blob.size();
            for (auto form : {std::make_pair(&c->chunks, &c->chunk_off), std::make_pair(&c->mono, &c->mono_off), std::make_pair(&c->fine, &c->fine_off)})
                for (auto& ck : *form.first) {
                    form.second->push_back((uint32_t)((blob.size() - c->off_prog) / 4));
                    blob.insert(blob.end(), ck.prog.begin(), ck.prog.end());
                }
            pad4();
            c->off_alpha = blob.size();
            for (const Ext& e : c->alpha_pows) blob.insert(blob.end(), e.c, e.c + 4);
            c->off_gkr = blob.size();
            for (const Ext& e : c->gkr_pows) blob.insert(blob.end(), e.c, e.c + 4);
            // the polynomial identities' affine forms, collapsed for this proof's alpha (zc_poly.hpp)
            c->poly_off.assign(c->macros.size(), 0);
            for (size_t mi = 0; mi < c->macros.size(); mi++) {
                const ZcMacro& m = c->macros[mi];
                if (m.kind != ZC_HINT_POLY) continue;
                if (!have_rho) {
                    SP1HIP_REQUIRE(!kb::ext_eq(alpha, kb::ext_zero()), "the batching challenge is zero");
                    rho = kb::ext_inv(alpha); have_rho = true;
                }
                while (blob.size() & 7) blob.push_back(0);
                c->poly_off[mi] = blob.size();
                zc_poly_table(c->plan->polys[m.aux0], c->plan->poly_segs[m.aux0], c->alpha_pows.data() + m.first_constraint, rho, &blob, poly_scratch);
            }
            st.push_back(std::move(c));
        }
        SP1HIP_TRY(d_blob.alloc(std::max<size_t>(blob.size(), 4) * 4, s));
        SP1HIP_TRY(stage.upload(d_blob.p, blob.data(), blob.size() * 4));
        for (auto& c : st) {
            c->p_prog = d_blob.u32() + c->off_prog;
            c->p_alpha = d_blob.u32() + c->off_alpha;
            c->p_gkr = d_blob.u32() + c->off_gkr;
            c->p_blob = d_blob.u32();
        }
        return SP1HIP_SUCCESS;
    }

    // ---- set-up, 3: the transcript's batching challenge, the eq tables, the buffers of the rounds, the first round's plan
    int setup_rounds() {
        zeta.resize(L);
        memcpy(zeta.data(), h_zeta, (size_t)L * 16);
        tr.begin(challenger);
        // eq(zeta[0 .. t), .) for every t < L in ONE launch (basefold.hip: table t is an ext SoA of length 2^t at word offset
        // 4 (2^t - 1)); round r reads table L - r - 1. Three small launches per round before.
        SP1HIP_TRY(d_eq_all.alloc(((size_t)1 << L) * 16, s));
        SP1HIP_TRY(eq_prefix_tables_soa_async(zeta.data(), L - 1, d_eq_all.u32(), s));
        sums.resize(n_chips);
        h_sums.resize((size_t)n_chips * 64);
        SP1HIP_TRY(d_sums.alloc((size_t)n_chips * 256, s));
        // The folded extension tables of all chips live in two ping-pong buffers sized once (round r writes half r & 1;
        // every round's tables are half the size of the previous round's): no allocation inside the round loop — it used to
        // be ~66 arena calls per round.
        {
            size_t words[2] = {4, 4};
            for (int half = 0; half < 2; half++)
                for (int i = 0; i < n_chips; i++) {
                    uint64_t rows = chips[i].real_rows;
                    for (int k = 0; k < half && rows; k++) rows = (rows + 1) / 2;
                    if (rows == 0) continue;
                    const uint64_t out_rows = (rows + 1) / 2;
                    for (uint32_t width : {chips[i].main_width, chips[i].prep_width})
                        if (width) words[half] += (((size_t)out_rows * width * 4 + 3) & ~(size_t)3);
                }
            SP1HIP_TRY(d_fold[0].alloc(words[0] * 4, s));
            SP1HIP_TRY(d_fold[1].alloc(words[1] * 4, s));
        }
        timer.setup_done();
        fork_enabled = env_flag("SP1HIP_ZC_FORK", true);
        bivariate = env_flag("SP1HIP_ZC_BIVARIATE", true) && L >= 2;
        return plan_next(0);
    }

    // biv: the plan of rounds 0 AND 1 together (bivariate kernels): the units are row quads, the table update folds by both
    // challenges (zc_fix2_kernel) into the buffer round 1 would have written, the reduction ranges carry the quad of the first padded row
    int plan_round(int r, const std::vector<uint64_t>& vrows, const std::vector<const uint32_t*>& vmain,
                   const std::vector<const uint32_t*>& vprep, RoundPlan& rp, bool biv) {
        const uint64_t unit = biv ? 4 : 2;                  // rows per term
        // descriptors: one per (chip with real rows, chunk); a chip's blocks are contiguous. Chips are grouped by how
        // their programs run this round — (program staged in LDS?, workgroup width the LDS register file allows) — and
        // every group is one launch over its contiguous block range.
        std::vector<ZcDesc>& descs = rp.descs;
        std::vector<ZcChipRange>& ranges = rp.ranges;
        std::vector<int>& desc_chip = rp.desc_chip;
        std::vector<Group>& groups = rp.groups;
        std::vector<char> use_mono(n_chips, 0);
        for (int i = 0; i < n_chips; i++) {
            ChipState& c = *st[i];
            if (vrows[i] == 0) continue;
            const uint32_t terms = (uint32_t)((vrows[i] + unit - 1) / unit);
            uint32_t mono_regs = 1;
            for (auto& ck : c.mono) mono_regs = std::max(mono_regs, ck.n_regs);
            const uint32_t mono_wg = (r == 0 && !biv) ? zc_wg_for<true>(mono_regs, 128) : zc_wg_for<false>(mono_regs, 128);
            // the undivided program pays off when chunking recomputes a lot (long dependency chains shared by many
            // constraints); a program of self-contained constraints runs as chunks in every round: same work, small
            // register files, and as many workgroups as there are constraints
            size_t chunk_words = 0, mono_words = 0;
            for (auto& ck : c.chunks) chunk_words += ck.prog.size();
            for (auto& ck : c.mono) mono_words += ck.prog.size();
            // (a shorter undivided program with the same register file is NOT enough: measured on the term-major Poseidon2
            // program — 2,804 words undivided against 3,808 in 28 chunks, 20 registers either way — the undivided form is
            // 36 % slower: 45 KB of instruction words stream through a 16 KB scalar cache, a chunk's 2-5 KB stay in it)
            use_mono[i] = c.chunks.size() > 1 && terms >= ZC_MONO_MIN_TERMS && mono_wg != 0 && 2 * chunk_words > 3 * mono_words;
            if (!use_mono[i] && terms <= ZC_FINE_MAX_TERMS && c.fine.size() > c.chunks.size()) use_mono[i] = 2;
            const std::vector<Chunk>& cks = use_mono[i] == 1 ? c.mono : use_mono[i] == 2 ? c.fine : c.chunks;
            uint32_t regs = 1, instr = 1;
            for (auto& ck : cks) { regs = std::max(regs, ck.n_regs); instr = std::max<uint32_t>(instr, (uint32_t)(ck.prog.size() / 4)); }
            // programs stream through the scalar cache (wave-uniform s_load_dwordx4 straight into SGPRs: no LDS read and no
            // v_readfirstlane per instruction word, and the whole LDS budget goes to the register file). Staging programs
            // of up to SP1HIP_ZC_STAGE_MAX instructions in LDS instead was the default until it was measured 3-5 % slower
            // (recursion shard 14.6 vs 13.8 ms of round kernels, core-shaped 10.4 vs 10.1); the VGPR / scratch tier still stages.
            const uint32_t stage_max = (uint32_t)env_uint("SP1HIP_ZC_STAGE_MAX", 0);   // read per call (tests)
            bool staged = instr <= stage_max;
            uint32_t wg = (r == 0 && !biv) ? zc_wg_for<true>(regs, staged ? 128 + (size_t)instr * 16 : 128) : zc_wg_for<false>(regs, staged ? 128 + (size_t)instr * 16 : 128);
            if (wg == 0 && use_mono[i] != 2) {      // the file does not fit LDS even for one wave: the finest cut of the program
                use_mono[i] = 2;
                regs = 1; instr = 1;
                for (auto& ck : c.fine) { regs = std::max(regs, ck.n_regs); instr = std::max<uint32_t>(instr, (uint32_t)(ck.prog.size() / 4)); }
                staged = instr <= stage_max;
                wg = (r == 0 && !biv) ? zc_wg_for<true>(regs, staged ? 128 + (size_t)instr * 16 : 128) : zc_wg_for<false>(regs, staged ? 128 + (size_t)instr * 16 : 128);
            }
            SP1HIP_REQUIRE(wg != 0, "constraint program too large: one constraint keeps more than 160 extension values live (the LDS register file of one wave)");
            // A launch allocates its LDS register file for the LARGEST file among its chips, so a group is made of chips that keep
            // the same number of workgroups resident per CU on their own: until round 6 every chip of one workgroup width shared a
            // launch, and SyscallInstrs (32 rows, 23 registers) held the Add / Addi / Sub / Addw chips (7 registers, 4.5 million
            // rows of a fibonacci shard) to 3 workgroups of 128 lanes per CU where their own files allow 11. Chips too short for
            // occupancy to matter (the rounds that run the fine cut) share one group per width whatever their files.
            uint32_t resident = 0;
            if (terms > ZC_FINE_MAX_TERMS) {
                const size_t per_wg = (staged ? 128 + (size_t)instr * 16 : 128) + ((r == 0 && !biv) ? zc_rf_lane_bytes<true>(regs) : zc_rf_lane_bytes<false>(regs)) * wg;
                resident = (uint32_t)std::min<size_t>(ZC_LDS_CU / per_wg, 2048 / wg);
            }
            size_t g = 0;
            for (; g < groups.size(); g++) if (groups[g].staged == staged && groups[g].wg == wg && groups[g].resident == resident) break;
            if (g == groups.size()) groups.push_back(Group{staged, wg, resident, 1, 1, 0, 0, {}});
            groups[g].max_regs = std::max(groups[g].max_regs, regs);
            groups[g].max_instr = std::max(groups[g].max_instr, instr);
            groups[g].chips.push_back(i);
        }
        uint32_t& total_blocks = rp.total_blocks;
        total_blocks = 0;
        for (auto& g : groups) {
            g.block_lo = total_blocks;
            for (int i : g.chips) {
                ChipState& c = *st[i];
                const uint32_t terms = (uint32_t)((vrows[i] + unit - 1) / unit);
                const uint32_t bp = g.wg ? g.wg : 256u;
                uint32_t blocks = (terms + bp - 1) / bp;
                if (blocks > ZC_MAX_PAIRS / bp) blocks = std::max(1u, ZC_MAX_PAIRS / bp);
                const std::vector<Chunk>& cks = use_mono[i] == 1 ? c.mono : use_mono[i] == 2 ? c.fine : c.chunks;
                const std::vector<uint32_t>& offs = use_mono[i] == 1 ? c.mono_off : use_mono[i] == 2 ? c.fine_off : c.chunk_off;
                ZcChipRange rg{total_blocks, 0, biv ? (uint32_t)(vrows[i] / 4) : terms - 1, 0};
                for (size_t q = 0; q < cks.size(); q++) {
                    ZcDesc d{};
                    d.prog = c.p_prog + (size_t)offs[q] * 4;
                    d.n_instr = (uint32_t)(cks[q].prog.size() / 4);
                    d.main = vmain[i]; d.prep = vprep[i]; d.main_w = c.in->main_width; d.prep_w = c.in->prep_width;
                    d.rows = (uint32_t)vrows[i]; d.alpha_pows = c.p_alpha; d.gkr_pows = c.p_gkr;
                    d.block_start = total_blocks; d.n_blocks = blocks;
                    d.alpha_off = cks[q].alpha_off; d.flags = (q == 0 && !biv) ? 1u : 0u;
                    d.block_pairs = bp;
                    total_blocks += blocks;
                    descs.push_back(d);
                }
                rg.n_blocks = total_blocks - rg.block_start;
                ranges.push_back(rg);
                desc_chip.push_back(i);
            }
            g.n_blocks = total_blocks - g.block_lo;
        }
        // the fused pieces of hinted sub-AIRs: one launch per kind (each kind is its own kernel with its own register budget),
        // one block range — and one reduction range — per (kind, chip)
        uint32_t (&macro_lo)[ZC_MACRO_KINDS + 1] = rp.macro_lo;
        uint32_t (&macro_n)[ZC_MACRO_KINDS + 1] = rp.macro_n;
        // the polynomial identities: one lane per row pair while the round is large, one wave per pair once the tallest chip that has
        // them is down to ZC_POLY_WAVE_MAX_TERMS pairs
        {
            uint64_t max_terms = 0;
            for (int i = 0; i < n_chips; i++)
                for (const ZcMacro& m : st[i]->macros) if (m.kind == ZC_HINT_POLY && vrows[i]) max_terms = std::max<uint64_t>(max_terms, (vrows[i] + unit - 1) / unit);
            rp.poly_wave = !biv && r > 0 && max_terms > 0 && max_terms <= ZC_POLY_WAVE_MAX_TERMS;
        }
        for (uint32_t kind = ZC_HINT_POSEIDON2; kind < ZC_MACRO_KINDS; kind++) {
            if (kind == ZC_MACRO_BOTH_SEPTIC) continue;                   // (a launch shape, not a hint kind)
            macro_lo[kind] = total_blocks;
            for (int i = 0; i < n_chips; i++) {
                ChipState& c = *st[i];
                if (vrows[i] == 0) continue;
                const uint32_t terms = (uint32_t)((vrows[i] + unit - 1) / unit);
                const bool wave_form = kind == ZC_HINT_POLY && rp.poly_wave;
                const uint32_t blocks = wave_form ? std::min<uint32_t>((terms + 3) / 4, 1024u) : std::min<uint32_t>((terms + 255) / 256, 512u);
                ZcChipRange rg{total_blocks, 0, biv ? (uint32_t)(vrows[i] / 4) : terms - 1, 0};
                for (size_t mi = 0; mi < c.macros.size(); mi++) {
                    const ZcMacro& m = c.macros[mi];
                    if (m.kind != kind) continue;
                    for (uint32_t q = 0; q < m.n_pieces(); q++) {
                        ZcDesc d{};
                        if (kind == ZC_HINT_POLY) d.prog = c.p_blob + c.poly_off[mi];
                        d.main = vmain[i]; d.prep = vprep[i]; d.main_w = c.in->main_width; d.prep_w = c.in->prep_width;
                        d.rows = (uint32_t)vrows[i]; d.alpha_pows = c.p_alpha; d.gkr_pows = c.p_gkr;
                        d.block_start = total_blocks; d.n_blocks = blocks;
                        d.alpha_off = m.first_constraint; d.flags = ZC_DESC_MACRO | (q << 8) | (m.kind << 12);
                        d.block_pairs = wave_form ? 4 : 256; d.pad = m.base_col; d.aux0 = m.aux0; d.aux1 = m.aux1;
                            total_blocks += blocks;
                        descs.push_back(d);
                    }
                }
                rg.n_blocks = total_blocks - rg.block_start;
                if (rg.n_blocks) { ranges.push_back(rg); desc_chip.push_back(i); }
            }
            macro_n[kind] = total_blocks - macro_lo[kind];
        }
        // the bivariate rounds' GKR corner sums (zc_biv_corner_kernel): per chip, slices of ZC_CORNER_COLS columns x blocks of 256 quads,
        // one reduction range per chip
        macro_lo[ZC_RANGE_CORNERS] = total_blocks;
        if (biv)
            for (int i = 0; i < n_chips; i++) {
                ChipState& c = *st[i];
                if (vrows[i] == 0) continue;
                const uint32_t quads = (uint32_t)((vrows[i] + 3) / 4), width = c.in->main_width + c.in->prep_width;
                const uint32_t blocks = std::min<uint32_t>((quads + 255) / 256, 512u);
                ZcChipRange rg{total_blocks, 0, (uint32_t)(vrows[i] / 4), 0};
                for (uint32_t c0 = 0; c0 < width; c0 += ZC_CORNER_COLS) {
                    ZcDesc d{};
                    d.main = vmain[i]; d.prep = vprep[i]; d.main_w = c.in->main_width; d.prep_w = c.in->prep_width;
                    d.rows = (uint32_t)vrows[i]; d.alpha_pows = c.p_alpha; d.gkr_pows = c.p_gkr;
                    d.block_start = total_blocks; d.n_blocks = blocks;
                    d.flags = ZC_DESC_MACRO | (ZC_RANGE_CORNERS << 12);
                    d.block_pairs = 256; d.aux0 = c0; d.aux1 = std::min(width, c0 + ZC_CORNER_COLS);
                    total_blocks += blocks;
                    descs.push_back(d);
                }
                rg.n_blocks = total_blocks - rg.block_start;
                if (rg.n_blocks) { ranges.push_back(rg); desc_chip.push_back(i); }
            }
        macro_n[ZC_RANGE_CORNERS] = total_blocks - macro_lo[ZC_RANGE_CORNERS];
        // the table update that ends this round needs nothing from the transcript but alpha (a kernel argument): plan
        // it now, so that every descriptor of the round goes up in ONE copy
        std::vector<ZcFixDesc>& fds = rp.fds;
        std::vector<uint32_t*>& fresh = rp.fresh;              // the folded tables: slices of the round's half of the ping-pong buffer
        std::vector<std::pair<int, bool>>& owner = rp.owner;   // (chip, is_main)
        uint32_t& fix_blocks = rp.fix_blocks;
        fix_blocks = 0;
        size_t fold_words = 0;
        uint32_t* const fold_base = (uint32_t*)d_fold[biv ? 1 : (r & 1)].p;
        for (int i = 0; i < n_chips; i++) {
            ChipState& c = *st[i];
            if (vrows[i] == 0) continue;
            const uint64_t out_rows = (vrows[i] + unit - 1) / unit;
            for (int which = 0; which < 2; which++) {
                const uint32_t width = which == 0 ? c.in->main_width : c.in->prep_width;
                if (width == 0) continue;
                uint32_t* const nb = fold_base + fold_words;
                fold_words += ((size_t)out_rows * width * 4 + 3) & ~(size_t)3;
                ZcFixDesc fd{};
                fd.in = which == 0 ? vmain[i] : vprep[i];
                fd.out = nb;
                fd.rows = (uint32_t)vrows[i]; fd.width = width; fd.block_start = fix_blocks;
                fd.bpc = (uint32_t)((out_rows + ZC_FIX_ROWS - 1) / ZC_FIX_ROWS);
                fd.bpc_magic = (uint32_t)((((uint64_t)1 << 32) / fd.bpc) & 0xffffffffull);      // (bpc == 1 is special-cased in the kernel)
                fd.n_blocks = fd.bpc * width;
                fix_blocks += fd.n_blocks;
                fds.push_back(fd);
                fresh.push_back(nb);
                owner.push_back({i, which == 0});
            }
        }
        const size_t off_ranges = rp.off_ranges = (descs.size() * sizeof(ZcDesc) + 15) & ~(size_t)15;
        const size_t off_fds = rp.off_fds = (off_ranges + ranges.size() * sizeof(ZcChipRange) + 15) & ~(size_t)15;
        const size_t pack_bytes = rp.pack_bytes = off_fds + fds.size() * sizeof(ZcFixDesc);
        std::vector<uint8_t>& pack = rp.pack;
        pack.assign(std::max<size_t>(pack_bytes, 16), 0);
        if (!descs.empty()) memcpy(pack.data(), descs.data(), descs.size() * sizeof(ZcDesc));
        if (!ranges.empty()) memcpy(pack.data() + off_ranges, ranges.data(), ranges.size() * sizeof(ZcChipRange));
        if (!fds.empty()) memcpy(pack.data() + off_fds, fds.data(), fds.size() * sizeof(ZcFixDesc));
        // the tables the round AFTER this one reads (once the fix launch planned above has run)
        rp.rows_next = vrows; rp.main_next = vmain; rp.prep_next = vprep;
        for (size_t k = 0; k < fds.size(); k++) {
            if (owner[k].second) rp.main_next[owner[k].first] = fresh[k]; else rp.prep_next[owner[k].first] = fresh[k];
        }
        for (int i = 0; i < n_chips; i++) if (rp.rows_next[i]) rp.rows_next[i] = (rp.rows_next[i] + unit - 1) / unit;
        return SP1HIP_SUCCESS;
    }
    int upload_plan(const RoundPlan& rp, int which) {
        if (rp.pack.size() > descs_cap2[which]) {
            d_descs2[which].release();
            descs_cap2[which] = rp.pack.size();
            SP1HIP_TRY(d_descs2[which].alloc(descs_cap2[which], s));
        }
        return stage.upload(d_descs2[which].p, rp.pack.data(), rp.pack_bytes);
    }
    // Plans round r, unless it has a plan already, from the tables the last planned round leaves (round 0: the caller's) and sends
    // its descriptors up, into buffer r & 1 — behind whatever is running: see RoundPlan. The bivariate plan of rounds 0 and 1 takes
    // buffer 1 (round 2's plan takes buffer 0 while the bivariate launches still read theirs), and round 1 has no plan of its own.
    int plan_next(int r) {
        if (r >= L || (int)plans.size() > r) return SP1HIP_SUCCESS;
        if (r == 0) {
            std::vector<uint64_t> rows0(n_chips);
            std::vector<const uint32_t*> main0(n_chips), prep0(n_chips);
            for (int i = 0; i < n_chips; i++) { rows0[i] = tr.chip[i].rows; main0[i] = st[i]->d_main; prep0[i] = st[i]->d_prep; }
            plans.emplace_back(new RoundPlan());
            SP1HIP_TRY(plan_round(0, rows0, main0, prep0, *plans.back(), bivariate));
            return upload_plan(*plans.back(), bivariate ? 1 : 0);
        }
        const RoundPlan& prev = *plans.back();
        while ((int)plans.size() <= r) plans.emplace_back(new RoundPlan());
        SP1HIP_TRY(plan_round(r, prev.rows_next, prev.main_next, prev.prep_next, *plans.back(), false));
        return upload_plan(*plans.back(), r & 1);
    }
    PlanViews device_plan(const RoundPlan& rp, int which) const {
        const uint8_t* base = (const uint8_t*)d_descs2[which].p;
        return PlanViews{(const ZcDesc*)base, (const ZcChipRange*)(base + rp.off_ranges), (const ZcFixDesc*)(base + rp.off_fds)};
    }

    // The hand-over of a round's sums. They reach the host through the mailbox slot when they fit it (they do for any real machine):
    // the reduce kernel, launched by `launch_reduce(rs_pub)`, then publishes them itself (ticket on the round-sync counters, payload
    // in the mailbox slot); else they are fetched from d_src. Between that launch and the wait, behind the running launches, the
    // round `next_round` is planned and its descriptors go up.
    template <class LaunchReduce>
    int publish_and_wait(size_t n_words, const void* d_src, uint32_t* h_out, int next_round, LaunchReduce&& launch_reduce) {
        const bool direct = n_words + 1 <= MAILBOX_WORDS;
        const RoundSync rs_pub = direct ? RoundSync{rsync.d_counter, (volatile uint32_t*)mb.h_slot} : RoundSync{};
        if (direct) { rsync.pending = true; mb.pending = true; }
        SP1HIP_TRY(launch_reduce(rs_pub));
        SP1HIP_TRY(plan_next(next_round));
        timer.lap(ZcTimer::PLAN);
        if (direct) { SP1HIP_TRY(mb.wait_next(h_out, n_words)); rsync.pending = false; }
        else SP1HIP_TRY(mb.fetch(d_src, n_words, h_out));
        timer.lap(ZcTimer::WAIT);
        return SP1HIP_SUCCESS;
    }
    // after the launch of the table update that rp plans: the chips read the folded tables (the arena is stream-ordered: the old
    // table is recycled behind this launch)
    void apply_fix(const RoundPlan& rp) {
        for (size_t k = 0; k < rp.fds.size(); k++) {
            ChipState& c = *st[rp.owner[k].first];
            if (rp.owner[k].second) c.d_main = rp.fresh[k]; else c.d_prep = rp.fresh[k];
        }
    }

    // ================= rounds 0 and 1 from ONE pass over the base-field traces (see zc_biv_node) =================
    // the launches of the bivariate plan, joined in front of the reduction (as in the later rounds); bsums: the sums of its ranges
    int bivariate_sums(const RoundPlan& rp, std::vector<uint32_t>& bsums) {
        const uint32_t eq_len = 1u << (L - 2);
        const uint32_t* d_eq = d_eq_all.u32() + 4 * (((size_t)1 << (L - 2)) - 1);    // eq over the L - 2 variables of the quad index
        const int n_descs = (int)rp.descs.size(), n_ranges = (int)rp.ranges.size();
        const PlanViews dp = device_plan(rp, 1);
        const ZcDesc* dd = dp.descs;
        partial_cap = (size_t)rp.total_blocks * ZC_BIV_NODES * 8 * 4;
        SP1HIP_TRY(d_partial.alloc(partial_cap, s));
        DevBuf d_bsums;
        SP1HIP_TRY(d_bsums.alloc(bsums.size() * 4, s));
        ScopedTimer tm("zerocheck_round", s);
        RoundFork fork;
        SP1HIP_TRY(fork.begin(s, fork_enabled && rp.n_launches() > 1 && active_provers() <= 1));
        hipStream_t ls;
        // these launches fill the device together (the round is throughput-bound: 5.1 ms on the core shard however they are
        // placed): the largest interpreter group on the caller's stream, the Poseidon2 pieces on the second, the other
        // interpreter groups on the third, the septic pieces on the fourth
        // (the interpreter groups, longest first — workgroups x instructions —, each on the less loaded of the caller's stream and
        // the third: since the groups are cut by residency there are up to ten of them, and one stream for all but the largest
        // serialised 6 ms of launches)
        {
            std::vector<size_t> by_work(rp.groups.size());
            for (size_t g = 0; g < by_work.size(); g++) by_work[g] = g;
            auto work = [&](size_t g) { return (double)rp.groups[g].n_blocks * (double)rp.groups[g].max_instr; };
            std::stable_sort(by_work.begin(), by_work.end(), [&](size_t a, size_t b) { return work(a) > work(b); });
            double load0 = 0, load2 = 0;
            for (size_t gi : by_work) {
                const auto& g = rp.groups[gi];
                const int slot = load0 <= load2 ? 0 : 2;
                (slot == 0 ? load0 : load2) += work(gi);
                SP1HIP_TRY(fork.stream_of(slot, &ls));
                SP1HIP_TRY(launch_biv_round(g, dd, n_descs, d_eq, eq_len, d_publics.u32(), d_partial.u32(), ls));
            }
        }
#define SP1HIP_ZC_BIV_MACRO_LAUNCH(KIND, SLOT)                                                                                           \
        if (rp.macro_n[KIND]) {                                                                                                \
            SP1HIP_TRY(fork.stream_of(SLOT, &ls));                                                                             \
            hipLaunchKernelGGL((zc_biv_macro_kernel<KIND>), dim3(rp.macro_n[KIND] * (uint32_t)ZC_BIV_NODES), dim3(256), 0, ls, dd, n_descs, d_eq, eq_len, d_partial.u32(), rp.macro_lo[KIND], ctx->d_rc); \
            SP1HIP_LAUNCH_CHECK();                                                                                             \
        }
        // the second stream: the long fused launches, longest first (a Keccak shard's pieces 3.0 ms, the MulOperation pieces of a
        // fibonacci shard 2.7 ms, Poseidon2 1.0-6.0 ms where the Global chip is tall), then the short ones (the polynomial
        // identities, the GKR corner sums, the septic curve pieces); the third stream: behind its interpreter groups the septic
        // sum pieces (6.6 ms on a shard with 1.7 million Global rows). On such a shard the short launches behind the septic sum
        // were a 1.4 ms tail with the device nearly idle, and in front of it they delay the longest launch by as much.
        if (rp.macro_n[ZC_HINT_KECCAK]) {          // four nodes per pass: three node-group workgroups per block
            SP1HIP_TRY(fork.stream_of(1, &ls));
            hipLaunchKernelGGL(zc_biv_keccak_kernel, dim3(rp.macro_n[ZC_HINT_KECCAK] * ZC_BIV_GROUPS), dim3(256), 0, ls, dd, n_descs, d_eq, eq_len, d_partial.u32(), rp.macro_lo[ZC_HINT_KECCAK]);
            SP1HIP_LAUNCH_CHECK();
        }
        SP1HIP_ZC_BIV_MACRO_LAUNCH(3u, 2)
        SP1HIP_ZC_BIV_MACRO_LAUNCH(6u, 1)
        SP1HIP_ZC_BIV_MACRO_LAUNCH(1u, 1)
        if (rp.macro_n[ZC_HINT_POLY]) {            // all twelve nodes per workgroup
            SP1HIP_TRY(fork.stream_of(1, &ls));
            hipLaunchKernelGGL(zc_biv_poly_kernel, dim3(rp.macro_n[ZC_HINT_POLY]), dim3(256), 0, ls, dd, n_descs, d_eq, eq_len, d_partial.u32(), rp.macro_lo[ZC_HINT_POLY]);
            SP1HIP_LAUNCH_CHECK();
        }
        if (rp.macro_n[ZC_RANGE_CORNERS]) {         // the GKR corner sums: columns in slices
            SP1HIP_TRY(fork.stream_of(1, &ls));
            hipLaunchKernelGGL(zc_biv_corner_kernel, dim3(rp.macro_n[ZC_RANGE_CORNERS]), dim3(256), 0, ls, dd, n_descs, d_eq, eq_len, d_partial.u32(), rp.macro_lo[ZC_RANGE_CORNERS]);
            SP1HIP_LAUNCH_CHECK();
        }
        SP1HIP_ZC_BIV_MACRO_LAUNCH(2u, 1)
#undef SP1HIP_ZC_BIV_MACRO_LAUNCH
        SP1HIP_TRY(fork.join());
        return publish_and_wait((size_t)n_ranges * ZC_BIV_SUM_WORDS, d_bsums.p, bsums.data(), 2, [&](const RoundSync& rs_pub) -> int {
            hipLaunchKernelGGL(zc_biv_reduce_kernel, dim3(n_ranges * ZC_BIV_NODES), dim3(256), 0, s, dp.ranges, d_partial.u32(), d_eq, eq_len, d_bsums.u32(), rs_pub, mb.seq + 1);
            SP1HIP_LAUNCH_CHECK();
            return SP1HIP_SUCCESS;
        });
    }
    int run_bivariate_rounds() {
        const RoundPlan& rp = *plans[0];
        std::vector<uint32_t> bsums((size_t)std::max<size_t>(rp.ranges.size(), 1) * ZC_BIV_SUM_WORDS);
        if (!rp.descs.empty()) SP1HIP_TRY(bivariate_sums(rp, bsums));
        SP1HIP_TRY(plan_next(2));                                    // (a plan without descriptors: nothing was launched above)
        std::vector<BivNodes> H(n_chips);
        assemble_biv_nodes(rp.desc_chip, bsums, tr.chip, H);
        const CubicBasis& cubic = cubic_basis();
        std::vector<std::array<Ext, 3>> hv(n_chips);
        // ---- round 0 binds Y (the last variable): h(t) = (1 - z_X) H(0, t) + z_X H(1, t)
        const Ext zX = zeta[L - 2], zY = zeta[L - 1];
        for (int i = 0; i < n_chips; i++) {
            if (tr.chip[i].rows == 0) continue;
            for (int k = 0; k < 3; k++) { const int t = k == 0 ? 0 : k + 1; hv[i][k] = (kb::ext_one() - zX) * H[i][0][t] + zX * H[i][1][t]; }
        }
        const Ext a0 = tr.round_messages(zY, hv);
        tr.update_claims();                                          // (round 1's node values need eq_adj and the claims of round 0)
        // ---- round 1 binds X: h(t) = eq(z_Y, a0) x the cubic through H(t, 0), H(t, 1), H(t, 2), H(t, 4) at a0
        Ext Lk[4];                                                   // C_k(a0)
        for (int k = 0; k < 4; k++) {
            Ext acc = kb::ext_from_base(cubic.c[k][3]);
            for (int d = 2; d >= 0; d--) acc = acc * a0 + kb::ext_from_base(cubic.c[k][d]);
            Lk[k] = acc;
        }
        for (int i = 0; i < n_chips; i++) {
            const ChipClaim& c = tr.chip[i];
            if (c.rows == 0) continue;
            for (int k = 0; k < 3; k++) {
                const int t = k == 0 ? 0 : k + 1;                   // index of 0, 2, 4 in {0, 1, 2, 4}
                const Ext v = H[i][t][0] * Lk[0] + H[i][t][1] * Lk[1] + H[i][t][2] * Lk[2] + H[i][t][3] * Lk[3];
                hv[i][k] = c.eq_adj * v;                            // eq_adj = eq(z_Y, a0) since round_messages
            }
        }
        const Ext a1 = tr.round_messages(zX, hv);
        timer.lap(ZcTimer::UNI);
        // ---- the tables folded by both challenges
        if (!rp.fds.empty()) {
            ScopedTimer tm("zerocheck_fix", s);
            hipLaunchKernelGGL(zc_fix2_kernel, dim3(rp.fix_blocks), dim3(256), 0, s, device_plan(rp, 1).fds, (int)rp.fds.size(), a0, a1);
            SP1HIP_LAUNCH_CHECK();
            apply_fix(rp);
        }
        tr.update_claims();                                          // (behind the launch of the table update)
        tr.fold_rows(4);
        return SP1HIP_SUCCESS;
    }

    // ================= a round that binds one variable =================
    // longest expected launch first, each on the stream with the least expected work so far (a fused piece is one
    // long dependent chain per workgroup: ~75 / 50 / 60 us at its floor, an interpreter group ~50; above the floor
    // a launch grows with its workgroups per 1024 resident ones)
    struct Launch { int kind; size_t group; double est; int slot; };           // kind 0: interpreter group, 1..3: fused pieces
    static void order_launches(const RoundPlan& rp, int r, bool forked, std::vector<Launch>& order) {
        const std::vector<Group>& groups = rp.groups;
        const uint32_t* macro_n = rp.macro_n;
        static const double floor_us[ZC_MACRO_KINDS] = {45.0, 75.0, 45.0, 60.0, 60.0, 120.0, 45.0, 90.0};
        // (an interpreter group's length grows with its longest program too: 100 instructions are the unit the floor was measured at)
        for (size_t g = 0; g < groups.size(); g++) order.push_back({0, g, floor_us[0] * (1.0 + groups[g].n_blocks * 3 / 1024.0 * std::max(groups[g].max_instr, 25u) / 100.0), 0});
        const bool both_septic = forked && r > 0 && macro_n[2] && macro_n[3] && (uint64_t)rp.total_blocks * 3 <= ZC_SMALL_ROUND_WGS;
        for (int kind = 1; kind <= 3; kind++) {
            if (!macro_n[kind] || (both_septic && kind == 2)) continue;
            if (both_septic && kind == 3) order.push_back({(int)ZC_MACRO_BOTH_SEPTIC, 0, floor_us[3] * (1.0 + (macro_n[2] + macro_n[3]) * 3 / 1024.0), 0});
            else order.push_back({kind, 0, floor_us[kind] * (1.0 + macro_n[kind] * 3 / 1024.0), 0});
        }
        if (macro_n[ZC_HINT_KECCAK]) order.push_back({(int)ZC_HINT_KECCAK, 0, floor_us[ZC_HINT_KECCAK] * (1.0 + macro_n[ZC_HINT_KECCAK] * 3 / 1024.0), 0});
        if (macro_n[ZC_HINT_MUL]) order.push_back({(int)ZC_HINT_MUL, 0, floor_us[ZC_HINT_MUL] * (1.0 + macro_n[ZC_HINT_MUL] * 3 / 1024.0), 0});
        if (macro_n[ZC_HINT_POLY]) order.push_back({(int)ZC_HINT_POLY, 0, floor_us[ZC_HINT_POLY] * (1.0 + macro_n[ZC_HINT_POLY] * 3 / 1024.0), 0});
        if (forked) {
            std::stable_sort(order.begin(), order.end(), [](const Launch& a, const Launch& b) { return a.est > b.est; });
            double load[ZC_FORK_STREAMS + 1] = {0, 7, 14, 21};          // (the launches leave the host ~7 us apart)
            // (in the rounds whose launches fill the device the kernel on the fourth queue starts ~0.84 ms after the others —
            // profiles/r04_gap_trace_timeline.txt — and four queues still beat three: 2.0 against 2.2 ms in round 2)
            for (Launch& ln : order) {
                int best = 0;
                for (int k = 1; k <= ZC_N_FORK; k++) if (load[k] < load[best]) best = k;
                ln.slot = best;
                load[best] += ln.est;
            }
        }
    }
    // the launches of round r, the reduction, the hand-over of its sums into h_sums
    int round_sums(int r, const RoundPlan& rp) {
        const int nv = L - r;                       // variables left
        // eq(zeta[0 .. nv-1), .) is shared by every chip with real rows
        const uint32_t* d_eq = d_eq_all.u32() + 4 * (((size_t)1 << (nv - 1)) - 1);
        const uint32_t eq_len = 1u << (nv - 1);
        const int n_descs = (int)rp.descs.size(), n_ranges = (int)rp.ranges.size();
        const PlanViews dp = device_plan(rp, r & 1);
        const ZcDesc* dd = dp.descs;
        if ((size_t)rp.total_blocks * 24 * 4 > partial_cap) {
            d_partial.release();
            partial_cap = (size_t)rp.total_blocks * 24 * 4;
            SP1HIP_TRY(d_partial.alloc(partial_cap, s));
        }
        ScopedTimer tm("zerocheck_round", s);      // (the reference's SP1_GPU_ZEROCHECK_ROUND_TIMING switch)
        RoundFork fork;                            // SP1HIP_ZC_FORK=0: one stream
        SP1HIP_TRY(fork.begin(s, fork_enabled && rp.n_launches() > 1 && rp.total_blocks <= ZC_FORK_MAX_BLOCKS && active_provers() <= 1));
        std::vector<Launch> order;
        order_launches(rp, r, fork.forked, order);
        for (const Launch& ln : order) {
            hipStream_t ls;
            SP1HIP_TRY(fork.stream_of(ln.slot, &ls));
            if (ln.kind == 0) {
                const auto& g = rp.groups[ln.group];
                // One workgroup evaluating the three nodes of its rows (rows leave HBM once) was measured on the core-shaped
                // shard: 12.5 ms of round kernels against 11.0 ms with a workgroup per node — the re-reads already meet in the
                // memory-side cache (FETCH_SIZE counts those hits), and fusing costs a third of the parallelism. Removed.
                if (r == 0) SP1HIP_TRY(launch_round<true>(g, dd, n_descs, d_eq, eq_len, d_publics.u32(), d_partial.u32(), ls));
                else SP1HIP_TRY(launch_round<false>(g, dd, n_descs, d_eq, eq_len, d_publics.u32(), d_partial.u32(), ls));
                continue;
            }
#define SP1HIP_ZC_MACRO_LAUNCH(KIND)                                                                                                   \
            if (ln.kind == (int)KIND) {                                                                                            \
                if (r == 0) hipLaunchKernelGGL((zc_macro_kernel<true, KIND>), dim3(rp.macro_n[KIND] * 3), dim3(256), 0, ls, dd, n_descs, d_eq, eq_len, d_partial.u32(), rp.macro_lo[KIND], ctx->d_rc); \
                else hipLaunchKernelGGL((zc_macro_kernel<false, KIND>), dim3(rp.macro_n[KIND] * 3), dim3(256), 0, ls, dd, n_descs, d_eq, eq_len, d_partial.u32(), rp.macro_lo[KIND], ctx->d_rc); \
                SP1HIP_LAUNCH_CHECK();                                                                                             \
            }
            SP1HIP_ZC_MACRO_LAUNCH(1u)
            SP1HIP_ZC_MACRO_LAUNCH(2u)
            SP1HIP_ZC_MACRO_LAUNCH(3u)
            SP1HIP_ZC_MACRO_LAUNCH(6u)
            if (ln.kind == (int)ZC_HINT_POLY) {       // the three nodes per workgroup
                if (rp.poly_wave) hipLaunchKernelGGL(zc_poly_wave_kernel, dim3(rp.macro_n[ZC_HINT_POLY]), dim3(256), 0, ls, dd, n_descs, d_eq, eq_len, d_partial.u32(), rp.macro_lo[ZC_HINT_POLY]);
                else if (r == 0) hipLaunchKernelGGL(zc_poly_kernel<true>, dim3(rp.macro_n[ZC_HINT_POLY]), dim3(256), 0, ls, dd, n_descs, d_eq, eq_len, d_partial.u32(), rp.macro_lo[ZC_HINT_POLY]);
                else hipLaunchKernelGGL(zc_poly_kernel<false>, dim3(rp.macro_n[ZC_HINT_POLY]), dim3(256), 0, ls, dd, n_descs, d_eq, eq_len, d_partial.u32(), rp.macro_lo[ZC_HINT_POLY]);
                SP1HIP_LAUNCH_CHECK();
            }
            SP1HIP_ZC_MACRO_LAUNCH(5u)
#undef SP1HIP_ZC_MACRO_LAUNCH
            if (ln.kind == (int)ZC_MACRO_BOTH_SEPTIC) {          // (never round 0: that round is far above the small-round bound)
                hipLaunchKernelGGL((zc_macro_kernel<false, ZC_MACRO_BOTH_SEPTIC>), dim3((rp.macro_n[2] + rp.macro_n[3]) * 3), dim3(256), 0, ls, dd, n_descs, d_eq, eq_len, d_partial.u32(), rp.macro_lo[2], ctx->d_rc);
                SP1HIP_LAUNCH_CHECK();
            }
        }
        SP1HIP_TRY(fork.join());
        return publish_and_wait((size_t)n_ranges * 16, d_sums.p, h_sums.data(), r + 1, [&](const RoundSync& rs_pub) -> int {
            if (r == 0) hipLaunchKernelGGL(zc_reduce_kernel<true>, dim3(n_ranges), dim3(256), 0, s, dp.ranges, d_partial.u32(), d_eq, eq_len, d_sums.u32(), rs_pub, mb.seq + 1);
            else hipLaunchKernelGGL(zc_reduce_kernel<false>, dim3(n_ranges), dim3(256), 0, s, dp.ranges, d_partial.u32(), d_eq, eq_len, d_sums.u32(), rs_pub, mb.seq + 1);
            SP1HIP_LAUNCH_CHECK();
            return SP1HIP_SUCCESS;
        });
    }
    int run_round(int r) {
        const RoundPlan& rp = *plans[r];
        if (!rp.descs.empty()) SP1HIP_TRY(round_sums(r, rp));
        SP1HIP_TRY(plan_next(r + 1));                                // (a round without descriptors: nothing was launched above)
        {   // a chip with fused pieces has a second range: its sums ADD to the interpreter's (the eq entry is the same)
            std::vector<char> have(n_chips, 0);
            for (size_t k = 0; k < rp.desc_chip.size(); k++) {
                const int ci = rp.desc_chip[k];
                const uint32_t* src = h_sums.data() + k * 16;
                if (!have[ci]) { memcpy(sums[ci].data(), src, 64); have[ci] = 1; }
                else for (int w = 0; w < 12; w++) sums[ci][w] = kb::add(sums[ci][w], src[w]);
            }
        }
        std::vector<std::array<Ext, 3>> hv(n_chips);
        tr.node_values(sums, hv);
        const Ext a_r = tr.round_messages(zeta[L - r - 1], hv);
        timer.lap(ZcTimer::UNI);
        if (!rp.fds.empty()) {
            const ZcFixDesc* d_fix = device_plan(rp, r & 1).fds;
            ScopedTimer tm("zerocheck_fix", s);
            if (r == 0) hipLaunchKernelGGL(zc_fix_kernel<true>, dim3(rp.fix_blocks), dim3(256), 0, s, d_fix, (int)rp.fds.size(), a_r);
            else hipLaunchKernelGGL(zc_fix_kernel<false>, dim3(rp.fix_blocks), dim3(256), 0, s, d_fix, (int)rp.fds.size(), a_r);
            SP1HIP_LAUNCH_CHECK();
            apply_fix(rp);
        }
        tr.update_claims();                                           // (behind the launch of the table update: the device is busy again)
        tr.fold_rows(2);
        return SP1HIP_SUCCESS;
    }

    // ---- proof: PartialSumcheckProof + per-chip component evaluations (prep then main); the transcript observes the openings
    int write_proof() {
        ByteOut w;
        w.u64((uint64_t)L);
        for (auto& m : tr.msgs) { w.u64(m.size()); for (auto& cf : m) w.ext(cf); }
        Ext claimed = kb::ext_zero(), final_eval = kb::ext_zero();
        for (auto& cl : tr.claims) claimed = claimed * tr.lambda + cl;
        for (int i = 0; i < n_chips; i++) final_eval = final_eval * tr.lambda + tr.round_claims[i];      // (a chip's polynomial of the last round at its challenge)
        w.ext(claimed);
        w.u64(tr.point.size());
        for (auto& x : tr.point) w.ext(x);
        w.ext(final_eval);
        w.u64((uint64_t)n_chips);
        std::vector<std::vector<Ext>> chip_evals(n_chips);
        {   // one row is left of every table: ext [1 x w] = w*4 words (col, coord). Gather them all, one hand-over.
            std::vector<ZcGatherDesc> gd;
            size_t total_words = 0;
            for (int i = 0; i < n_chips; i++) {
                ChipState& c = *st[i];
                const uint32_t wp = c.in->prep_width, wm = c.in->main_width;
                if (tr.chip[i].rows && wp) gd.push_back({c.d_prep, wp * 4, (uint32_t)total_words});
                total_words += (size_t)wp * 4;
                if (tr.chip[i].rows && wm) gd.push_back({c.d_main, wm * 4, (uint32_t)total_words});
                total_words += (size_t)wm * 4;
            }
            std::vector<uint32_t> flat(total_words, 0);
            if (!gd.empty()) {
                DevBuf d_gd, d_flat;
                SP1HIP_TRY(d_gd.alloc(gd.size() * sizeof(ZcGatherDesc), s));
                SP1HIP_TRY(d_flat.alloc(total_words * 4, s));
                SP1HIP_HIP(hipMemsetAsync(d_flat.p, 0, total_words * 4, s));
                SP1HIP_TRY(stage.upload(d_gd.p, gd.data(), gd.size() * sizeof(ZcGatherDesc)));
                hipLaunchKernelGGL(zc_gather_kernel, dim3((unsigned)gd.size()), dim3(256), 0, s, (const ZcGatherDesc*)d_gd.p, d_flat.u32());
                SP1HIP_LAUNCH_CHECK();
                SP1HIP_TRY(mb.fetch(d_flat.p, total_words, flat.data()));     // also keeps `gd` valid long enough
            }
            size_t off = 0;
            for (int i = 0; i < n_chips; i++) {
                const uint32_t wtot = st[i]->in->prep_width + st[i]->in->main_width;
                for (uint32_t k = 0; k < wtot; k++, off += 4)
                    chip_evals[i].push_back(Ext{{flat[off], flat[off + 1], flat[off + 2], flat[off + 3]}});
                w.u64(chip_evals[i].size());
                for (auto& e : chip_evals[i]) w.ext(e);
            }
        }
        // observe the openings (shard.rs:L609-L640)
        challenger_observe(challenger, kb::to_monty((uint32_t)n_chips));
        for (int i = 0; i < n_chips; i++) {
            const uint32_t wp = st[i]->in->prep_width, wm = st[i]->in->main_width;
            challenger_observe(challenger, kb::to_monty(wp));
            for (uint32_t k = 0; k < wp; k++) for (int q = 0; q < 4; q++) challenger_observe(challenger, chip_evals[i][k].c[q]);
            challenger_observe(challenger, kb::to_monty(wm));
            for (uint32_t k = 0; k < wm; k++) for (int q = 0; q < 4; q++) challenger_observe(challenger, chip_evals[i][wp + k].c[q]);
        }
        if (w.b.size() != need) { set_error("internal error: zerocheck proof size %zu != %zu", w.b.size(), need); return SP1HIP_ERROR_RUNTIME; }
        memcpy(h_proof, w.b.data(), need);
        *proof_len = need;
        return SP1HIP_SUCCESS;
    }
};

static int zerocheck_prove_impl(ZcProver& p) {
    SP1HIP_TRY(p.check_arguments());
    SP1HIP_TRY(p.setup_chips());
    SP1HIP_TRY(p.setup_rounds());
    if (p.bivariate) SP1HIP_TRY(p.run_bivariate_rounds());
    for (int r = p.bivariate ? 2 : 0; r < p.L; r++) SP1HIP_TRY(p.run_round(r));
    p.tr.update_claims();
    p.timer.rounds_done();
    SP1HIP_TRY(p.write_proof());
    p.timer.report(p.L);
    return SP1HIP_SUCCESS;
}

// standalone form of the per-round table update, with the reference's per-column padding value
template <bool FIRST>
__global__ __launch_bounds__(256) void fix_last_variable_kernel(const uint32_t* __restrict__ in, uint32_t rows, uint32_t width,
                                                                kb::Ext alpha, const uint32_t* __restrict__ padding,
                                                                uint32_t* __restrict__ out) {
    using K = KT<FIRST>;
    const uint32_t out_rows = (rows + 1) / 2;
    const size_t t = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (t >= (size_t)out_rows * width) return;
    const uint32_t c = (uint32_t)(t / out_rows), i = (uint32_t)(t % out_rows);
    typename K::T x = K::load(in, c, rows, 2 * i), y;
    if (2 * i + 1 < rows) y = K::load(in, c, rows, 2 * i + 1);
    else if (!padding) y = K::zero();
    else y = K::load(padding, c, 1, 0);                   // a one-row table in the same layout
    const kb::Ext r = kb::ext_add(K::scale(alpha, K::sub(y, x)), K::to_ext(x));
#pragma unroll
    for (int q = 0; q < 4; q++) out[((size_t)c * 4 + q) * out_rows + i] = r.c[q];
}
}  // namespace sp1hip

using namespace sp1hip;

extern "C" int sp1hip_zerocheck_biv_interp_host(uint32_t r00, uint32_t r01, uint32_t r10, uint32_t r11, uint32_t node, uint32_t* out) {
    SP1HIP_REQUIRE(out && node < (uint32_t)ZC_BIV_NODES, "node out of range");
    SP1HIP_REQUIRE(r00 < kb::P && r01 < kb::P && r10 < kb::P && r11 < kb::P, "word not reduced");
    *out = zc_biv_interp(r00, r01, r10, r11, zc_biv_node(node));
    return SP1HIP_SUCCESS;
}

extern "C" int sp1hip_fix_last_variable(const uint32_t* d_in, uint64_t rows, uint32_t width, int in_is_ext, sp1hip_ext_t alpha,
                                        const uint32_t* d_padding, uint32_t* d_out, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(rows < ((uint64_t)1 << 32), "too many rows");
    if (rows == 0 || width == 0) return SP1HIP_SUCCESS;
    SP1HIP_REQUIRE(d_in && d_out && d_in != d_out, "bad buffers");
    const kb::Ext a{{alpha.c[0], alpha.c[1], alpha.c[2], alpha.c[3]}};
    const uint64_t total = ((rows + 1) / 2) * width;
    SP1HIP_REQUIRE((total + 255) / 256 < ((uint64_t)1 << 31), "table too large for one launch");
    const dim3 grid((unsigned)((total + 255) / 256));
    if (in_is_ext) hipLaunchKernelGGL(fix_last_variable_kernel<false>, grid, dim3(256), 0, S(stream), d_in, (uint32_t)rows, width, a, d_padding, d_out);
    else hipLaunchKernelGGL(fix_last_variable_kernel<true>, grid, dim3(256), 0, S(stream), d_in, (uint32_t)rows, width, a, d_padding, d_out);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}

extern "C" int sp1hip_zerocheck_prove(const sp1hip_zc_chip_t* chips, int n_chips, int max_log_row_count,
                                      const sp1hip_ext_t* h_zeta, const sp1hip_ext_t* h_openings, sp1hip_ext_t alpha,
                                      sp1hip_ext_t gkr_batch, const uint32_t* h_publics, int n_publics,
                                      sp1hip_challenger_t* challenger, uint8_t* h_proof, size_t* proof_len,
                                      sp1hip_stream_t stream) {
    // the caller's transcript only advances if the proof is produced
    sp1hip_challenger_t* backup = nullptr;
    if (challenger) SP1HIP_TRY(sp1hip_challenger_clone(challenger, &backup));
    int st;
    {
        ZcProver p(chips, n_chips, max_log_row_count, h_zeta, h_openings, alpha, gkr_batch, h_publics, n_publics, challenger, h_proof, proof_len, stream);
        st = zerocheck_prove_impl(p);
    }
    if (st != SP1HIP_SUCCESS && challenger) challenger_restore(challenger, backup);
    sp1hip_challenger_free(backup);
    return st;
}
