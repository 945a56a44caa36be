// sp1_amd/csrc/outer_basefold.hip — the BaseFold opening under the outer (BN254) configuration: the wrap proof's
// `SP1OuterGlobalContext` (/root/reference/slop/crates/bn254/src/lib.rs:L60-L90) run through
//   `BasefoldProver::commit_mles`                    /root/reference/slop/crates/basefold-prover/src/prover.rs:L78-L99
//   `BasefoldProver::prove_trusted_mle_evaluations`  prover.rs:L102-L243 -> fri.rs:L31-L129
// with Poseidon2-BN254 trees (outer.hip) and the MultiField32Challenger (outer_host.cpp) in place of the KoalaBear ones.
//
// Everything that is field work is the inner prover's (basefold.hip): batching, the RS encode of the batched message, both
// folds, zero_val, the query gathers and the Montgomery -> canonical pass over the opened VALUES. New here:
//  * outer_leaf_hash_pairs: one lane per fold-round leaf (two extension elements = 8 KoalaBear words = one reduce_31 chunk
//    in lane 0, lanes 1 and 2 zero), one permutation, one digest store;
//  * the tree finish with hand-over (outer_finish_tree: the one-workgroup tail publishes [zero_val | root | commitment]);
//  * the digests of the opened PATHS leave Montgomery form in a pass of their own (BN254 words, 8 per digest);
//  * the bincode of a digest: Hash<F, Bn254Fr, 1> = u64(32) + the 32 little-endian bytes of the canonical value (40 bytes).
// The host keeps the transcript; one device -> host hand-over per fold round. PoW witnesses: the smallest one.
#include <algorithm>
#include <array>
#include <atomic>
#include <cstring>
#include <memory>
#include <vector>

#include "basefold_host.hpp"
#include "outer_tree.hpp"

sp1hip::OuterChallenger* outer_challenger_inner(sp1hip_outer_challenger_t* ch);

struct sp1hip_outer_basefold_data_s {
    int lg_n = 0, lg_blowup = 0;
    std::vector<sp1hip_tensor_t> mles;                    // caller-owned inputs [2^lg_n x w], column-major
    std::vector<std::unique_ptr<sp1hip::DeviceBuf>> cws;  // codewords [2^(lg_n+lg_blowup) x w]
    std::vector<sp1hip_tensor_t> cw_tensors;
    sp1hip::DeviceBuf tree;
    uint32_t root[8], commit[8];                          // Montgomery words
    uint32_t total_width = 0;
    // see sp1hip_basefold_data_s (prover.hip): a handle read on another stream than the one that made it waits for the device
    // before its blocks go back to that stream's free list
    std::atomic<bool> foreign_use{false};
    ~sp1hip_outer_basefold_data_s() { if (foreign_use) (void)hipDeviceSynchronize(); }
};

namespace sp1hip {
namespace {

constexpr size_t DIGEST_BYTES = 40;           // u64 length prefix + 32 bytes

// Leaf i of a fold round = (cw[2 i], cw[2 i + 1]) of the SoA extension codeword: 8 words, one chunk.
__global__ __launch_bounds__(256) void outer_leaf_hash_pairs_kernel(const uint32_t* __restrict__ cw, uint32_t n,
                                                                    uint32_t* __restrict__ leaves) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (n >> 1)) return;
    uint32_t v[8];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint2 t = *reinterpret_cast<const uint2*>(cw + (size_t)k * n + 2 * (size_t)i);
        v[k] = kb::from_monty(t.x);
        v[4 + k] = kb::from_monty(t.y);
    }
    Fr x[3] = {bn254::to_monty(bn254::pack31(v)), bn254::zero(), bn254::zero()};
    outer::permute(x, c_outer_rc);
    store_fr(leaves + (size_t)i * 8, x[0]);
}

// Opened path digests: Montgomery -> canonical words in place.
__global__ __launch_bounds__(256) void outer_digests_from_monty_kernel(uint32_t* __restrict__ digests, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    store_fr(digests + (size_t)i * 8, bn254::from_monty(load_fr(digests + (size_t)i * 8)));
}

int commit_ext_pairs_outer(const uint32_t* d_cw, int lg_n, uint32_t* d_tree, uint32_t* d_root_and_commit, hipStream_t s,
                           const uint32_t* d_publish_extra, uint32_t* h_publish_slot, uint32_t publish_seq) {
    const uint32_t n = 1u << lg_n, leaves = n >> 1;
    {
        ScopedTimer t("outer_leaf_hash_pairs", s);
        hipLaunchKernelGGL(outer_leaf_hash_pairs_kernel, dim3((leaves + 255) / 256), dim3(256), 0, s, d_cw, n, d_tree);
    }
    SP1HIP_LAUNCH_CHECK();
    return outer_finish_tree(d_tree, lg_n - 1, 8, d_root_and_commit, s, d_publish_extra, h_publish_slot, publish_seq);
}

void digest_canonical(const uint32_t* monty, uint32_t (&canon)[8]) {
    uint32_t m[8];
    memcpy(m, monty, 32);
    outer_host_from_monty(m, canon);
}

struct OuterWriter : ByteWriter {
    void digest_canonical_words(const uint32_t* c) {         // 8 canonical words == the 32 little-endian bytes
        u64(32);
        if (uint8_t* q = take(32)) memcpy(q, c, 32);
    }
    void digest(const uint32_t* monty) {
        uint32_t c[8];
        digest_canonical(monty, c);
        digest_canonical_words(c);
    }
};

// values: canonical KoalaBear words; root: Montgomery; paths: canonical BN254 words (8 per digest)
void write_opening(OuterWriter& w, const uint32_t* values, size_t n_values, size_t n_idx, size_t width, const uint32_t* root,
                   size_t lg_h, const uint32_t* paths) {
    w.u64(n_values);
    w.canonical_words(values, n_values);
    w.u64(2); w.u64(n_idx); w.u64(width);
    w.digest(root);
    w.u64(lg_h);
    w.u64(width);
    w.u64(n_idx * lg_h);
    for (size_t k = 0; k < n_idx * lg_h; k++) w.digest_canonical_words(paths + 8 * k);
    w.u64(2); w.u64(n_idx); w.u64(lg_h);
}

size_t opening_size(size_t n_idx, size_t width, size_t lg_h) {
    return 8 + 4 * n_idx * width + 24 + DIGEST_BYTES + 8 + 8 + 8 + DIGEST_BYTES * n_idx * lg_h + 24;
}

size_t proof_size(int dim, const uint32_t* widths, int n_rounds, const sp1hip_fri_config_t& cfg) {
    const size_t q = (size_t)cfg.num_queries;
    size_t sz = 8 + (size_t)dim * 32 + 8 + (size_t)dim * DIGEST_BYTES + 8;
    for (int r = 0; r < n_rounds; r++) sz += opening_size(q, widths[r], (size_t)dim + cfg.log_blowup);
    sz += 8;
    for (int r = 0; r < dim; r++) sz += opening_size(q, 8, (size_t)dim + cfg.log_blowup - 1 - r);
    return sz + 16 + 4 + 4;
}

kb::Ext sample_ext(OuterChallenger& ch) {
    kb::Ext e;
    for (int k = 0; k < 4; k++) e.c[k] = kb::to_monty(ch.sample());
    return e;
}
void observe_ext(OuterChallenger& ch, const kb::Ext& e) {
    for (int k = 0; k < 4; k++) ch.observe(kb::from_monty(e.c[k]));
}

// `work` is a clone of the caller's transcript: the caller takes its state over only when the proof is complete.
int prove_trusted_mle_evaluations(std::vector<kb::Ext> point, sp1hip_outer_basefold_data_s* const* rounds, int n_rounds,
                                  const kb::Ext* claims, size_t n_claims, const sp1hip_fri_config_t& cfg,
                                  sp1hip_outer_challenger_t* work, uint8_t* out, size_t out_cap, size_t* out_len, hipStream_t s) {
    OuterChallenger& ch = *outer_challenger_inner(work);
    const int dim = (int)point.size();
    const int lb = cfg.log_blowup;
    const size_t nq = (size_t)cfg.num_queries;
    std::vector<sp1hip_tensor_t> mles;
    for (int r = 0; r < n_rounds; r++)
        for (auto& m : rounds[r]->mles) mles.push_back(m);
    const size_t total_len = n_claims;

    OuterWriter w;
    w.p = out;
    w.cap = out_cap;
    uint32_t batch_witness, pow_witness;
    {
        ScopedTimer t("outer_bf_grind", s);
        SP1HIP_TRY(sp1hip_outer_challenger_grind(work, 5, &batch_witness, s));
    }
    std::vector<kb::Ext> bpt(log2_ceil(total_len));
    for (auto& x : bpt) x = sample_ext(ch);
    std::vector<kb::Ext> coeffs = partial_lagrange_host(bpt);

    const size_t n = (size_t)1 << dim, N0 = n << lb;
    DeviceBuf d_coeffs, d_mle[2], d_eq;
    SP1HIP_TRY(d_coeffs.alloc(total_len * 16, s));
    SP1HIP_TRY(d_mle[0].alloc(n * 16, s));
    SP1HIP_TRY(d_mle[1].alloc(n * 8 + 16, s));
    SP1HIP_TRY(d_eq.alloc(n * 16, s));      // every prefix table of eq(point[0..t), .), t < dim: round r reads table dim - r - 1
    Mailbox mb;
    SP1HIP_TRY(mb.init(s));
    PinnedStage stage;
    SP1HIP_TRY(stage.init(s));
    std::vector<std::unique_ptr<DeviceBuf>> cws, trees;
    {
        ScopedTimer t("outer_bf_batch_encode", s);
        SP1HIP_TRY(stage.upload(d_coeffs.p, coeffs.data(), total_len * 16));
        SP1HIP_TRY(sp1hip_basefold_batch(mles.data(), (int)mles.size(), dim, d_coeffs.u32(), d_mle[0].u32(), s));
        cws.emplace_back(new DeviceBuf());
        SP1HIP_TRY(cws.back()->alloc(N0 * 16, s));
        SP1HIP_TRY(sp1hip_rs_encode_batch(cws.back()->u32(), d_mle[0].u32(), dim, lb, 4, s));
    }
    kb::Ext cur_claim = kb::ext_zero();
    for (size_t i = 0; i < n_claims; i++) cur_claim = kb::ext_add(cur_claim, kb::ext_mul(claims[i], coeffs[i]));

    ch.observe((uint32_t)dim);
    DeviceBuf d_rb;  // [0..4) zero_val, [4..20) root+commit, [20..24) final poly
    SP1HIP_TRY(d_rb.alloc(24 * 4, s));
    std::vector<std::array<uint32_t, 8>> round_roots, fri_commitments;
    std::vector<kb::Ext> uni;
    int cur = 0;
    SP1HIP_TRY(eq_prefix_tables_soa_async(point.data(), dim - 1, d_eq.u32(), s));
    auto eq_table = [&](int t) { return d_eq.u32() + 4 * (((size_t)1 << t) - 1); };     // eq over the first t coordinates
    DeviceBuf d_fold_partial;
    SP1HIP_TRY(d_fold_partial.alloc((((size_t)n / 2 + 255) / 256) * 16, s));
    for (int r = 0; r < dim; r++) {
        const int lg_c = dim - r + lb;
        trees.emplace_back(new DeviceBuf());
        SP1HIP_TRY(trees.back()->alloc((((size_t)2 << (lg_c - 1)) - 1) * 32, s));
        cws.emplace_back(new DeviceBuf());
        SP1HIP_TRY(cws.back()->alloc(((size_t)1 << (lg_c - 1)) * 16, s));
    }
    SP1HIP_TRY(ext_fixed_at_zero_async(d_mle[cur].u32(), dim, eq_table(dim - 1), d_rb.u32(), s));
    {
        ScopedTimer t("outer_bf_commit_phase", s);
        for (int r = 0; r < dim; r++) {
            const int lg_m = dim - r;             // current mle has 2^lg_m entries
            const int lg_c = lg_m + lb;           // current codeword has 2^lg_c entries
            kb::Ext last = point.back();
            point.pop_back();
            // the tree's last kernel hands [zero_val | root | commitment] to the host
            SP1HIP_TRY(commit_ext_pairs_outer(cws[r]->u32(), lg_c, trees[r]->u32(), d_rb.u32() + 4, s, d_rb.u32(), mb.h_slot, mb.seq + 1));
            uint32_t rb[20];
            SP1HIP_TRY(mb.wait_next(rb, 20));
            kb::Ext zero_val{{rb[0], rb[1], rb[2], rb[3]}};
            kb::Ext one_val = kb::ext_add(kb::ext_mul(kb::ext_sub(cur_claim, zero_val), kb::ext_inv(last)), zero_val);
            uni.push_back(zero_val);
            uni.push_back(one_val);
            observe_ext(ch, zero_val);
            observe_ext(ch, one_val);
            std::array<uint32_t, 8> root, commit;
            memcpy(root.data(), rb + 4, 32);
            memcpy(commit.data(), rb + 12, 32);
            round_roots.push_back(root);
            fri_commitments.push_back(commit);
            SP1HIP_TRY(sp1hip_outer_challenger_observe_commitment(work, commit.data()));
            kb::Ext beta = sample_ext(ch);
            // both folds and the next round's zero_val partials in one launch
            SP1HIP_TRY(fold_round_async(cws[r]->u32(), lg_c, d_mle[cur].u32(), lg_m, beta, cws[r + 1]->u32(), d_mle[cur ^ 1].u32(),
                                        lg_m >= 2 ? eq_table(lg_m - 2) : nullptr, d_rb.u32(), d_fold_partial.u32(), s));
            cur ^= 1;
            cur_claim = kb::ext_add(zero_val, kb::ext_mul(beta, one_val));
        }
    }
    // final_poly = first ext element of the last codeword (length 2^lb)
    {
        const size_t len = (size_t)1 << lb;
        for (int k = 0; k < 4; k++)
            SP1HIP_HIP(hipMemcpyAsync(d_rb.u32() + 20 + k, cws.back()->u32() + (size_t)k * len, 4, hipMemcpyDeviceToDevice, s));
    }
    uint32_t fp[4];
    SP1HIP_TRY(mb.fetch(d_rb.u32() + 20, 4, fp));
    kb::Ext final_poly{{fp[0], fp[1], fp[2], fp[3]}};
    observe_ext(ch, final_poly);
    {
        ScopedTimer t("outer_bf_grind", s);
        SP1HIP_TRY(sp1hip_outer_challenger_grind(work, cfg.proof_of_work_bits, &pow_witness, s));
    }
    std::vector<uint32_t> q(nq);
    for (auto& x : q) x = ch.sample() & (uint32_t)((1u << (dim + lb)) - 1);

    w.u64((uint64_t)dim);
    for (auto& e : uni) w.ext(e);
    w.u64((uint64_t)dim);
    for (auto& c : fri_commitments) w.digest(c.data());

    // Query phase: every opening into ONE device buffer, the values of all openings first (KoalaBear words), then the
    // paths of all openings (BN254 digests): each region leaves Montgomery form in one launch of its own kind.
    struct Slot { size_t vals_off, n_vals, paths_off, n_paths; };
    std::vector<Slot> slots;
    size_t n_val_words = 0, n_path_words = 0;
    for (int r = 0; r < n_rounds; r++) {
        slots.push_back(Slot{n_val_words, nq * rounds[r]->total_width, n_path_words, nq * (size_t)(dim + lb) * 8});
        n_val_words += slots.back().n_vals;
        n_path_words += slots.back().n_paths;
    }
    for (int r = 0; r < dim; r++) {
        slots.push_back(Slot{n_val_words, nq * 8, n_path_words, nq * (size_t)(dim + lb - r - 1) * 8});
        n_val_words += slots.back().n_vals;
        n_path_words += slots.back().n_paths;
    }
    for (auto& sl : slots) sl.paths_off += n_val_words;
    const size_t words = n_val_words + n_path_words;
    SP1HIP_REQUIRE(words < ((size_t)1 << 32), "opening buffer too large");
    ScopedTimer t_open("outer_bf_openings", s);
    DeviceBuf d_idx, d_open, d_descs;
    SP1HIP_TRY(d_idx.alloc(nq * 4, s));
    SP1HIP_TRY(d_open.alloc(std::max<size_t>(words, 1) * 4, s));
    SP1HIP_TRY(stage.upload(d_idx.p, q.data(), nq * 4));
    for (int r = 0; r < n_rounds; r++) {
        sp1hip_outer_basefold_data_s* pd = rounds[r];
        const Slot& sl = slots[r];
        SP1HIP_TRY(sp1hip_merkle_open(pd->cw_tensors.data(), (int)pd->cw_tensors.size(), dim + lb, pd->tree.u32(), d_idx.u32(), nq,
                                      d_open.u32() + sl.vals_off, d_open.u32() + sl.paths_off, s));
    }
    {   // every fold round's pairs and paths in one launch
        std::vector<FoldOpenDesc> descs(dim);
        for (int r = 0; r < dim; r++) {
            const Slot& sl = slots[n_rounds + r];
            descs[r] = FoldOpenDesc{cws[r]->u32(), trees[r]->u32(), (uint32_t)(dim + lb - r), (uint32_t)sl.vals_off, (uint32_t)sl.paths_off, 0u};
        }
        SP1HIP_TRY(d_descs.alloc(descs.size() * sizeof(FoldOpenDesc), s));
        SP1HIP_TRY(stage.upload(d_descs.p, descs.data(), descs.size() * sizeof(FoldOpenDesc)));
        SP1HIP_TRY(open_fold_rounds(reinterpret_cast<const FoldOpenDesc*>(d_descs.p), dim, dim + lb, d_idx.u32(), nq, d_open.u32(), s));
    }
    SP1HIP_TRY(sp1hip_from_monty(d_open.u32(), n_val_words, (sp1hip_stream_t)s));
    if (n_path_words) {
        const uint32_t nd = (uint32_t)(n_path_words / 8);
        hipLaunchKernelGGL(outer_digests_from_monty_kernel, dim3((nd + 255) / 256), dim3(256), 0, s, d_open.u32() + n_val_words, nd);
        SP1HIP_LAUNCH_CHECK();
    }
    std::vector<uint32_t> opened_pageable;
    PinnedBlock dl{nullptr};
    struct Release { PinnedBlock* b; ~Release() { if (b->h) pinned_stage_release(*b); } } release{&dl};
    const uint32_t* opened = nullptr;
    if (words * 4 <= PINNED_STAGE_BYTES && pinned_stage_acquire(&dl) == SP1HIP_SUCCESS) {
        SP1HIP_HIP(hipMemcpyAsync(dl.h, d_open.p, words * 4, hipMemcpyDeviceToHost, s));
        SP1HIP_TRY(mb.fetch(nullptr, 0, nullptr));             // (its completion also covers the uploads above)
        opened = reinterpret_cast<const uint32_t*>(dl.h);
    } else {
        dl.h = nullptr;
        opened_pageable.resize(std::max<size_t>(words, 1));
        SP1HIP_HIP(hipMemcpyAsync(opened_pageable.data(), d_open.p, words * 4, hipMemcpyDeviceToHost, s));
        SP1HIP_HIP(hipStreamSynchronize(s));
        opened = opened_pageable.data();
    }
    w.u64((uint64_t)n_rounds);
    for (int r = 0; r < n_rounds; r++) {
        const Slot& sl = slots[r];
        write_opening(w, opened + sl.vals_off, sl.n_vals, nq, rounds[r]->total_width, rounds[r]->root, (size_t)(dim + lb), opened + sl.paths_off);
    }
    w.u64((uint64_t)dim);
    for (int r = 0; r < dim; r++) {
        const Slot& sl = slots[n_rounds + r];
        write_opening(w, opened + sl.vals_off, sl.n_vals, nq, 8, round_roots[r].data(), (size_t)(dim + lb - r - 1), opened + sl.paths_off);
    }
    w.ext(final_poly);
    w.felt(pow_witness);
    w.felt(batch_witness);
    SP1HIP_REQUIRE(!w.overflow, "internal error: outer BaseFold proof larger than its computed size");
    *out_len = w.n;
    return SP1HIP_SUCCESS;
}

}  // namespace
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

int sp1hip_outer_commit_mles_data(const sp1hip_tensor_t* mles, int n_mles, int lg_n, int lg_blowup, uint32_t h_commit[8],
                                  sp1hip_outer_basefold_data_t** out, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(mles && n_mles > 0 && out && h_commit, "bad argument");
    SP1HIP_REQUIRE(lg_n >= 0 && lg_blowup >= 0 && lg_n + lg_blowup <= kb::TWO_ADICITY, "size out of range");
    hipStream_t s = S(stream);
    const DeviceCtx* ctx;
    SP1HIP_TRY(get_device_ctx(&ctx));   // also configures the memory pool before the first allocation
    std::unique_ptr<sp1hip_outer_basefold_data_s> pd(new sp1hip_outer_basefold_data_s());
    pd->lg_n = lg_n;
    pd->lg_blowup = lg_blowup;
    const int lg_h = lg_n + lg_blowup;
    const size_t N = (size_t)1 << lg_h;
    for (int i = 0; i < n_mles; i++) {
        SP1HIP_REQUIRE(mles[i].d_data && mles[i].width > 0, "null or empty mle");
        pd->mles.push_back(mles[i]);
        pd->cws.emplace_back(new DeviceBuf());
        SP1HIP_TRY(pd->cws.back()->alloc(N * mles[i].width * 4, s));
        pd->cw_tensors.push_back({pd->cws.back()->u32(), mles[i].width});
        pd->total_width += mles[i].width;
    }
    SP1HIP_TRY(pd->tree.alloc((2 * N - 1) * 32, s));
    DeviceBuf rc;
    SP1HIP_TRY(rc.alloc(64, s));
    for (int i = 0; i < n_mles; i++)
        SP1HIP_TRY(sp1hip_rs_encode_batch(pd->cws[i]->u32(), mles[i].d_data, lg_n, lg_blowup, mles[i].width, stream));
    SP1HIP_TRY(sp1hip_outer_merkle_commit(pd->cw_tensors.data(), n_mles, lg_h, pd->tree.u32(), rc.u32(), stream));
    uint32_t h[16];
    Mailbox mb;
    SP1HIP_TRY(mb.init(s));
    SP1HIP_TRY(mb.fetch(rc.p, 16, h));
    memcpy(pd->root, h, 32);
    memcpy(pd->commit, h + 8, 32);
    memcpy(h_commit, pd->commit, 32);
    *out = pd.release();
    return SP1HIP_SUCCESS;
}

void sp1hip_outer_basefold_data_free(sp1hip_outer_basefold_data_t* data) { delete data; }

size_t sp1hip_outer_basefold_proof_size(int dim, const uint32_t* round_widths, int n_rounds, sp1hip_fri_config_t config) {
    return proof_size(dim, round_widths, n_rounds, config);
}

int sp1hip_outer_basefold_prove(const sp1hip_ext_t* h_point, int dim, sp1hip_outer_basefold_data_t* const* rounds, int n_rounds,
                                const sp1hip_ext_t* h_claims, size_t n_claims, sp1hip_fri_config_t config,
                                sp1hip_outer_challenger_t* challenger, uint8_t* h_proof, size_t* proof_len, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(h_point && rounds && n_rounds > 0 && h_claims && challenger && proof_len, "null argument");
    SP1HIP_REQUIRE(dim >= 1 && dim <= kb::TWO_ADICITY, "dim out of range");
    SP1HIP_REQUIRE(config.num_queries > 0 && config.log_blowup >= 0 && config.proof_of_work_bits >= 0 && config.proof_of_work_bits < 31,
                   "bad config");
    SP1HIP_REQUIRE(dim + config.log_blowup <= kb::TWO_ADICITY, "instance exceeds two-adicity");
    std::vector<uint32_t> widths;
    size_t total_len = 0;
    for (int r = 0; r < n_rounds; r++) {
        SP1HIP_REQUIRE(rounds[r], "null round");
        SP1HIP_REQUIRE(rounds[r]->lg_n == dim, "eval point dimension mismatch");
        SP1HIP_REQUIRE(rounds[r]->lg_blowup == config.log_blowup, "round committed with a different blowup");
        widths.push_back(rounds[r]->total_width);
        total_len += rounds[r]->total_width;
    }
    SP1HIP_REQUIRE(total_len == n_claims, "one evaluation claim per committed column expected");
    for (int r = 0; r < n_rounds; r++)
        if (rounds[r]->tree.s != S(stream)) rounds[r]->foreign_use = true;
    const size_t need = proof_size(dim, widths.data(), n_rounds, config);
    if (!h_proof || *proof_len < need) {
        *proof_len = need;
        set_error("sp1hip_outer_basefold_prove: proof buffer too small, need %zu bytes", need);
        return SP1HIP_ERROR_BUFFER_TOO_SMALL;
    }
    std::vector<kb::Ext> point(dim);
    memcpy(point.data(), h_point, (size_t)dim * 16);
    // commit to the transcript only on success: the proof runs on a clone
    sp1hip_outer_challenger_t* work = nullptr;
    SP1HIP_TRY(sp1hip_outer_challenger_clone(challenger, &work));
    struct Free { sp1hip_outer_challenger_t* h; ~Free() { sp1hip_outer_challenger_free(h); } } free_work{work};
    size_t written = 0;
    SP1HIP_TRY(prove_trusted_mle_evaluations(point, rounds, n_rounds, reinterpret_cast<const kb::Ext*>(h_claims), n_claims, config,
                                             work, h_proof, need, &written, S(stream)));      // written in place
    if (written != need) {
        set_error("internal error: outer proof size %zu != expected %zu", written, need);
        return SP1HIP_ERROR_RUNTIME;
    }
    *proof_len = written;
    *outer_challenger_inner(challenger) = *outer_challenger_inner(work);
    return SP1HIP_SUCCESS;
}

}  // extern "C"
