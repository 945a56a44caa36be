// sp1_amd/csrc/outer_basefold.hip — the BaseFold opening under the outer (BN254) configuration: what the wrap proof's
// `SP1OuterGlobalContext` (/root/reference/slop/crates/bn254/src/lib.rs:L60-L90) runs through
//   sp1hip_outer_commit_mles_data  `BasefoldProver::commit_mles`                    /root/reference/slop/crates/basefold-prover/src/prover.rs:L78-L99
//   sp1hip_outer_basefold_prove    `BasefoldProver::prove_trusted_mle_evaluations`  prover.rs:L102-L243 -> fri.rs:L31-L129
//
// The opening is the inner prover's round loop (prover.hip: basefold_prove_with) and the commit fills the inner prover's handle
// (basefold_host.hpp: BasefoldData); everything that is field work — batching, the RS encode, both folds, zero_val, the query
// gathers — is basefold.hip's. Here is only what the hash changes, the OuterBasefoldBackend:
//  * the transcript: the MultiField32Challenger (outer_host.cpp), KoalaBear words converted at the boundary, digests through
//    observe_commitment;
//  * the tree of a fold round: outer_leaf_hash_pairs, one lane per leaf (two extension elements = 8 KoalaBear words = one
//    reduce_31 chunk in lane 0, lanes 1 and 2 zero), one permutation, one digest store, then the tree finish with hand-over
//    (outer_finish_tree: the one-workgroup tail publishes [zero_val | root | commitment]);
//  * the digests of the opened PATHS leave Montgomery form in a pass of their own (BN254 words, 8 per digest) behind the pass
//    over the opened VALUES;
//  * the bincode of a digest: Hash<F, Bn254Fr, 1> = u64(32) + the 32 little-endian bytes of the canonical value (40 bytes).
// The bytes differ from the inner proof in the digests only. PoW witnesses: the smallest one.
#include <cstring>
#include <memory>
#include <vector>

#include "basefold_host.hpp"
#include "outer_tree.hpp"

sp1hip::OuterChallenger* outer_challenger_inner(sp1hip_outer_challenger_t* ch);

struct sp1hip_outer_basefold_data_s : sp1hip::BasefoldData {};

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

struct OuterBasefoldBackend final : BasefoldBackend {
    sp1hip_outer_challenger_t* caller;
    sp1hip_outer_challenger_t* work = nullptr;
    explicit OuterBasefoldBackend(sp1hip_outer_challenger_t* c) : caller(c) {}
    ~OuterBasefoldBackend() override { sp1hip_outer_challenger_free(work); }
    const char* entry_point() const override { return "sp1hip_outer_basefold_prove"; }
    const char* stage_timer(BasefoldStage stage) const override {
        switch (stage) {
            case BF_GRIND: return "outer_bf_grind";
            case BF_BATCH_ENCODE: return "outer_bf_batch_encode";
            case BF_COMMIT_PHASE: return "outer_bf_commit_phase";
            case BF_OPENINGS: return "outer_bf_openings";
        }
        return nullptr;
    }
    int begin() override { return sp1hip_outer_challenger_clone(caller, &work); }
    void observe(uint32_t monty) override { outer_challenger_inner(work)->observe(kb::from_monty(monty)); }
    kb::Ext sample_ext() override {
        kb::Ext e;
        for (int k = 0; k < 4; k++) e.c[k] = kb::to_monty(outer_challenger_inner(work)->sample());
        return e;
    }
    uint32_t sample_bits(int bits) override { return outer_challenger_inner(work)->sample() & (uint32_t)((1u << bits) - 1); }
    int observe_commitment(const uint32_t commit[8]) override { return sp1hip_outer_challenger_observe_commitment(work, commit); }
    int grind(int bits, uint32_t* witness_monty, hipStream_t s) override {
        return sp1hip_outer_challenger_grind(work, bits, witness_monty, s);
    }
    void accept() override { *outer_challenger_inner(caller) = *outer_challenger_inner(work); }
    int commit_pairs(const uint32_t* d_cw, int lg_c, uint32_t* d_tree, uint32_t* d_root_and_commit, hipStream_t s,
                     const uint32_t* d_publish_extra, uint32_t* h_publish_slot, uint32_t publish_seq) override {
        return commit_ext_pairs_outer(d_cw, lg_c, d_tree, d_root_and_commit, s, d_publish_extra, h_publish_slot, publish_seq);
    }
    // each region in one launch of its own kind: KoalaBear words, then BN254 digests
    int openings_from_monty(uint32_t* d_values, size_t n_value_words, uint32_t* d_paths, size_t n_path_words, hipStream_t s) override {
        SP1HIP_TRY(sp1hip_from_monty(d_values, n_value_words, (sp1hip_stream_t)s));
        if (n_path_words) {
            const uint32_t nd = (uint32_t)(n_path_words / 8);
            hipLaunchKernelGGL(outer_digests_from_monty_kernel, dim3((nd + 255) / 256), dim3(256), 0, s, d_paths, nd);
            SP1HIP_LAUNCH_CHECK();
        }
        return SP1HIP_SUCCESS;
    }
    size_t digest_bytes() const override { return DIGEST_BYTES; }
    void write_digest(ByteWriter& w, const uint32_t* monty) const override {
        uint32_t m[8], c[8];
        memcpy(m, monty, 32);
        outer_host_from_monty(m, c);
        write_path_digests(w, c, 1);
    }
    void write_path_digests(ByteWriter& w, const uint32_t* canonical, size_t n) const override {
        for (size_t k = 0; k < n; k++) {                     // 8 canonical words == the 32 little-endian bytes
            w.u64(32);
            w.canonical_words(canonical + 8 * k, 8);
        }
    }
};

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
    for (int i = 0; i < n_mles; i++) SP1HIP_REQUIRE(mles[i].d_data && mles[i].width > 0, "null or empty mle");
    SP1HIP_TRY(basefold_data_alloc(pd.get(), mles, n_mles, lg_n, lg_blowup, s));
    DeviceBuf rc;
    SP1HIP_TRY(rc.alloc(64, s));
    for (int i = 0; i < n_mles; i++)
        SP1HIP_TRY(sp1hip_rs_encode_batch(pd->cws[i]->u32(), mles[i].d_data, lg_n, lg_blowup, mles[i].width, stream));
    SP1HIP_TRY(sp1hip_outer_merkle_commit(pd->cw_tensors.data(), n_mles, lg_n + lg_blowup, pd->tree.u32(), rc.u32(), stream));
    SP1HIP_TRY(basefold_data_fetch_commit(pd.get(), rc.u32(), h_commit, s));
    *out = pd.release();
    return SP1HIP_SUCCESS;
}

void sp1hip_outer_basefold_data_free(sp1hip_outer_basefold_data_t* data) { delete data; }

size_t sp1hip_outer_basefold_proof_size(int dim, const uint32_t* round_widths, int n_rounds, sp1hip_fri_config_t config) {
    return basefold_proof_size(DIGEST_BYTES, dim, round_widths, n_rounds, config);
}

int sp1hip_outer_basefold_prove(const sp1hip_ext_t* h_point, int dim, sp1hip_outer_basefold_data_t* const* rounds, int n_rounds,
                                const sp1hip_ext_t* h_claims, size_t n_claims, sp1hip_fri_config_t config,
                                sp1hip_outer_challenger_t* challenger, uint8_t* h_proof, size_t* proof_len, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(rounds && n_rounds > 0 && challenger, "null argument");
    std::vector<BasefoldData*> data(rounds, rounds + n_rounds);
    OuterBasefoldBackend be(challenger);
    return basefold_prove_with(be, h_point, dim, data.data(), n_rounds, h_claims, n_claims, config, h_proof, proof_len, stream);
}

}  // extern "C"
