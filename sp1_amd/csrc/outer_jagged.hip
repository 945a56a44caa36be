// sp1_amd/csrc/outer_jagged.hip — the stacked and jagged PCS under the outer (BN254) configuration: what a wrap-shard prover
// calls for `commit_traces` / `setup` and for the shard proof's `evaluation_proof`.
//
//   sp1hip_outer_stacked_commit   `StackedPcsProver::commit_multilinears`   /root/reference/slop/crates/stacked/src/prover.rs:L59-L94
//   sp1hip_outer_jagged_commit    `JaggedProver::commit_multilinears`       /root/reference/slop/crates/jagged/src/prover.rs:L106-L160
//   sp1hip_outer_jagged_prove     `JaggedProver::prove_trusted_evaluations` prover.rs:L162-L328
// with `SP1OuterGlobalContext` (/root/reference/slop/crates/bn254/src/lib.rs:L60-L90).
//
// Nothing here is a kernel. The dense stacking is stacked.hip's (stacked_commit_dense), the commitment of the stacked batches is
// sp1hip_outer_commit_mles_data, the jagged wrap is two host permutations (outer_host.cpp), and the evaluation proof is the
// inner prover's round loop (jagged.hip: jagged_prove_with) over the MultiField32Challenger and sp1hip_outer_basefold_prove.
// The bytes differ from the inner proof in two places only: the BaseFold proof (40-byte digests) and
// `merkle_tree_commitments` (one 40-byte digest per round where the inner proof has 8 KoalaBear words).
#include <cstring>
#include <memory>
#include <vector>

#include "device_ctx.hpp"
#include "jagged_host.hpp"
#include "outer_poseidon2.hpp"
#include "stacked_data.hpp"

sp1hip::OuterChallenger* outer_challenger_inner(sp1hip_outer_challenger_t* ch);

namespace sp1hip {
namespace {

struct OuterJaggedBackend final : JaggedBackend {
    sp1hip_outer_challenger_t* caller;
    sp1hip_outer_challenger_t* work = nullptr;
    sp1hip_outer_stacked_data_t* const* rounds;
    int n_rounds;
    OuterJaggedBackend(sp1hip_outer_challenger_t* c, sp1hip_outer_stacked_data_t* const* r, int n) : caller(c), rounds(r), n_rounds(n) {}
    ~OuterJaggedBackend() override { sp1hip_outer_challenger_free(work); }
    const char* entry_point() const override { return "sp1hip_outer_jagged_prove"; }
    int begin() override { return sp1hip_outer_challenger_clone(caller, &work); }
    void observe(uint32_t monty) override { outer_challenger_inner(work)->observe(kb::from_monty(monty)); }
    kb::Ext sample_ext() override {
        kb::Ext e;
        for (int k = 0; k < 4; k++) e.c[k] = kb::to_monty(outer_challenger_inner(work)->sample());
        return e;
    }
    void accept() override { *outer_challenger_inner(caller) = *outer_challenger_inner(work); }
    size_t opening_size(int dim, const uint32_t* widths, int n, sp1hip_fri_config_t config) const override {
        return sp1hip_outer_basefold_proof_size(dim, widths, n, config);
    }
    int open(const sp1hip_ext_t* h_point, int dim, const sp1hip_ext_t* h_claims, size_t n_claims, sp1hip_fri_config_t config,
             uint8_t* h_proof, size_t* len, sp1hip_stream_t stream) override {
        std::vector<sp1hip_outer_basefold_data_t*> bf;
        for (int r = 0; r < n_rounds; r++) bf.push_back(rounds[r]->basefold);
        return sp1hip_outer_basefold_prove(h_point, dim, bf.data(), n_rounds, h_claims, n_claims, config, work, h_proof, len, stream);
    }
    // Hash<KoalaBear, Bn254Fr, 1>: u64(32) + the 32 little-endian bytes of the canonical value
    size_t commitment_bytes() const override { return 40; }
    void write_commitment(int round, uint8_t* dst) const override {
        uint32_t m[8], c[8];
        memcpy(m, rounds[round]->commit, 32);
        outer_host_from_monty(m, c);
        const uint64_t len = 32;
        memcpy(dst, &len, 8);
        memcpy(dst + 8, c, 32);
    }
};

}  // namespace
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

int sp1hip_outer_stacked_commit(const sp1hip_table_t* tables, int n_tables, int log_stacking_height, int batch_size, int lg_blowup,
                                uint32_t h_commit[8], uint64_t* num_added_vals, sp1hip_outer_stacked_data_t** out,
                                sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(h_commit && out, "bad argument");
    hipStream_t s = S(stream);
    std::unique_ptr<sp1hip_outer_stacked_data_s> sd(new sp1hip_outer_stacked_data_s());
    SP1HIP_TRY(stacked_commit_dense(tables, n_tables, log_stacking_height, batch_size, lg_blowup, sd.get(), num_added_vals, s,
                                    [&](const FillBatch& fill_batch) -> int {
        SP1HIP_REQUIRE(sd->area > 0, "an outer commitment needs at least one table value (the outer tree has no zero-width leaf)");
        // every batch is copied into the dense buffer in front of the encodes, on the stream that runs them
        for (int b = 0; b < (int)sd->batches.size(); b++) SP1HIP_TRY(fill_batch(b, s));
        return sp1hip_outer_commit_mles_data(sd->batches.data(), (int)sd->batches.size(), log_stacking_height, lg_blowup, sd->commit,
                                             &sd->basefold, stream);
    }));
    memcpy(h_commit, sd->commit, 32);
    *out = sd.release();
    return SP1HIP_SUCCESS;
}

int sp1hip_outer_jagged_commit(const sp1hip_table_t* tables, int n_tables, int max_log_row_count, int log_stacking_height,
                               int batch_size, int lg_blowup, uint32_t h_commit[8], sp1hip_outer_stacked_data_t** out,
                               sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(h_commit && out, "bad argument");
    JaggedTables t;
    SP1HIP_TRY(jagged_select_tables(tables, n_tables, max_log_row_count, &t));
    uint32_t stacked[8];
    uint64_t added = 0;
    SP1HIP_TRY(sp1hip_outer_stacked_commit(t.dense.data(), (int)t.dense.size(), log_stacking_height, batch_size, lg_blowup, stacked,
                                           &added, out, stream));
    // compress(stacked commitment, hash([n + 2, rows.., cols..])) under the outer sponge: two short host permutations
    const std::vector<uint32_t> meta = jagged_finish_counts(added, max_log_row_count, std::move(t), *out);
    uint32_t h[8], c[8];
    outer_host_hash(meta.data(), meta.size(), h);
    outer_host_compress(stacked, h, c);
    memcpy(h_commit, c, 32);
    memcpy((*out)->jagged_commit, c, 32);
    return SP1HIP_SUCCESS;
}

void sp1hip_outer_stacked_data_free(sp1hip_outer_stacked_data_t* data) { delete data; }

int sp1hip_outer_stacked_data_info(const sp1hip_outer_stacked_data_t* data, sp1hip_outer_basefold_data_t** basefold, int* n_batches,
                                   const uint32_t** d_dense, uint64_t* padded_area, uint32_t stacked_commit[8],
                                   uint32_t jagged_commit[8], size_t* n_tables, uint64_t* row_counts, uint64_t* column_counts,
                                   size_t counts_capacity) {
    SP1HIP_REQUIRE(data, "null argument");
    if (basefold) *basefold = data->basefold;
    if (n_batches) *n_batches = (int)data->batches.size();
    if (d_dense) *d_dense = (const uint32_t*)data->d_dense;
    if (padded_area) *padded_area = data->padded;
    if (stacked_commit) memcpy(stacked_commit, data->commit, 32);
    if (jagged_commit) {
        SP1HIP_REQUIRE(data->jagged, "not a jagged commitment");
        memcpy(jagged_commit, data->jagged_commit, 32);
    }
    if (n_tables) *n_tables = data->row_counts.size();
    if (row_counts || column_counts) {
        SP1HIP_REQUIRE(counts_capacity >= data->row_counts.size(), "counts_capacity smaller than the number of tables");
        for (size_t i = 0; i < data->row_counts.size(); i++) {
            if (row_counts) row_counts[i] = data->row_counts[i];
            if (column_counts) column_counts[i] = data->column_counts[i];
        }
    }
    return SP1HIP_SUCCESS;
}

int sp1hip_outer_stacked_batch(const sp1hip_outer_stacked_data_t* data, int k, sp1hip_tensor_t* batch) {
    SP1HIP_REQUIRE(data && batch && k >= 0 && k < (int)data->batches.size(), "bad argument");
    *batch = data->batches[k];
    return SP1HIP_SUCCESS;
}

size_t sp1hip_outer_jagged_proof_size(sp1hip_outer_stacked_data_t* const* rounds, int n_rounds, sp1hip_fri_config_t config) {
    if (!rounds || n_rounds <= 0 || !rounds[0]) return 0;
    const int lsh = rounds[0]->log_stacking_height;
    std::vector<uint32_t> widths;
    std::vector<size_t> tables;
    uint64_t area = 0;
    for (int r = 0; r < n_rounds; r++) {
        if (!rounds[r] || !rounds[r]->jagged) return 0;
        widths.push_back((uint32_t)(rounds[r]->padded >> lsh));
        tables.push_back(rounds[r]->row_counts.size());
        area += rounds[r]->padded;
    }
    return jagged_proof_size_with(sp1hip_outer_basefold_proof_size(lsh, widths.data(), n_rounds, config), 40, widths, tables, area);
}

int sp1hip_outer_jagged_prove(const sp1hip_ext_t* h_z_row, int max_log_row_count, sp1hip_outer_stacked_data_t* const* rounds,
                              int n_rounds, const sp1hip_ext_t* h_claims, const size_t* claims_per_round, sp1hip_fri_config_t config,
                              sp1hip_outer_challenger_t* challenger, uint8_t* h_proof, size_t* proof_len, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(rounds && n_rounds > 0 && n_rounds <= 8 && challenger, "bad argument");
    std::vector<StackedCore*> cores(rounds, rounds + n_rounds);
    OuterJaggedBackend be(challenger, rounds, n_rounds);
    return jagged_prove_with(be, h_z_row, max_log_row_count, cores.data(), n_rounds, h_claims, claims_per_round, config, h_proof,
                             proof_len, stream);
}

}  // extern "C"
