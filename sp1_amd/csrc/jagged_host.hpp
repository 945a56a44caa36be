// sp1_amd/csrc/jagged_host.hpp — the seam between the jagged evaluation proof (jagged.hip) and the configuration it runs
// under. `JaggedProver::prove_trusted_evaluations` is field work — the jagged sumcheck, the jagged-eval sumcheck, the column
// evaluations — around three things that depend on the hash: the transcript, the dense (BaseFold) opening it ends in, and the
// bytes of a commitment. jagged_prove_with (jagged.hip: the argument checks, then JgProver::prove, a member function per phase; the
// kernels are in jagged_kernels.hpp) is the one round loop; the inner prover (jagged.hip: KoalaBear Poseidon2,
// DuplexChallenger) and the outer one (outer_jagged.hip: Poseidon2-BN254, MultiField32Challenger) are two JaggedBackends.
#pragma once
#include <vector>

#include "kb31.hpp"
#include "stacked_data.hpp"

namespace sp1hip {

struct JaggedBackend {
    virtual ~JaggedBackend() {}
    virtual const char* entry_point() const = 0;      // the C entry point, for messages
    // ---- transcript: the proof runs on a clone of the caller's challenger; accept() hands the state over on success
    virtual int begin() = 0;
    virtual void observe(uint32_t monty) = 0;         // one KoalaBear word
    virtual kb::Ext sample_ext() = 0;
    virtual void accept() = 0;
    // ---- the dense PCS of the committed rounds (in the order the rounds were passed to jagged_prove_with)
    virtual size_t opening_size(int dim, const uint32_t* round_widths, int n_rounds, sp1hip_fri_config_t config) const = 0;
    // bincode of the BaseFold proof into h_proof (capacity *len on entry, size on return), on the clone's transcript
    virtual int open(const sp1hip_ext_t* h_point, int dim, const sp1hip_ext_t* h_claims, size_t n_claims, sp1hip_fri_config_t config,
                     uint8_t* h_proof, size_t* len, sp1hip_stream_t stream) = 0;
    // ---- `merkle_tree_commitments[round]` as the proof carries it
    virtual size_t commitment_bytes() const = 0;
    virtual void write_commitment(int round, uint8_t* dst) const = 0;
};

// bincode(JaggedPcsProof) size: dense opening + batch evaluations + two sumchecks + counts + commitments + tail
size_t jagged_proof_size_with(size_t opening_bytes, size_t commitment_bytes, const std::vector<uint32_t>& round_widths,
                              const std::vector<size_t>& tables_per_round, uint64_t total_area);

// The argument checks, the size protocol (SP1HIP_ERROR_BUFFER_TOO_SMALL sets *proof_len), the proof, the bytes.
int jagged_prove_with(JaggedBackend& be, const sp1hip_ext_t* h_z_row, int max_log_row_count, StackedCore* const* rounds, int n_rounds,
                      const sp1hip_ext_t* h_claims, const size_t* claims_per_round, sp1hip_fri_config_t config, uint8_t* h_proof,
                      size_t* proof_len, sp1hip_stream_t stream);

}  // namespace sp1hip
