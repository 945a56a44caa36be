// sp1_amd/csrc/basefold_host.hpp — the seam between the BaseFold opening (prover.hip) and the configuration it runs under.
// `BasefoldProver::prove_trusted_mle_evaluations` is field work — batching, the RS encode, the folds, the query gathers — around
// what depends on the hash: the transcript, the tree of a fold round, the way opened digests leave Montgomery form and the bytes
// of a digest. basefold_prove_with is the one round loop; the inner prover (prover.hip: KoalaBear Poseidon2, DuplexChallenger)
// and the outer one (outer_basefold.hip: Poseidon2-BN254, MultiField32Challenger) are two BasefoldBackends. Also here: the
// handle core both commits fill (BasefoldData), the arena-backed device buffer, the bincode writer, the batching coefficients,
// and the internal entry points of the field kernels (basefold.hip) the loop launches.
#pragma once
#include <atomic>
#include <memory>
#include <vector>

#include "device_ctx.hpp"
#include "round_sync.hpp"
#include "tensor_table.hpp"

namespace sp1hip {

int merkle_finish_tree(uint32_t*, int, uint32_t, uint32_t*, const DeviceCtx*, hipStream_t, const uint32_t* = nullptr, uint32_t* = nullptr, uint32_t = 0);
void leaf_hash_plan(const sp1hip_tensor_t* tensors, int n_tensors, std::vector<LeafPart>* parts);
int leaf_hash_part(const uint32_t* const* d_cols, uint32_t width, int k, int n_parts, uint32_t height, uint32_t* d_carry,
                   uint32_t* d_tree, const DeviceCtx* ctx, hipStream_t s);
int commit_ext_pairs(const uint32_t* d_cw, int lg_n, uint32_t* d_tree, uint32_t* d_root_and_commit, hipStream_t s,
                     const uint32_t* d_publish_extra = nullptr, uint32_t* h_publish_slot = nullptr, uint32_t publish_seq = 0);
int fold_round_async(const uint32_t* d_cw, int lg_c, const uint32_t* d_mle, int lg_m, const kb::Ext& beta, uint32_t* d_cw_out,
                     uint32_t* d_mle_out, const uint32_t* d_eq_next, uint32_t* d_zero_val, uint32_t* d_partial, hipStream_t s);
int open_ext_pairs(const uint32_t* d_cw, int lg_n, const uint32_t* d_indices, size_t n_idx, uint32_t* d_values, hipStream_t s);
int shift_indices(uint32_t* d_idx, size_t n, hipStream_t s);
struct FoldOpenDesc { const uint32_t* cw; const uint32_t* tree; uint32_t lg_c, vals_off, paths_off, pad; };   // basefold.hip
int open_fold_rounds(const FoldOpenDesc* d_descs, int n_rounds, int max_lg_c, const uint32_t* d_indices, size_t n_idx,
                     uint32_t* d_out, hipStream_t s);
int ext_fixed_at_zero_async(const uint32_t* d_mle, int lg_n, const uint32_t* d_eq, uint32_t* d_out, hipStream_t s);
int eq_prefix_tables_soa_async(const kb::Ext* h_point, int d, uint32_t* d_out, hipStream_t s);

// ---------------------------------------------------------------- prover data
// Buffers come from the stream-keyed arena (runtime.hip): steady-state proving re-uses the same HBM
// blocks without touching the driver.
struct DeviceBuf {
    void* p = nullptr;
    hipStream_t s = nullptr;
    size_t n = 0;
    int alloc(size_t bytes, hipStream_t stream) {
        s = stream;
        n = bytes;
        return arena_alloc(&p, bytes, stream);
    }
    ~DeviceBuf() { arena_free(p, n, s); }
    DeviceBuf() = default;
    DeviceBuf(const DeviceBuf&) = delete;
    DeviceBuf& operator=(const DeviceBuf&) = delete;
    uint32_t* u32() const { return (uint32_t*)p; }
};

// bincode writer straight into the caller's proof buffer (the BaseFold proof of a core shard is 1.4 MB: building it in a
// vector and copying it out — here, then again in the jagged and the shard wrappers — was five copies of it per proof)
struct ByteWriter {
    uint8_t* p = nullptr;
    size_t cap = 0, n = 0;
    bool overflow = false;
    uint8_t* take(size_t k) {
        if (n + k > cap) { overflow = true; return nullptr; }
        uint8_t* q = p + n;
        n += k;
        return q;
    }
    void u64(uint64_t v) { if (uint8_t* q = take(8)) memcpy(q, &v, 8); }      // little-endian host
    void u32(uint32_t v) { if (uint8_t* q = take(4)) memcpy(q, &v, 4); }
    void felt(uint32_t monty) { u32(kb::from_monty(monty)); }
    void felts(const uint32_t* m, size_t k) {
        uint8_t* q = take(4 * k);
        if (!q) return;
        for (size_t i = 0; i < k; i++) {
            const uint32_t c = kb::from_monty(m[i]);     // canonical word == its four bytes
            memcpy(q + 4 * i, &c, 4);
        }
    }
    void ext(const kb::Ext& e) { felts(e.c, 4); }
    void canonical_words(const uint32_t* c, size_t k) {  // words the device has already taken out of Montgomery form
        if (uint8_t* q = take(4 * k)) memcpy(q, c, 4 * k);
    }
};

inline int log2_ceil(size_t x) { int l = 0; while (((size_t)1 << l) < x) l++; return l; }

inline std::vector<kb::Ext> partial_lagrange_host(const std::vector<kb::Ext>& pt) {
    std::vector<kb::Ext> ev{kb::ext_one()};
    for (const kb::Ext& x : pt) {
        std::vector<kb::Ext> nx(ev.size() * 2);
        for (size_t i = 0; i < ev.size(); i++) {
            kb::Ext prod = kb::ext_mul(ev[i], x);
            nx[2 * i] = kb::ext_sub(ev[i], prod);
            nx[2 * i + 1] = prod;
        }
        ev.swap(nx);
    }
    return ev;
}

// ---------------------------------------------------------------- the committed round
// `BasefoldProverData` (/root/reference/slop/crates/basefold-prover/src/prover.rs:L25-L31): what sp1hip_basefold_data_t and
// sp1hip_outer_basefold_data_t are. Nothing in it depends on the hash: root and commit are 8 words either way (KoalaBear
// Montgomery words inside, the Montgomery words of one BN254 element outside).
struct BasefoldData {
    int lg_n = 0, lg_blowup = 0;
    std::vector<sp1hip_tensor_t> mles;            // caller-owned inputs [2^lg_n x w], column-major
    std::vector<std::unique_ptr<DeviceBuf>> cws;  // codewords [2^(lg_n+lg_blowup) x w]
    std::vector<sp1hip_tensor_t> cw_tensors;
    DeviceBuf tree;
    uint32_t root[8], commit[8];
    uint32_t total_width = 0;
    // The blocks go back to the free list of the stream that created them, which orders their reuse behind that stream's
    // work only. A handle that was also read on ANOTHER stream (a proving key's preprocessed commitment is opened by every
    // prover, each on its own stream) waits for the device before it lets go.
    std::atomic<bool> foreign_use{false};
    ~BasefoldData() { if (foreign_use) (void)hipDeviceSynchronize(); }
};

// The two halves of `commit_mles` that do not depend on the tree (prover.hip). basefold_data_alloc: the codewords and the tree
// of a commitment to `mles` on s; fills mles, cws, cw_tensors and total_width. basefold_data_fetch_commit: the 16 words
// [root | commit] the tree left at d_root_and_commit, through the mailbox into the handle and h_commit.
int basefold_data_alloc(BasefoldData* pd, const sp1hip_tensor_t* mles, int n_mles, int lg_n, int lg_blowup, hipStream_t s);
int basefold_data_fetch_commit(BasefoldData* pd, const uint32_t* d_root_and_commit, uint32_t h_commit[8], hipStream_t s);

// ---------------------------------------------------------------- the opening
enum BasefoldStage { BF_GRIND, BF_BATCH_ENCODE, BF_COMMIT_PHASE, BF_OPENINGS };

struct BasefoldBackend {
    virtual ~BasefoldBackend() {}
    virtual const char* entry_point() const = 0;      // the C entry point, for messages
    // the name a stage is timed under (sp1hip_timers_*); none: the stage records no events
    virtual const char* stage_timer(BasefoldStage) const { return nullptr; }
    // ---- transcript, in KoalaBear Montgomery words: the proof runs on a clone of the caller's challenger; accept() hands the
    // state over on success
    virtual int begin() = 0;
    virtual void observe(uint32_t monty) = 0;
    virtual kb::Ext sample_ext() = 0;
    virtual uint32_t sample_bits(int bits) = 0;
    virtual int observe_commitment(const uint32_t commit[8]) = 0;     // a fold round's commitment as the tree handed it over
    virtual int grind(int bits, uint32_t* witness_monty, hipStream_t s) = 0;
    virtual void accept() = 0;
    // ---- the tree over the paired leaves of a fold round's codeword (commit_ext_pairs' contract: the last kernel publishes
    // [d_publish_extra[0..4) | root | commitment] into the mailbox slot under sequence number publish_seq)
    virtual int commit_pairs(const uint32_t* d_cw, int lg_c, uint32_t* d_tree, uint32_t* d_root_and_commit, hipStream_t s,
                             const uint32_t* d_publish_extra, uint32_t* h_publish_slot, uint32_t publish_seq) = 0;
    // ---- the finished opening buffer out of Montgomery form, in place: the values of every opening (KoalaBear words), and
    // right behind them (d_paths == d_values + n_value_words) the path digests of every opening, 8 words each
    virtual int openings_from_monty(uint32_t* d_values, size_t n_value_words, uint32_t* d_paths, size_t n_path_words, hipStream_t s) = 0;
    // ---- the bincode of a digest
    virtual size_t digest_bytes() const = 0;
    virtual void write_digest(ByteWriter& w, const uint32_t* monty) const = 0;                           // roots, fri_commitments
    virtual void write_path_digests(ByteWriter& w, const uint32_t* canonical, size_t n) const = 0;      // n opened path entries
};

// bincode(BasefoldProof) size with digests of digest_bytes each
size_t basefold_proof_size(size_t digest_bytes, int dim, const uint32_t* round_widths, int n_rounds, const sp1hip_fri_config_t& cfg);

// The argument checks, the size protocol (SP1HIP_ERROR_BUFFER_TOO_SMALL sets *proof_len), the proof, the bytes.
int basefold_prove_with(BasefoldBackend& be, const sp1hip_ext_t* h_point, int dim, BasefoldData* const* rounds, int n_rounds,
                        const sp1hip_ext_t* h_claims, size_t n_claims, sp1hip_fri_config_t config, uint8_t* h_proof, size_t* proof_len,
                        sp1hip_stream_t stream);

}  // namespace sp1hip
