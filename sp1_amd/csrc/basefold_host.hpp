// sp1_amd/csrc/basefold_host.hpp — host-side pieces shared by the two BaseFold provers (prover.hip: the inner KoalaBear
// Poseidon2 configuration; outer_basefold.hip: the outer BN254 one): the arena-backed device buffer, the bincode writer, the
// batching coefficients, and the internal entry points of the field kernels (basefold.hip) both round loops launch.
#pragma once
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

}  // namespace sp1hip
