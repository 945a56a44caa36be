// sp1_amd/csrc/outer_tree.hpp — device pieces of the outer (BN254) Merkle tree shared by its kernels (outer.hip: row leaves,
// layers, the one-workgroup tail; outer_basefold.hip: the pair leaves of a BaseFold fold round), and the host entry that
// finishes a tree whose leaf layer is in place.
#pragma once
#include "common.hpp"
#include "outer_poseidon2.hpp"

namespace sp1hip {

// Compresses the leaf layer at d_tree (2^lg_height digests) up to the root and writes root | commitment (16 words).
// h_publish_slot != null: the one-workgroup tail also publishes [d_publish_extra[0..4) | root | commitment] to that mailbox
// slot with sequence number publish_seq (Mailbox::wait_next on the host side), as merkle_finish_tree does for the inner tree.
int outer_finish_tree(uint32_t* d_tree, int lg_height, uint32_t total_width, uint32_t* d_root_and_commit, hipStream_t s,
                      const uint32_t* d_publish_extra = nullptr, uint32_t* h_publish_slot = nullptr, uint32_t publish_seq = 0);

namespace {

using bn254::Fr;

__constant__ outer::RoundConstants c_outer_rc = OUTER_RC_INIT;

constexpr uint32_t OUTER_TOP_MAX = 512;       // leaves handed to the one-workgroup tail

__device__ __forceinline__ Fr load_fr(const uint32_t* p) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    return Fr{{a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w}};
}
__device__ __forceinline__ void store_fr(uint32_t* p, const Fr& x) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(x.w[0], x.w[1], x.w[2], x.w[3]);
    q[1] = make_uint4(x.w[4], x.w[5], x.w[6], x.w[7]);
}

__device__ __forceinline__ Fr compress(const Fr& l, const Fr& r) {
    Fr x[3] = {l, r, bn254::zero()};
    outer::permute(x, c_outer_rc);
    return x[0];
}

}  // namespace
}  // namespace sp1hip
