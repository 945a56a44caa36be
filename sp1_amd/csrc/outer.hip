// sp1_amd/csrc/outer.hip — the outer (BN254) commitment layer on gfx950: batched Poseidon2-BN254 permutations, the Merkle
// tensor commitment over KoalaBear tensors with one BN254 element per digest, openings, commit_mles, and the device grind
// of the outer transcript.
//
// Replaces, for the wrap prover's `SP1OuterGlobalContext` (/root/reference/slop/crates/bn254/src/lib.rs:L60-L90):
//   `MerkleTreeTcs` commit / open (/root/reference/slop/crates/merkle-tree/src/tcs.rs:L134-L184) with the hasher
//   MultiField32PaddingFreeSponge<KB, Fr, Perm, 3, 16, 1> and the compressor TruncatedPermutation<Perm, 2, 1, 3>
//   (statement: /root/reference/crates/recursion/circuit/src/hash.rs:L190-L221), and the grinding of
//   MultiField32Challenger (/root/reference/sp1-gpu/crates/basefold/src/grinding_challenger.rs:L104-L145).
//
// Kernel shapes (DESIGN.md §Outer commitments):
//  * outer_leaf_hash: one lane per row; the lane walks the concatenated row 16 columns per block (two chunks of 8, packed by
//    reduce_31 into lanes 0 and 1), every column load coalesced across the wave. A chunk may straddle two tensors: the
//    column table (tensor_table.hpp) flattens the message, so a chunk is just 8 consecutive global columns.
//  * outer_compress_layer: one lane per parent (64 B in, 32 B out); outer_compress_top: the last <= 512 leaves in one
//    workgroup, then the commitment compress(root, hash([lg_height, width])).
//  * outer_grind: one lane per candidate witness over a precomputed base state; the smallest hit by a global atomic min.
// Everything is ALU-bound (~240 Montgomery products per permutation against 16-64 bytes moved).
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "kb31.hpp"
#include "outer_tree.hpp"
#include "tensor_table.hpp"

sp1hip::OuterChallenger* outer_challenger_inner(sp1hip_outer_challenger_t* ch);

namespace sp1hip {
namespace {

using bn254::Fr;
using bn254::MulForm;

template <MulForm F>
__global__ __launch_bounds__(256) void outer_permute_kernel(uint32_t* __restrict__ states, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Fr x[3] = {load_fr(states + 24 * i), load_fr(states + 24 * i + 8), load_fr(states + 24 * i + 16)};
    outer::permute<F>(x, c_outer_rc);
    store_fr(states + 24 * i, x[0]);
    store_fr(states + 24 * i + 8, x[1]);
    store_fr(states + 24 * i + 16, x[2]);
}

// reduce_31 of the (at most 8) columns c0 .. c0 + n of row `row`, in Montgomery form
__device__ __forceinline__ Fr load_chunk(const uint32_t* const* __restrict__ cols, uint32_t c0, uint32_t n, uint32_t row) {
    uint32_t v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = (uint32_t)j < n ? kb::from_monty(gptr(cols[c0 + j])[row]) : 0u;
    return bn254::to_monty(bn254::pack31(v));
}

__global__ __launch_bounds__(256) void outer_leaf_hash_kernel(const uint32_t* const* __restrict__ cols, uint32_t total_width,
                                                              uint32_t height, uint32_t* __restrict__ leaves) {
    const uint32_t row = blockIdx.x * 256u + threadIdx.x;
    if (row >= height) return;
    Fr x[3] = {bn254::zero(), bn254::zero(), bn254::zero()};
    for (uint32_t c = 0; c < total_width; c += 16) {
        const uint32_t n = min(16u, total_width - c);
        x[0] = load_chunk(cols, c, min(8u, n), row);
        if (n > 8) x[1] = load_chunk(cols, c + 8, n - 8, row);    // a short last block leaves lane 1 as it is
        outer::permute(x, c_outer_rc);
    }
    store_fr(leaves + (size_t)row * 8, x[0]);
}

__global__ __launch_bounds__(256) void outer_compress_layer_kernel(const uint32_t* __restrict__ children, uint32_t n_parents,
                                                                   uint32_t* __restrict__ parents) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_parents) return;
    store_fr(parents + (size_t)i * 8, compress(load_fr(children + (size_t)i * 16), load_fr(children + (size_t)i * 16 + 8)));
}

// One workgroup: `layer` holds n (power of two, <= OUTER_TOP_MAX) digests, the parents follow level after level. The shape
// digest hash([lg_height, width]) (one permutation of reduce_31([lg_height, width]) in lane 0) is computed by the last wave
// next to the first level; then thread 0 writes the root and the commitment.
// Optional hand-over to the host in the same launch (a BaseFold round of outer_basefold.hip waits for [4 extra words | root |
// commitment]): payload, then — once the stores are acknowledged — the sequence number, like merkle.hip's compress_top_kernel.
__global__ __launch_bounds__(256) void outer_compress_top_kernel(uint32_t* layer, uint32_t n, uint32_t lg_height, uint32_t total_width,
                                                                 uint32_t* __restrict__ root_and_commit,
                                                                 const uint32_t* __restrict__ publish_extra,
                                                                 volatile uint32_t* publish_slot, uint32_t publish_seq) {
    __shared__ uint32_t shape[8];
    if (threadIdx.x == 255) {
        uint32_t v[8] = {lg_height, total_width, 0, 0, 0, 0, 0, 0};
        Fr x[3] = {bn254::to_monty(bn254::pack31(v)), bn254::zero(), bn254::zero()};
        outer::permute(x, c_outer_rc);
#pragma unroll
        for (int k = 0; k < 8; k++) shape[k] = x[0].w[k];
    }
    uint32_t* cur = layer;
    while (n > 1) {
        uint32_t* nxt = cur + (size_t)n * 8;
        const uint32_t np = n >> 1;
        for (uint32_t i = threadIdx.x; i < np; i += blockDim.x)
            store_fr(nxt + (size_t)i * 8, compress(load_fr(cur + (size_t)i * 16), load_fr(cur + (size_t)i * 16 + 8)));
        __syncthreads();
        cur = nxt;
        n = np;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const Fr root = load_fr(cur);
    Fr s;
#pragma unroll
    for (int k = 0; k < 8; k++) s.w[k] = shape[k];
    const Fr commit = compress(root, s);
    store_fr(root_and_commit, root);
    store_fr(root_and_commit + 8, commit);
    if (publish_slot == nullptr) return;
#pragma unroll
    for (int k = 0; k < 4; k++) publish_slot[1 + k] = publish_extra[k];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        publish_slot[5 + k] = root.w[k];
        publish_slot[13 + k] = commit.w[k];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the slot is uncached host memory: acknowledged stores, then seq
    __hip_atomic_store(const_cast<uint32_t*>(publish_slot), publish_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// x mod p_KB for a 64-bit x = hi 2^32 + lo: hi 2^32 = mul(hi, R2) in Montgomery arithmetic (R2 = 2^64 mod p)
__device__ __forceinline__ uint32_t kb_reduce_u32(uint32_t x) {
    x = x >= 2 * kb::P ? x - 2 * kb::P : x;
    return x >= kb::P ? x - kb::P : x;
}
__device__ __forceinline__ uint32_t kb_reduce_u64(uint32_t lo, uint32_t hi) {
    return kb::add(kb::mul(kb_reduce_u32(hi), kb::R2), kb_reduce_u32(lo));
}

struct GrindBase { uint32_t lanes[3][8]; };   // passed by value: the sponge as the witness's duplex sees it
// Each lane tests one candidate w: lane `chunk` = Montgomery(base integer + w 2^shift), permute, and the first sample is
// chunk 3 of split_32(lane 1): the top 64 bits of canonical lane 1, reduced into KoalaBear.
__global__ __launch_bounds__(256) void outer_grind_kernel(GrindBase base, int chunk, int shift, uint32_t mask, uint32_t first,
                                                          uint32_t count, uint32_t* result) {
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= count) return;
    const uint32_t w = first + t;
    if (w >= kb::P) return;
    const int k = shift >> 5, sh = shift & 31;
    Fr put;
#pragma unroll
    for (int i = 0; i < 8; i++)                                   // no dynamic register indexing: selects over all limbs
        put.w[i] = (i == k ? w << sh : 0u) | (i == k + 1 && sh > 1 ? w >> (32 - sh) : 0u);
    Fr x[3], b;
#pragma unroll
    for (int i = 0; i < 8; i++) {                                 // (word-wise selects: chunk is 0 or 1)
        x[0].w[i] = base.lanes[0][i];
        x[1].w[i] = base.lanes[1][i];
        x[2].w[i] = base.lanes[2][i];
        b.w[i] = chunk == 0 ? x[0].w[i] : x[1].w[i];
    }
    const Fr lane = bn254::to_monty(bn254::add_lazy(b, put));
#pragma unroll
    for (int i = 0; i < 8; i++) {
        x[0].w[i] = chunk == 0 ? lane.w[i] : x[0].w[i];
        x[1].w[i] = chunk == 1 ? lane.w[i] : x[1].w[i];
    }
    outer::permute(x, c_outer_rc);
    const Fr lane1 = bn254::from_monty(x[1]);
    if ((kb_reduce_u64(lane1.w[6], lane1.w[7]) & mask) == 0) atomicMin(result, w);
}

int merkle_commit(const sp1hip_tensor_t* tensors, int n_tensors, int lg_height, uint32_t* d_tree, uint32_t* d_root_and_commit,
                  hipStream_t s) {
    SP1HIP_REQUIRE(lg_height >= 0 && lg_height <= 30, "lg_height out of range");
    SP1HIP_REQUIRE(d_tree && d_root_and_commit, "null output");
    TensorTable tab;
    uint32_t tw = 0;
    SP1HIP_TRY(make_tensor_table(tensors, n_tensors, &tab, &tw));
    SP1HIP_REQUIRE(tw > 0, "width 0: nothing to commit");
    const uint32_t height = 1u << lg_height;
    AsyncScratch cols;
    SP1HIP_TRY(cols.alloc((size_t)tw * sizeof(uint32_t*), s));
    SP1HIP_TRY(expand_columns_async(tab, tw, height, (const uint32_t**)cols.p, s));
    {
        ScopedTimer t("outer_leaf_hash", s);
        hipLaunchKernelGGL(outer_leaf_hash_kernel, dim3((height + 255) / 256), dim3(256), 0, s, (const uint32_t* const*)cols.p, tw,
                           height, d_tree);
    }
    SP1HIP_LAUNCH_CHECK();
    return outer_finish_tree(d_tree, lg_height, tw, d_root_and_commit, s);
}

}  // namespace

int outer_finish_tree(uint32_t* d_tree, int lg_height, uint32_t total_width, uint32_t* d_root_and_commit, hipStream_t s,
                      const uint32_t* d_publish_extra, uint32_t* h_publish_slot, uint32_t publish_seq) {
    ScopedTimer t("outer_compress", s);
    uint32_t* cur = d_tree;
    uint32_t n = 1u << lg_height;
    while (n > OUTER_TOP_MAX) {
        const uint32_t np = n / 2;
        hipLaunchKernelGGL(outer_compress_layer_kernel, dim3((np + 255) / 256), dim3(256), 0, s, cur, np, cur + (size_t)n * 8);
        SP1HIP_LAUNCH_CHECK();
        cur += (size_t)n * 8;
        n = np;
    }
    hipLaunchKernelGGL(outer_compress_top_kernel, dim3(1), dim3(256), 0, s, cur, n, (uint32_t)lg_height, total_width,
                       d_root_and_commit, d_publish_extra, (volatile uint32_t*)h_publish_slot, publish_seq);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

int sp1hip_outer_poseidon2_permute(uint32_t* d_states, size_t n, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(d_states || n == 0, "null states");
    if (!n) return SP1HIP_SUCCESS;
    // SP1HIP_OUTER_MUL=lohi: the mul_lo / mul_hi form of the Montgomery product (bench/bench_outer.py compares the two)
    const char* e = getenv("SP1HIP_OUTER_MUL");
    const bool lohi = e && !strcmp(e, "lohi");
    if (lohi)
        hipLaunchKernelGGL(outer_permute_kernel<MulForm::LoHi>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), d_states, n);
    else
        hipLaunchKernelGGL(outer_permute_kernel<MulForm::Mad>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, S(stream), d_states, n);
    SP1HIP_LAUNCH_CHECK();
    return SP1HIP_SUCCESS;
}

int sp1hip_outer_merkle_commit(const sp1hip_tensor_t* tensors, int n_tensors, int lg_height, uint32_t* d_tree,
                               uint32_t* d_root_and_commit, sp1hip_stream_t stream) {
    return merkle_commit(tensors, n_tensors, lg_height, d_tree, d_root_and_commit, S(stream));
}

// The tree has the inner tree's layout (8 words per node, leaf layer first) and the opened values are rows of the same
// column-major tensors, so the inner opening kernels serve both.
int sp1hip_outer_merkle_open(const sp1hip_tensor_t* tensors, int n_tensors, int lg_height, const uint32_t* d_tree,
                             const uint32_t* d_indices, size_t n_idx, uint32_t* d_values, uint32_t* d_paths,
                             sp1hip_stream_t stream) {
    return sp1hip_merkle_open(tensors, n_tensors, lg_height, d_tree, d_indices, n_idx, d_values, d_paths, stream);
}

int sp1hip_outer_commit_mles(const sp1hip_tensor_t* mles, int n_mles, int lg_n, int lg_blowup, uint32_t* const* d_codewords,
                             uint32_t* d_tree, uint32_t h_commit[8], sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(mles && n_mles > 0 && d_codewords && d_tree && h_commit, "null argument");
    SP1HIP_REQUIRE(lg_n >= 0 && lg_blowup >= 0 && lg_n + lg_blowup <= 30, "lg_n + lg_blowup out of range");
    std::vector<sp1hip_tensor_t> cws(n_mles);
    for (int k = 0; k < n_mles; k++) {
        SP1HIP_REQUIRE(d_codewords[k], "null codeword buffer");
        SP1HIP_TRY(sp1hip_rs_encode_batch(d_codewords[k], mles[k].d_data, lg_n, lg_blowup, mles[k].width, stream));
        cws[k] = sp1hip_tensor_t{d_codewords[k], mles[k].width};
    }
    hipStream_t s = S(stream);
    uint32_t* d_rc16 = nullptr;
    SP1HIP_TRY(arena_alloc((void**)&d_rc16, 64, s));
    int st = merkle_commit(cws.data(), n_mles, lg_n + lg_blowup, d_tree, d_rc16, s);
    uint32_t h16[16];
    if (st == SP1HIP_SUCCESS) {
        hipError_t e = hipMemcpyAsync(h16, d_rc16, 64, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) st = map_hip_error(e, "sp1hip_outer_commit_mles");
    }
    arena_free(d_rc16, 64, s);
    SP1HIP_TRY(st);
    memcpy(h_commit, h16 + 8, 32);
    return SP1HIP_SUCCESS;
}

int sp1hip_outer_challenger_grind(sp1hip_outer_challenger_t* ch, int bits, uint32_t* witness, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(ch && witness, "null argument");
    SP1HIP_REQUIRE(bits >= 0 && bits < 31, "bits out of range");
    OuterChallenger& c = *outer_challenger_inner(ch);
    hipStream_t s = S(stream);
    GrindBase gb;
    int chunk = 0, shift = 0;
    outer_grind_base(c, gb.lanes, &chunk, &shift);
    const uint32_t mask = (uint32_t)((1u << bits) - 1);
    AsyncScratch buf;
    SP1HIP_TRY(buf.alloc(4, s));
    uint32_t* d_res = (uint32_t*)buf.p;
    SP1HIP_HIP(hipMemsetAsync(d_res, 0xff, 4, s));
    uint32_t found = 0xffffffffu;
    const uint32_t batch = 1u << std::min(22, bits + 3);
    for (uint64_t first = 0; first < kb::P && found == 0xffffffffu; first += batch) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(batch, kb::P - first);
        hipLaunchKernelGGL(outer_grind_kernel, dim3((cnt + 255) / 256), dim3(256), 0, s, gb, chunk, shift, mask, (uint32_t)first, cnt,
                           d_res);
        SP1HIP_LAUNCH_CHECK();
        SP1HIP_HIP(hipMemcpyAsync(&found, d_res, 4, hipMemcpyDeviceToHost, s));
        SP1HIP_HIP(hipStreamSynchronize(s));
    }
    if (found == 0xffffffffu) { set_error("outer grind: no witness found"); return SP1HIP_ERROR_RUNTIME; }
    c.observe(found);                                              // check_witness on the host transcript
    if ((c.sample() & mask) != 0) { set_error("outer grind: internal error, witness rejected by the host transcript"); return SP1HIP_ERROR_RUNTIME; }
    *witness = kb::to_monty(found);
    return SP1HIP_SUCCESS;
}

}  // extern "C"
