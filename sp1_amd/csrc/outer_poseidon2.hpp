// sp1_amd/csrc/outer_poseidon2.hpp — Poseidon2 over the BN254 scalar field (width 3, x^5, 8 full + 56 partial rounds): the
// permutation of the outer (wrap) configuration, and the host transcript built on it.
//
// Round structure (restated from /root/reference/slop/crates/bn254/src/lib.rs:L24-L58): the external layer
// x_i += x0 + x1 + x2 (circ(2, 1, 1)) once, 4 full rounds (rc on every lane, x^5 on every lane, external layer), 56 partial
// rounds (rc and x^5 on lane 0, internal layer x -> [x0 + s, x1 + s, 2 x2 + s] with s = x0 + x1 + x2), 4 full rounds.
// Constants: outer_poseidon2_rc.inc, written by sp1_amd/gen_outer_constants.py.
//
// Device form: the state is 24 VGPRs; the 56 partial rounds are a serial chain on lane 0, so throughput comes from many
// independent states per CU (one state per lane), not from ILP inside one permutation. The round counter is uniform, so
// the constants (in __constant__ memory, outer.hip) are fetched with scalar loads.
#pragma once
#include "bn254.hpp"

namespace outer {

using bn254::Fr;
using bn254::MulForm;

struct RoundConstants {
    uint32_t full[8][3][8];        // Montgomery words: full rounds 0..3, then 4..7
    uint32_t partial[56][8];
};
#define OUTER_RC_INIT {OUTER_RC_FULL_WORDS, OUTER_RC_PARTIAL_WORDS}

BN_HD Fr load(const uint32_t (&w)[8]) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.w[i] = w[i];
    return r;
}

// x_i += x0 + x1 + x2 (inputs canonical; each sum < 4p is exact in 256 bits)
BN_HD void external_layer(Fr (&x)[3]) {
    const Fr s = bn254::add_lazy(bn254::add_lazy(x[0], x[1]), x[2]);
    x[0] = bn254::reduce_4p(bn254::add_lazy(x[0], s));
    x[1] = bn254::reduce_4p(bn254::add_lazy(x[1], s));
    x[2] = bn254::reduce_4p(bn254::add_lazy(x[2], s));
}
// [x0 + s, x1 + s, 2 x2 + s] (2 x2 + s < 5p)
BN_HD void internal_layer(Fr (&x)[3]) {
    const Fr s = bn254::add_lazy(bn254::add_lazy(x[0], x[1]), x[2]);
    x[0] = bn254::reduce_4p(bn254::add_lazy(x[0], s));
    x[1] = bn254::reduce_4p(bn254::add_lazy(x[1], s));
    x[2] = bn254::reduce_5p(bn254::add_lazy(bn254::add_lazy(x[2], x[2]), s));
}
template <MulForm F> BN_HD Fr sbox(const Fr& x) {
    const Fr x2 = bn254::sqr<F>(x);
    const Fr x4 = bn254::sqr<F>(x2);
    return bn254::mul<F>(x4, x);
}

// (the three lanes are written out: a loop over them, around ~3k instructions of unrolled products, would exceed LLVM's
// pragma-unroll threshold, stay rolled and put the state in scratch)
template <MulForm F> BN_HD void full_round(Fr (&x)[3], const uint32_t (&rc)[3][8]) {
    x[0] = sbox<F>(bn254::add(x[0], load(rc[0])));
    x[1] = sbox<F>(bn254::add(x[1], load(rc[1])));
    x[2] = sbox<F>(bn254::add(x[2], load(rc[2])));
    external_layer(x);
}

template <MulForm F = MulForm::Mad> BN_HD void permute(Fr (&x)[3], const RoundConstants& rc) {
    external_layer(x);
#pragma unroll 1
    for (int r = 0; r < 4; r++) {
        full_round<F>(x, rc.full[r]);
    }
#pragma unroll 1
    for (int r = 0; r < 56; r++) {
        x[0] = sbox<F>(bn254::add(x[0], load(rc.partial[r])));
        internal_layer(x);
    }
#pragma unroll 1
    for (int r = 4; r < 8; r++) {
        full_round<F>(x, rc.full[r]);
    }
}

}  // namespace outer

namespace sp1hip {

// The host permutation (outer_host.cpp: 4 x 64-bit limbs, unsigned __int128 products): 3 lanes of 8 Montgomery words.
void outer_host_permute(uint32_t (&state)[3][8]);
// Host helpers on 8-word values: canonical -> Montgomery, Montgomery -> canonical.
void outer_host_to_monty(const uint32_t (&in)[8], uint32_t (&out)[8]);
void outer_host_from_monty(const uint32_t (&in)[8], uint32_t (&out)[8]);
// The outer sponge and compressor on the host, for the few permutations of a commitment's metadata (the jagged wrap):
// MultiField32PaddingFreeSponge over n canonical KoalaBear words (reduce_31 chunks of 8, 16 words per permutation, a short
// last block leaves the lanes it does not reach as they are) and compress = permute([l, r, 0])[0]. Digests: Montgomery words.
void outer_host_hash(const uint32_t* canonical, size_t n, uint32_t (&out)[8]);
void outer_host_compress(const uint32_t (&l)[8], const uint32_t (&r)[8], uint32_t (&out)[8]);

// MultiField32Challenger<KoalaBear, Bn254Fr, Perm, 3, 2> (stated in full by the in-circuit verifier of outer proofs,
// /root/reference/crates/recursion/circuit/src/challenger.rs:L258-L345, L455-L473). KoalaBear words are kept canonical.
struct OuterChallenger {
    uint32_t sponge[3][8] = {};      // Montgomery words
    uint32_t in[16];                 // canonical KoalaBear
    int n_in = 0;
    uint32_t out[8];                 // canonical KoalaBear: split_32(lane 0), split_32(lane 1); popped from the end
    int n_out = 0;

    void duplexing();
    void observe(uint32_t canonical);
    uint32_t sample();               // canonical
};
// The packed integer (not Montgomery) reduce_31(in[8 c .. n_in)) of the chunk the next observed element lands in, and the
// sponge lanes as the duplex that follows will see them: the device grind writes the candidate into lane c of that state.
void outer_grind_base(const OuterChallenger& ch, uint32_t (&lanes)[3][8], int* chunk, int* shift);

}  // namespace sp1hip
