// sp1_amd/csrc/outer_host.cpp — the outer (BN254) permutation and the MultiField32Challenger transcript on the HOST (x86-64,
// no device code in this translation unit).
//
// The host arithmetic is its own formulation, independent of bn254.hpp's 32-bit device limbs: 4 x 64-bit limbs, CIOS
// Montgomery products through unsigned __int128, every intermediate reduced to [0, p). The GPU tests compare the device
// permutation against this one word for word, and tests/outer_model.py (Python ints) pins both.
#include <cstring>

#include "common.hpp"
#include "kb31.hpp"
#include "outer_poseidon2.hpp"

namespace sp1hip {
namespace {

typedef unsigned __int128 u128;
struct F4 { uint64_t l[4]; };

const uint32_t P32[8] = OUTER_P_WORDS;
const uint32_t R2_32[8] = OUTER_R2_WORDS;
const outer::RoundConstants RC = OUTER_RC_INIT;

F4 from32(const uint32_t* w) { F4 r; memcpy(r.l, w, 32); return r; }
void to32(const F4& a, uint32_t* w) { memcpy(w, a.l, 32); }
const F4& P4() { static const F4 p = from32(P32); return p; }
uint64_t np64() {                              // -p^-1 mod 2^64 (Newton iteration on the low limb)
    static const uint64_t v = [] {
        const uint64_t p0 = P4().l[0];
        uint64_t inv = 1;
        for (int i = 0; i < 7; i++) inv *= 2 - p0 * inv;
        return (uint64_t)0 - inv;
    }();
    return v;
}

bool geq(const F4& a, const F4& b) {
    for (int i = 3; i >= 0; i--)
        if (a.l[i] != b.l[i]) return a.l[i] > b.l[i];
    return true;
}
F4 sub_raw(const F4& a, const F4& b) {
    F4 r;
    uint64_t borrow = 0;
    for (int i = 0; i < 4; i++) {
        const u128 d = (u128)a.l[i] - b.l[i] - borrow;
        r.l[i] = (uint64_t)d;
        borrow = (uint64_t)(d >> 64) & 1;
    }
    return r;
}
F4 addm(const F4& a, const F4& b) {            // a, b < p (p < 2^254: no carry out of 256 bits)
    F4 r;
    uint64_t c = 0;
    for (int i = 0; i < 4; i++) {
        const u128 s = (u128)a.l[i] + b.l[i] + c;
        r.l[i] = (uint64_t)s;
        c = (uint64_t)(s >> 64);
    }
    return geq(r, P4()) ? sub_raw(r, P4()) : r;
}
F4 mulm(const F4& a, const F4& b) {            // a b 2^-256 mod p, a, b < p
    const F4& p = P4();
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        uint64_t carry = 0;
        for (int j = 0; j < 4; j++) {
            const u128 s = (u128)a.l[j] * b.l[i] + t[j] + carry;
            t[j] = (uint64_t)s;
            carry = (uint64_t)(s >> 64);
        }
        u128 s = (u128)t[4] + carry;
        t[4] = (uint64_t)s;
        t[5] = (uint64_t)(s >> 64);
        const uint64_t m = t[0] * np64();
        s = (u128)m * p.l[0] + t[0];
        carry = (uint64_t)(s >> 64);
        for (int j = 1; j < 4; j++) {
            s = (u128)m * p.l[j] + t[j] + carry;
            t[j - 1] = (uint64_t)s;
            carry = (uint64_t)(s >> 64);
        }
        s = (u128)t[4] + carry;
        t[3] = (uint64_t)s;
        t[4] = t[5] + (uint64_t)(s >> 64);
    }
    F4 r = {{t[0], t[1], t[2], t[3]}};
    return (t[4] || geq(r, p)) ? sub_raw(r, p) : r;
}
F4 sbox(const F4& x) {
    const F4 x2 = mulm(x, x), x4 = mulm(x2, x2);
    return mulm(x4, x);
}
void external_layer(F4 (&x)[3]) {
    const F4 s = addm(addm(x[0], x[1]), x[2]);
    for (int i = 0; i < 3; i++) x[i] = addm(x[i], s);
}

void permute4(F4 (&x)[3]) {
    external_layer(x);
    for (int r = 0; r < 8; r++) {
        if (r == 4) {
            for (int k = 0; k < 56; k++) {
                x[0] = sbox(addm(x[0], from32(RC.partial[k])));
                const F4 s = addm(addm(x[0], x[1]), x[2]);
                x[0] = addm(x[0], s);
                x[1] = addm(x[1], s);
                x[2] = addm(addm(x[2], x[2]), s);
            }
        }
        for (int i = 0; i < 3; i++) x[i] = sbox(addm(x[i], from32(RC.full[r][i])));
        external_layer(x);
    }
}

// canonical BN254 (8 words) -> the 64-bit chunk k reduced into KoalaBear (split_32)
uint32_t split_chunk(const uint32_t (&canon)[8], int k) {
    const uint64_t v = (uint64_t)canon[2 * k] | ((uint64_t)canon[2 * k + 1] << 32);
    return (uint32_t)(v % kb::P);
}

void pack_chunk(const uint32_t* vals, int n, uint32_t (&out)[8]) {
    uint32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; i++) v[i] = vals[i];
    const bn254::Fr r = bn254::pack31(v);
    memcpy(out, r.w, 32);
}

}  // namespace

void outer_host_permute(uint32_t (&state)[3][8]) {
    F4 x[3] = {from32(state[0]), from32(state[1]), from32(state[2])};
    permute4(x);
    for (int i = 0; i < 3; i++) to32(x[i], state[i]);
}
void outer_host_to_monty(const uint32_t (&in)[8], uint32_t (&out)[8]) { to32(mulm(from32(in), from32(R2_32)), out); }
void outer_host_from_monty(const uint32_t (&in)[8], uint32_t (&out)[8]) {
    const F4 one = {{1, 0, 0, 0}};
    to32(mulm(from32(in), one), out);
}

void outer_host_hash(const uint32_t* canonical, size_t n, uint32_t (&out)[8]) {
    uint32_t st[3][8] = {};
    for (size_t c = 0; c < n; c += 16) {
        const size_t k = n - c < 16 ? n - c : 16;
        uint32_t packed[8];
        pack_chunk(canonical + c, (int)(k < 8 ? k : 8), packed);
        outer_host_to_monty(packed, st[0]);
        if (k > 8) {
            pack_chunk(canonical + c + 8, (int)(k - 8), packed);
            outer_host_to_monty(packed, st[1]);
        }
        outer_host_permute(st);
    }
    memcpy(out, st[0], 32);
}
void outer_host_compress(const uint32_t (&l)[8], const uint32_t (&r)[8], uint32_t (&out)[8]) {
    uint32_t st[3][8] = {};
    memcpy(st[0], l, 32);
    memcpy(st[1], r, 32);
    outer_host_permute(st);
    memcpy(out, st[0], 32);
}

void OuterChallenger::duplexing() {
    for (int c = 0; 8 * c < n_in; c++) {
        uint32_t packed[8];
        pack_chunk(in + 8 * c, n_in - 8 * c < 8 ? n_in - 8 * c : 8, packed);
        outer_host_to_monty(packed, sponge[c]);
    }
    n_in = 0;
    outer_host_permute(sponge);
    for (int lane = 0; lane < 2; lane++) {
        uint32_t canon[8];
        outer_host_from_monty(sponge[lane], canon);
        for (int k = 0; k < 4; k++) out[4 * lane + k] = split_chunk(canon, k);
    }
    n_out = 8;
}
void OuterChallenger::observe(uint32_t canonical) {
    n_out = 0;
    in[n_in++] = canonical;
    if (n_in == 16) duplexing();
}
uint32_t OuterChallenger::sample() {
    if (n_in != 0 || n_out == 0) duplexing();
    return out[--n_out];
}

void outer_grind_base(const OuterChallenger& ch, uint32_t (&lanes)[3][8], int* chunk, int* shift) {
    memcpy(lanes, ch.sponge, sizeof lanes);
    const int c = ch.n_in / 8;
    for (int i = 0; i < c; i++) {
        uint32_t packed[8];
        pack_chunk(ch.in + 8 * i, 8, packed);
        outer_host_to_monty(packed, lanes[i]);
    }
    pack_chunk(ch.in + 8 * c, ch.n_in - 8 * c, lanes[c]);
    *chunk = c;
    *shift = 31 * (ch.n_in - 8 * c);
}

}  // namespace sp1hip

struct sp1hip_outer_challenger_s { sp1hip::OuterChallenger ch; };

using namespace sp1hip;

namespace {
bool canonical_bn254(const uint32_t* w) {
    for (int i = 7; i >= 0; i--)
        if (w[i] != P32[i]) return w[i] < P32[i];
    return false;
}
}  // namespace

extern "C" {

int sp1hip_outer_poseidon2_permute_host(uint32_t* h_states, size_t n) {
    SP1HIP_REQUIRE(h_states || n == 0, "null states");
    for (size_t i = 0; i < 3 * n; i++) SP1HIP_REQUIRE(canonical_bn254(h_states + 8 * i), "state words must be canonical (< p) Montgomery words");
    for (size_t i = 0; i < n; i++) outer_host_permute(*reinterpret_cast<uint32_t (*)[3][8]>(h_states + 24 * i));
    return SP1HIP_SUCCESS;
}

int sp1hip_outer_challenger_new(sp1hip_outer_challenger_t** out) {
    SP1HIP_REQUIRE(out, "null output");
    *out = new sp1hip_outer_challenger_s();
    return SP1HIP_SUCCESS;
}
int sp1hip_outer_challenger_clone(const sp1hip_outer_challenger_t* ch, sp1hip_outer_challenger_t** out) {
    SP1HIP_REQUIRE(ch && out, "null argument");
    *out = new sp1hip_outer_challenger_s(*ch);
    return SP1HIP_SUCCESS;
}
void sp1hip_outer_challenger_free(sp1hip_outer_challenger_t* ch) { delete ch; }
int sp1hip_outer_challenger_observe(sp1hip_outer_challenger_t* ch, const uint32_t* felts, size_t n) {
    SP1HIP_REQUIRE(ch && (felts || n == 0), "null argument");
    for (size_t i = 0; i < n; i++) SP1HIP_REQUIRE(felts[i] < kb::P, "non-reduced field word");
    for (size_t i = 0; i < n; i++) ch->ch.observe(kb::from_monty(felts[i]));
    return SP1HIP_SUCCESS;
}
int sp1hip_outer_challenger_observe_commitment(sp1hip_outer_challenger_t* ch, const uint32_t* digest8) {
    SP1HIP_REQUIRE(ch && digest8, "null argument");
    SP1HIP_REQUIRE(canonical_bn254(digest8), "digest is not a canonical (< p) Montgomery word");
    uint32_t m[8], canon[8];
    memcpy(m, digest8, 32);
    outer_host_from_monty(m, canon);
    for (int k = 0; k < 4; k++) ch->ch.observe(split_chunk(canon, k));
    return SP1HIP_SUCCESS;
}
int sp1hip_outer_challenger_sample(sp1hip_outer_challenger_t* ch, uint32_t* out) {
    SP1HIP_REQUIRE(ch && out, "null argument");
    *out = kb::to_monty(ch->ch.sample());
    return SP1HIP_SUCCESS;
}
int sp1hip_outer_challenger_sample_ext(sp1hip_outer_challenger_t* ch, sp1hip_ext_t* out) {
    SP1HIP_REQUIRE(ch && out, "null argument");
    for (int k = 0; k < 4; k++) out->c[k] = kb::to_monty(ch->ch.sample());
    return SP1HIP_SUCCESS;
}
int sp1hip_outer_challenger_sample_bits(sp1hip_outer_challenger_t* ch, int bits, uint32_t* out) {
    SP1HIP_REQUIRE(ch && out && bits >= 0 && bits < 32, "bad argument");
    *out = ch->ch.sample() & (uint32_t)(((uint64_t)1 << bits) - 1);
    return SP1HIP_SUCCESS;
}
int sp1hip_outer_challenger_check_witness(sp1hip_outer_challenger_t* ch, int bits, uint32_t witness, int* ok) {
    SP1HIP_REQUIRE(ch && ok && bits >= 0 && bits < 32 && witness < kb::P, "bad argument");
    ch->ch.observe(kb::from_monty(witness));
    *ok = (ch->ch.sample() & (uint32_t)(((uint64_t)1 << bits) - 1)) == 0 ? 1 : 0;
    return SP1HIP_SUCCESS;
}
int sp1hip_outer_challenger_state(const sp1hip_outer_challenger_t* ch, uint32_t* out50) {
    SP1HIP_REQUIRE(ch && out50, "null argument");
    memset(out50, 0, 50 * 4);
    memcpy(out50, ch->ch.sponge, 96);
    out50[24] = (uint32_t)ch->ch.n_in;
    for (int i = 0; i < ch->ch.n_in; i++) out50[25 + i] = kb::to_monty(ch->ch.in[i]);
    out50[41] = (uint32_t)ch->ch.n_out;
    for (int i = 0; i < ch->ch.n_out; i++) out50[42 + i] = kb::to_monty(ch->ch.out[i]);
    return SP1HIP_SUCCESS;
}

}  // extern "C"

// (sp1hip_outer_challenger_grind is in outer.hip: it launches the device search)
sp1hip::OuterChallenger* outer_challenger_inner(sp1hip_outer_challenger_t* ch) { return ch ? &ch->ch : nullptr; }
