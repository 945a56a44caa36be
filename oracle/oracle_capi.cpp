#include <omp.h>
// oracle/oracle_capi.cpp — TEST INFRASTRUCTURE ONLY.
//
// C ABI over the CPU oracle (kb_field.hpp / kb_hash.hpp / kb_pcs.hpp / kb_zerocheck.hpp) so that
// tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg can drive it through ctypes.
// Nothing in sp1_amd/ (the product) may link, load or call this library.
// All field words crossing this ABI are Montgomery u32 (R = 2^32) unless a name says "canonical".
#include <cstdio>
#include <cstdlib>

#include "kb_zerocheck.hpp"
#include "kb_jagged.hpp"
#include "kb_gkr.hpp"
#include "kb_shard.hpp"

using namespace orc;

static inline const F* FP(const uint32_t* p) { return reinterpret_cast<const F*>(p); }
static inline F* FP(uint32_t* p) { return reinterpret_cast<F*>(p); }
static inline E load_e(const uint32_t* p) { E e; memcpy(&e, p, 16); return e; }
static inline Digest load_d(const uint32_t* p) { Digest d; memcpy(&d, p, 32); return d; }

#include "bb_commit.hpp"

extern "C" {

// ---- field ----------------------------------------------------------------------------------
void orc_to_monty(uint32_t* x, size_t n) { for (size_t i = 0; i < n; i++) x[i] = F::from_canonical(x[i]).v; }
void orc_from_monty(uint32_t* x, size_t n) { for (size_t i = 0; i < n; i++) x[i] = F::raw(x[i]).canonical(); }
uint32_t orc_two_adic_generator(int bits) { return two_adic_generator(bits).v; }
void orc_ext_mul(const uint32_t* a, const uint32_t* b, uint32_t* out) { E r = load_e(a) * load_e(b); memcpy(out, &r, 16); }
void orc_ext_inv(const uint32_t* a, uint32_t* out) { E r = einv(load_e(a)); memcpy(out, &r, 16); }

// ---- hash -----------------------------------------------------------------------------------
void orc_permute(uint32_t* s16) { permute(FP(s16)); }
void orc_hash(const uint32_t* in, size_t n, uint32_t* out8) { Digest d = hash_slice(FP(in), n); memcpy(out8, &d, 32); }
void orc_compress(const uint32_t* l, const uint32_t* r, uint32_t* out8) {
    Digest d = compress(load_d(l), load_d(r));
    memcpy(out8, &d, 32);
}

// ---- challenger -----------------------------------------------------------------------------
void* orc_challenger_new() { return new Challenger(); }
void* orc_challenger_clone(void* c) { return new Challenger(*static_cast<Challenger*>(c)); }
void orc_challenger_free(void* c) { delete static_cast<Challenger*>(c); }
void orc_challenger_observe(void* c, const uint32_t* x, size_t n) {
    for (size_t i = 0; i < n; i++) static_cast<Challenger*>(c)->observe(F::raw(x[i]));
}
uint32_t orc_challenger_sample(void* c) { return static_cast<Challenger*>(c)->sample().v; }
void orc_challenger_sample_ext(void* c, uint32_t* out4) { E e = static_cast<Challenger*>(c)->sample_ext(); memcpy(out4, &e, 16); }
uint32_t orc_challenger_sample_bits(void* c, int bits) { return static_cast<Challenger*>(c)->sample_bits(bits); }
uint32_t orc_challenger_grind(void* c, int bits) { return static_cast<Challenger*>(c)->grind(bits).v; }
int orc_challenger_check_witness(void* c, int bits, uint32_t w) { return static_cast<Challenger*>(c)->check_witness(bits, F::raw(w)); }
// state dump: 16 sponge words, n_in, in[8], n_out, out[8]  (34 words)
void orc_challenger_state(void* c, uint32_t* out34) {
    Challenger* ch = static_cast<Challenger*>(c);
    memset(out34, 0, 34 * 4);
    for (int i = 0; i < 16; i++) out34[i] = ch->state[i].v;
    out34[16] = (uint32_t)ch->in.size();
    for (size_t i = 0; i < ch->in.size(); i++) out34[17 + i] = ch->in[i].v;
    out34[25] = (uint32_t)ch->out.size();
    for (size_t i = 0; i < ch->out.size(); i++) out34[26 + i] = ch->out[i].v;
}

// ---- RS encode / folds / multilinear ----------------------------------------------------------
void orc_rs_encode(const uint32_t* in, int log_n, int w, int log_blowup, uint32_t* out) {
    rs_encode(FP(in), log_n, w, log_blowup, FP(out));
}
void orc_fold_even_odd(const uint32_t* cw, int log_N, const uint32_t* beta, uint32_t* out) {
    std::vector<E> v((size_t)1 << log_N);
    memcpy(v.data(), cw, v.size() * 16);
    std::vector<E> r = fold_even_odd(v, load_e(beta));
    memcpy(out, r.data(), r.size() * 16);
}
void orc_fold_mle(const uint32_t* m, int log_n, const uint32_t* beta, uint32_t* out) {
    std::vector<E> v((size_t)1 << log_n);
    memcpy(v.data(), m, v.size() * 16);
    std::vector<E> r = fold_mle(v, load_e(beta));
    memcpy(out, r.data(), r.size() * 16);
}
void orc_partial_lagrange(const uint32_t* point, int dim, uint32_t* out) {
    std::vector<E> p(dim);
    memcpy(p.data(), point, (size_t)dim * 16);
    std::vector<E> r = partial_lagrange(p);
    memcpy(out, r.data(), r.size() * 16);
}
void orc_eval_mle(const uint32_t* mle, int log_n, int w, const uint32_t* point, uint32_t* out) {
    std::vector<E> p(log_n);
    memcpy(p.data(), point, (size_t)log_n * 16);
    std::vector<E> r = eval_mle_at_point(FP(mle), (size_t)1 << log_n, w, p);
    memcpy(out, r.data(), r.size() * 16);
}

// ---- Merkle tensor commitment ---------------------------------------------------------------
void* orc_merkle_commit(const uint32_t** tensors, const int* widths, int n, size_t height, uint32_t* commit8) {
    std::vector<TensorRef> ts;
    for (int i = 0; i < n; i++) ts.push_back({FP(tensors[i]), height, widths[i]});
    MerkleTree* mt = new MerkleTree(merkle_commit(ts));
    memcpy(commit8, &mt->commit, 32);
    return mt;
}
void orc_merkle_free(void* t) { delete static_cast<MerkleTree*>(t); }
// leaf-first concatenated layers: (2*height - 1) digests
void orc_merkle_layers(void* t, uint32_t* out) {
    MerkleTree* mt = static_cast<MerkleTree*>(t);
    size_t o = 0;
    for (auto& l : mt->layers) { memcpy(out + o * 8, l.data(), l.size() * 32); o += l.size(); }
}
void orc_merkle_root(void* t, uint32_t* out8) { memcpy(out8, &static_cast<MerkleTree*>(t)->root, 32); }
// paths out: [n_idx][log_height][8]
void orc_merkle_paths(void* t, const uint64_t* idx, size_t n_idx, uint32_t* out) {
    std::vector<size_t> v(idx, idx + n_idx);
    TcsProof p = merkle_prove_openings(*static_cast<MerkleTree*>(t), v);
    memcpy(out, p.paths.data(), p.paths.size() * 32);
}
int orc_merkle_verify(const uint32_t* commit8, const uint64_t* idx, size_t n_idx, const uint32_t* values, size_t width,
                      size_t log_height, const uint32_t* root8, const uint32_t* paths) {
    TcsProof p;
    p.merkle_root = load_d(root8);
    p.log_tensor_height = log_height;
    p.width = width;
    p.paths.resize(n_idx * log_height);
    memcpy(p.paths.data(), paths, p.paths.size() * 32);
    std::vector<size_t> v(idx, idx + n_idx);
    return (int)merkle_verify(load_d(commit8), v, FP(values), width, width, log_height, p);
}

// ---- BaseFold -------------------------------------------------------------------------------
struct PdHandle { std::shared_ptr<BasefoldProverData> pd; };

void* orc_commit_mles(const uint32_t** mles, const int* widths, int n, int log_n, int log_blowup, uint32_t* commit8) {
    std::vector<MleRef> ms;
    for (int i = 0; i < n; i++) ms.push_back({FP(mles[i]), log_n, widths[i]});
    FriConfig cfg;
    cfg.log_blowup = log_blowup;
    PdHandle* h = new PdHandle{commit_mles(ms, cfg)};
    memcpy(commit8, &h->pd->tree.commit, 32);
    return h;
}
void orc_pd_free(void* h) { delete static_cast<PdHandle*>(h); }
void orc_pd_codeword(void* h, int k, uint32_t* out) {
    auto& cw = static_cast<PdHandle*>(h)->pd->codewords[k];
    memcpy(out, cw.data(), cw.size() * 4);
}
void orc_pd_layers(void* h, uint32_t* out) { orc_merkle_layers(&static_cast<PdHandle*>(h)->pd->tree, out); }

// mles / widths / pds are flattened over rounds; mles_per_round[r] gives the split.
// claims: one ext per column, flattened round -> mle -> column.
// returns the proof length; writes at most cap bytes (call with cap = 0 to size).
size_t orc_basefold_prove(const uint32_t* point, int dim, int n_rounds, const int* mles_per_round,
                          const uint32_t** mles, const int* widths, const uint32_t* claims, void** pds,
                          int log_blowup, int num_queries, int pow_bits, void* challenger, uint8_t* out, size_t cap) {
    std::vector<E> pt(dim);
    memcpy(pt.data(), point, (size_t)dim * 16);
    std::vector<std::vector<MleRef>> rounds;
    std::vector<std::vector<std::vector<E>>> cl;
    std::vector<std::shared_ptr<BasefoldProverData>> pdata;
    int k = 0;
    size_t co = 0;
    for (int r = 0; r < n_rounds; r++) {
        rounds.emplace_back();
        cl.emplace_back();
        for (int m = 0; m < mles_per_round[r]; m++, k++) {
            rounds.back().push_back({FP(mles[k]), dim, widths[k]});
            std::vector<E> ev(widths[k]);
            memcpy(ev.data(), claims + co * 4, ev.size() * 16);
            co += widths[k];
            cl.back().push_back(std::move(ev));
        }
        pdata.push_back(static_cast<PdHandle*>(pds[r])->pd);
    }
    FriConfig cfg{log_blowup, num_queries, pow_bits};
    BasefoldProof p = basefold_prove(pt, rounds, cl, pdata, cfg, *static_cast<Challenger*>(challenger));
    std::vector<uint8_t> b = serialize_proof(p);
    if (b.size() <= cap) memcpy(out, b.data(), b.size());
    return b.size();
}

// returns 0 on success, BfError code otherwise, -1 on malformed blob
int orc_basefold_verify(const uint32_t* commitments, int n_rounds, const uint32_t* point, int dim,
                        const uint32_t* claims, const int* claims_per_round, const uint8_t* blob, size_t len,
                        int log_blowup, int num_queries, int pow_bits, void* challenger) {
    try {
        BasefoldProof p = deserialize_proof(blob, len);
        std::vector<Digest> cs(n_rounds);
        memcpy(cs.data(), commitments, (size_t)n_rounds * 32);
        std::vector<E> pt(dim);
        memcpy(pt.data(), point, (size_t)dim * 16);
        std::vector<std::vector<E>> cl;
        size_t co = 0;
        for (int r = 0; r < n_rounds; r++) {
            std::vector<E> ev(claims_per_round[r]);
            memcpy(ev.data(), claims + co * 4, ev.size() * 16);
            co += ev.size();
            cl.push_back(std::move(ev));
        }
        FriConfig cfg{log_blowup, num_queries, pow_bits};
        return (int)basefold_verify(cs, pt, cl, p, cfg, *static_cast<Challenger*>(challenger));
    } catch (const std::exception& e) {
        return -1;
    }
}

// ---- stacked interleave + jagged wrapper ------------------------------------------------------
// returns number of batches; if out != NULL writes batches back-to-back (each [2^lsh][w_b] row-major)
// and their widths into out_widths.
size_t orc_interleave(const uint32_t** tables, const uint64_t* rows, const int* cols, int n, size_t batch_size,
                      int lsh, uint32_t* out, int* out_widths) {
    std::vector<TensorRef> ts;
    for (int i = 0; i < n; i++) ts.push_back({FP(tables[i]), (size_t)rows[i], cols[i]});
    auto bs = interleave_fixed_rate(batch_size, ts, lsh);
    if (out) {
        size_t o = 0;
        for (size_t i = 0; i < bs.size(); i++) {
            memcpy(out + o, bs[i].data.data(), bs[i].data.size() * 4);
            o += bs[i].data.size();
            out_widths[i] = bs[i].width;
        }
    }
    return bs.size();
}
void orc_jagged_commit_wrap(const uint32_t* commit8, const uint64_t* rows, const uint64_t* cols, int n,
                            uint64_t num_added_vals, int max_log_row_count, uint32_t* out8) {
    Digest d = jagged_commit_wrap(load_d(commit8), std::vector<size_t>(rows, rows + n),
                                  std::vector<size_t>(cols, cols + n), num_added_vals, max_log_row_count);
    memcpy(out8, &d, 32);
}

// ---- zerocheck ----------------------------------------------------------------------------------
static std::vector<ZcAir> make_airs(int n, const uint32_t** progs, const int* prog_lens, const int* main_w, const int* prep_w,
                                    const int* n_constraints) {
    std::vector<ZcAir> airs(n);
    for (int i = 0; i < n; i++) {
        airs[i].main_width = main_w[i];
        airs[i].prep_width = prep_w[i];
        airs[i].num_constraints = n_constraints[i];
        for (int k = 0; k < prog_lens[i]; k++) airs[i].prog.push_back({progs[i][3 * k], progs[i][3 * k + 1], progs[i][3 * k + 2]});
    }
    return airs;
}

// 1: orc_zerocheck_prove restates the prover that takes the first two rounds from one pass over the base tables (kb_zerocheck.hpp,
// zc_real_row_values_in_round1_node0): the same bytes on a satisfying trace, comparable with that prover on any other table
static int g_zc_two_round_form = 0;
void orc_set_zc_two_round_form(int on) { g_zc_two_round_form = on; }

// openings: per chip main evals then prep evals (ext), flattened. Returns blob size.
size_t orc_zerocheck_prove(int n_chips, const uint32_t** progs, const int* prog_lens, const int* main_w, const int* prep_w,
                           const int* n_constraints, const uint32_t** mains, const uint32_t** preps, const uint64_t* real_rows,
                           const uint32_t* openings, int max_log_row_count, const uint32_t* zeta, const uint32_t* alpha,
                           const uint32_t* gkr, const uint32_t* publics, int n_publics, void* challenger, uint8_t* out,
                           size_t cap) {
    std::vector<ZcAir> airs = make_airs(n_chips, progs, prog_lens, main_w, prep_w, n_constraints);
    std::vector<ZcChipInput> chips(n_chips);
    size_t o = 0;
    for (int i = 0; i < n_chips; i++) {
        chips[i].air = &airs[i];
        chips[i].main = FP(mains[i]);
        chips[i].prep = preps[i] ? FP(preps[i]) : nullptr;
        chips[i].real_rows = real_rows[i];
        for (int c = 0; c < main_w[i]; c++, o++) chips[i].main_opening.push_back(load_e(openings + 4 * o));
        for (int c = 0; c < prep_w[i]; c++, o++) chips[i].prep_opening.push_back(load_e(openings + 4 * o));
    }
    std::vector<E> z(max_log_row_count);
    memcpy(z.data(), zeta, (size_t)max_log_row_count * 16);
    std::vector<F> pv(n_publics);
    memcpy(pv.data(), publics, (size_t)n_publics * 4);
    ZcProof p = zerocheck_prove(chips, max_log_row_count, z, load_e(alpha), load_e(gkr), pv, *static_cast<Challenger*>(challenger),
                                g_zc_two_round_form != 0 && max_log_row_count >= 2);
    std::vector<uint8_t> b = serialize_zc_proof(p);
    if (b.size() <= cap) memcpy(out, b.data(), b.size());
    return b.size();
}

int orc_zerocheck_verify(int n_chips, const uint32_t** progs, const int* prog_lens, const int* main_w, const int* prep_w,
                         const int* n_constraints, const uint64_t* heights, const uint32_t* openings, int max_log_row_count,
                         const uint32_t* zeta, const uint32_t* alpha, const uint32_t* gkr, const uint32_t* publics,
                         int n_publics, const uint8_t* blob, size_t len, void* challenger) {
    try {
        std::vector<ZcAir> airs = make_airs(n_chips, progs, prog_lens, main_w, prep_w, n_constraints);
        std::vector<const ZcAir*> ap;
        std::vector<size_t> hs(heights, heights + n_chips);
        std::vector<std::vector<E>> mo(n_chips), po(n_chips);
        size_t o = 0;
        for (int i = 0; i < n_chips; i++) {
            ap.push_back(&airs[i]);
            for (int c = 0; c < main_w[i]; c++, o++) mo[i].push_back(load_e(openings + 4 * o));
            for (int c = 0; c < prep_w[i]; c++, o++) po[i].push_back(load_e(openings + 4 * o));
        }
        ByteReader r{blob, len};
        ZcProof p;
        size_t n = r.u64();
        if (n > len) return -1;
        for (size_t i = 0; i < n; i++) {
            size_t k = r.u64();
            if (k > len) return -1;
            UniPoly u(k);
            for (auto& c : u) c = r.e();
            p.univariate_polys.push_back(u);
        }
        p.claimed_sum = r.e();
        n = r.u64();
        if (n > len) return -1;
        p.point.resize(n);
        for (auto& x : p.point) x = r.e();
        p.eval = r.e();
        n = r.u64();
        if ((int)n != n_chips) return -1;
        for (size_t i = 0; i < n; i++) {
            size_t k = r.u64();
            if ((int)k != main_w[i] + prep_w[i]) return -1;
            std::vector<E> ev(k);
            for (auto& x : ev) x = r.e();
            p.chip_evals.push_back(ev);
        }
        if (r.o != len) return -1;
        std::vector<E> z(max_log_row_count);
        memcpy(z.data(), zeta, (size_t)max_log_row_count * 16);
        std::vector<F> pv(n_publics);
        memcpy(pv.data(), publics, (size_t)n_publics * 4);
        return zerocheck_verify(ap, hs, mo, po, max_log_row_count, z, load_e(alpha), load_e(gkr), pv, p,
                                *static_cast<Challenger*>(challenger));
    } catch (const std::exception&) {
        return -1;
    }
}

// round consistency of a PartialSumcheckProof given its own point (no transcript): used on the golden proof
int orc_sumcheck_rounds_consistent(const uint32_t* polys, int n_rounds, int n_coeffs, const uint32_t* claimed_sum,
                                   const uint32_t* point, const uint32_t* eval) {
    std::vector<UniPoly> us(n_rounds, UniPoly(n_coeffs));
    for (int r = 0; r < n_rounds; r++) memcpy(us[r].data(), polys + (size_t)r * n_coeffs * 4, (size_t)n_coeffs * 16);
    std::vector<E> pt(n_rounds);
    memcpy(pt.data(), point, (size_t)n_rounds * 16);
    if (uni_eval_one_plus_eval_zero(us[0]) != load_e(claimed_sum)) return 1;
    // proof.point = [alpha_last, ..., alpha_first]
    for (int r = 1; r < n_rounds; r++)
        if (uni_eval(us[r - 1], pt[n_rounds - r]) != uni_eval_one_plus_eval_zero(us[r])) return 2 + r;
    if (uni_eval(us[n_rounds - 1], pt[0]) != load_e(eval)) return 2;
    return 0;
}

// ---- jagged PCS evaluation proof ----------------------------------------------
struct JaggedRoundHandle { JaggedRoundData d; Digest commit; };

void* orc_jagged_commit(const uint32_t** tables, const uint64_t* rows, const int* cols, int n, int max_log_row_count,
                        int lsh, size_t batch_size, int log_blowup, uint32_t* commit8) {
    std::vector<TensorRef> ts;
    for (int i = 0; i < n; i++) ts.push_back({FP(tables[i]), (size_t)rows[i], cols[i]});
    FriConfig cfg;
    cfg.log_blowup = log_blowup;
    JaggedRoundHandle* h = new JaggedRoundHandle();
    h->commit = jagged_commit(ts, max_log_row_count, lsh, batch_size, cfg, &h->d);
    memcpy(commit8, &h->commit, 32);
    return h;
}
void orc_jagged_round_free(void* h) { delete static_cast<JaggedRoundHandle*>(h); }

static std::vector<std::vector<E>> split_claims(const uint32_t* claims, const int* per_round, int n_rounds) {
    std::vector<std::vector<E>> cl;
    size_t co = 0;
    for (int r = 0; r < n_rounds; r++) {
        std::vector<E> ev(per_round[r]);
        memcpy(ev.data(), claims + co * 4, ev.size() * 16);
        co += ev.size();
        cl.push_back(std::move(ev));
    }
    return cl;
}

size_t orc_jagged_prove(const uint32_t* z_row, int max_log_row_count, int n_rounds, void** rounds, const uint32_t* claims,
                        const int* claims_per_round, int lsh, int log_blowup, int num_queries, int pow_bits,
                        void* challenger, uint8_t* out, size_t cap) {
    std::vector<E> zr(max_log_row_count);
    memcpy(zr.data(), z_row, (size_t)max_log_row_count * 16);
    std::vector<JaggedRoundData> rd;
    for (int r = 0; r < n_rounds; r++) rd.push_back(static_cast<JaggedRoundHandle*>(rounds[r])->d);
    FriConfig cfg{log_blowup, num_queries, pow_bits};
    JaggedProof p = jagged_prove(zr, split_claims(claims, claims_per_round, n_rounds), rd, max_log_row_count, lsh, cfg,
                                 *static_cast<Challenger*>(challenger));
    std::vector<uint8_t> b = serialize_jagged_proof(p);
    if (b.size() <= cap) memcpy(out, b.data(), b.size());
    return b.size();
}

// 0 = accepted, > 0 = the restated verifier's error code, -1 = malformed blob
int orc_jagged_verify(const uint32_t* commitments, int n_rounds, const uint32_t* z_row, int max_log_row_count,
                      const uint32_t* claims, const int* claims_per_round, const uint8_t* blob, size_t len, int lsh,
                      int log_blowup, int num_queries, int pow_bits, void* challenger) {
    try {
        JaggedProof p = deserialize_jagged_proof(blob, len);
        std::vector<Digest> cs(n_rounds);
        memcpy(cs.data(), commitments, (size_t)n_rounds * 32);
        std::vector<E> zr(max_log_row_count);
        memcpy(zr.data(), z_row, (size_t)max_log_row_count * 16);
        FriConfig cfg{log_blowup, num_queries, pow_bits};
        return jagged_verify(cs, zr, split_claims(claims, claims_per_round, n_rounds), p, max_log_row_count, lsh, cfg,
                             *static_cast<Challenger*>(challenger));
    } catch (const std::exception&) {
        return -1;
    }
}

// pieces, for kernel-level parity tests
void orc_partial_jagged_table(const uint64_t* heights, size_t n_cols, int max_log_row_count, const uint32_t* z_row,
                              const uint32_t* z_col, int z_col_dim, uint32_t* out) {
    JaggedParams pp = JaggedParams::from_column_heights(std::vector<size_t>(heights, heights + n_cols), max_log_row_count);
    std::vector<E> zr(max_log_row_count), zc(z_col_dim);
    memcpy(zr.data(), z_row, zr.size() * 16);
    memcpy(zc.data(), z_col, zc.size() * 16);
    std::vector<E> t = partial_jagged_table(pp, zr, zc);
    memcpy(out, t.data(), t.size() * 16);
}
void orc_full_jagged_eval(const uint64_t* heights, size_t n_cols, const uint32_t* z_row, int z_row_dim, const uint32_t* z_col,
                          int z_col_dim, const uint32_t* z_index, int z_index_dim, uint32_t* out4) {
    JaggedParams pp = JaggedParams::from_column_heights(std::vector<size_t>(heights, heights + n_cols), z_row_dim);
    std::vector<E> zr(z_row_dim), zc(z_col_dim), zi(z_index_dim);
    memcpy(zr.data(), z_row, zr.size() * 16);
    memcpy(zc.data(), z_col, zc.size() * 16);
    memcpy(zi.data(), z_index, zi.size() * 16);
    E r = full_jagged_little_polynomial_evaluation(pp.prefix, zr, zc, zi);
    memcpy(out4, &r, 16);
}

// ---- LogUp-GKR -------------------------------------------------------------------
// Interaction program of one chip (uint32 words): [n_interactions, then per interaction: is_send, kind, n_values,
// vcol(multiplicity), vcol(value 0), ...]; vcol = [n_terms, constant (canonical), then n_terms x (is_main, column,
// weight (canonical))].
static VCol parse_vcol(const uint32_t*& p) {
    VCol v;
    const uint32_t nt = *p++;
    v.constant = F::from_canonical(*p++);
    for (uint32_t t = 0; t < nt; t++) { v.terms.push_back({(int)p[0], (int)p[1], F::from_canonical(p[2])}); p += 3; }
    return v;
}
static std::vector<GkrChip> make_gkr_chips(int n, const char** names, const uint32_t** progs, const int* main_w, const int* prep_w,
                                           const uint32_t** mains, const uint32_t** preps, const uint64_t* rows) {
    std::vector<GkrChip> chips(n);
    for (int k = 0; k < n; k++) {
        GkrChip& c = chips[k];
        c.name = names[k];
        c.main_width = main_w[k]; c.prep_width = prep_w[k];
        c.main = mains ? FP(mains[k]) : nullptr;
        c.prep = (preps && preps[k]) ? FP(preps[k]) : nullptr;
        c.real_rows = rows ? (size_t)rows[k] : 0;
        const uint32_t* p = progs[k];
        const uint32_t ni = *p++;
        for (uint32_t i = 0; i < ni; i++) {
            GkrInteraction in;
            in.is_send = *p++ != 0;
            in.kind = *p++;
            const uint32_t nv = *p++;
            in.multiplicity = parse_vcol(p);
            for (uint32_t j = 0; j < nv; j++) in.values.push_back(parse_vcol(p));
            c.interactions.push_back(std::move(in));
        }
    }
    return chips;
}

size_t orc_gkr_prove(int n_chips, const char** names, const uint32_t** progs, const int* main_w, const int* prep_w,
                     const uint32_t** mains, const uint32_t** preps, const uint64_t* rows, int L, void* challenger, uint8_t* out,
                     size_t cap) {
    std::vector<GkrChip> chips = make_gkr_chips(n_chips, names, progs, main_w, prep_w, mains, preps, rows);
    GkrProof p = g_gkr_sparse ? gkr_prove_sparse(chips, L, *static_cast<Challenger*>(challenger)) : gkr_prove(chips, L, *static_cast<Challenger*>(challenger));
    std::vector<uint8_t> b = serialize_gkr_proof(p);
    if (b.size() <= cap) memcpy(out, b.data(), b.size());
    return b.size();
}

// A machine's eval_public_values (kb_gkr.hpp PvProgram) from the two program encodings of sp1_amd/air.py: `zc_prog` [zc_len][3]
// (PUBLIC / CONST loads only), `gkr_prog` = one InteractionProgram whose main columns are the public words. Null zc_prog = none.
static bool make_pv_program(const uint32_t* zc_prog, int zc_len, int n_constraints, const uint32_t* gkr_prog, int num_pv_elts,
                            int proof_max_num_pvs, int max_kind_arity, PvProgram* out) {
    if (!zc_prog) return false;
    const int zero = 0;
    const uint32_t* zp[1] = {zc_prog};
    out->air = make_airs(1, zp, &zc_len, &zero, &zero, &n_constraints)[0];
    for (auto& in : out->air.prog) {
        if (in.op == ZC_LOAD_MAIN || in.op == ZC_LOAD_PREP) throw std::runtime_error("public-values constraints read a trace column");
        if (in.op == ZC_PUBLIC && in.a >= (uint32_t)num_pv_elts) throw std::runtime_error("public value index out of range");
    }
    const char* name = "PublicValues";
    const uint32_t* gp[1] = {gkr_prog};
    out->interactions = make_gkr_chips(1, &name, gp, &num_pv_elts, &zero, nullptr, nullptr, nullptr)[0].interactions;
    for (auto& in : out->interactions) {
        std::vector<const VCol*> cols{&in.multiplicity};
        for (auto& v : in.values) cols.push_back(&v);
        for (const VCol* v : cols)
            for (auto& t : v->terms)
                if (!std::get<0>(t) || std::get<1>(t) < 0 || std::get<1>(t) >= num_pv_elts) throw std::runtime_error("public-values interaction column out of range");
    }
    out->num_pv_elts = num_pv_elts; out->proof_max_num_pvs = proof_max_num_pvs; out->max_kind_arity = (size_t)max_kind_arity;
    return true;
}

// 0 = accepted; > 0 = error code of the restated verifier; -1 = malformed blob. With check_interactions == 0 the
// chips are ignored (n_chips may be 0) and beta_seed_dim must be given. pv_*: the machine's eval_public_values and the shard's
// public values (Montgomery words); pv_zc_prog == null = a machine without one.
int orc_gkr_verify_pv(int n_chips, const char** names, const uint32_t** progs, const int* main_w, const int* prep_w,
                      const uint64_t* heights, int L, const uint8_t* blob, size_t len, int check_interactions, int beta_seed_dim,
                      void* challenger, const uint32_t* pv_zc_prog, int pv_zc_len, int pv_n_constraints, const uint32_t* pv_gkr_prog,
                      int num_pv_elts, int max_kind_arity, const uint32_t* publics, int n_publics) {
    try {
        GkrProof p = deserialize_gkr_proof(blob, len);
        std::vector<GkrChip> chips;
        std::vector<size_t> hs;
        if (check_interactions) {
            chips = make_gkr_chips(n_chips, names, progs, main_w, prep_w, nullptr, nullptr, nullptr);
            hs.assign(heights, heights + n_chips);
        }
        PvProgram pvp;
        const bool has_pv = make_pv_program(pv_zc_prog, pv_zc_len, pv_n_constraints, pv_gkr_prog, num_pv_elts, 0, max_kind_arity, &pvp);
        std::vector<F> pv(has_pv ? n_publics : 0);
        if (has_pv) {
            if (n_publics < num_pv_elts) return 9;
            memcpy(pv.data(), publics, (size_t)n_publics * 4);
        }
        return gkr_verify(chips, hs, L, p, check_interactions != 0, check_interactions ? -1 : beta_seed_dim,
                          *static_cast<Challenger*>(challenger), has_pv ? &pvp : nullptr, has_pv ? &pv : nullptr);
    } catch (const std::exception&) {
        return -1;
    }
}
int orc_gkr_verify(int n_chips, const char** names, const uint32_t** progs, const int* main_w, const int* prep_w,
                   const uint64_t* heights, int L, const uint8_t* blob, size_t len, int check_interactions, int beta_seed_dim,
                   void* challenger) {
    return orc_gkr_verify_pv(n_chips, names, progs, main_w, prep_w, heights, L, blob, len, check_interactions, beta_seed_dim, challenger,
                             nullptr, 0, 0, nullptr, 0, 1, nullptr, 0);
}

// ---- whole shard proof ------------------------------------------------------------------------------------
static std::vector<ShardChip> make_shard_chips(int n, const char** names, const uint32_t** zc_progs, const int* zc_lens,
                                               const int* main_w, const int* prep_w, const int* n_constraints,
                                               const uint32_t** gkr_progs, const uint32_t** mains, const uint32_t** preps,
                                               const uint64_t* rows) {
    std::vector<ShardChip> chips(n);
    if (n == 0) return chips;
    std::vector<ZcAir> airs = make_airs(n, zc_progs, zc_lens, main_w, prep_w, n_constraints);
    std::vector<GkrChip> g = make_gkr_chips(n, names, gkr_progs, main_w, prep_w, mains, preps, rows);
    for (int k = 0; k < n; k++) {
        chips[k].name = names[k];
        chips[k].air = airs[k];
        chips[k].interactions = g[k].interactions;
        chips[k].main = g[k].main; chips[k].prep = g[k].prep; chips[k].real_rows = g[k].real_rows;
    }
    return chips;
}

size_t orc_shard_prove(int n, const char** names, const uint32_t** zc_progs, const int* zc_lens, const int* main_w, const int* prep_w,
                       const int* n_constraints, const uint32_t** gkr_progs, const uint32_t** mains, const uint32_t** preps,
                       const uint64_t* rows, const uint32_t* publics, int n_publics, void* prep_round, int L, int lsh,
                       size_t batch, int log_blowup, int num_queries, int pow_bits, void* challenger, uint8_t* out, size_t cap) {
    std::vector<ShardChip> chips = make_shard_chips(n, names, zc_progs, zc_lens, main_w, prep_w, n_constraints, gkr_progs, mains, preps, rows);
    std::vector<F> pv(n_publics);
    memcpy(pv.data(), publics, (size_t)n_publics * 4);
    ShardParams sp{L, lsh, batch, FriConfig{log_blowup, num_queries, pow_bits}};
    ShardProof p = shard_prove(chips, pv, static_cast<JaggedRoundHandle*>(prep_round)->d, sp, *static_cast<Challenger*>(challenger));
    std::vector<uint8_t> b = serialize_shard_proof(p);
    if (b.size() <= cap) memcpy(out, b.data(), b.size());
    return b.size();
}

// CPU-baseline aids: choose the LogUp-GKR formulation of orc_shard_prove / orc_gkr_prove and read the stage times of the
// calling thread's last orc_shard_prove (commit, LogUp-GKR, zerocheck, jagged evaluation proof)
void orc_set_gkr_sparse(int on) { g_gkr_sparse = on; }
// OpenMP threads of this process's oracle (tests with several oracle processes on one box: the environment variable is read
// when the OpenMP runtime loads, which torch's import has usually done already)
void orc_set_threads(int n) { if (n > 0) omp_set_num_threads(n); }
void orc_stage_seconds(double* out4) { for (int k = 0; k < 4; k++) out4[k] = g_stage_seconds[k]; }

// with_chips == 0: n may be 0; everything chip-independent is checked (the reference's real proof).
// pv_*: the machine's eval_public_values (make_pv_program); pv_zc_prog == null = a machine without one.
int orc_shard_verify_pv(int n, const char** names, const uint32_t** zc_progs, const int* zc_lens, const int* main_w, const int* prep_w,
                        const int* n_constraints, const uint32_t** gkr_progs, const uint32_t* prep_commit8, const uint8_t* blob,
                        size_t len, int L, int lsh, int log_blowup, int num_queries, int pow_bits, int with_chips, int beta_seed_dim,
                        void* challenger, const uint32_t* pv_zc_prog, int pv_zc_len, int pv_n_constraints, const uint32_t* pv_gkr_prog,
                        int num_pv_elts, int proof_max_num_pvs, int max_kind_arity) {
    try {
        ShardProof p = deserialize_shard_proof(blob, len);
        std::vector<ShardChip> chips;
        if (with_chips) chips = make_shard_chips(n, names, zc_progs, zc_lens, main_w, prep_w, n_constraints, gkr_progs, nullptr, nullptr, nullptr);
        ShardParams sp{L, lsh, 0, FriConfig{log_blowup, num_queries, pow_bits}};
        PvProgram pvp;
        const bool has_pv = make_pv_program(pv_zc_prog, pv_zc_len, pv_n_constraints, pv_gkr_prog, num_pv_elts, proof_max_num_pvs, max_kind_arity, &pvp);
        if (has_pv && p.public_values.size() < (size_t)num_pv_elts) return 4;
        return shard_verify(chips, load_d(prep_commit8), p, sp, with_chips != 0, beta_seed_dim, *static_cast<Challenger*>(challenger),
                            has_pv ? &pvp : nullptr);
    } catch (const std::exception&) {
        return -1;
    }
}
int orc_shard_verify(int n, const char** names, const uint32_t** zc_progs, const int* zc_lens, const int* main_w, const int* prep_w,
                     const int* n_constraints, const uint32_t** gkr_progs, const uint32_t* prep_commit8, const uint8_t* blob,
                     size_t len, int L, int lsh, int log_blowup, int num_queries, int pow_bits, int with_chips, int beta_seed_dim,
                     void* challenger) {
    return orc_shard_verify_pv(n, names, zc_progs, zc_lens, main_w, prep_w, n_constraints, gkr_progs, prep_commit8, blob, len, L, lsh,
                               log_blowup, num_queries, pow_bits, with_chips, beta_seed_dim, challenger, nullptr, 0, 0, nullptr, 0, 0, 1);
}

// ---- BabyBear commit path (bb_commit.hpp): mles [n][w_k] row-major Montgomery words (R = 2^32 mod the BabyBear prime)
// -> codewords (optional), the Merkle tree leaf-first (optional), commitment[8]
void orc_bb_commit_mles(const uint32_t* const* mles, const int* widths, int n_mles, int log_n, int log_blowup, uint32_t* commit,
                        uint32_t* const* codewords_out, uint32_t* tree_out) {
    const size_t N = (size_t)1 << (log_n + log_blowup);
    std::vector<std::vector<orcbb::F>> cw(n_mles);
    std::vector<const orcbb::F*> ptrs;
    std::vector<int> ws(widths, widths + n_mles);
    for (int k = 0; k < n_mles; k++) {
        cw[k].resize(N * (size_t)widths[k]);
        orcbb::rs_encode(reinterpret_cast<const orcbb::F*>(mles[k]), log_n, widths[k], log_blowup, cw[k].data());
        ptrs.push_back(cw[k].data());
        if (codewords_out && codewords_out[k]) memcpy(codewords_out[k], cw[k].data(), cw[k].size() * 4);
    }
    std::vector<orcbb::Digest> tree;
    orcbb::Digest c;
    orcbb::merkle_commit(ptrs, ws, N, &tree, &c);
    for (int i = 0; i < 8; i++) commit[i] = c.d[i].v;
    if (tree_out) memcpy(tree_out, tree.data(), tree.size() * sizeof(orcbb::Digest));
}
// tensors [h][w_k] row-major of any content (not codewords) -> tree[2 h - 1][8] leaf-first, commitment[8]
void orc_bb_merkle_commit(const uint32_t* const* tensors, const int* widths, int n_tensors, size_t h, uint32_t* tree_out, uint32_t* commit) {
    std::vector<const orcbb::F*> ptrs;
    for (int k = 0; k < n_tensors; k++) ptrs.push_back(reinterpret_cast<const orcbb::F*>(tensors[k]));
    std::vector<int> ws(widths, widths + n_tensors);
    std::vector<orcbb::Digest> tree;
    orcbb::Digest c;
    orcbb::merkle_commit(ptrs, ws, h, &tree, &c);
    for (int i = 0; i < 8; i++) commit[i] = c.d[i].v;
    memcpy(tree_out, tree.data(), tree.size() * sizeof(orcbb::Digest));
}
void orc_bb_rs_encode(const uint32_t* in, int log_n, int w, int log_blowup, uint32_t* out) {
    orcbb::rs_encode(reinterpret_cast<const orcbb::F*>(in), log_n, w, log_blowup, reinterpret_cast<orcbb::F*>(out));
}
void orc_bb_permute(uint32_t* states, size_t n) {
    for (size_t i = 0; i < n; i++) orcbb::permute(reinterpret_cast<orcbb::F*>(states + 16 * i));
}
uint32_t orc_bb_two_adic_generator(int bits) { return orcbb::two_adic_generator(bits).canonical(); }

}  // extern "C"
