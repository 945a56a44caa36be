// sp1_amd/csrc/zc_kernels.hpp — the device side of the zerocheck: the LDS register file, the bytecode interpreter
// (zc_round_kernel), the fused pieces (zc_macro_kernel), the bivariate first two rounds (zc_biv_*), the polynomial-identity
// kernels, the reductions, the table updates (zc_fix_kernel, zc_fix2_kernel) and the final gather. Included by zerocheck.hip
// only: the launches instantiate these templates, so kernels and launch sites share one translation unit. The instruction-word
// encoding the interpreter reads is in zc_device.hpp (the host compiler, zc_compile.cpp, writes it).
#pragma once
#include "device_ctx.hpp"
#include "round_sync.hpp"
#include "zc_device.hpp"
#include "zc_poseidon2.hpp"
#include "zc_keccak.hpp"
#include "zc_mul.hpp"
#include "zc_poly.hpp"

namespace sp1hip {

// ---- register file -------------------------------------------------------------------------------
// The program is wave-uniform, so register numbers are SGPR values. The file lives in LDS (the only tier since round 5: the
// VGPR-vector files of rounds 1-4 — s_set_gpr_idx triples per word — and the per-lane scratch files for programs with more
// than 64 live values — 4 to 16 KB of scratch per lane — are gone; a program whose register file does not fit the 160 KB of
// LDS even for one wave is cut into finer chunks by the planner, zc_wg_for / plan_round).
template <bool FIRST, int MAXR> struct RegFile;

// The file: register i of a lane at slot i * (workgroup width) + lane (16 B slots for extension values: one
// ds_read_b128 / ds_write_b128 per access, conflict-free). Indexing a VGPR vector with a wave-uniform index costs an
// s_set_gpr_idx_on / v_mov / s_set_gpr_idx_off triple per word — ~36 instructions of pure register traffic around a
// 12-instruction extension add; the LDS file makes an interpreted op cost its arithmetic plus three LDS accesses,
// and leaves the VGPRs to the arithmetic (measured per-op cost: add 75 -> ~20 instructions, multiply 147 -> ~100).
// The slot stride is the workgroup size: programs with many live values run in narrower workgroups (128 / 64 lanes) so
// that the file still fits the LDS budget (launch_round).
// (pointers carry the LDS address space explicitly: a generic pointer here turns every access into a FLAT instruction)
typedef uint32_t zc_lds_word_t __attribute__((address_space(3)));
typedef uint32_t zc_lds_quad_t __attribute__((ext_vector_type(4), address_space(3)));
typedef uint32_t zc_quad_t __attribute__((ext_vector_type(4)));
template <> struct RegFile<true, 0> {
    zc_lds_word_t* base;           // this lane's slot of register 0
    uint32_t stride;
    __device__ __forceinline__ uint32_t get(uint32_t i) const { return base[i * stride]; }
    __device__ __forceinline__ void set(uint32_t i, uint32_t v) { base[i * stride] = v; }
};
template <> struct RegFile<false, 0> {
    zc_lds_quad_t* base;
    uint32_t stride;
    __device__ __forceinline__ kb::Ext get(uint32_t i) const { const zc_quad_t v = base[i * stride]; return kb::Ext{{v.x, v.y, v.z, v.w}}; }
    __device__ __forceinline__ void set(uint32_t i, const kb::Ext& v) { zc_quad_t q = {v.c[0], v.c[1], v.c[2], v.c[3]}; base[i * stride] = q; }
};

typedef uint32_t zc_word_t __attribute__((ext_vector_type(4)));       // one instruction: op | flags, dst, a, b
typedef const zc_word_t __attribute__((address_space(4)))* zc_const_prog_t;

// ---- the first two rounds in one pass over the base-field traces ("bivariate", the reference's
// sp1-gpu/crates/sys/include/zerocheck/bivariate.cuh:L1-L118 restated for this interpreter) ---------------------------------
// Rows are taken four at a time (row 4 q + 2 X + Y: Y is the last variable, bound by round 0, X the one round 1 binds) and the
// constraint polynomial is summed on the grid {0, 1, 2, 4}^2 minus its four boolean corners (constraints vanish on real rows,
// and a padded row's value cancels against the geq correction): per node e the kernels leave
//     A_e = sum_q eq(q) C(T_q(X_e, Y_e)),      T_q(X, Y) = r00 + X (r10 - r00) + Y (r01 - r00) + X Y (r11 - r10 - r01 + r00)
// with eq over the nv - 2 variables of the quad index, and the four corner sums B of the (linear) GKR batching term; the host
// assembles BOTH round messages from them (zerocheck.hip: run_bivariate_rounds): round 0 needs H(X, t) for X in {0, 1}, t in {0, 2, 4}, round 1
// the cubic through H(t, 0), H(t, 1), H(t, 2), H(t, 4) at the first challenge. Everything is base-field arithmetic — round 1's
// extension-field pass over the once-folded tables (the most expensive round of the sequential form) and one of the two table
// updates disappear. Node order (X, Y): (0,2) (0,4) (1,2) (1,4) (2,0) (2,1) (2,2) (2,4) (4,0) (4,1) (4,2) (4,4).
constexpr int ZC_BIV_NODES = 12;
struct ZcBivNode { uint32_t cx, cy, cxy; };
__host__ __device__ __forceinline__ ZcBivNode zc_biv_node(uint32_t e) {       // wave-uniform e: the fields stay in SGPRs
    constexpr uint32_t XS[12] = {0, 0, 1, 1, 2, 2, 2, 2, 4, 4, 4, 4}, YS[12] = {2, 4, 2, 4, 0, 1, 2, 4, 0, 1, 2, 4};
    return ZcBivNode{XS[e], YS[e], XS[e] * YS[e]};
}
// v < 2^36 -> v mod p, reduced: with v = t 2^31 + lo, v - t p = lo + t (2^24 - 1) < 2 p
__host__ __device__ __forceinline__ uint32_t zc_reduce36(uint64_t v) {
    const uint32_t t = (uint32_t)(v >> 31), lo = (uint32_t)v & 0x7fffffffu;
    const uint32_t r = lo + t * 0xffffffu;
    return kb::umin(r, r - kb::P);
}
__host__ __device__ __forceinline__ uint32_t zc_biv_interp(uint32_t r00, uint32_t r01, uint32_t r10, uint32_t r11, const ZcBivNode& nd) {
    const uint32_t dy = kb::sub(r01, r00), dx = kb::sub(r10, r00), dxy = kb::sub(kb::sub(r11, r10), dy);
    return zc_reduce36((uint64_t)r00 + (uint64_t)nd.cx * dx + (uint64_t)nd.cy * dy + (uint64_t)nd.cxy * dxy);   // <= (1 + 4 + 4 + 16) p
}
// column `col` of the quad q at node nd (rows past the table's height are zero: the virtual padding)
__device__ __forceinline__ uint32_t zc_biv_leaf(const uint32_t* tbl, uint32_t col, uint32_t rows, uint32_t q, const ZcBivNode& nd) {
    const zc_global_words_t g = (zc_global_words_t)tbl + (size_t)col * rows;
    const uint32_t r = 4 * q;
    const uint32_t r00 = g[r], r01 = r + 1 < rows ? g[r + 1] : 0u, r10 = r + 2 < rows ? g[r + 2] : 0u, r11 = r + 3 < rows ? g[r + 3] : 0u;
    return zc_biv_interp(r00, r01, r10, r11, nd);
}

// Four nodes per pass: the interpreter's cost per base-field operation is mostly decode and register-file traffic, so one pass
// of the program carries the values of FOUR grid nodes (nodes 4 g .. 4 g + 3) in an Ext-shaped container — the instruction is
// decoded once, the register file is the extension rounds' (16-byte slots), the arithmetic is element-wise.
struct KT4 {
    using T = kb::Ext;
    static __device__ __forceinline__ T zero() { return kb::ext_zero(); }
    static __device__ __forceinline__ T from_f(uint32_t x) { return kb::Ext{{x, x, x, x}}; }
    static __device__ __forceinline__ T add(const T& a, const T& b) { return kb::ext_add(a, b); }
    static __device__ __forceinline__ T sub(const T& a, const T& b) { return kb::ext_sub(a, b); }
    static __device__ __forceinline__ T mul(const T& a, const T& b) {
        return kb::Ext{{kb::mul(a.c[0], b.c[0]), kb::mul(a.c[1], b.c[1]), kb::mul(a.c[2], b.c[2]), kb::mul(a.c[3], b.c[3])}};
    }
};
struct KC4 {
    static __device__ __forceinline__ kb::Ext addc(const kb::Ext& a, uint32_t c) { return kb::Ext{{kb::add(a.c[0], c), kb::add(a.c[1], c), kb::add(a.c[2], c), kb::add(a.c[3], c)}}; }
    static __device__ __forceinline__ kb::Ext subc(const kb::Ext& a, uint32_t c) { return kb::Ext{{kb::sub(a.c[0], c), kb::sub(a.c[1], c), kb::sub(a.c[2], c), kb::sub(a.c[3], c)}}; }
    static __device__ __forceinline__ kb::Ext csub(uint32_t c, const kb::Ext& a) { return kb::Ext{{kb::sub(c, a.c[0]), kb::sub(c, a.c[1]), kb::sub(c, a.c[2]), kb::sub(c, a.c[3])}}; }
    static __device__ __forceinline__ kb::Ext mulc(const kb::Ext& a, uint32_t c) { return kb::ext_mul_base(a, c); }
};
// column `col` of the quad q at the four nodes of group g: the rows are loaded once
__device__ __forceinline__ kb::Ext zc_biv_leaf4(const uint32_t* tbl, uint32_t col, uint32_t rows, uint32_t q, uint32_t grp) {
    const zc_global_words_t g = (zc_global_words_t)tbl + (size_t)col * rows;
    const uint32_t r = 4 * q;
    const uint32_t r00 = g[r], r01 = r + 1 < rows ? g[r + 1] : 0u, r10 = r + 2 < rows ? g[r + 2] : 0u, r11 = r + 3 < rows ? g[r + 3] : 0u;
    const uint32_t dy = kb::sub(r01, r00), dx = kb::sub(r10, r00), dxy = kb::sub(kb::sub(r11, r10), dy);
    kb::Ext out;
#pragma unroll
    for (uint32_t n = 0; n < 4; n++) {
        const ZcBivNode nd = zc_biv_node(4 * grp + n);
        out.c[n] = zc_reduce36((uint64_t)r00 + (uint64_t)nd.cx * dx + (uint64_t)nd.cy * dy + (uint64_t)nd.cxy * dxy);
    }
    return out;
}

// One pass of the program at node t. With `gkr`, the first load of every column also accumulates
// gkr_pow[column] * value into *g (main columns first, then preprocessed): the batching term costs no
// extra loads. `prog` points to LDS (or global memory for very long programs).
// BIV: i is a quad index and t a node GROUP of the bivariate grid (nodes 4 t .. 4 t + 3, KT4: four base-field values per
// register, the extension rounds' register file); the four constraint sums are ADDED to g[0..4), no GKR term here.
template <bool FIRST, int MAXR, bool BIV = false, typename PROG>
__device__ __forceinline__ kb::Ext run_program(RegFile<(BIV ? false : FIRST), MAXR>& reg, PROG prog, const ZcDesc& d,
                                               const uint32_t* __restrict__ publics, uint32_t i, int t, const bool gkr, kb::Ext* g) {
    using K = typename std::conditional<BIV, KT4, KT<FIRST>>::type;
    using KCc = typename std::conditional<BIV, KC4, KC<FIRST>>::type;
    using T = typename K::T;
    kb::Ext acc = kb::ext_zero();
    T prev = K::zero();                   // the value the last value-producing instruction produced (operand forwarding)
    auto next = prog[0];                  // instruction words are fetched one instruction ahead of their use
    for (uint32_t k = 0; k < d.n_instr; k++) {
        const auto w = next;              // wave-uniform: decode once, keep the fields in SGPRs
        if (k + 1 < d.n_instr) next = prog[k + 1];
        const uint32_t opw = __builtin_amdgcn_readfirstlane(w.x), dst = __builtin_amdgcn_readfirstlane(w.y);
        const uint32_t x = __builtin_amdgcn_readfirstlane(w.z), y = __builtin_amdgcn_readfirstlane(w.w);
        const uint32_t op = opw & 0xffu;
        if (op <= ZC_LOAD_PREP) {         // 1..4 consecutive columns: every global load is in flight before the first use
            const uint32_t cnt = ((opw >> 16) & 3u) + 1;
            const uint32_t* tbl = op == ZC_LOAD_MAIN ? d.main : d.prep;
            const uint32_t gbase = op == ZC_LOAD_MAIN ? 0u : d.main_w;
            if constexpr (BIV) {
                T v[4];
#pragma unroll
                for (uint32_t j = 0; j < 4; j++)
                    if (j < cnt) v[j] = zc_biv_leaf4(tbl, x + j, d.rows, i, (uint32_t)t);
#pragma unroll
                for (uint32_t j = 0; j < 4; j++)
                    if (j < cnt) {
                        if (!(opw & ZC_DST_TEMP)) reg.set(dst + j, v[j]);
                        prev = v[j];
                    }
                continue;
            } else {
            T r0[4], r1[4];
            const bool odd = 2 * i + 1 < d.rows;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++)
                if (j < cnt) {
                    r0[j] = K::load(tbl, x + j, d.rows, 2 * i);
                    r1[j] = (t != 0 && odd) ? K::load(tbl, x + j, d.rows, 2 * i + 1) : K::zero();
                }
#pragma unroll
            for (uint32_t j = 0; j < 4; j++)
                if (j < cnt) {
                    T v = r0[j];
                    if (t != 0) {
                        const T s2 = K::add(K::sub(r1[j], r0[j]), K::sub(r1[j], r0[j]));
                        v = t == 2 ? K::add(s2, r0[j]) : K::add(K::add(s2, s2), r0[j]);
                    }
                    if (gkr && (opw & (ZC_GKR_FLAG << j))) *g = kb::ext_add(*g, K::scale(load_ext_aos(d.gkr_pows, gbase + x + j), v));
                    if (!(opw & ZC_DST_TEMP)) reg.set(dst + j, v);
                    prev = v;
                }
            continue;
            }
        }
        if (op == ZC_TOUCH) {
            if constexpr (!BIV) {
                if (gkr) {
                    T v = leaf<FIRST>(y ? d.prep : d.main, x, d.rows, i, t);
                    *g = kb::ext_add(*g, K::scale(load_ext_aos(d.gkr_pows, (y ? d.main_w : 0u) + x), v));
                }
            }
            continue;
        }
        if (op == ZC_ASSERT_ZERO) {                                   // y: the constraint's index; `prev` stays what it was
            const T a = (opw & ZC_A_PREV) ? prev : reg.get(x);
            if constexpr (BIV) {
                const kb::Ext pw = load_ext_aos(d.alpha_pows, y);
#pragma unroll
                for (int n = 0; n < 4; n++) g[n] = kb::ext_add(g[n], kb::ext_mul_base(pw, a.c[n]));
            } else {
                acc = kb::ext_add(acc, K::scale(load_ext_aos(d.alpha_pows, y), a));
            }
            continue;
        }
        // The forwarded value `prev` is dead once this instruction has read it, so the A operand is loaded INTO it when it
        // is not the forwarded value itself: no operand copies at the merge of the "forwarded" and "register file" paths
        // (they were 8 v_mov per extension-field instruction). The host puts the forwarded operand of a binary
        // instruction first (ADD / MUL commute, SUB becomes RSUB); ZC_B_PREV then means "b is the same value as a".
        T res;
        if (op == ZC_MADC) {
            if (opw & ZC_B_PREV) {                                    // the running sum is the forwarded value
                const T term = (opw & ZC_A_PREV) ? prev : reg.get(x);
                res = K::add(prev, KCc::mulc(term, y));
            } else {
                const T accv = reg.get(dst >> 16);
                if (!(opw & ZC_A_PREV)) prev = reg.get(x);
                res = K::add(accv, KCc::mulc(prev, y));
            }
        } else if (op == ZC_MAD || op == ZC_MSB) {
            T accv;
            if (opw & ZC_B_PREV) {                                    // the running sum is the forwarded value
                accv = prev;
                prev = reg.get(x);
            } else {
                accv = reg.get(dst >> 16);
                if (!(opw & ZC_A_PREV)) prev = reg.get(x);
            }
            const T m = K::mul(prev, reg.get(y));
            res = op == ZC_MAD ? K::add(accv, m) : K::sub(accv, m);
        } else if (op == ZC_CONST) {
            res = K::from_f(x);                                       // host pre-converts to Montgomery
        } else if (op == ZC_PUBLIC) {
            res = K::from_f(publics[x]);
        } else {
            if (!(opw & ZC_A_PREV)) prev = reg.get(x);
            switch (op) {
                case ZC_ADD: res = K::add(prev, (opw & ZC_B_PREV) ? prev : reg.get(y)); break;
                case ZC_SUB: res = K::sub(prev, (opw & ZC_B_PREV) ? prev : reg.get(y)); break;
                case ZC_RSUB: res = K::sub(reg.get(y), prev); break;
                case ZC_MUL: res = K::mul(prev, (opw & ZC_B_PREV) ? prev : reg.get(y)); break;
                case ZC_NEG: res = K::sub(K::zero(), prev); break;
                case ZC_ADDC: res = KCc::addc(prev, y); break;
                case ZC_SUBC: res = KCc::subc(prev, y); break;
                case ZC_CSUB: res = KCc::csub(y, prev); break;
                default: res = KCc::mulc(prev, y); break;      // ZC_MULC
            }
        }
        prev = res;
        if (!(opw & ZC_DST_TEMP)) reg.set(dst & 0xffffu, res);
    }
    return acc;
}

// last descriptor whose block_start <= bid (binary search; everything stays wave-uniform)
__device__ __forceinline__ ZcDesc zc_find_desc(const ZcDesc* __restrict__ descs, int n, uint32_t bid) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (__builtin_amdgcn_readfirstlane(descs[mid].block_start) <= bid) lo = mid; else hi = mid - 1;
    }
    return descs[lo];
}

// the sums of one range from its partials -> (y0, y2, y4, eq[th]); all threads of the workgroup call this, the results are
// valid in threads 0..3 (word k of each extension element)
template <bool FIRST>
__device__ __forceinline__ void zc_reduce_range(const ZcChipRange& d, const uint32_t* __restrict__ partial, const uint32_t* __restrict__ eq,
                                                uint32_t eq_len, uint32_t (&acc)[10][24], uint32_t& y0, uint32_t& y2, uint32_t& y4, uint32_t& e) {
    const uint32_t word = threadIdx.x % 24, grp = threadIdx.x / 24, n_grp = min(blockDim.x / 24u, 10u);
    auto ld = [&](const uint32_t* q) -> uint32_t { return *q; };
    if (grp < n_grp) {
        // eight independent partial sums: the loads of a lane are then eight deep in flight instead of one behind each add
        // (a tall chip has thousands of blocks: the plain loop was 100-130 us in each of the first three rounds)
        const uint32_t* p = partial + (size_t)d.block_start * 24 + word;
        uint32_t a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint32_t b = grp;
        for (; b + 7 * n_grp < d.n_blocks; b += 8 * n_grp)
#pragma unroll
            for (int u = 0; u < 8; u++) a[u] = kb::add(a[u], ld(p + (size_t)(b + n_grp * u) * 24));
        for (; b < d.n_blocks; b += n_grp) a[0] = kb::add(a[0], ld(p + (size_t)b * 24));
        acc[grp][word] = kb::add(kb::add(kb::add(a[0], a[1]), kb::add(a[2], a[3])), kb::add(kb::add(a[4], a[5]), kb::add(a[6], a[7])));
    }
    __syncthreads();
    if (threadIdx.x < 24) {
        uint32_t a = 0;
        for (uint32_t g = 0; g < n_grp; g++) a = kb::add(a, acc[g][threadIdx.x]);
        acc[0][threadIdx.x] = a;
    }
    __syncthreads();
    y0 = y2 = y4 = e = 0;
    if (threadIdx.x < 4) {
        const uint32_t k = threadIdx.x;
        // S[p][0..4) = A of pass p, S[p][4..8) = B of pass p
        const uint32_t A0 = acc[0][k], B0 = acc[0][4 + k], A1 = acc[0][8 + k], B1 = acc[0][12 + k], A2 = acc[0][16 + k];
        if (FIRST) {       // g0 = A0, g2 = B0, C(2) = A1, C(4) = A2
            y0 = A0;
            y2 = kb::add(A1, B0);
            y4 = kb::add(A2, kb::sub(kb::add(B0, B0), A0));
        } else {           // C(0) = A0, g0 = B0, C(2) = A1, g2 = B1, C(4) = A2
            y0 = kb::add(A0, B0);
            y2 = kb::add(A1, B1);
            y4 = kb::add(A2, kb::sub(kb::add(B1, B1), B0));
        }
        e = d.th < eq_len ? eq[(size_t)k * eq_len + d.th] : 0u;
    }
}
// payload words [1 + 16 range ..) of the host slot: system-scope stores from threads 0..3
__device__ __forceinline__ void zc_store_host_sums(volatile uint32_t* host_slot, uint32_t range, uint32_t y0, uint32_t y2, uint32_t y4, uint32_t e) {
    if (threadIdx.x < 4) {
        const uint32_t k = threadIdx.x;
        uint32_t* h = const_cast<uint32_t*>(host_slot) + 1 + (size_t)range * 16;
        __hip_atomic_store(h + k, y0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(h + 4 + k, y2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(h + 8 + k, y4, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(h + 12 + k, e, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// One launch per sumcheck round covers EVERY chip and the three interpolation nodes:
//   blockIdx.x = 3 b + p -> (chip, block b of 256 row pairs), pass p (node t = 2p).
// A pass-p workgroup writes two extension partial sums [A | B] (8 words):
//   round 0 :  p=0: A = sum eq g(0), B = sum eq g(2)   (GKR batching term only; constraints vanish at 0)
//              p=1: A = sum eq C(2)                     p=2: A = sum eq C(4)
//   later   :  p=0: A = sum eq C(0), B = sum eq g(0)    p=1: A = sum eq C(2), B = sum eq g(2)    p=2: A = sum eq C(4)
// g(4) = 2 g(2) - g(0) is linear, so the three nodes can run in different workgroups and the late, tiny
// rounds (latency-bound: one wave interprets the whole program serially) run all chips and nodes at once.
// STAGED: the program is copied to LDS once per workgroup (short chunked programs); otherwise every wave streams it
// from global memory through the scalar cache (constant address space: wave-uniform s_load_dwordx4), which leaves the
// whole LDS budget to the register file — the form used for a chip's undivided program in the large rounds.

template <bool FIRST, int MAXR, bool STAGED>
__global__ __launch_bounds__(256) void zc_round_kernel(const ZcDesc* __restrict__ descs, int n_descs,
                                                       const uint32_t* __restrict__ eq, uint32_t eq_len,
                                                       const uint32_t* __restrict__ publics, uint32_t* __restrict__ partial,
                                                       uint32_t rf_off, uint32_t block_base) {
    using K = KT<FIRST>;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* red = lds;                                   // [4][8] reduction scratch
    uint4* lprog = reinterpret_cast<uint4*>(lds + 32);
    RegFile<FIRST, MAXR> reg;
    if constexpr (MAXR == 0) {                             // LDS file behind the (staged) program
        reg.base = (decltype(reg.base))(lds + rf_off) + threadIdx.x;
        reg.stride = blockDim.x;
    }
    if (threadIdx.x < 32) red[threadIdx.x] = 0;            // workgroups narrower than 4 waves leave slots untouched
    // The three nodes of a block of row pairs are three CONSECUTIVE workgroups: dispatched together (to different XCDs),
    // their re-reads of the same table rows meet in the memory-side cache instead of HBM (one workgroup evaluating
    // all three nodes was measured slower, see the host side).
    const uint32_t bid = block_base + blockIdx.x / 3u;
    const int only_pass = (int)(blockIdx.x % 3u);
    const ZcDesc d = zc_find_desc(descs, n_descs, bid);
    if constexpr (STAGED) {
        const uint4* src = reinterpret_cast<const uint4*>(d.prog);
        for (uint32_t k = threadIdx.x; k < d.n_instr; k += blockDim.x) lprog[k] = src[k];
    }
    __syncthreads();
    const uint32_t terms = (d.rows + 1) / 2;
    kb::Ext sa[3], sb[3];
#pragma unroll
    for (int p = 0; p < 3; p++) { sa[p] = kb::ext_zero(); sb[p] = kb::ext_zero(); }
    // a block is d.block_pairs row pairs (= the workgroup width of the chip's launch group: one pass of the program
    // per workgroup while the round is large; the partial-sum layout only knows blocks)
    for (uint32_t base = (bid - d.block_start) * d.block_pairs; base < terms; base += d.n_blocks * d.block_pairs)
    for (uint32_t i = base + threadIdx.x; i < min(base + d.block_pairs, terms); i += blockDim.x) {
        kb::Ext e;
#pragma unroll
        for (int k = 0; k < 4; k++) e.c[k] = eq[(size_t)k * eq_len + i];
#pragma unroll
        for (int pass = 0; pass < 3; pass++) {
            if (pass != only_pass) continue;
            kb::Ext va = kb::ext_zero(), vb = kb::ext_zero();
            if (FIRST && pass == 0) {
                if (d.flags & 1u)
                for (uint32_t c = 0; c < d.main_w; c++) {
                    const kb::Ext pw = load_ext_aos(d.gkr_pows, c);
                    va = kb::ext_add(va, K::scale(pw, leaf<FIRST>(d.main, c, d.rows, i, 0)));
                    vb = kb::ext_add(vb, K::scale(pw, leaf<FIRST>(d.main, c, d.rows, i, 2)));
                }
                if (d.flags & 1u)
                for (uint32_t c = 0; c < d.prep_w; c++) {
                    const kb::Ext pw = load_ext_aos(d.gkr_pows, d.main_w + c);
                    va = kb::ext_add(va, K::scale(pw, leaf<FIRST>(d.prep, c, d.rows, i, 0)));
                    vb = kb::ext_add(vb, K::scale(pw, leaf<FIRST>(d.prep, c, d.rows, i, 2)));
                }
            } else if constexpr (STAGED) {
                va = run_program<FIRST, MAXR>(reg, (const zc_word_t*)lprog, d, publics, i, 2 * pass, !FIRST && pass < 2, &vb);
            } else {
                va = run_program<FIRST, MAXR>(reg, (zc_const_prog_t)(uintptr_t)d.prog, d, publics, i, 2 * pass, !FIRST && pass < 2, &vb);
            }
            sa[pass] = kb::ext_add(sa[pass], kb::ext_mul(va, e));
            sb[pass] = kb::ext_add(sb[pass], kb::ext_mul(vb, e));
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int pass = 0; pass < 3; pass++) {
        if (pass != only_pass) continue;
        uint32_t v[8];
#pragma unroll
        for (int k = 0; k < 4; k++) { v[k] = sa[pass].c[k]; v[4 + k] = sb[pass].c[k]; }
#pragma unroll
        for (int k = 0; k < 8; k++) v[k] = zc_wave_sum(v[k]);
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 8; k++) red[wave * 8 + k] = v[k];
        }
        __syncthreads();
        if (threadIdx.x < 8) {
            const uint32_t k = threadIdx.x;
            partial[((size_t)bid * 3 + pass) * 8 + k] = kb::add(kb::add(red[k], red[8 + k]), kb::add(red[16 + k], red[24 + k]));
        }
    }
}


// The fused Poseidon2 pieces (zc_poseidon2.hpp): one workgroup = 256 row pairs of one piece at one node, like the interpreter's
// workgroups and into the same partial-sum layout; descriptor flags bit 1 marks a macro piece, bits 8..11 its index q, `pad`
// its first main column. Every column of the permutation is loaded exactly once per piece; the loads a piece OWNS carry the
// GKR-opening batching term, so the interpreter's pieces never touch those columns for it (the planner pre-marks them).
constexpr uint32_t ZC_DESC_MACRO = 2u;
// KIND of a launch that carries the pieces of BOTH septic kinds (they are adjacent block ranges; the kind comes from the descriptor): in
// the small rounds every launch is at its latency floor and the two septic launches would share a hardware queue (a process has four)
constexpr uint32_t ZC_MACRO_BOTH_SEPTIC = 4u;
constexpr uint32_t ZC_MACRO_KINDS = 8;        // kinds 1..3, the launch shape 4, Keccak = 5, MulOperation products = 6, polynomial identities = 7
constexpr uint32_t ZC_POLY_WAVE_MAX_TERMS = 4096;    // row pairs of the tallest chip with polynomial identities below which a round runs them one wave per pair
constexpr uint32_t ZC_RANGE_CORNERS = ZC_MACRO_KINDS;   // (not a hint kind: the block range of zc_biv_corner_kernel in a bivariate plan)
template <bool FIRST, uint32_t KIND>
__global__ __launch_bounds__(256) void zc_macro_kernel(const ZcDesc* __restrict__ descs, int n_descs, const uint32_t* __restrict__ eq,
                                                       uint32_t eq_len, uint32_t* __restrict__ partial, uint32_t block_base,
                                                       const p2::RoundConstants* __restrict__ rc_p) {
    using K = KT<FIRST>;
    using F = typename std::conditional<FIRST, P2Base, P2Ext>::type;
    using T = typename K::T;
    __shared__ uint32_t red[32];
    if (threadIdx.x < 32) red[threadIdx.x] = 0;
    const uint32_t bid = block_base + blockIdx.x / 3u;
    const int pass = (int)(blockIdx.x % 3u), t = 2 * pass;
    const ZcDesc d = zc_find_desc(descs, n_descs, bid);
    const uint32_t q = (d.flags >> 8) & 15u, base_col = d.pad;       // (every descriptor of this launch has kind KIND)
    const auto* rc = (const p2::RoundConstants __attribute__((address_space(4)))*)(uintptr_t)rc_p;    // wave-uniform: scalar loads
    __syncthreads();
    const uint32_t terms = (d.rows + 1) / 2;
    const bool gkr = !FIRST && pass < 2;
    kb::Ext sa = kb::ext_zero(), sb = kb::ext_zero();
    if (!(FIRST && pass == 0))                         // round 0, node 0: the constraints vanish and the GKR pass is the interpreter's
    for (uint32_t base = (bid - d.block_start) * d.block_pairs; base < terms; base += d.n_blocks * d.block_pairs)
    for (uint32_t i = base + threadIdx.x; i < min(base + d.block_pairs, terms); i += blockDim.x) {
        kb::Ext e;
#pragma unroll
        for (int k = 0; k < 4; k++) e.c[k] = eq[(size_t)k * eq_len + i];
        kb::Ext va = kb::ext_zero(), vb = kb::ext_zero();
        auto ld_at = [&](uint32_t col, bool owned) -> T {
            const T v = leaf<FIRST>(d.main, col, d.rows, i, t);
            if (gkr && owned) vb = kb::ext_add(vb, K::scale(load_ext_aos(d.gkr_pows, col), v));
            return v;
        };
        auto ld = [&](uint32_t c, bool owned) -> T { return ld_at(base_col + c, owned); };
        auto sink = [&](uint32_t j, const T& v) { va = kb::ext_add(va, K::scale(load_ext_aos(d.alpha_pows, d.alpha_off + j), v)); };
        auto alpha = [&](uint32_t j) -> kb::Ext { return load_ext_aos(d.alpha_pows, d.alpha_off + j); };
        auto emit = [&](const kb::Ext& v) { va = kb::ext_add(va, v); };
        if constexpr (KIND == ZC_HINT_POSEIDON2) zc_p2_piece<F>(q, rc, ld, sink);
        else if constexpr (KIND == ZC_HINT_KECCAK) zc_keccak_piece<F>(q, ld, sink);
        else if constexpr (KIND == ZC_HINT_MUL) zc_mul_piece<F>(q, ld, [&](uint32_t c, bool owned) -> T { return ld_at(d.aux0 + c, owned); }, sink);
        else if constexpr (KIND == ZC_HINT_SEPTIC_CURVE) zc_septic_curve_piece_w<F, K>(q, ld, alpha, emit);
        else if (KIND == ZC_MACRO_BOTH_SEPTIC && ((d.flags >> 12) & 15u) == ZC_HINT_SEPTIC_CURVE) zc_septic_curve_piece_w<F, K>(q, ld, alpha, emit);   // (wave-uniform)
        else zc_septic_sum_piece_w<F, K>(q, ld, [&](uint32_t c, bool owned) -> T { return ld_at(d.aux0 + c, owned); },
                                         [&]() -> T { return ld_at(d.aux1, false); }, alpha, emit);
        sa = kb::ext_add(sa, kb::ext_mul(va, e));
        sb = kb::ext_add(sb, kb::ext_mul(vb, e));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t v[8];
#pragma unroll
    for (int k = 0; k < 4; k++) { v[k] = sa.c[k]; v[4 + k] = sb.c[k]; }
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = zc_wave_sum(v[k]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 8; k++) red[wave * 8 + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const uint32_t k = threadIdx.x;
        partial[((size_t)bid * 3 + pass) * 8 + k] = kb::add(kb::add(red[k], red[8 + k]), kb::add(red[16 + k], red[24 + k]));
    }
}

// ---- bivariate kernels. Interpreter: blockIdx.x = 3 b + g -> (block b of `block_pairs` row QUADS of one chunk, node group g =
// nodes 4 g .. 4 g + 3, four node values per register: KT4). A node's slot is [A | B] like the single-round kernels': A = sum eq
// C(node e); B = 0 here (the GKR batching term's corner sums come from zc_biv_corner_kernel's slots). partial[(12 bid + e) * 8 ..).
constexpr uint32_t ZC_BIV_GROUPS = 3;
template <int MAXR, bool STAGED>
__global__ __launch_bounds__(256) void zc_biv_round_kernel(const ZcDesc* __restrict__ descs, int n_descs,
                                                           const uint32_t* __restrict__ eq, uint32_t eq_len,
                                                           const uint32_t* __restrict__ publics, uint32_t* __restrict__ partial,
                                                           uint32_t rf_off, uint32_t block_base) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t* red = lds;                                   // [4][8] reduction scratch
    uint4* lprog = reinterpret_cast<uint4*>(lds + 32);
    RegFile<false, MAXR> reg;                              // four base-field values per register (KT4)
    if constexpr (MAXR == 0) {
        reg.base = (decltype(reg.base))(lds + rf_off) + threadIdx.x;
        reg.stride = blockDim.x;
    }
    if (threadIdx.x < 32) red[threadIdx.x] = 0;
    const uint32_t bid = block_base + blockIdx.x / ZC_BIV_GROUPS;
    const uint32_t grp = blockIdx.x % ZC_BIV_GROUPS;
    const ZcDesc d = zc_find_desc(descs, n_descs, bid);
    if constexpr (STAGED) {
        const uint4* src = reinterpret_cast<const uint4*>(d.prog);
        for (uint32_t k = threadIdx.x; k < d.n_instr; k += blockDim.x) lprog[k] = src[k];
    }
    __syncthreads();
    const uint32_t quads = (d.rows + 3) / 4;
    kb::Ext sa[4];
#pragma unroll
    for (int n = 0; n < 4; n++) sa[n] = kb::ext_zero();
    for (uint32_t base = (bid - d.block_start) * d.block_pairs; base < quads; base += d.n_blocks * d.block_pairs)
    for (uint32_t i = base + threadIdx.x; i < min(base + d.block_pairs, quads); i += blockDim.x) {
        kb::Ext e;
#pragma unroll
        for (int k = 0; k < 4; k++) e.c[k] = eq[(size_t)k * eq_len + i];
        kb::Ext va[4] = {kb::ext_zero(), kb::ext_zero(), kb::ext_zero(), kb::ext_zero()};
        if constexpr (STAGED) (void)run_program<true, MAXR, true>(reg, (const zc_word_t*)lprog, d, publics, i, (int)grp, false, va);
        else (void)run_program<true, MAXR, true>(reg, (zc_const_prog_t)(uintptr_t)d.prog, d, publics, i, (int)grp, false, va);
#pragma unroll
        for (int n = 0; n < 4; n++) sa[n] = kb::ext_add(sa[n], kb::ext_mul(va[n], e));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int n = 0; n < 4; n++) {
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) v[k] = zc_wave_sum(sa[n].c[k]);
        __syncthreads();
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) red[wave * 8 + k] = v[k];
        }
        __syncthreads();
        if (threadIdx.x < 8) {                             // (words 4..7 of `red` stay zero: the B half)
            const uint32_t k = threadIdx.x;
            partial[((size_t)bid * ZC_BIV_NODES + 4 * grp + n) * 8 + k] = kb::add(kb::add(red[k], red[8 + k]), kb::add(red[16 + k], red[24 + k]));
        }
    }
}

// The GKR batching term's corner sums of the bivariate rounds: B_n = sum_q eq(q) sum_c gkr_pow[c] * column c at row 4 q + n.
// Until round 6 the first chunk's node-group-0 workgroups of a chip walked ALL its columns for them, one after the other per lane:
// for the 2,640-column Keccak chip 400,000 dependent instructions on 477 waves — 6.2 ms, the longest launch of a Keccak shard's
// zerocheck by a factor of two, with the device idle around it. Here a workgroup takes 256 quads x ZC_CORNER_COLS columns:
// blockIdx.x = block of the launch's range; d.aux0 / d.aux1 = the slice [c0, c1) of the chip's main-then-preprocessed columns.
// Writes the B half of nodes 0..3 (what the interpreter's first chunk used to leave) and zeros everywhere else of its slots.
constexpr uint32_t ZC_CORNER_COLS = 32;
__global__ __launch_bounds__(256) void zc_biv_corner_kernel(const ZcDesc* __restrict__ descs, int n_descs, const uint32_t* __restrict__ eq,
                                                            uint32_t eq_len, uint32_t* __restrict__ partial, uint32_t block_base) {
    using K = KT<true>;
    __shared__ uint32_t red[4 * 16];
    const uint32_t bid = block_base + blockIdx.x;
    const ZcDesc d = zc_find_desc(descs, n_descs, bid);
    const uint32_t c0 = d.aux0, c1 = d.aux1;
    const uint32_t quads = (d.rows + 3) / 4;
    kb::Ext sb[4] = {kb::ext_zero(), kb::ext_zero(), kb::ext_zero(), kb::ext_zero()};
    for (uint32_t base = (bid - d.block_start) * d.block_pairs; base < quads; base += d.n_blocks * d.block_pairs)
    for (uint32_t i = base + threadIdx.x; i < min(base + d.block_pairs, quads); i += blockDim.x) {
        kb::Ext e;
#pragma unroll
        for (int k = 0; k < 4; k++) e.c[k] = eq[(size_t)k * eq_len + i];
        kb::Ext vb[4] = {kb::ext_zero(), kb::ext_zero(), kb::ext_zero(), kb::ext_zero()};
#pragma unroll 4
        for (uint32_t c = c0; c < c1; c++) {
            const kb::Ext pw = load_ext_aos(d.gkr_pows, c);
            const uint32_t* tbl = c < d.main_w ? d.main : d.prep;
            const uint32_t col = c < d.main_w ? c : c - d.main_w;
#pragma unroll
            for (uint32_t n = 0; n < 4; n++)
                if (4 * i + n < d.rows) vb[n] = kb::ext_add(vb[n], K::scale(pw, K::load(tbl, col, d.rows, 4 * i + n)));
        }
#pragma unroll
        for (int n = 0; n < 4; n++) sb[n] = kb::ext_add(sb[n], kb::ext_mul(vb[n], e));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int n = 0; n < 4; n++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t w = zc_wave_sum(sb[n].c[k]);
            if (lane == 0) red[wave * 16 + 4 * n + k] = w;
        }
    __syncthreads();
    if (threadIdx.x < ZC_BIV_NODES * 8) {
        const uint32_t node = threadIdx.x / 8, k = threadIdx.x % 8;
        uint32_t v = 0;
        if (node < 4 && k >= 4) {
            const uint32_t j = 4 * node + (k - 4);
            v = kb::add(kb::add(red[j], red[16 + j]), kb::add(red[32 + j], red[48 + j]));
        }
        partial[((size_t)bid * ZC_BIV_NODES + node) * 8 + k] = v;
    }
}

// the fused pieces on the bivariate grid (base-field arithmetic: the pieces' P2Base forms; no GKR term here)
template <uint32_t KIND>
__global__ __launch_bounds__(256) void zc_biv_macro_kernel(const ZcDesc* __restrict__ descs, int n_descs, const uint32_t* __restrict__ eq,
                                                           uint32_t eq_len, uint32_t* __restrict__ partial, uint32_t block_base,
                                                           const p2::RoundConstants* __restrict__ rc_p) {
    using K = KT<true>;
    __shared__ uint32_t red[32];
    if (threadIdx.x < 32) red[threadIdx.x] = 0;
    const uint32_t bid = block_base + blockIdx.x / (uint32_t)ZC_BIV_NODES;
    const uint32_t node = blockIdx.x % (uint32_t)ZC_BIV_NODES;
    const ZcBivNode nd = zc_biv_node(node);
    const ZcDesc d = zc_find_desc(descs, n_descs, bid);
    const uint32_t q = (d.flags >> 8) & 15u, base_col = d.pad;
    const auto* rc = (const p2::RoundConstants __attribute__((address_space(4)))*)(uintptr_t)rc_p;
    __syncthreads();
    const uint32_t quads = (d.rows + 3) / 4;
    kb::Ext sa = kb::ext_zero();
    for (uint32_t base = (bid - d.block_start) * d.block_pairs; base < quads; base += d.n_blocks * d.block_pairs)
    for (uint32_t i = base + threadIdx.x; i < min(base + d.block_pairs, quads); i += blockDim.x) {
        kb::Ext e;
#pragma unroll
        for (int k = 0; k < 4; k++) e.c[k] = eq[(size_t)k * eq_len + i];
        kb::Ext va = kb::ext_zero();
        auto ld_at = [&](uint32_t col, bool) -> uint32_t { return zc_biv_leaf(d.main, col, d.rows, i, nd); };
        auto ld = [&](uint32_t c, bool owned) -> uint32_t { return ld_at(base_col + c, owned); };
        auto sink = [&](uint32_t j, const uint32_t& v) { va = kb::ext_add(va, K::scale(load_ext_aos(d.alpha_pows, d.alpha_off + j), v)); };
        auto alpha = [&](uint32_t j) -> kb::Ext { return load_ext_aos(d.alpha_pows, d.alpha_off + j); };
        auto emit = [&](const kb::Ext& v) { va = kb::ext_add(va, v); };
        if constexpr (KIND == ZC_HINT_POSEIDON2) zc_p2_piece<P2Base>(q, rc, ld, sink);
        else if constexpr (KIND == ZC_HINT_KECCAK) zc_keccak_piece<P2Base>(q, ld, sink);
        else if constexpr (KIND == ZC_HINT_MUL) zc_mul_piece<P2Base>(q, ld, [&](uint32_t c, bool owned) -> uint32_t { return ld_at(d.aux0 + c, owned); }, sink);
        else if constexpr (KIND == ZC_HINT_SEPTIC_CURVE) zc_septic_curve_piece_w<P2Base, K>(q, ld, alpha, emit);
        else zc_septic_sum_piece_w<P2Base, K>(q, ld, [&](uint32_t c, bool owned) -> uint32_t { return ld_at(d.aux0 + c, owned); },
                                              [&]() -> uint32_t { return ld_at(d.aux1, false); }, alpha, emit);
        sa = kb::ext_add(sa, kb::ext_mul(va, e));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = zc_wave_sum(sa.c[k]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) red[wave * 8 + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 8) {
        const uint32_t k = threadIdx.x;
        partial[((size_t)bid * ZC_BIV_NODES + node) * 8 + k] = k < 4 ? kb::add(kb::add(red[k], red[8 + k]), kb::add(red[16 + k], red[24 + k])) : 0u;
    }
}

// ---- polynomial identities (zc_poly.hpp, hint kind 7): sum_t A_t B_t + R with affine forms A_t, B_t, R whose coefficients the host
// collapsed for this proof's alpha (table at d.prog: header, then 8-word entries). An affine form's value at a node of a row pair is
// the interpolation of its values on the two rows, so ONE workgroup (blockIdx.x = block) loads every column of its 256 row pairs once
// and leaves the sums of all three nodes: partial slots as the per-node kernels write them. The columns the identity owns (carry and
// witness limbs: nothing else reads them) carry their GKR batching term in the extension rounds.
struct ZcPolyTable {
    zc_const_words_t tb;
    __device__ __forceinline__ uint32_t word(uint32_t off) const { return tb[off]; }
    __device__ __forceinline__ kb::Ext coef(uint32_t off) const { return kb::Ext{{tb[off + 4], tb[off + 5], tb[off + 6], tb[off + 7]}}; }
};
__device__ __forceinline__ kb::Ext zc_ext_times_pow2(kb::Ext v, uint32_t k) {          // k in {0, 1, 2, 4, 8, 16}: compile-time after unrolling
    if (k == 0) return kb::ext_zero();
    for (uint32_t m = 1; m < k; m <<= 1) v = kb::ext_add(v, v);
    return v;
}
template <bool FIRST>
__global__ __launch_bounds__(256) void zc_poly_kernel(const ZcDesc* __restrict__ descs, int n_descs, const uint32_t* __restrict__ eq,
                                                      uint32_t eq_len, uint32_t* __restrict__ partial, uint32_t block_base) {
    using K = KT<FIRST>;
    using T = typename K::T;
    __shared__ uint32_t red[4 * 24];
    const uint32_t bid = block_base + blockIdx.x;
    const ZcDesc d = zc_find_desc(descs, n_descs, bid);
    const ZcPolyTable tab{(zc_const_words_t)(uintptr_t)d.prog};
    const uint32_t n_terms = tab.word(0), n_rest = tab.word(1), n_owned = tab.word(2);
    const uint32_t terms = (d.rows + 1) / 2;
    kb::Ext sa[3] = {kb::ext_zero(), kb::ext_zero(), kb::ext_zero()}, sb[2] = {kb::ext_zero(), kb::ext_zero()};
    for (uint32_t base = (bid - d.block_start) * d.block_pairs; base < terms; base += d.n_blocks * d.block_pairs)
    for (uint32_t i = base + threadIdx.x; i < min(base + d.block_pairs, terms); i += blockDim.x) {
        kb::Ext e;
#pragma unroll
        for (int k = 0; k < 4; k++) e.c[k] = eq[(size_t)k * eq_len + i];
        const bool has1 = 2 * i + 1 < d.rows;
        uint32_t off = ZC_POLY_HDR;
        // the values of one affine form on the two rows of the pair (its constant entry first)
        auto form = [&](uint32_t n, kb::Ext& f0, kb::Ext& f1) {
            f0 = f1 = tab.coef(off);
            off += ZC_POLY_ENTRY;
#pragma unroll 4
            for (uint32_t k = 0; k < n; k++, off += ZC_POLY_ENTRY) {
                const uint32_t col = tab.word(off);
                const kb::Ext c = tab.coef(off);
                const T x0 = K::load(d.main, col, d.rows, 2 * i);
                const T x1 = has1 ? K::load(d.main, col, d.rows, 2 * i + 1) : K::zero();
                f0 = kb::ext_add(f0, K::scale(c, x0));
                f1 = kb::ext_add(f1, K::scale(c, x1));
            }
        };
        kb::Ext v0 = kb::ext_zero(), v2 = kb::ext_zero(), v4 = kb::ext_zero();      // eq * C at the three nodes
        for (uint32_t t = 0; t < n_terms; t++) {
            kb::Ext a0, a1, b0, b1;
            form(tab.word(4 + 3 * t), a0, a1);
            form(tab.word(5 + 3 * t), b0, b1);
            a0 = kb::ext_mul(a0, e); a1 = kb::ext_mul(a1, e);
            const kb::Ext da = kb::ext_sub(a1, a0), db = kb::ext_sub(b1, b0);
            const kb::Ext da2 = kb::ext_add(da, da), db2 = kb::ext_add(db, db);
            const kb::Ext a2 = kb::ext_add(a0, da2), b2 = kb::ext_add(b0, db2);
            kb::Ext p0 = FIRST ? kb::ext_zero() : kb::ext_mul(a0, b0), p2 = kb::ext_mul(a2, b2), p4 = kb::ext_mul(kb::ext_add(a2, da2), kb::ext_add(b2, db2));
            const uint32_t n2 = tab.word(6 + 3 * t);
            if (n2 != ZC_POLY_NONE) {                                               // (wave-uniform)
                kb::Ext c0, c1;
                form(n2, c0, c1);
                const kb::Ext dc = kb::ext_sub(c1, c0), dc2 = kb::ext_add(dc, dc), c2 = kb::ext_add(c0, dc2);
                if (!FIRST) p0 = kb::ext_mul(p0, c0);
                p2 = kb::ext_mul(p2, c2);
                p4 = kb::ext_mul(p4, kb::ext_add(c2, dc2));
            }
            v0 = kb::ext_add(v0, p0); v2 = kb::ext_add(v2, p2); v4 = kb::ext_add(v4, p4);
        }
        kb::Ext r0, r1, g0 = kb::ext_zero(), g1 = kb::ext_zero();
        form(n_rest, r0, r1);
#pragma unroll 2
        for (uint32_t k = 0; k < n_owned; k++, off += ZC_POLY_ENTRY) {
            const uint32_t col = tab.word(off);
            const kb::Ext c = tab.coef(off);
            const T x0 = K::load(d.main, col, d.rows, 2 * i);
            const T x1 = has1 ? K::load(d.main, col, d.rows, 2 * i + 1) : K::zero();
            r0 = kb::ext_add(r0, K::scale(c, x0));
            r1 = kb::ext_add(r1, K::scale(c, x1));
            if (!FIRST) {
                const kb::Ext gp = load_ext_aos(d.gkr_pows, col);
                g0 = kb::ext_add(g0, K::scale(gp, x0));
                g1 = kb::ext_add(g1, K::scale(gp, x1));
            }
        }
        r0 = kb::ext_mul(r0, e); r1 = kb::ext_mul(r1, e);
        const kb::Ext dr = kb::ext_sub(r1, r0), dr2 = kb::ext_add(dr, dr), r2 = kb::ext_add(r0, dr2);
        if (!FIRST) sa[0] = kb::ext_add(sa[0], kb::ext_add(v0, r0));
        sa[1] = kb::ext_add(sa[1], kb::ext_add(v2, r2));
        sa[2] = kb::ext_add(sa[2], kb::ext_add(v4, kb::ext_add(r2, dr2)));
        if (!FIRST) {
            g0 = kb::ext_mul(g0, e); g1 = kb::ext_mul(g1, e);
            const kb::Ext dg = kb::ext_sub(g1, g0);
            sb[0] = kb::ext_add(sb[0], g0);
            sb[1] = kb::ext_add(sb[1], kb::ext_add(g0, kb::ext_add(dg, dg)));
        }
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t v[24];
#pragma unroll
    for (int pass = 0; pass < 3; pass++)
#pragma unroll
        for (int k = 0; k < 4; k++) { v[pass * 8 + k] = zc_wave_sum(sa[pass].c[k]); v[pass * 8 + 4 + k] = pass < 2 ? zc_wave_sum(sb[pass].c[k]) : 0u; }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 24; k++) red[wave * 24 + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 24) {
        const uint32_t k = threadIdx.x;
        uint32_t acc = red[k];
        for (uint32_t w = 1; w < blockDim.x / 64; w++) acc = kb::add(acc, red[w * 24 + k]);
        partial[((size_t)bid * 3 + k / 8) * 8 + (k & 7u)] = acc;
    }
}

// The same in the SMALL extension rounds, one WAVE per row pair: a lane of zc_poly_kernel walks every entry of every form of its
// pair — ~350 dependent load-multiply steps for a 48-limb field operation —, and once a round has only a few thousand pairs that
// walk is the round: 400 us per round whatever its size, 6.5 ms of a bls12-381 Fp shard's 23.8 ms of zerocheck. Here the 64 lanes
// of a wave take the entries of a form 64 at a time and the form is a wave sum; workgroup = 4 pairs (d.block_pairs = 4).
__global__ __launch_bounds__(256) void zc_poly_wave_kernel(const ZcDesc* __restrict__ descs, int n_descs, const uint32_t* __restrict__ eq,
                                                           uint32_t eq_len, uint32_t* __restrict__ partial, uint32_t block_base) {
    using K = KT<false>;
    __shared__ uint32_t red[4 * 24];
    const uint32_t bid = block_base + blockIdx.x;
    const ZcDesc d = zc_find_desc(descs, n_descs, bid);
    const ZcPolyTable tab{(zc_const_words_t)(uintptr_t)d.prog};
    const zc_global_words_t tg = (zc_global_words_t)d.prog;           // (entries are read per lane)
    const zc_global_words_t gp = (zc_global_words_t)d.gkr_pows;
    const uint32_t n_terms = tab.word(0), n_rest = tab.word(1), n_owned = tab.word(2);
    const uint32_t terms = (d.rows + 1) / 2;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    kb::Ext sa[3] = {kb::ext_zero(), kb::ext_zero(), kb::ext_zero()}, sb[2] = {kb::ext_zero(), kb::ext_zero()};
    auto wsum = [&](kb::Ext& v) {
#pragma unroll
        for (int k = 0; k < 4; k++) v.c[k] = zc_wave_sum(v.c[k]);
    };
    for (uint32_t i = (bid - d.block_start) * 4 + wave; i < terms; i += d.n_blocks * 4) {     // (wave-uniform)
        kb::Ext e;
#pragma unroll
        for (int k = 0; k < 4; k++) e.c[k] = eq[(size_t)k * eq_len + i];
        const bool has1 = 2 * i + 1 < d.rows;
        uint32_t off = ZC_POLY_HDR;
        // one affine form on the two rows: `n` entries behind an optional constant entry; with_gkr: the owned columns' batching term too
        auto form = [&](uint32_t n, bool with_const, kb::Ext& f0, kb::Ext& f1, kb::Ext* g0, kb::Ext* g1) {
            const uint32_t first = off + (with_const ? ZC_POLY_ENTRY : 0u);
            kb::Ext p0 = kb::ext_zero(), p1 = kb::ext_zero(), q0 = kb::ext_zero(), q1 = kb::ext_zero();
            for (uint32_t k = lane; k < n; k += 64) {
                const uint32_t o = first + ZC_POLY_ENTRY * k;
                const uint32_t col = tg[o];
                const kb::Ext c{{tg[o + 4], tg[o + 5], tg[o + 6], tg[o + 7]}};
                const kb::Ext x0 = K::load(d.main, col, d.rows, 2 * i);
                const kb::Ext x1 = has1 ? K::load(d.main, col, d.rows, 2 * i + 1) : kb::ext_zero();
                p0 = kb::ext_add(p0, kb::ext_mul(x0, c));
                p1 = kb::ext_add(p1, kb::ext_mul(x1, c));
                if (g0) {
                    const kb::Ext w{{gp[4 * col], gp[4 * col + 1], gp[4 * col + 2], gp[4 * col + 3]}};
                    q0 = kb::ext_add(q0, kb::ext_mul(x0, w));
                    q1 = kb::ext_add(q1, kb::ext_mul(x1, w));
                }
            }
            wsum(p0); wsum(p1);
            if (with_const) { const kb::Ext c0 = tab.coef(off); p0 = kb::ext_add(p0, c0); p1 = kb::ext_add(p1, c0); }
            f0 = p0; f1 = p1;
            if (g0) { wsum(q0); wsum(q1); *g0 = q0; *g1 = q1; }
            off = first + ZC_POLY_ENTRY * n;
        };
        kb::Ext v0 = kb::ext_zero(), v2 = kb::ext_zero(), v4 = kb::ext_zero();
        for (uint32_t t = 0; t < n_terms; t++) {
            kb::Ext a0, a1, b0, b1;
            form(tab.word(4 + 3 * t), true, a0, a1, nullptr, nullptr);
            form(tab.word(5 + 3 * t), true, b0, b1, nullptr, nullptr);
            a0 = kb::ext_mul(a0, e); a1 = kb::ext_mul(a1, e);
            const kb::Ext da = kb::ext_sub(a1, a0), db = kb::ext_sub(b1, b0);
            const kb::Ext da2 = kb::ext_add(da, da), db2 = kb::ext_add(db, db);
            const kb::Ext a2 = kb::ext_add(a0, da2), b2 = kb::ext_add(b0, db2);
            kb::Ext p0 = kb::ext_mul(a0, b0), p2 = kb::ext_mul(a2, b2), p4 = kb::ext_mul(kb::ext_add(a2, da2), kb::ext_add(b2, db2));
            const uint32_t n2 = tab.word(6 + 3 * t);
            if (n2 != ZC_POLY_NONE) {
                kb::Ext c0, c1;
                form(n2, true, c0, c1, nullptr, nullptr);
                const kb::Ext dc = kb::ext_sub(c1, c0), dc2 = kb::ext_add(dc, dc), c2 = kb::ext_add(c0, dc2);
                p0 = kb::ext_mul(p0, c0); p2 = kb::ext_mul(p2, c2); p4 = kb::ext_mul(p4, kb::ext_add(c2, dc2));
            }
            v0 = kb::ext_add(v0, p0); v2 = kb::ext_add(v2, p2); v4 = kb::ext_add(v4, p4);
        }
        kb::Ext r0, r1, o0, o1, g0, g1;
        form(n_rest, true, r0, r1, nullptr, nullptr);
        form(n_owned, false, o0, o1, &g0, &g1);
        r0 = kb::ext_mul(kb::ext_add(r0, o0), e); r1 = kb::ext_mul(kb::ext_add(r1, o1), e);
        const kb::Ext dr = kb::ext_sub(r1, r0), dr2 = kb::ext_add(dr, dr), r2 = kb::ext_add(r0, dr2);
        sa[0] = kb::ext_add(sa[0], kb::ext_add(v0, r0));
        sa[1] = kb::ext_add(sa[1], kb::ext_add(v2, r2));
        sa[2] = kb::ext_add(sa[2], kb::ext_add(v4, kb::ext_add(r2, dr2)));
        g0 = kb::ext_mul(g0, e); g1 = kb::ext_mul(g1, e);
        const kb::Ext dg = kb::ext_sub(g1, g0);
        sb[0] = kb::ext_add(sb[0], g0);
        sb[1] = kb::ext_add(sb[1], kb::ext_add(g0, kb::ext_add(dg, dg)));
    }
    if (lane == 0) {                                                   // (every lane of a wave holds the same sums)
#pragma unroll
        for (int pass = 0; pass < 3; pass++)
#pragma unroll
            for (int k = 0; k < 4; k++) { red[wave * 24 + pass * 8 + k] = sa[pass].c[k]; red[wave * 24 + pass * 8 + 4 + k] = pass < 2 ? sb[pass].c[k] : 0u; }
    }
    __syncthreads();
    if (threadIdx.x < 24) {
        const uint32_t k = threadIdx.x;
        const uint32_t acc = kb::add(kb::add(red[k], red[24 + k]), kb::add(red[48 + k], red[72 + k]));
        partial[((size_t)bid * 3 + k / 8) * 8 + (k & 7u)] = acc;
    }
}

// The bivariate rounds: row quads, the twelve nodes of the grid from the forms' values on the four rows (base-field words).
__global__ __launch_bounds__(256) void zc_biv_poly_kernel(const ZcDesc* __restrict__ descs, int n_descs, const uint32_t* __restrict__ eq,
                                                          uint32_t eq_len, uint32_t* __restrict__ partial, uint32_t block_base) {
    __shared__ uint32_t red[4 * 48];
    const uint32_t bid = block_base + blockIdx.x;
    const ZcDesc d = zc_find_desc(descs, n_descs, bid);
    const ZcPolyTable tab{(zc_const_words_t)(uintptr_t)d.prog};
    const uint32_t n_terms = tab.word(0), n_rest = tab.word(1), n_owned = tab.word(2);
    const uint32_t quads = (d.rows + 3) / 4;
    kb::Ext sa[ZC_BIV_NODES];
#pragma unroll
    for (int n = 0; n < ZC_BIV_NODES; n++) sa[n] = kb::ext_zero();
    for (uint32_t base = (bid - d.block_start) * d.block_pairs; base < quads; base += d.n_blocks * d.block_pairs)
    for (uint32_t i = base + threadIdx.x; i < min(base + d.block_pairs, quads); i += blockDim.x) {
        kb::Ext e;
#pragma unroll
        for (int k = 0; k < 4; k++) e.c[k] = eq[(size_t)k * eq_len + i];
        const uint32_t r = 4 * i;
        uint32_t off = ZC_POLY_HDR;
        auto form = [&](uint32_t n, kb::Ext (&f)[4]) {              // f: the form on rows r .. r + 3 = (X, Y) = (0,0) (0,1) (1,0) (1,1)
            f[0] = f[1] = f[2] = f[3] = tab.coef(off);
            off += ZC_POLY_ENTRY;
#pragma unroll 2
            for (uint32_t k = 0; k < n; k++, off += ZC_POLY_ENTRY) {
                const uint32_t col = tab.word(off);
                const kb::Ext c = tab.coef(off);
                const zc_global_words_t g = (zc_global_words_t)d.main + (size_t)col * d.rows;
                const uint32_t x00 = g[r], x01 = r + 1 < d.rows ? g[r + 1] : 0u, x10 = r + 2 < d.rows ? g[r + 2] : 0u, x11 = r + 3 < d.rows ? g[r + 3] : 0u;
                f[0] = kb::ext_add(f[0], kb::ext_mul_base(c, x00));
                f[1] = kb::ext_add(f[1], kb::ext_mul_base(c, x01));
                f[2] = kb::ext_add(f[2], kb::ext_mul_base(c, x10));
                f[3] = kb::ext_add(f[3], kb::ext_mul_base(c, x11));
            }
        };
        // f -> (f00, dX, dY, dXY): the form at node (X, Y) is f00 + X dX + Y dY + X Y dXY
        auto slopes = [&](kb::Ext (&f)[4]) {
            const kb::Ext dy = kb::ext_sub(f[1], f[0]), dx = kb::ext_sub(f[2], f[0]);
            f[3] = kb::ext_sub(kb::ext_sub(f[3], f[2]), dy);
            f[1] = dx; f[2] = dy;
        };
        auto at = [&](const kb::Ext (&f)[4], const ZcBivNode& nd) -> kb::Ext {
            return kb::ext_add(kb::ext_add(f[0], zc_ext_times_pow2(f[1], nd.cx)), kb::ext_add(zc_ext_times_pow2(f[2], nd.cy), zc_ext_times_pow2(f[3], nd.cxy)));
        };
        for (uint32_t t = 0; t < n_terms; t++) {
            kb::Ext a[4], b[4];
            form(tab.word(4 + 3 * t), a);
            form(tab.word(5 + 3 * t), b);
#pragma unroll
            for (int k = 0; k < 4; k++) a[k] = kb::ext_mul(a[k], e);
            slopes(a); slopes(b);
            const uint32_t n2 = tab.word(6 + 3 * t);
            if (n2 == ZC_POLY_NONE) {                                               // (wave-uniform)
#pragma unroll
                for (int n = 0; n < ZC_BIV_NODES; n++) {
                    const ZcBivNode nd = zc_biv_node(n);
                    sa[n] = kb::ext_add(sa[n], kb::ext_mul(at(a, nd), at(b, nd)));
                }
            } else {
                kb::Ext c[4];
                form(n2, c);
                slopes(c);
#pragma unroll
                for (int n = 0; n < ZC_BIV_NODES; n++) {
                    const ZcBivNode nd = zc_biv_node(n);
                    sa[n] = kb::ext_add(sa[n], kb::ext_mul(kb::ext_mul(at(a, nd), at(b, nd)), at(c, nd)));
                }
            }
        }
        kb::Ext rr[4];
        form(n_rest + n_owned, rr);                                 // (the owned columns follow the rest's: no GKR term in these rounds)
#pragma unroll
        for (int k = 0; k < 4; k++) rr[k] = kb::ext_mul(rr[k], e);
        slopes(rr);
#pragma unroll
        for (int n = 0; n < ZC_BIV_NODES; n++) sa[n] = kb::ext_add(sa[n], at(rr, zc_biv_node(n)));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t v[48];
#pragma unroll
    for (int n = 0; n < ZC_BIV_NODES; n++)
#pragma unroll
        for (int k = 0; k < 4; k++) v[n * 4 + k] = zc_wave_sum(sa[n].c[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 48; k++) red[wave * 48 + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < 48) {
        const uint32_t k = threadIdx.x;
        uint32_t acc = red[k];
        for (uint32_t w = 1; w < blockDim.x / 64; w++) acc = kb::add(acc, red[w * 48 + k]);
        partial[((size_t)bid * ZC_BIV_NODES + k / 4) * 8 + (k & 3u)] = acc;
        partial[((size_t)bid * ZC_BIV_NODES + k / 4) * 8 + 4 + (k & 3u)] = 0u;
    }
}

// The Keccak pieces on the bivariate grid, FOUR nodes per pass (node group g = nodes 4 g .. 4 g + 3, like the interpreter's KT4
// passes): the pieces are bound by the bandwidth their column loads draw from the caches, and one node per workgroup reads the
// four rows of every column twelve times. Here the rows are loaded once per group and interpolated to the group's four nodes; the
// arithmetic is element-wise on the 4-vector. blockIdx.x = 3 b + g.
struct P2Base4 {
    using T = kb::Ext;                                   // four base-field node values
    static __device__ __forceinline__ T add(const T& a, const T& b) { return kb::ext_add(a, b); }
    static __device__ __forceinline__ T sub(const T& a, const T& b) { return kb::ext_sub(a, b); }
    static __device__ __forceinline__ T mul(const T& a, const T& b) { return KT4::mul(a, b); }
    static __device__ __forceinline__ T addc(const T& a, uint32_t c) { return KC4::addc(a, c); }
    static __device__ __forceinline__ T mulc(const T& a, uint32_t c) { return kb::ext_mul_base(a, c); }
};
__global__ __launch_bounds__(256) void zc_biv_keccak_kernel(const ZcDesc* __restrict__ descs, int n_descs, const uint32_t* __restrict__ eq,
                                                            uint32_t eq_len, uint32_t* __restrict__ partial, uint32_t block_base) {
    using K = KT<true>;
    __shared__ uint32_t red[4][32];
    const uint32_t bid = block_base + blockIdx.x / ZC_BIV_GROUPS;
    const uint32_t grp = blockIdx.x % ZC_BIV_GROUPS;
    const ZcBivNode n0 = zc_biv_node(4 * grp), n1 = zc_biv_node(4 * grp + 1), n2 = zc_biv_node(4 * grp + 2), n3 = zc_biv_node(4 * grp + 3);
    const ZcDesc d = zc_find_desc(descs, n_descs, bid);
    const uint32_t q = (d.flags >> 8) & 15u, base_col = d.pad;
    const uint32_t quads = (d.rows + 3) / 4;
    kb::Ext sa[4] = {kb::ext_zero(), kb::ext_zero(), kb::ext_zero(), kb::ext_zero()};
    for (uint32_t base = (bid - d.block_start) * d.block_pairs; base < quads; base += d.n_blocks * d.block_pairs)
    for (uint32_t i = base + threadIdx.x; i < min(base + d.block_pairs, quads); i += blockDim.x) {
        kb::Ext e;
#pragma unroll
        for (int k = 0; k < 4; k++) e.c[k] = eq[(size_t)k * eq_len + i];
        kb::Ext va[4] = {kb::ext_zero(), kb::ext_zero(), kb::ext_zero(), kb::ext_zero()};
        auto ld = [&](uint32_t c, bool) -> kb::Ext {
            const zc_global_words_t g = (zc_global_words_t)d.main + (size_t)(base_col + c) * d.rows;
            const uint32_t r = 4 * i;
            const uint32_t r00 = g[r], r01 = r + 1 < d.rows ? g[r + 1] : 0u, r10 = r + 2 < d.rows ? g[r + 2] : 0u, r11 = r + 3 < d.rows ? g[r + 3] : 0u;
            return kb::Ext{{zc_biv_interp(r00, r01, r10, r11, n0), zc_biv_interp(r00, r01, r10, r11, n1), zc_biv_interp(r00, r01, r10, r11, n2),
                            zc_biv_interp(r00, r01, r10, r11, n3)}};
        };
        auto sink = [&](uint32_t j, const kb::Ext& v) {
            const kb::Ext a = load_ext_aos(d.alpha_pows, d.alpha_off + j);
#pragma unroll
            for (int n = 0; n < 4; n++) va[n] = kb::ext_add(va[n], K::scale(a, v.c[n]));
        };
        zc_keccak_piece<P2Base4>(q, ld, sink);
#pragma unroll
        for (int n = 0; n < 4; n++) sa[n] = kb::ext_add(sa[n], kb::ext_mul(va[n], e));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int n = 0; n < 4; n++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t v = zc_wave_sum(sa[n].c[k]);
            if (lane == 0) red[wave][n * 4 + k] = v;
        }
    __syncthreads();
    if (threadIdx.x < 32) {
        const uint32_t n = threadIdx.x >> 3, k = threadIdx.x & 7u;
        const uint32_t w = n * 4 + (k & 3u);
        partial[((size_t)bid * ZC_BIV_NODES + 4 * grp + n) * 8 + k] =
            k < 4 ? kb::add(kb::add(red[0][w], red[1][w]), kb::add(red[2][w], red[3][w])) : 0u;
    }
}

// One workgroup per (range, node): the node's [A | B] summed over the range's blocks. Per range the output is A_0..11 (12 ext),
// the four corner sums B_0..3 (4 ext), eq[th] (1 ext): out[range][68] and, with a host slot, payload words [1 + 68 range ..);
// the last workgroup of the launch publishes `seq`. (One workgroup per range took 235 us for a chip of 12k blocks.)
constexpr uint32_t ZC_BIV_SUM_WORDS = 68;
__global__ __launch_bounds__(256) void zc_biv_reduce_kernel(const ZcChipRange* __restrict__ ranges, const uint32_t* __restrict__ partial,
                                                            const uint32_t* __restrict__ eq, uint32_t eq_len,
                                                            uint32_t* __restrict__ out, RoundSync rs, uint32_t seq) {
    __shared__ uint32_t acc[32][8];
    const uint32_t range = blockIdx.x / (uint32_t)ZC_BIV_NODES, node = blockIdx.x % (uint32_t)ZC_BIV_NODES;
    const ZcChipRange d = ranges[range];
    const uint32_t word = threadIdx.x & 7u, grp = threadIdx.x >> 3;       // 32 groups of 8 words
    {
        const uint32_t* p = partial + ((size_t)d.block_start * ZC_BIV_NODES + node) * 8 + word;
        uint32_t a[4] = {0, 0, 0, 0};
        uint32_t b = grp;
        for (; b + 96 < d.n_blocks; b += 128)
#pragma unroll
            for (int u = 0; u < 4; u++) a[u] = kb::add(a[u], p[(size_t)(b + 32 * u) * (ZC_BIV_NODES * 8)]);
        for (; b < d.n_blocks; b += 32) a[0] = kb::add(a[0], p[(size_t)b * (ZC_BIV_NODES * 8)]);
        acc[grp][word] = kb::add(kb::add(a[0], a[1]), kb::add(a[2], a[3]));
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        // words 0..3: A_node -> [4 node ..), words 4..7: B_node -> [48 + 4 node ..) for node < 4, words 8..11: eq[th] -> [64 ..) from node 0
        const uint32_t w = threadIdx.x;
        uint32_t val = 0, dst = 0xffffffffu;
        if (w < 8) {
            for (uint32_t g = 0; g < 32; g++) val = kb::add(val, acc[g][w]);
            if (w < 4) dst = 4 * node + w;
            else if (node < 4) dst = 48 + 4 * node + (w - 4);
        } else if (node == 0) {
            const uint32_t k = w - 8;
            val = d.th < eq_len ? eq[(size_t)k * eq_len + d.th] : 0u;
            dst = 64 + k;
        }
        if (dst != 0xffffffffu) {
            out[(size_t)range * ZC_BIV_SUM_WORDS + dst] = val;
            if (rs.host_slot != nullptr)
                __hip_atomic_store(const_cast<uint32_t*>(rs.host_slot) + 1 + (size_t)range * ZC_BIV_SUM_WORDS + dst, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
    if (rs.host_slot == nullptr) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && rs_ticket_is_last_acq_rel(rs.counter, blockIdx.x, gridDim.x)) rs_publish_seq(rs.host_slot, seq);
}

// One workgroup per chip: sums its workgroups' partials and forms (y0, y2, y4, eq[th]) -> out[chip][16].
template <bool FIRST>
__global__ __launch_bounds__(256) void zc_reduce_kernel(const ZcChipRange* __restrict__ ranges, const uint32_t* __restrict__ partial,
                                                        const uint32_t* __restrict__ eq, uint32_t eq_len,
                                                        uint32_t* __restrict__ out, RoundSync rs, uint32_t seq) {
    __shared__ uint32_t acc[10][24];
    const ZcChipRange d = ranges[blockIdx.x];
    uint32_t y0, y2, y4, e;
    zc_reduce_range<FIRST>(d, partial, eq, eq_len, acc, y0, y2, y4, e);
    if (threadIdx.x < 4) {
        const uint32_t k = threadIdx.x;
        uint32_t* o = out + (size_t)blockIdx.x * 16;
        o[k] = y0; o[4 + k] = y2; o[8 + k] = y4;
        o[12 + k] = e;
    }
    // the round's result goes to the host from HERE (payload words [1 + 16 chip ..)): system-scope stores, and below the
    // workgroup that arrives last publishes the sequence number — no mailbox kernel behind this one
    if (rs.host_slot != nullptr) zc_store_host_sums(rs.host_slot, blockIdx.x, y0, y2, y4, e);
    if (rs.host_slot == nullptr) return;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0 && rs_ticket_is_last_acq_rel(rs.counter, blockIdx.x, gridDim.x)) rs_publish_seq(rs.host_slot, seq);
}

// out[i][c] = x + alpha (y - x), x = row 2i, y = row 2i + 1 (zero beyond the real rows); out is an ext table.
// One launch per round for every table of every chip. A workgroup owns ZC_FIX_ROWS consecutive rows of ONE column (8 per
// lane): the column comes from the block index with a multiply-high and the table from a binary search. The former form —
// one element per thread over the flattened table, 64-bit division and modulo per element, a linear scan of the ~45
// descriptors per workgroup — launched 786k workgroups for the first round's 2e8 elements and ran at 3.2 TB/s.
constexpr uint32_t ZC_FIX_ROWS = 2048;          // output rows of one column per workgroup (8 per lane)
template <bool FIRST>
__global__ __launch_bounds__(256) void zc_fix_kernel(const ZcFixDesc* __restrict__ descs, int n_descs, kb::Ext alpha) {
    using K = KT<FIRST>;
    int lo = 0, hi = n_descs - 1;                                    // last descriptor with block_start <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (__builtin_amdgcn_readfirstlane(descs[mid].block_start) <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const ZcFixDesc d = descs[lo];
    const uint32_t out_rows = (d.rows + 1) / 2;
    const uint32_t lb = blockIdx.x - d.block_start;
    uint32_t c = d.bpc == 1 ? lb : __umulhi(lb, d.bpc_magic);       // floor(lb / bpc), at most 2 short
    uint32_t tile = lb - c * d.bpc;
    if (tile >= d.bpc) { tile -= d.bpc; c++; }
    if (tile >= d.bpc) { tile -= d.bpc; c++; }
    const uint32_t i0 = tile * ZC_FIX_ROWS, i1 = min(out_rows, i0 + ZC_FIX_ROWS);
    for (uint32_t i = i0 + threadIdx.x; i < i1; i += 256u) {
        typename K::T x = K::load(d.in, c, d.rows, 2 * i);
        typename K::T y = (2 * i + 1 < d.rows) ? K::load(d.in, c, d.rows, 2 * i + 1) : K::zero();
        const kb::Ext r = kb::ext_add(K::scale(alpha, K::sub(y, x)), K::to_ext(x));
#pragma unroll
        for (int q = 0; q < 4; q++) gptr(d.out)[((size_t)c * 4 + q) * out_rows + i] = r.c[q];
    }
}

// The table update behind the bivariate rounds: out[q][c] = T_q(X = a1, Y = a0) — the fold by the first challenge and then by
// the second, from the base-field rows (fix_last_variable.rs applied twice): one pass, 4 A bytes read and 4 A written instead of
// 4 A + 8 A read and 8 A + 4 A written by two updates. Descriptors as for zc_fix_kernel with out_rows = ceil(rows / 4).
__global__ __launch_bounds__(256) void zc_fix2_kernel(const ZcFixDesc* __restrict__ descs, int n_descs, kb::Ext a0, kb::Ext a1) {
    int lo = 0, hi = n_descs - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (__builtin_amdgcn_readfirstlane(descs[mid].block_start) <= blockIdx.x) lo = mid; else hi = mid - 1;
    }
    const ZcFixDesc d = descs[lo];
    const uint32_t out_rows = (d.rows + 3) / 4;
    const uint32_t lb = blockIdx.x - d.block_start;
    uint32_t c = d.bpc == 1 ? lb : __umulhi(lb, d.bpc_magic);
    uint32_t tile = lb - c * d.bpc;
    if (tile >= d.bpc) { tile -= d.bpc; c++; }
    if (tile >= d.bpc) { tile -= d.bpc; c++; }
    const uint32_t i0 = tile * ZC_FIX_ROWS, i1 = min(out_rows, i0 + ZC_FIX_ROWS);
    const zc_global_words_t g = (zc_global_words_t)d.in + (size_t)c * d.rows;
    for (uint32_t i = i0 + threadIdx.x; i < i1; i += 256u) {
        const uint32_t r = 4 * i;
        const uint32_t r00 = g[r], r01 = r + 1 < d.rows ? g[r + 1] : 0u, r10 = r + 2 < d.rows ? g[r + 2] : 0u, r11 = r + 3 < d.rows ? g[r + 3] : 0u;
        const uint32_t dy = kb::sub(r01, r00), dx = kb::sub(r10, r00), dxy = kb::sub(kb::sub(r11, r10), dy);
        kb::Ext lo_row = kb::ext_mul_base(a0, dy);             // row 2 i of the once-folded table: r00 + a0 (r01 - r00)
        lo_row.c[0] = kb::add(lo_row.c[0], r00);
        kb::Ext slope = kb::ext_mul_base(a0, dxy);             // (row 2 i + 1) - (row 2 i) = (r10 - r00) + a0 ((r11 - r10) - (r01 - r00))
        slope.c[0] = kb::add(slope.c[0], dx);
        const kb::Ext res = kb::ext_add(lo_row, kb::ext_mul(slope, a1));
#pragma unroll
        for (int k = 0; k < 4; k++) gptr(d.out)[((size_t)c * 4 + k) * out_rows + i] = res.c[k];
    }
}

struct ZcGatherDesc { const uint32_t* src; uint32_t n_words, dst_off; };
__global__ __launch_bounds__(256) void zc_gather_kernel(const ZcGatherDesc* __restrict__ descs, uint32_t* __restrict__ out) {
    const ZcGatherDesc d = descs[blockIdx.x];
    for (uint32_t i = threadIdx.x; i < d.n_words; i += 256) out[d.dst_off + i] = gptr(d.src)[i];
}

}  // namespace sp1hip
