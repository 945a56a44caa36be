// sp1_amd/csrc/gkr_kernels.hpp — the device side of LogUp-GKR: the first layer and the fraction tree, the per-layer eq tables,
// the two-rounds-per-pass sumcheck kernel (gkr_pass), its up-to-four-rounds forms for the flat launches (gkr_pass_deep,
// gkr_pass_deep_fold) and the trace openings, with the descriptors the host fills for them.
// Included by gkr.hip only (the prover and its launches; the layout and the shape of the stage are described there).
#pragma once
#include "col_dot.hpp"
#include "device_ctx.hpp"
#include "round_sync.hpp"

namespace sp1hip {
namespace gkr {

using Ext = kb::Ext;

__device__ __forceinline__ Ext ld_ext(const Ext* p, uint32_t i) {
    const q4_t v = gptr(reinterpret_cast<const q4_t*>(p))[i];
    return Ext{{v.x, v.y, v.z, v.w}};
}
__device__ __forceinline__ void st_ext(Ext* p, uint32_t i, const Ext& e) {
    const q4_t v = {e.c[0], e.c[1], e.c[2], e.c[3]};
    gptr(reinterpret_cast<q4_t*>(p))[i] = v;
}

// the same into fine-grained HOST memory: system-scope stores (sc0 sc1: past the write-back L2, which would otherwise keep
// the line until the kernel ends)
__device__ __forceinline__ void st_ext_host(Ext* p, uint32_t i, const Ext& e) {
    uint32_t* w = reinterpret_cast<uint32_t*>(p + i);
#pragma unroll
    for (int k = 0; k < 4; k++) __hip_atomic_store(w + k, e.c[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- block reduction of NS ext accumulators -> partials[block][4 NS]
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = kb::add(v, __shfl_down(v, off, 64));
    return v;
}
template <int NS>
__device__ __forceinline__ void block_reduce_store(const Ext (&acc)[NS], uint32_t* out) {
    __shared__ uint32_t sm[4][4 * NS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int s = 0; s < NS; s++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t w = wave_sum(acc[s].c[k]);
            if (lane == 0) sm[wave][4 * s + k] = w;
        }
    __syncthreads();
    if (threadIdx.x < 4 * NS) {
        uint32_t a = 0;
        for (int i = 0; i < 4; i++) a = kb::add(a, sm[i][threadIdx.x]);
        out[threadIdx.x] = a;
    }
}
template <int NS>
__global__ __launch_bounds__(256) void reduce_partials(const uint32_t* __restrict__ partials, uint32_t n, uint32_t* out) {
    Ext acc[NS];
#pragma unroll
    for (int s = 0; s < NS; s++) acc[s] = kb::ext_zero();
    for (uint32_t i = threadIdx.x; i < n; i += 256)
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const uint32_t* q = partials + ((size_t)i * NS + s) * 4;
            acc[s] = kb::ext_add(acc[s], Ext{{q[0], q[1], q[2], q[3]}});
        }
    block_reduce_store<NS>(acc, out);
}

// Layout of the circuit levels (numerators / denominators per interaction): a fold kernel's lane wants 8 consecutive
// entries (two row pairs), a sums-only kernel's 4, the fraction tree's 2 — 128 / 64 / 32 B at that lane stride. Inside every
// complete block of 512 entries, entry e lives at (e mod 8) * 64 + (e div 8) mod 64: the fold's loads are contiguous 1 KiB
// runs, the sums-only loads two 512 B runs, the tree's four 256 B runs, and the writers (one entry per lane) fill whole
// 128 B lines. The last, incomplete block keeps the natural order (nothing grows; the <= 2-entry level the host reads is
// untouched). Same idea as folded_pos below.
__device__ __forceinline__ uint32_t level_pos(uint32_t e, uint32_t len) {
    return (e | 511u) < len ? ((e & ~511u) | ((e & 7u) << 6) | ((e >> 3) & 63u)) : e;
}

// ================================================================ first layer
// Per (chip, interaction): program words in device memory, column-major traces. The words are the host's form of one
// interaction of sp1_amd/air.py's InteractionProgram with everything that does not depend on the row folded in once the
// challenges are known: [is_send, n, head[4], vcol(multiplicity), n x (beta index, vcol(value))] — head = alpha + beta_0 kind +
// sum over the CONSTANT values c_j of beta_(1+j) c_j (a third of a core shard's message words are constants: byte opcodes, the
// 16 of a range check, zero operands), the n remaining values name their beta.
struct IntDesc {
    const uint32_t* prog;      // this interaction's words
    const uint32_t* main;      // column-major [main_w][rows]
    const uint32_t* prep;
    uint32_t rows;
    uint32_t* n_out;           // base numerators [rows]
    Ext* d_out;                // ext denominators [rows]
};

typedef const uint32_t __attribute__((address_space(4)))* prog_words_t;      // interaction programs: wave-uniform, read-only -> scalar loads
__device__ __forceinline__ uint32_t vcol_apply(prog_words_t& p, const IntDesc& d, uint32_t r) {
    const uint32_t nt = p[0];
    uint32_t acc = p[1];                                   // constant (Montgomery)
    p += 2;
    for (uint32_t t = 0; t < nt; t++, p += 3) {
        const uint32_t* col = (p[0] ? d.main : d.prep) + (size_t)p[1] * d.rows;
        const uint32_t v = gptr(col)[r], wgt = p[2];             // most weights are one (a wave-uniform test): no product then
        acc = kb::add(acc, wgt == kb::R1 ? v : kb::mul(v, wgt));
    }
    return acc;
}

// betas: [n_betas] ext (partial Lagrange of beta_seed)
__global__ __launch_bounds__(256) void first_layer_kernel(const IntDesc* __restrict__ descs, const Ext* __restrict__ betas) {
    const IntDesc d = descs[blockIdx.y];
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < d.rows; r += gridDim.x * blockDim.x) {
        prog_words_t p = (prog_words_t)(uintptr_t)d.prog;
        const bool is_send = p[0] != 0;
        const uint32_t nv = p[1];
        Ext den{{p[2], p[3], p[4], p[5]}};                 // head (see above)
        p += 6;
        uint32_t m = vcol_apply(p, d, r);
        if (!is_send) m = kb::sub(0u, m);
        for (uint32_t j = 0; j < nv; j++) {
            const uint32_t bi = *p++;
            den = kb::ext_add(den, kb::ext_mul_base(ld_ext(betas, bi), vcol_apply(p, d, r)));
        }
        const uint32_t rp = level_pos(r, d.rows);
        gptr(d.n_out)[rp] = m;
        st_ext(d.d_out, rp, den);
    }
}

// ================================================================ fraction tree
struct TransDesc {
    const void* n_in;          // base (level L) or ext
    const Ext* d_in;
    Ext* n_out;
    Ext* d_out;
    uint32_t rows_in;
};

template <bool NBASE>
__device__ __forceinline__ Ext load_n(const void* p, uint32_t i) {
    if (NBASE) return kb::ext_from_base(gptr((const uint32_t*)p)[i]);
    return ld_ext((const Ext*)p, i);
}

template <bool NBASE>
__global__ __launch_bounds__(256) void transition_kernel(const TransDesc* __restrict__ descs) {
    const TransDesc d = descs[blockIdx.y];
    const uint32_t rows_out = (d.rows_in + 1) / 2;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < rows_out; r += gridDim.x * blockDim.x) {
        const uint32_t ia = level_pos(2 * r, d.rows_in), ib = level_pos(2 * r + 1, d.rows_in), io = level_pos(r, rows_out);
        const Ext da = ld_ext(d.d_in, ia);
        if (2 * r + 1 < d.rows_in) {
            const Ext db = ld_ext(d.d_in, ib);
            Ext n;
            if (NBASE) {
                const uint32_t na = gptr((const uint32_t*)d.n_in)[ia], nb = gptr((const uint32_t*)d.n_in)[ib];
                n = kb::ext_add(kb::ext_mul_base(db, na), kb::ext_mul_base(da, nb));
            } else {
                n = kb::ext_add(kb::ext_mul(db, load_n<false>(d.n_in, ia)), kb::ext_mul(da, load_n<false>(d.n_in, ib)));
            }
            st_ext(d.n_out, io, n);
            st_ext(d.d_out, io, kb::ext_mul(da, db));
        } else {                                           // partner is a padding row: (0, 1)
            st_ext(d.n_out, io, load_n<NBASE>(d.n_in, ia));
            st_ext(d.d_out, io, da);
        }
    }
}

// ---- the first layer and the two tree levels below it in ONE pass over the traces (round 6). A lane owns FOUR consecutive
// rows of one interaction: it evaluates their fractions (level L), combines them in pairs (level L - 1) and the pairs again
// (level L - 2) in registers and stores all three levels — level L is never read back to build the tree (20 B per entry) and
// level L - 1 (32 B per entry pair) neither: 44 B per first-layer entry move where first_layer_kernel + two transition
// launches moved 80. Column reads are one 16 B load per lane and term (rows % 4 == 0: every table this library's tracers
// make), 1 KiB per wave instruction. Same field operations in the same order as the separate kernels: bit-identical levels.
struct FirstDesc {
    const uint32_t* prog;      // this interaction's words
    const uint32_t* main;      // column-major [main_w][rows]
    const uint32_t* prep;
    uint32_t rows;
    uint32_t* n0_out;          // level L: base numerators [rows]
    Ext* d0_out;               //          ext denominators [rows]
    Ext* n1_out; Ext* d1_out;  // level L - 1 [ceil(rows / 2)]
    Ext* n2_out; Ext* d2_out;  // level L - 2 [ceil(rows / 4)]
};

// vcol over rows 4 q .. 4 q + 3 (rows >= 4 q + 1; lanes past the table's end hold zeros)
__device__ __forceinline__ void vcol_apply4(prog_words_t& p, const FirstDesc& d, uint32_t q, bool vec, uint32_t (&out)[4]) {
    const uint32_t nt = p[0], c0 = p[1];
    p += 2;
#pragma unroll
    for (int j = 0; j < 4; j++) out[j] = c0;
    for (uint32_t t = 0; t < nt; t++, p += 3) {
        const uint32_t* col = (p[0] ? d.main : d.prep) + (size_t)p[1] * d.rows;
        const uint32_t wgt = p[2];
        uint32_t v[4];
        if (vec) {
            const q4_t x = gptr(reinterpret_cast<const q4_t*>(col))[q];
            v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
        } else {
#pragma unroll
            for (int j = 0; j < 4; j++) v[j] = 4 * q + j < d.rows ? gptr(col)[4 * q + j] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 4; j++) out[j] = kb::add(out[j], wgt == kb::R1 ? v[j] : kb::mul(v[j], wgt));
    }
}

__global__ __launch_bounds__(256) void first_layers_kernel(const FirstDesc* __restrict__ descs, const Ext* __restrict__ betas) {
    const FirstDesc d = descs[blockIdx.y];
    const uint32_t quads = (d.rows + 3) / 4, rows1 = (d.rows + 1) / 2, rows2 = (rows1 + 1) / 2;
    const bool vec = (d.rows & 3u) == 0;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += gridDim.x * blockDim.x) {
        prog_words_t p = (prog_words_t)(uintptr_t)d.prog;
        const bool is_send = p[0] != 0;
        const uint32_t nv = p[1];
        const Ext head{{p[2], p[3], p[4], p[5]}};
        p += 6;
        uint32_t m[4], val[4];
        vcol_apply4(p, d, q, vec, m);
        Ext den[4];
#pragma unroll
        for (int j = 0; j < 4; j++) { if (!is_send) m[j] = kb::sub(0u, m[j]); den[j] = head; }
        // den += sum_k beta_k value_k with delayed reduction: the four products of a coefficient ride one 64-bit accumulator
        // (4 (p - 1)^2 < 2^64 - 2^58, kb::monty_reduce_wide) — 4 wide multiply-adds per value and row and one reduction per
        // four values, where ext_mul_base + ext_add is four reductions and four modular additions per value
        uint64_t acc[4][4];
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[j][c] = 0;
        uint32_t pending = 0;
        for (uint32_t k = 0; k < nv; k++) {
            const uint32_t bi = *p++;
            vcol_apply4(p, d, q, vec, val);
            const Ext b = ld_ext(betas, bi);
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int c = 0; c < 4; c++) acc[j][c] += (uint64_t)b.c[c] * val[j];
            if (++pending == 4 || k + 1 == nv) {
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int c = 0; c < 4; c++) { den[j].c[c] = kb::add(den[j].c[c], kb::monty_reduce_wide(acc[j][c])); acc[j][c] = 0; }
                pending = 0;
            }
        }
        const uint32_t live = min(4u, d.rows - 4 * q);     // rows of this quad that exist
#pragma unroll
        for (int j = 0; j < 4; j++)
            if ((uint32_t)j < live) {
                const uint32_t rp = level_pos(4 * q + j, d.rows);
                gptr(d.n0_out)[rp] = m[j];
                st_ext(d.d0_out, rp, den[j]);
            }
        // level L - 1: rows 2 q, 2 q + 1 (transition_kernel<true>: a missing partner is the padding fraction (0, 1))
        Ext n1[2], d1[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if ((uint32_t)(2 * h + 1) < live) {
                n1[h] = kb::ext_add(kb::ext_mul_base(den[2 * h + 1], m[2 * h]), kb::ext_mul_base(den[2 * h], m[2 * h + 1]));
                d1[h] = kb::ext_mul(den[2 * h], den[2 * h + 1]);
            } else { n1[h] = kb::ext_from_base(m[2 * h]); d1[h] = den[2 * h]; }
            if ((uint32_t)(2 * h) < live) {
                const uint32_t io = level_pos(2 * q + h, rows1);
                st_ext(d.n1_out, io, n1[h]); st_ext(d.d1_out, io, d1[h]);
            }
        }
        // level L - 2: row q (transition_kernel<false>)
        const uint32_t io = level_pos(q, rows2);
        if (live > 2) {
            st_ext(d.n2_out, io, kb::ext_add(kb::ext_mul(d1[1], n1[0]), kb::ext_mul(d1[0], n1[1])));
            st_ext(d.d2_out, io, kb::ext_mul(d1[0], d1[1]));
        } else { st_ext(d.n2_out, io, n1[0]); st_ext(d.d2_out, io, d1[0]); }
    }
}

// Two tree levels per launch below that: a lane reads four entries of level l, stores two of level l - 1 and one of l - 2.
struct Trans2Desc {
    const Ext* n_in; const Ext* d_in;
    Ext* n1_out; Ext* d1_out; Ext* n2_out; Ext* d2_out;
    uint32_t rows_in;
};
__global__ __launch_bounds__(256) void transition2_kernel(const Trans2Desc* __restrict__ descs) {
    const Trans2Desc d = descs[blockIdx.y];
    const uint32_t quads = (d.rows_in + 3) / 4, rows1 = (d.rows_in + 1) / 2, rows2 = (rows1 + 1) / 2;
    for (uint32_t q = blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += gridDim.x * blockDim.x) {
        const uint32_t live = min(4u, d.rows_in - 4 * q);
        Ext n[4], dd[4];
#pragma unroll
        for (int j = 0; j < 4; j++)
            if ((uint32_t)j < live) { const uint32_t ip = level_pos(4 * q + j, d.rows_in); n[j] = ld_ext(d.n_in, ip); dd[j] = ld_ext(d.d_in, ip); }
        Ext n1[2], d1[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            if ((uint32_t)(2 * h + 1) < live) {
                n1[h] = kb::ext_add(kb::ext_mul(dd[2 * h + 1], n[2 * h]), kb::ext_mul(dd[2 * h], n[2 * h + 1]));
                d1[h] = kb::ext_mul(dd[2 * h], dd[2 * h + 1]);
            } else if ((uint32_t)(2 * h) < live) { n1[h] = n[2 * h]; d1[h] = dd[2 * h]; }
            if ((uint32_t)(2 * h) < live) {
                const uint32_t io = level_pos(2 * q + h, rows1);
                st_ext(d.n1_out, io, n1[h]); st_ext(d.d1_out, io, d1[h]);
            }
        }
        const uint32_t io = level_pos(q, rows2);
        if (live > 2) {
            st_ext(d.n2_out, io, kb::ext_add(kb::ext_mul(d1[1], n1[0]), kb::ext_mul(d1[0], n1[1])));
            st_ext(d.d2_out, io, kb::ext_mul(d1[0], d1[1]));
        } else { st_ext(d.n2_out, io, n1[0]); st_ext(d.d2_out, io, d1[0]); }
    }
}

// ================================================================ eq tables of one layer
// out holds, for t = 0 .. v, the partial-Lagrange table of the first t coordinates of `pt` at offset 2^t - 1... i.e.
// table t occupies [2^t - 1, 2^(t+1) - 1). Thread g -> (t, i).
struct PointArg { Ext c[32]; };
// out2 = lambda * out: the sums weigh a row's numerators with lambda T and its denominators with T (gkr_pass), so that
// lambda costs no product of its own
// (eq_layer_tables_kernel below builds both: the row prefix tables T / lambda T, and the partial-Lagrange table of ALL
// coordinates of the interaction point — on the device, so that a layer starts without a host-built table and its upload
// on the critical path; the host builds its own copy of every prefix table for the interaction-variable rounds WHILE the
// device runs the row rounds)
// Both tables of a layer in ONE launch (a launch call is ~4.7 us of host time on the layer's critical path): workgroups
// [0, full_blocks) build the interaction table, the rest the row prefix tables.
__global__ __launch_bounds__(256) void eq_layer_tables_kernel(PointArg pi, int niv, Ext* __restrict__ eq_int, uint32_t full_blocks,
                                                              PointArg pa, int v, Ext lambda, Ext* __restrict__ T, Ext* __restrict__ TL) {
    if (blockIdx.x < full_blocks) {
        const uint32_t i = blockIdx.x * 256u + threadIdx.x;
        if (i >= (1u << niv)) return;
        Ext acc = kb::ext_one();
        for (int j = 0; j < niv; j++) {
            const bool bit = (i >> (niv - 1 - j)) & 1u;
            acc = kb::ext_mul(acc, bit ? pi.c[j] : kb::ext_sub(kb::ext_one(), pi.c[j]));
        }
        st_ext(eq_int, i, acc);
        return;
    }
    const uint32_t g = (blockIdx.x - full_blocks) * 256u + threadIdx.x + 1;       // 1 .. 2^(v+1) - 1
    if (g >= (2u << v)) return;
    const int t = 31 - __clz(g);
    const uint32_t i = g - (1u << t);
    Ext acc = kb::ext_one();
    for (int j = 0; j < t; j++) {
        const bool bit = (i >> (t - 1 - j)) & 1u;
        acc = kb::ext_mul(acc, bit ? pa.c[j] : kb::ext_sub(kb::ext_one(), pa.c[j]));
    }
    st_ext(T, g - 1, acc);
    st_ext(TL, g - 1, kb::ext_mul(acc, lambda));
}

// ================================================================ sumcheck over the row variables: two rounds per pass
// A layer's sumcheck  sum_x eq(pt, x) F(x),  F = lambda (n0 d1 + n1 d0) + d0 d1,  binds the row variables last-first.
// One PASS over the tables serves TWO rounds (the reference's look-ahead, /root/reference/sp1-gpu/crates/sys/lib/logup_gkr/
// lookahead.cu:L44-L141, on a different grid and a different work split). With X the last row variable, Y the one before it
// and q the remaining bits of a row index, the four rows 4q .. 4q+3 of a table are its values at (Y, X) in {0,1}^2, every
// table is bilinear in (X, Y) there and F is multi-quadratic, so
//      G(X, Y) = sum_q eq(pt'', q) F_q(X, Y)            (9 coefficients)
// is known from its values on the grid {0, 1, inf}^2 — "inf" = the leading coefficient, i.e. F evaluated on the DIFFERENCES
// of the rows, so the grid costs additions only. The host then has both rounds in closed form, no interpolation and no
// inversion:    p_a(X) = PA eq(pt_a, X) ((1 - pt_b) G(X, 0) + pt_b G(X, 1)),    p_b(Y) = PA eq(pt_a, alpha_a) eq(pt_b, Y) G(alpha_a, Y).
// The next pass folds with BOTH challenges while it loads (rows 4r .. 4r+3 -> row r; the half-folded layer is never
// written) and accumulates the grid of the following two rounds from the folded rows in registers. A layer of v row
// variables is 1 + ceil(v / 2) launches and hand-overs instead of v + 1, and every table is read once per TWO rounds.
// (The tail of a layer — FLAT launches, latency and not work — goes further: up to four rounds per pass, "deep passes" below.
// What is said here holds for every tiled pass and for the flat passes that sum and fold at most two rounds.)
//
// Work split: one LANE per OUTPUT ROW — the fold is embarrassingly parallel, every load is a coalesced 16 B / lane run in
// the existing lane-blocked layouts (a lane reads 4 input rows = what one lane of the one-round kernels read), and the
// register footprint is one row, not one quad. The four rows of a grid cell then sit in the four lanes of a DPP quad:
//   * the pure points (0,0), (1,0), (0,1), (1,1) are the rows themselves: lane j evaluates F on its own row;
//   * a difference point needs F on a difference of two rows = B_D d0_D + A_D d1_D: two products, split over the two lanes of
//     the pair (one takes B d0, the other A d1; the sign of a difference cancels in the product), operands by quad_perm;
//   * (inf, inf) is the difference of the differences.
// 7 extension products per row (2 to weigh the row, 2 + 1 + 1 + 1 for the grid) against 6.5 for a lane-per-quad split, and
// lane j's accumulators mean different grid points for different j: they are separated by class (lane mod 4) once, at the
// end of the kernel, into the 10 sums the host wants.
// lambda rides on the eq weight: with w = eq weight of the cell and wl = lambda w (a second table, built with the first),
// F w = (wl n1) d0 + (wl n0 + w d0) d1 is three products per row to form B = wl n1 and A = wl n0 + w d0 and then two per
// grid point instead of four (and on the top layer, whose numerators are base-field words, wl n is four base products).
// Padding rows are the constants (0, 1): F = 1 on every padding cell and the cells' eq mass is 1 - (mass of the real cells),
// as in the one-round kernels (`eq_correction_term`, logup_poly.rs:L521-L530).
struct PassDesc {
    const void* src[4];        // FIRST: {level N, level D, -, -} (row r = entries 2r, 2r+1); else {n0, d0, n1, d1}
    Ext* dst[4];               // folded n0, d0, n1, d1
    uint32_t rows_in;          // real rows of the layer before this pass folds (FIRST: ceil(rows_x / 2))
    uint32_t rows_x;           // FIRST only: real entries of the level
    uint32_t eq_int_index;     // global interaction index
    uint32_t tile0;            // tiled launch: first workgroup of this interaction; FLAT: first lane slot
};

// workgroup -> (interaction, range of its rows): the interactions differ by orders of magnitude in height, so the
// launch is a flat list of equally sized tiles; descs[].tile0 is ascending
__device__ __forceinline__ uint32_t find_desc(const PassDesc* __restrict__ descs, uint32_t K, uint32_t b) {
    uint32_t lo = 0, hi = K;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (descs[mid].tile0 <= b) lo = mid; else hi = mid;
    }
    return lo;
}
struct Row { Ext n0, d0, n1, d1; };

// Layout of the folded tables in scratch: a lane of the next pass wants rows 4k .. 4k+3 of each table, i.e. 64 B at a
// 64 B lane stride — every load instruction of a wave would touch 32 cache lines for 1 KiB (measured: the L1/TA rate
// co-bounds the large rounds with the VALUs; with coalesced addresses the same kernel runs 25 % faster). So inside every
// complete block of 256 rows, row r lives at (r mod 4) * 64 + (r div 4) mod 64: the four loads of a wave are four
// contiguous 1 KiB runs, and the stores of the producing pass (one row per lane) are four 256 B runs each. The
// last (incomplete) block of a table keeps the natural order, so tables never grow and short tables (what the host
// fetches after the last fold) are untouched.
__device__ __forceinline__ uint32_t folded_pos(uint32_t r, uint32_t len) {
    return (r | 255u) < len ? ((r & ~255u) | ((r & 3u) << 6) | ((r >> 2) & 63u)) : r;
}

__device__ __forceinline__ Row padding_row() { return Row{kb::ext_zero(), kb::ext_one(), kb::ext_zero(), kb::ext_one()}; }

// row r of the layer as this pass finds it (before its fold)
template <bool FIRST, bool NBASE>
__device__ __forceinline__ Row load_row(const PassDesc& d, uint32_t r) {
    Row q = padding_row();
    if (r >= d.rows_in) return q;
    if (FIRST) {
        const uint32_t ea = level_pos(2 * r, d.rows_x), eb = level_pos(2 * r + 1, d.rows_x);
        q.n0 = load_n<NBASE>(d.src[0], ea);
        q.d0 = ld_ext((const Ext*)d.src[1], ea);
        if (2 * r + 1 < d.rows_x) { q.n1 = load_n<NBASE>(d.src[0], eb); q.d1 = ld_ext((const Ext*)d.src[1], eb); }
    } else {
        const uint32_t rp = folded_pos(r, d.rows_in);
        q.n0 = ld_ext((const Ext*)d.src[0], rp); q.d0 = ld_ext((const Ext*)d.src[1], rp);
        q.n1 = ld_ext((const Ext*)d.src[2], rp); q.d1 = ld_ext((const Ext*)d.src[3], rp);
    }
    return q;
}

__device__ __forceinline__ Ext lerp(const Ext& a, const Ext& b, const Ext& t) { return kb::ext_add(a, kb::ext_mul(kb::ext_sub(b, a), t)); }   // t: the round's challenge (wave-uniform, second)
__device__ __forceinline__ Row lerp_row(const Row& a, const Row& b, const Ext& t) {
    return Row{lerp(a.n0, b.n0, t), lerp(a.d0, b.d0, t), lerp(a.n1, b.n1, t), lerp(a.d1, b.d1, t)};
}
// the same when the numerators are base-field words (coordinate 0 only): a + t (b - a) is four base products
__device__ __forceinline__ Ext lerp_base(uint32_t a, uint32_t b, const Ext& t) {
    Ext e = kb::ext_mul_base(t, kb::sub(b, a));
    e.c[0] = kb::add(e.c[0], a);
    return e;
}
template <bool NBASE>
__device__ __forceinline__ Row lerp_row_in(const Row& a, const Row& b, const Ext& t) {
    if (!NBASE) return lerp_row(a, b, t);
    return Row{lerp_base(a.n0.c[0], b.n0.c[0], t), lerp(a.d0, b.d0, t), lerp_base(a.n1.c[0], b.n1.c[0], t), lerp(a.d1, b.d1, t)};
}

// output row `ro` of a pass that binds FV variables: rows ro 2^FV .. of the input folded with a0 (last variable), then a1
template <int FV, bool FIRST, bool NBASE>
__device__ __forceinline__ Row fold_row(const PassDesc& d, uint32_t ro, const Ext& a0, const Ext& a1) {
    if constexpr (FV == 0) return load_row<FIRST, NBASE>(d, ro);
    Row in[FV == 0 ? 1 : (1 << FV)];
    // every load of the row is issued before the first use: one exposed memory latency per row
#pragma unroll
    for (int j = 0; j < (1 << FV); j++) in[j] = load_row<FIRST, NBASE>(d, (ro << FV) + j);
    if constexpr (FV == 1) return lerp_row_in<NBASE>(in[0], in[1], a0);
    else {
        const Row lo = lerp_row_in<NBASE>(in[0], in[1], a0), hi = lerp_row_in<NBASE>(in[2], in[3], a0);
        return lerp_row(lo, hi, a1);
    }
}

template <int CTRL>
__device__ __forceinline__ Ext dpp_ext(const Ext& e) {
    return Ext{{p2::dpp_mov<CTRL>(e.c[0]), p2::dpp_mov<CTRL>(e.c[1]), p2::dpp_mov<CTRL>(e.c[2]), p2::dpp_mov<CTRL>(e.c[3])}};
}
__device__ __forceinline__ Ext sel_ext(bool c, const Ext& a, const Ext& b) {
    return Ext{{c ? a.c[0] : b.c[0], c ? a.c[1] : b.c[1], c ? a.c[2] : b.c[2], c ? a.c[3] : b.c[3]}};
}

// per-lane accumulators of a pass that sums SV rounds: what each one means depends on the lane's class (lane mod 2^SV)
template <int SV> struct GridAcc { Ext a[SV == 2 ? 5 : 3]; };
template <int SV>
__device__ __forceinline__ void grid_init(GridAcc<SV>& g) {
#pragma unroll
    for (int i = 0; i < (SV == 2 ? 5 : 3); i++) g.a[i] = kb::ext_zero();
}

// row = this lane's (folded) row; w = eq weight of its cell (zero for lanes past the last real cell), wl = lambda w;
// j = lane's position inside the cell. ALL lanes of the cell must be active. NB: the numerators are base-field words.
template <int SV, bool NB>
__device__ __forceinline__ void grid_accumulate(const Row& row, const Ext& w, const Ext& wl, uint32_t j, GridAcc<SV>& g) {
    const Ext A = kb::ext_add(NB ? kb::ext_mul_base(wl, row.n0.c[0]) : kb::ext_mul(row.n0, wl), kb::ext_mul(row.d0, w));
    const Ext B = NB ? kb::ext_mul_base(wl, row.n1.c[0]) : kb::ext_mul(row.n1, wl);
    g.a[0] = kb::ext_add(g.a[0], kb::ext_add(kb::ext_mul(B, row.d0), kb::ext_mul(A, row.d1)));       // the pure point of this lane
    // difference over the last variable (lanes j ^ 1): the even lane takes B d0, the odd lane A d1 — so every lane KEEPS one
    // pair of operands and SENDS the other pair, the one its partner works on
    const bool lo1 = (j & 1u) == 0;
    const Ext P = sel_ext(lo1, B, A), Q = sel_ext(lo1, row.d0, row.d1), PS = sel_ext(lo1, A, B), QS = sel_ext(lo1, row.d1, row.d0);
    const Ext DP = kb::ext_sub(P, dpp_ext<p2::DPP_QUAD_SWAP1>(PS)), DQ = kb::ext_sub(Q, dpp_ext<p2::DPP_QUAD_SWAP1>(QS));
    g.a[1] = kb::ext_add(g.a[1], kb::ext_mul(DP, DQ));
    if constexpr (SV == 2) {
        // difference over the variable before it (lanes j ^ 2): lanes 0, 1 take B d0, lanes 2, 3 A d1
        const bool lo2 = (j & 2u) == 0;
        const Ext P2 = sel_ext(lo2, B, A), Q2 = sel_ext(lo2, row.d0, row.d1), PS2 = sel_ext(lo2, A, B), QS2 = sel_ext(lo2, row.d1, row.d0);
        const Ext EP = kb::ext_sub(P2, dpp_ext<p2::DPP_QUAD_SWAP2>(PS2)), EQ = kb::ext_sub(Q2, dpp_ext<p2::DPP_QUAD_SWAP2>(QS2));
        g.a[2] = kb::ext_add(g.a[2], kb::ext_mul(EP, EQ));
        // both: lanes j and j ^ 2 hold first differences of the SAME pair of tables (B d0 on lanes 0 / 2, A d1 on 1 / 3), so
        // their difference is the mixed one; computed twice, counted once below
        const Ext FP = kb::ext_sub(DP, dpp_ext<p2::DPP_QUAD_SWAP2>(DP)), FQ = kb::ext_sub(DQ, dpp_ext<p2::DPP_QUAD_SWAP2>(DQ));
        g.a[3] = kb::ext_add(g.a[3], kb::ext_mul(FP, FQ));
    }
    if (j == 0) g.a[SV == 2 ? 4 : 2] = kb::ext_add(g.a[SV == 2 ? 4 : 2], w);                          // eq mass of the real cells
}

// SV = 2: G00 G10 G01 G11 | Gi0 Gi1 | G0i G1i | Gii | Seq   (first index: X = last variable; i = "inf")
// SV = 1: G0 G1 | Gi | Seq
template <int SV> struct GridOut { static constexpr int NS = SV == 2 ? 10 : 4; };
template <int SV>
__device__ __forceinline__ void grid_split(const GridAcc<SV>& g, uint32_t j, const Ext& scale, bool use_scale, Ext (&out)[GridOut<SV>::NS]) {
    const Ext z = kb::ext_zero();
    Ext a[SV == 2 ? 5 : 3];
#pragma unroll
    for (int i = 0; i < (SV == 2 ? 5 : 3); i++) a[i] = use_scale ? kb::ext_mul(g.a[i], scale) : g.a[i];
    if constexpr (SV == 2) {
        out[0] = j == 0 ? a[0] : z; out[1] = j == 1 ? a[0] : z; out[2] = j == 2 ? a[0] : z; out[3] = j == 3 ? a[0] : z;
        out[4] = j < 2 ? a[1] : z; out[5] = j < 2 ? z : a[1];
        out[6] = (j & 1u) == 0 ? a[2] : z; out[7] = (j & 1u) == 0 ? z : a[2];
        out[8] = j < 2 ? a[3] : z;
        out[9] = a[4];
    } else {
        out[0] = j == 0 ? a[0] : z; out[1] = j == 1 ? a[0] : z;
        out[2] = a[1];
        out[3] = a[2];
    }
}

// Small passes (FLAT): most of a proof's passes have a handful of rows per interaction — one workgroup per interaction is
// then 730 workgroups of a few busy lanes each, and what the launch costs is the 730 tickets and partial sums of its tail.
// FLAT launches give every LANE one row instead: lane p of the launch looks its descriptor up in a host-built table
// (flat_index[p]; descs[].tile0 = first slot of the interaction, slots per interaction = rows rounded up to whole cells)
// and weighs its own row with its interaction's eq factor.
struct FlatArgs { const uint16_t* index; uint32_t total_slots; };

// One pass: bind FV variables (fold rows ro 2^FV .. with a0, a1 and store row ro; FV = 0: read only), then accumulate the
// grid of the next SV rounds (SV = 0: the layer's last fold, nothing to sum). T = partial-Lagrange table of the row
// variables that remain after those SV rounds, TL = lambda T.
template <int FV, int SV, bool FIRST, bool NBASE, bool FLAT>
__global__ __launch_bounds__(256) void gkr_pass(const PassDesc* __restrict__ descs, const Ext* __restrict__ eq_int,
                                                const Ext* __restrict__ T, const Ext* __restrict__ TL, Ext a0, Ext a1,
                                                uint32_t* __restrict__ partials, RoundSync rs, uint32_t seq, uint32_t K,
                                                uint32_t tile_size, FlatArgs fa) {
    static_assert(FV + SV > 0 && FV <= 2 && SV <= 2, "a pass folds and / or sums");
    constexpr int SVS = SV == 0 ? 1 : SV;                    // (types only; SV = 0 never touches the grid)
    GridAcc<SVS> g;
    grid_init<SVS>(g);
    const uint32_t j = threadIdx.x & ((1u << SV) - 1u);
    // one row: fold, store, weigh, accumulate. valid = the lane has a slot; rows past rows_out inside a real cell are padding
    // (a padding row's numerators are zero: also as base words)
    auto do_row = [&](const PassDesc& d, uint32_t ro, bool valid, const Ext& wi, bool use_wi) {
        const uint32_t rows_out = (d.rows_in + (1u << FV) - 1u) >> FV;
        Row row = padding_row();
        if (valid && ro < rows_out) {
            row = fold_row<FV, FIRST, NBASE>(d, ro, a0, a1);
            if (FV > 0) {
                const uint32_t rq = folded_pos(ro, rows_out);
                if (SV == 0 && rs.host_slot != nullptr) {    // the layer's last fold, published from this kernel (see the tail)
                    st_ext_host(d.dst[0], rq, row.n0); st_ext_host(d.dst[1], rq, row.d0); st_ext_host(d.dst[2], rq, row.n1); st_ext_host(d.dst[3], rq, row.d1);
                } else {
                    st_ext(d.dst[0], rq, row.n0); st_ext(d.dst[1], rq, row.d0); st_ext(d.dst[2], rq, row.n1); st_ext(d.dst[3], rq, row.d1);
                }
            }
        }
        if constexpr (SV > 0) {
            const uint32_t cells = (rows_out + (1u << SV) - 1u) >> SV;
            const uint32_t c = ro >> SV;
            Ext w = kb::ext_zero(), wl = kb::ext_zero();
            if (valid && c < cells) {
                w = ld_ext(T, c); wl = ld_ext(TL, c);
                if (use_wi) { w = kb::ext_mul(w, wi); wl = kb::ext_mul(wl, wi); }
            }
            grid_accumulate<SVS, FIRST && NBASE && FV == 0>(row, w, wl, j, g);
        }
    };
    Ext scale = kb::ext_one();
    if (FLAT) {
        const uint32_t p = blockIdx.x * 256 + threadIdx.x;
        const bool valid = p < fa.total_slots;               // slots come in whole cells: a cell's lanes are valid together
        const PassDesc d = descs[valid ? fa.index[p] : 0];
        const Ext wi = SV > 0 ? ld_ext(eq_int, d.eq_int_index) : kb::ext_one();
        do_row(d, p - d.tile0, valid, wi, true);
    } else {
        const PassDesc d = descs[find_desc(descs, K, blockIdx.x)];
        const uint32_t rows_out = (d.rows_in + (1u << FV) - 1u) >> FV;
        const uint32_t slots = ((rows_out + (1u << SV) - 1u) >> SV) << SV;
        const uint32_t k0 = (blockIdx.x - d.tile0) * tile_size, k1 = min(slots, k0 + tile_size);
        // every lane runs every iteration (the grid exchanges rows between the lanes of a cell)
        for (uint32_t base = k0; base < k1; base += 256) do_row(d, base + threadIdx.x, base + threadIdx.x < k1, scale, false);
        if (SV > 0) scale = ld_ext(eq_int, d.eq_int_index);
    }
    if constexpr (SV > 0) {
        Ext out[GridOut<SVS>::NS];
        grid_split<SVS>(g, j, scale, !FLAT, out);
        rs_finish<GridOut<SVS>::NS>(out, partials, blockIdx.x, gridDim.x, rs, seq);
    } else if (rs.host_slot != nullptr) {
        // The layer's last fold stores its rows (one per interaction) STRAIGHT into the mapped host slot — the descriptors'
        // dst pointers point there — and the workgroup that arrives last publishes the sequence number: the host had been
        // waiting for a one-workgroup copy kernel behind this one (45 us for 46 KB of 4-byte uncached stores, once per layer).
        // Same ordering argument as rs_finish: system-scope stores to fine-grained host memory that the wave has been
        // acknowledged (vmcnt) are visible to the host, and the ticket orders the last workgroup's store behind everybody's.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x == 0 && rs_ticket_is_last_acq_rel(rs.counter, blockIdx.x, gridDim.x)) rs_publish_seq(rs.host_slot, seq);
    }
}

// ================================================================ deep passes: up to four rounds per pass in the FLAT launches
// Most launches of a proof are FLAT passes of a few busy lanes, and such a pass costs one latency chain — descriptor, rows, eq,
// products, reduction, ticket, publish, host wake-up, transcript, next launch — whatever it computes. The only way to shorten a
// layer's tail is fewer passes: the same identity as above holds for the last k unbound variables, G(X_1 .. X_k) is
// multi-quadratic and known from its values on {0, 1, inf}^k (3^k sums; gkr_rounds_host.hpp turns them into k round
// polynomials), and the next pass folds 2^k rows per output row with the k challenges. gkr_pass_deep is that pass for FV or
// SV in {3, 4}, FLAT only (plan_passes emits it where the slots, in whole cells of 2^SV rows, fit a flat launch); the tiled
// passes and every two-round flat pass stay gkr_pass, instruction for instruction.
//
// Fold: 2^FV input rows per output row as a binary tree (bit j of the input row index is the variable bound by challenge j),
// fully unrolled and without a branch per row, so the loads are issued as early as the registers allow. FV = 2: a lane per
// output row as in gkr_pass; FV = 3, 4 (gkr_pass_deep_fold): a lane per output row AND table.
// Grid, SV >= 3: with w the cell's eq weight, F w = B d0 + A d1 (A = wl n0 + w d0, B = wl n1, as in grid_accumulate) and all
// four of A, B, d0, d1 are multilinear in the cell's variables, so F w at a grid point is B_g d0_g + A_g d1_g with X_g the signed
// sum of table X over the rows the point selects: axis at 0 / 1 fixes the row bit, axis at inf takes (bit 1) - (bit 0). The
// cell's rows go to LDS once (row-major over the cells, so that lanes which work on the same point of neighbouring cells read
// consecutive 16 B), then one (point, cell) pair per lane and step: 2^(number of inf axes) rows per table, two products. The
// sign common to the four sums cancels in the products. The 256 >> SV cells of a point sit in consecutive lanes and are summed
// by shuffles; the workgroup's 3^SV + 1 sums (the last is the eq mass of its real cells) meet in LDS and leave through
// rs_finish_block_sums. Dependent steps on the critical chain: one LDS round trip, <= 2^SV adds per table, two products, log2
// (256 >> SV) shuffles — against 7 products and the DPP exchanges of a two-round pass.
struct DeepChallenges { Ext a[4]; };

// load_row without a branch: a row past the table's end reads the last real row (rows_in >= 1) and is replaced by the padding
// fraction afterwards — the 2^FV rows of a deep fold are 4 .. 8 loads each, and behind a branch per row every one of them would
// expose its own memory latency; like this all of them are in flight before the first use
template <bool FIRST, bool NBASE>
__device__ __forceinline__ Row load_row_select(const PassDesc& d, uint32_t r) {
    const bool live = r < d.rows_in;
    const uint32_t rc = live ? r : d.rows_in - 1;
    const Ext zero = kb::ext_zero(), one = kb::ext_one();
    Row q;
    bool live1 = live;
    if (FIRST) {
        const bool has1 = 2 * rc + 1 < d.rows_x;
        const uint32_t ea = level_pos(2 * rc, d.rows_x), eb = level_pos(has1 ? 2 * rc + 1 : 2 * rc, d.rows_x);
        q.n0 = load_n<NBASE>(d.src[0], ea); q.d0 = ld_ext((const Ext*)d.src[1], ea);
        q.n1 = load_n<NBASE>(d.src[0], eb); q.d1 = ld_ext((const Ext*)d.src[1], eb);
        live1 = live && has1;
    } else {
        const uint32_t rp = folded_pos(rc, d.rows_in);
        q.n0 = ld_ext((const Ext*)d.src[0], rp); q.d0 = ld_ext((const Ext*)d.src[1], rp);
        q.n1 = ld_ext((const Ext*)d.src[2], rp); q.d1 = ld_ext((const Ext*)d.src[3], rp);
    }
    return Row{sel_ext(live, q.n0, zero), sel_ext(live, q.d0, one), sel_ext(live1, q.n1, zero), sel_ext(live1, q.d1, one)};
}

// the (point, cell) steps of a deep grid take the points in the order of their number of inf axes, so that the lanes of a wave
// (64 / CELLS neighbouring points) add up the same number of rows: entry = point | rows fixed at one << 7 | inf axes << 11
template <int SV> struct DeepPoints {
    uint16_t e[81];
    constexpr DeepPoints() : e{} {
        int n = 0, np = 1;
        for (int j = 0; j < SV; j++) np *= 3;
        for (int m = 0; m <= SV; m++)
            for (int p = 0; p < np; p++) {
                int base = 0, inf = 0, cnt = 0;
                for (int a = 0, x = p; a < SV; a++, x /= 3) { base |= (x % 3 == 1) << a; inf |= (x % 3 == 2) << a; cnt += x % 3 == 2; }
                if (cnt == m) e[n++] = (uint16_t)(p | base << 7 | inf << 11);
            }
    }
};
template <int SV> __device__ const DeepPoints<SV> deep_points_table{};

template <int LV, bool FIRST, bool NBASE>
__device__ __forceinline__ Row fold_rows_deep(const PassDesc& d, uint32_t r0, const DeepChallenges& ch) {
    if constexpr (LV == 0) return load_row_select<FIRST, NBASE>(d, r0);
    else {
        const Row lo = fold_rows_deep<LV - 1, FIRST, NBASE>(d, r0, ch), hi = fold_rows_deep<LV - 1, FIRST, NBASE>(d, r0 + (1u << (LV - 1)), ch);
        if constexpr (LV == 1) return lerp_row_in<NBASE>(lo, hi, ch.a[0]);
        else return lerp_row(lo, hi, ch.a[LV - 1]);
    }
}

constexpr int deep_points(int sv) { int n = 1; for (int j = 0; j < sv; j++) n *= 3; return n; }
// sums a pass hands over: the two-round forms' 4 / 10 (GridOut), a deep grid's 3^SV + 1 (the same counts at SV = 1, 2)
constexpr int pass_sums(int sv) { return sv == 0 ? 0 : deep_points(sv) + 1; }

// The grid of a deep pass from LDS. The workgroup holds 256 / LPR rows (LPR lanes per row), i.e. CELLS = 256 / LPR >> SV whole
// cells. Every lane hands in the values it owns of row `row` (tables: [0] + [1] = A, [2] = B, [3] = d0, [4] = d1; bit t of
// `owns`), the lane that owns a cell's first row its eq weight; then one (point, cell) pair per lane and step, the cells of a
// point summed by shuffles, and the workgroup's 3^SV + 1 sums leave through rs_finish_block_sums.
template <int SV, int LPR>
__device__ __forceinline__ void deep_grid_finish(const Ext (&vals)[5], uint32_t owns, uint32_t row, bool owns_w, const Ext& w,
                                                 uint32_t* __restrict__ partials, RoundSync rs, uint32_t seq) {
    constexpr int CELLS = (256 / LPR) >> SV, ROWS = 1 << SV, NP = deep_points(SV), NS = NP + 1, STRIDE = CELLS + 1;
    constexpr int STEPS = (NS * CELLS + 255) / 256;
    static_assert(CELLS >= 1 && CELLS <= 32, "the cells of a point sit inside one wave");
    __shared__ Ext sm_row[5][ROWS * STRIDE];                 // at [row of the cell][cell]
    __shared__ Ext sm_w[CELLS];
    __shared__ uint32_t sm_sums[4 * NS];
    const uint32_t my = (row & (ROWS - 1u)) * STRIDE + (row >> SV);
#pragma unroll
    for (int t = LPR == 1 ? 1 : 0; t < 5; t++)
        if ((owns >> t) & 1u) sm_row[t][my] = vals[t];
    if (LPR == 1) sm_row[0][my] = vals[0];
    if (owns_w) sm_w[row >> SV] = w;
    __syncthreads();
#pragma unroll
    for (int step = 0; step < STEPS; step++) {
        const uint32_t id = step * 256 + threadIdx.x, slot = id / CELLS, cell = id % CELLS;
        uint32_t point = slot;                               // (slot NP: the eq mass)
        Ext v = kb::ext_zero();
        if (slot < (uint32_t)NP) {
            const uint32_t entry = deep_points_table<SV>.e[slot];
            point = entry & 127u;
            const uint32_t base = (entry >> 7) & 15u, inf = entry >> 11;   // row bits the point fixes at one; axes it takes the difference over
            Ext gA = kb::ext_zero(), gB = gA, g0 = gA, g1 = gA;
            uint32_t s = 0;
            do {                                             // the subsets s of inf: row base | s, sign (-1)^|s|
                const uint32_t at = (base | s) * STRIDE + cell;
                const Ext rA = LPR == 1 ? sm_row[0][at] : kb::ext_add(sm_row[0][at], sm_row[1][at]);
                if (__popc(s) & 1) { gA = kb::ext_sub(gA, rA); gB = kb::ext_sub(gB, sm_row[2][at]); g0 = kb::ext_sub(g0, sm_row[3][at]); g1 = kb::ext_sub(g1, sm_row[4][at]); }
                else { gA = kb::ext_add(gA, rA); gB = kb::ext_add(gB, sm_row[2][at]); g0 = kb::ext_add(g0, sm_row[3][at]); g1 = kb::ext_add(g1, sm_row[4][at]); }
                s = (s - inf) & inf;
            } while (s != 0);
            v = kb::ext_add(kb::ext_mul(gB, g0), kb::ext_mul(gA, g1));
        } else if (slot == (uint32_t)NP) v = sm_w[cell];
        // every lane of the wave takes part: the CELLS lanes of a point are consecutive and aligned
#pragma unroll
        for (int off = CELLS / 2; off >= 1; off >>= 1)
#pragma unroll
            for (int k = 0; k < 4; k++) v.c[k] = kb::add(v.c[k], __shfl_xor(v.c[k], off, 64));
        if (cell == 0 && slot < (uint32_t)NS)
#pragma unroll
            for (int k = 0; k < 4; k++) sm_sums[4 * point + k] = v.c[k];
    }
    __syncthreads();
    rs_finish_block_sums<NS>(sm_sums, partials, blockIdx.x, gridDim.x, rs, seq);
}

// FV in {0, 2}, SV in {3, 4}: one lane per output row (256 slots per workgroup), the fold of gkr_pass
template <int FV, int SV, bool FIRST, bool NBASE>
__global__ __launch_bounds__(256) void gkr_pass_deep(const PassDesc* __restrict__ descs, const Ext* __restrict__ eq_int,
                                                     const Ext* __restrict__ T, const Ext* __restrict__ TL, DeepChallenges ch,
                                                     uint32_t* __restrict__ partials, RoundSync rs, uint32_t seq, FlatArgs fa) {
    static_assert(FV <= 2 && SV > 2 && SV <= 4, "the two-round forms are gkr_pass, the deep folds gkr_pass_deep_fold");
    const uint32_t p = blockIdx.x * 256 + threadIdx.x;
    const bool valid = p < fa.total_slots;                   // slots come in whole cells: a cell's lanes are valid together
    const PassDesc d = descs[valid ? fa.index[p] : 0];
    const uint32_t ro = p - d.tile0;
    const uint32_t rows_out = (d.rows_in + (1u << FV) - 1u) >> FV;
    Row row = padding_row();                                 // rows past rows_out inside a real cell are padding
    if (valid && ro < rows_out) {
        row = fold_rows_deep<FV, FIRST, NBASE>(d, ro << FV, ch);
        if (FV > 0) {
            const uint32_t rq = folded_pos(ro, rows_out);
            st_ext(d.dst[0], rq, row.n0); st_ext(d.dst[1], rq, row.d0); st_ext(d.dst[2], rq, row.n1); st_ext(d.dst[3], rq, row.d1);
        }
    }
    const uint32_t cells = (rows_out + (1u << SV) - 1u) >> SV, c = ro >> SV;
    Ext w = kb::ext_zero(), wl = kb::ext_zero();             // zero for lanes past the last real cell
    if (valid && c < cells) {
        const Ext wi = ld_ext(eq_int, d.eq_int_index);
        w = kb::ext_mul(ld_ext(T, c), wi); wl = kb::ext_mul(ld_ext(TL, c), wi);
    }
    constexpr bool NB = FIRST && NBASE && FV == 0;           // the numerators are base-field words
    const Ext A = kb::ext_add(NB ? kb::ext_mul_base(wl, row.n0.c[0]) : kb::ext_mul(row.n0, wl), kb::ext_mul(row.d0, w));
    const Ext B = NB ? kb::ext_mul_base(wl, row.n1.c[0]) : kb::ext_mul(row.n1, wl);
    const Ext vals[5] = {A, kb::ext_zero(), B, row.d0, row.d1};
    deep_grid_finish<SV, 1>(vals, 0x1du, threadIdx.x, (threadIdx.x & ((1u << SV) - 1u)) == 0, w, partials, rs, seq);
}

// FV in {3, 4}: FOUR lanes per output row, lane q of the quad folds table q (n0, d0, n1, d1) alone. A deep fold is 2^FV - 1
// products per table, and with one lane per row the 60 products of FV = 4 were the pass (a wave per SIMD, most SIMDs of the
// device idle: (4, 4) measured 59 us against 27 for the same sums behind a two-round fold, and 24 like this); a quarter of that
// chain per lane, 64 slots per workgroup. The products that weigh the row go the same way — lane 0 wl n0, lane 1 w d0, lane 2 wl n1 — and A is summed
// where the grid is read. The sums come in grid order at every SV (the host reads them with row_rounds_from_grid).
template <int LV, bool FIRST, bool BASE>
__device__ __forceinline__ Ext fold_table_deep(const void* src, uint32_t q, uint32_t rows_in, uint32_t rows_x, uint32_t r0,
                                               const DeepChallenges& ch, const Ext& pad) {
    if constexpr (LV == 0) {
        bool live = r0 < rows_in;
        const uint32_t rc = live ? r0 : rows_in - 1;         // (rows_in >= 1: see load_row_select)
        uint32_t pos;
        if (FIRST) {                                         // row r = entries 2r, 2r + 1 of the level: lanes 0, 1 read the even one
            const uint32_t e = 2 * rc + (q >> 1);
            const bool has = e < rows_x;
            live = live && has;
            pos = level_pos(has ? e : 2 * rc, rows_x);
        } else pos = folded_pos(rc, rows_in);
        const Ext v = BASE ? kb::ext_from_base(gptr((const uint32_t*)src)[pos]) : ld_ext((const Ext*)src, pos);
        return sel_ext(live, v, pad);
    } else {
        const Ext lo = fold_table_deep<LV - 1, FIRST, BASE>(src, q, rows_in, rows_x, r0, ch, pad);
        const Ext hi = fold_table_deep<LV - 1, FIRST, BASE>(src, q, rows_in, rows_x, r0 + (1u << (LV - 1)), ch, pad);
        return lerp(lo, hi, ch.a[LV - 1]);
    }
}

template <int FV, int SV, bool FIRST, bool NBASE>
__global__ __launch_bounds__(256) void gkr_pass_deep_fold(const PassDesc* __restrict__ descs, const Ext* __restrict__ eq_int,
                                                          const Ext* __restrict__ T, const Ext* __restrict__ TL, DeepChallenges ch,
                                                          uint32_t* __restrict__ partials, RoundSync rs, uint32_t seq, FlatArgs fa) {
    static_assert(FV > 2 && FV <= 4 && SV <= 4, "the shallower folds are gkr_pass and gkr_pass_deep");
    const uint32_t q = threadIdx.x & 3u, row_wg = threadIdx.x >> 2, p = blockIdx.x * 64 + row_wg;
    const bool valid = p < fa.total_slots;                   // slots come in whole cells: a cell's lanes are valid together
    const PassDesc& d = descs[valid ? fa.index[p] : 0];
    const uint32_t rows_in = d.rows_in, ro = p - d.tile0;
    const uint32_t rows_out = (rows_in + (1u << FV) - 1u) >> FV;
    const Ext pad = (q & 1u) ? kb::ext_one() : kb::ext_zero();      // the padding fraction (0, 1)
    Ext val = pad;                                           // rows past rows_out inside a real cell are padding
    if (valid && ro < rows_out) {
        const void* src = FIRST ? d.src[q & 1u] : d.src[q];
        const uint32_t rows_x = FIRST ? d.rows_x : 0u;
        if (FIRST && NBASE && (q & 1u) == 0) val = fold_table_deep<FV, FIRST, true>(src, q, rows_in, rows_x, ro << FV, ch, pad);
        else val = fold_table_deep<FV, FIRST, false>(src, q, rows_in, rows_x, ro << FV, ch, pad);
        if (SV > 0 || rs.host_slot == nullptr) st_ext(d.dst[q], folded_pos(ro, rows_out), val);
    }
    if constexpr (SV == 0) {
        if (rs.host_slot != nullptr) {
            // The layer's last fold, published from this kernel (see gkr_pass). The quad's first lane stores the whole row, one
            // dword per 64 B of the slot and instruction as gkr_pass does: with each lane storing its own table — four lanes of
            // an instruction in one 64 B line of uncached host memory — this launch measured 620 - 690 us instead of 22.
            Ext t[4];
#pragma unroll
            for (int u = 0; u < 4; u++)
#pragma unroll
                for (int k = 0; k < 4; k++) t[u].c[k] = __shfl(val.c[k], (int)((threadIdx.x & 60u) + u), 64);
            if (q == 0 && valid && ro < rows_out) {
                const uint32_t rq = folded_pos(ro, rows_out);
                st_ext_host(d.dst[0], rq, t[0]); st_ext_host(d.dst[1], rq, t[1]); st_ext_host(d.dst[2], rq, t[2]); st_ext_host(d.dst[3], rq, t[3]);
            }
            // same tail as gkr_pass
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (threadIdx.x == 0 && rs_ticket_is_last_acq_rel(rs.counter, blockIdx.x, gridDim.x)) rs_publish_seq(rs.host_slot, seq);
        }
    } else {
        const uint32_t cells = (rows_out + (1u << SV) - 1u) >> SV, c = ro >> SV;
        Ext w = kb::ext_zero(), wl = kb::ext_zero();         // zero for lanes past the last real cell
        if (valid && c < cells) {
            const Ext wi = ld_ext(eq_int, d.eq_int_index);
            w = kb::ext_mul(ld_ext(T, c), wi); wl = kb::ext_mul(ld_ext(TL, c), wi);
        }
        // lane 0: wl n0 -> [0]; lane 1: w d0 -> [1], d0 -> [3]; lane 2: wl n1 -> [2]; lane 3: d1 -> [4]
        const Ext prod = q == 3 ? val : kb::ext_mul(val, q == 1 ? w : wl);
        const Ext vals[5] = {prod, prod, prod, val, val};
        const uint32_t owns = q == 0 ? 0x01u : q == 1 ? 0x0au : q == 2 ? 0x04u : 0x10u;
        deep_grid_finish<SV, 4>(vals, owns, row_wg, q == 0 && (row_wg & ((1u << SV) - 1u)) == 0, w, partials, rs, seq);
    }
}

// ================================================================ trace openings at the final point
struct OpenDesc { const uint32_t* cols; uint32_t rows, width, col0, out0; };   // one group of <= OPEN_COLS columns of one chip
constexpr int OPEN_COLS = COL_DOT_COLS;              // (8 columns per workgroup, sharing one read of the eq slice, measured slower: 1.33 vs 0.78 ms)
constexpr uint32_t OPEN_ROWS = COL_DOT_ROWS;
// Column sums against eq with delayed reduction (kb::DotAcc, col_dot_rows): 64 terms per lane, one reduction per column and lane.
// NC: the columns of this group (the last group of a table may have fewer than OPEN_COLS).
template <int NC>
__device__ __forceinline__ void open_columns_group(const OpenDesc& d, const uint32_t* __restrict__ eq, uint32_t eq_len,
                                                   uint32_t* __restrict__ partials, uint32_t total_cols, uint32_t (&sm)[4][4 * OPEN_COLS]) {
    const uint32_t r0 = blockIdx.y * OPEN_ROWS, r1 = min(r0 + OPEN_ROWS, d.rows);
    const uint32_t* col[NC];
    kb::DotAcc acc[NC];
    bool aligned = aligned16(eq) && (eq_len & 3u) == 0;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        col[c] = d.cols + (size_t)(d.col0 + c) * d.rows;
        aligned = aligned && aligned16(col[c]);
        kb::dot_init(acc[c]);
    }
    col_dot_rows<NC>(col, eq, eq_len, r0, r1, aligned, acc);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const Ext v = kb::dot_finish(acc[c]);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const uint32_t w = wave_sum(v.c[k]);
            if (lane == 0) sm[wave][4 * c + k] = w;
        }
    }
    __syncthreads();
    if (threadIdx.x < 4 * NC) {
        uint32_t a = 0;
        for (int i = 0; i < 4; i++) a = kb::add(a, sm[i][threadIdx.x]);
        partials[((size_t)blockIdx.y * total_cols + d.out0) * 4 + threadIdx.x] = a;
    }
}
__global__ __launch_bounds__(256) void open_columns_kernel(const OpenDesc* __restrict__ descs, const uint32_t* __restrict__ eq,
                                                           uint32_t eq_len, uint32_t* __restrict__ partials, uint32_t total_cols) {
    // consecutive workgroups = the column groups of one table over the SAME rows: their eq slice is re-read from the
    // caches, not from HBM
    __shared__ uint32_t sm[4][4 * OPEN_COLS];
    const OpenDesc d = descs[blockIdx.x];
    if (blockIdx.y * OPEN_ROWS >= d.rows) return;         // partials are zero-initialised
    switch (min(d.width - d.col0, (uint32_t)OPEN_COLS)) {
        case 1: open_columns_group<1>(d, eq, eq_len, partials, total_cols, sm); break;
        case 2: open_columns_group<2>(d, eq, eq_len, partials, total_cols, sm); break;
        case 3: open_columns_group<3>(d, eq, eq_len, partials, total_cols, sm); break;
        default: open_columns_group<4>(d, eq, eq_len, partials, total_cols, sm); break;
    }
}
// out[j] = sum over the chunks of partials[chunk][j]: 64 words per workgroup, four chunk lanes per word folded through LDS
// (one lane per word walking all chunks was a chain of n_chunks dependent adds: 50 us for 256 chunks)
__global__ __launch_bounds__(256) void open_sum_kernel(const uint32_t* __restrict__ partials, uint32_t n_chunks, uint32_t n_words, uint32_t* __restrict__ out) {
    __shared__ uint32_t sm[256];
    const uint32_t jl = threadIdx.x & 63u, cl = threadIdx.x >> 6, j = blockIdx.x * 64u + jl;
    uint32_t acc = 0;
    if (j < n_words)
        for (uint32_t c = cl; c < n_chunks; c += 4) acc = kb::add(acc, partials[(size_t)c * n_words + j]);
    sm[threadIdx.x] = acc;
    __syncthreads();
    if (cl == 0 && j < n_words) out[j] = kb::add(kb::add(sm[jl], sm[64 + jl]), kb::add(sm[128 + jl], sm[192 + jl]));
}
}  // namespace gkr
}  // namespace sp1hip
