// sp1_amd/csrc/zc_compile.hpp — what the zerocheck prover (zerocheck.hip) reads from the constraint-program compiler
// (zc_compile.cpp): the plan of a chip's program and the hinted sub-AIRs found in it.
#pragma once
#include <memory>
#include <vector>

#include "common.hpp"
#include "zc_device.hpp"
#include "zc_poseidon2.hpp"
#include "zc_keccak.hpp"
#include "zc_mul.hpp"
#include "zc_poly.hpp"

namespace sp1hip {

// host-side shorthands of the extension field, shared by the compiler and the prover
using Ext = kb::Ext;
static inline Ext operator+(const Ext& a, const Ext& b) { return kb::ext_add(a, b); }
static inline Ext operator-(const Ext& a, const Ext& b) { return kb::ext_sub(a, b); }
static inline Ext operator*(const Ext& a, const Ext& b) { return kb::ext_mul(a, b); }

struct ZcMacro {                 // a hinted sub-AIR: its constraints are [first_constraint, first_constraint + n_constraints())
    uint32_t kind, base_col, first_constraint, aux0 = 0, aux1 = 0;
    uint32_t n_c = 0;            // kind 7 (a polynomial identity, zc_poly.hpp: ZcPlan::polys[aux0]): its number of constraints
    uint32_t n_constraints() const { return kind == ZC_HINT_POLY ? n_c : kind == ZC_HINT_POSEIDON2 ? ZC_P2_CONSTRAINTS : kind == ZC_HINT_KECCAK ? ZC_KK_CONSTRAINTS : kind == ZC_HINT_MUL ? ZC_MUL_CONSTRAINTS : kind == ZC_HINT_SEPTIC_CURVE ? 7u : 14u; }
    // pieces the kernels run (the septic kinds: weighted forms, zc_septic_*_piece_w) / pieces of the host model (per-coefficient forms)
    uint32_t n_pieces() const { return kind == ZC_HINT_POLY ? 1u : kind == ZC_HINT_POSEIDON2 ? ZC_P2_PIECES : kind == ZC_HINT_KECCAK ? ZC_KK_PIECES : kind == ZC_HINT_MUL ? ZC_MUL_PIECES : kind == ZC_HINT_SEPTIC_CURVE ? 2u : 4u; }
    uint32_t n_host_pieces() const { return kind == ZC_HINT_SEPTIC_CURVE ? 1u : kind == ZC_HINT_SEPTIC_SUM ? 2u : n_pieces(); }
    // the columns whose GKR-opening term the fused pieces carry: [lo, lo + n) (a polynomial identity: the list ZcPoly::owned instead)
    void owned(uint32_t* lo, uint32_t* n) const {
        if (kind == ZC_HINT_POLY) { *lo = 0; *n = 0; }
        else if (kind == ZC_HINT_POSEIDON2) { *lo = base_col; *n = ZC_P2_COLUMNS; }
        else if (kind == ZC_HINT_KECCAK) { *lo = base_col; *n = ZC_KK_COLUMNS; }
        else if (kind == ZC_HINT_MUL) { *lo = base_col + MUL_CARRY; *n = ZC_MUL_OWNED; }
        else if (kind == ZC_HINT_SEPTIC_CURVE) { *lo = base_col; *n = 14; }
        else { *lo = aux0; *n = 28; }
    }
};

struct Chunk {
    std::vector<uint32_t> prog;   // allocated [n][4]
    uint32_t n_regs = 1, alpha_off = 0;
};

struct ZcPlan {                      // everything that depends on a chip's program only (cached per process)
    uint32_t n_instr = 0, main_w = 0, prep_w = 0;
    bool macros_enabled = true;      // SP1HIP_ZC_MACRO when the plan was made (part of the cache key)
    bool mul_enabled = true;         // whether the MulOperation hints are honoured (the chip's height, see zc_get_plan)
    std::vector<uint32_t> source;    // the caller's [n][3] program (collision check)
    std::vector<uint32_t> prog;      // allocated [n][4], whole program (padded-row evaluation)
    uint32_t n_regs = 1;
    std::vector<Chunk> chunks, mono, fine;
    std::vector<uint32_t> sched;     // the scheduled SSA the forms above were cut from
    std::vector<ZcMacro> macros;     // hinted sub-AIRs evaluated by fused kernels (zc_poseidon2.hpp); their asserts are not in the forms above
    std::vector<ZcPoly> polys;       // the polynomial identities among them (zc_poly.hpp), by ZcMacro::aux0
    std::vector<std::vector<ZcPolySeg>> poly_segs;   // their device-table segments, ready for a proof's alpha
};

// the last rounds (at most ZC_FINE_MAX_TERMS row pairs per chip: one wave, mostly idle lanes) are pure latency — one wave
// interprets a chunk serially at ~0.35 us per instruction — so they run a third form of the program (ZcPlan::fine), cut into
// pieces of ~ZC_FINE_LIMIT instructions with no regard for recomputation: more workgroups, each a third as long
constexpr uint32_t ZC_FINE_LIMIT = 32, ZC_FINE_MAX_TERMS = 64;

// The plan of `program` ([n_instr][3] SSA words), made once per process and looked up afterwards. `rows`: the chip's height in
// this proof (whether the MulOperation hints are honoured). chip_index: for the SP1HIP_ZC_DEBUG lines only.
int zc_get_plan(const uint32_t* program, uint32_t n_instr, uint32_t main_width, uint32_t prep_width, int chip_index,
                std::shared_ptr<const ZcPlan>* out, uint64_t rows = ~0ull);

// The plain SSA of `program` for the trace checker (trace_check.hip): HINT pseudo-instructions dropped, the caller's instruction
// order, immediates folded, registers allocated — and cut at assert boundaries into self-contained pieces of at most `max_regs`
// registers each (one piece when the whole program fits; a value two pieces need is recomputed in both). Every ASSERT_ZERO
// carries its index in the WHOLE program in operand b. No macro, no fused piece, no reordering: nothing of what a ZcPlan proves
// with. The program must already be known to be in SSA order with valid opcodes (validate_program of trace_check.hip does that for the checker).
int zc_plain_pieces(const uint32_t* program, uint32_t n_instr, uint32_t main_width, uint32_t prep_width, uint32_t max_regs,
                    std::vector<Chunk>* pieces);

// host evaluation of the whole program on an all-zero row (padded_row_adjustment, shard.rs:L524-L536): sum_k alpha_pows[k] * (the
// value of constraint k)
Ext zc_eval_zero_row(const ZcPlan& plan, const Ext* alpha_pows, const uint32_t* publics);

}  // namespace sp1hip
