// sp1_amd/csrc/zc_compile.cpp — the zerocheck's constraint-program compiler: host code only, no HIP runtime call.
//
// Constraints are data: an SSA program per chip (include/sp1hip.h, sp1_amd/air.py). Here it becomes what the interpreter of
// zc_kernels.hpp runs: immediates folded (fold_immediates), an instruction order chosen for the smallest register file
// (schedule_program, rematerialize_cheap), registers allocated by linear scan (allocate_registers), and the program cut at
// assert boundaries into self-contained chunks in three granularities (build_chunks). Hinted sub-AIRs (Poseidon2 permutation,
// septic curve, Keccak-f round, MulOperation, polynomial identities) are checked against the SSA on a pseudo-random row and
// leave the interpreted forms: fused pieces evaluate them (zc_poseidon2.hpp). Plans are cached per process
// (zc_get_plan). tests/test_zc_compiler.py drives all of it through sp1hip_zerocheck_plan_eval, without a GPU.
#include <algorithm>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "zc_compile.hpp"

namespace sp1hip {

constexpr uint32_t ZC_CHUNK_LIMIT = 96;    // target instructions per chunk (host-side program splitting)
constexpr uint32_t ZC_CHUNK_HARD_MAX = 320; // a chunk may grow to this while its asserts share most of their cones

// linear-scan register allocation of the SSA program (host)
static inline bool zc_is_imm(uint32_t op) { return op >= ZC_ADDC && op <= ZC_MULC; }

// ADD / SUB / MUL with a CONST operand -> the immediate forms (same instruction indices; the CONST instructions stay
// behind and drop out when the chunks collect the cones of the asserts).
static void fold_immediates(const uint32_t* ssa, uint32_t n, std::vector<uint32_t>* out) {
    out->assign(ssa, ssa + (size_t)n * 3);
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t op = ssa[3 * k], a = ssa[3 * k + 1], b = ssa[3 * k + 2];
        if (op != ZC_ADD && op != ZC_SUB && op != ZC_MUL) continue;
        const bool ca = ssa[3 * a] == ZC_CONST, cb = ssa[3 * b] == ZC_CONST;
        if (ca == cb) continue;                                 // none (or both: left to the generic path)
        uint32_t* o = out->data() + 3 * (size_t)k;
        const uint32_t var = ca ? b : a, c = ssa[3 * (ca ? a : b) + 1];
        o[1] = var; o[2] = c;
        o[0] = op == ZC_ADD ? ZC_ADDC : op == ZC_MUL ? ZC_MULC : (cb ? ZC_SUBC : ZC_CSUB);
    }
}

// Instruction scheduling (host). The k-th ASSERT_ZERO of the caller's program is constraint k; here every assert gets
// its index as an explicit operand, which frees the ORDER: asserts are sorted by the last (or first) trace column their
// cone touches, and every value is emitted right before its first use (depth-first from the asserts), the columns an
// assert needs first, in ascending order (so that runs of them merge into one load instruction). Constraints of real
// chips are local in the column layout (an operation's columns are contiguous), so this keeps few values alive at a
// time: the register file of a 250-column chip shrinks from "every shared sub-expression of the chip" to the handful
// one operation needs, which is what decides the workgroup width / occupancy of the interpreter (launch_round).
// mode 0: original order (asserts tagged only); 1: by last column; 2: by first column; 3: by last column over a program whose
// cheap values are rematerialised at every use (below), each load emitted right before the instruction that reads it.

// Rematerialisation (host), for the FieldOpCols chips (round 5: secp256k1 add / double, uint256): their constraints are
// coefficient-wise convolutions sum_i a[i] b[k - i] over 32-limb operands that are COLUMNS, 63 coefficients per field operation,
// ten operations per row. With every column loaded once and kept, ~100 values are live throughout (two operands, the carry, the
// byte decompositions of the point) and a wave's register file takes 120 KB of LDS: ONE wave per compute unit. Here every use of
// a column (and of a value computed from columns in at most 4 instructions — the high byte (u16 - low) / 256 of a memory limb —
// or in at most 7 if it is used at most 8 times) gets its own copy right before the user; a product then costs LOAD, LOAD (forwarded), MAD
// instead of MAD, the program is ~3x longer — and the file shrinks to the accumulators and the few values that are worth keeping.
static void rematerialize_cheap(const uint32_t* ssa, uint32_t n, std::vector<uint32_t>* out) {
    auto is_bin = [](uint32_t op) { return op == ZC_ADD || op == ZC_SUB || op == ZC_MUL; };
    auto is_un = [](uint32_t op) { return op == ZC_NEG || op == ZC_ASSERT_ZERO || zc_is_imm(op); };
    std::vector<uint32_t> uses(n, 0), cone(n, 1);
    std::vector<char> remat(n, 0);
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t op = ssa[3 * k];
        if (is_bin(op)) { uses[ssa[3 * k + 1]]++; uses[ssa[3 * k + 2]]++; }
        else if (is_un(op)) uses[ssa[3 * k + 1]]++;
    }
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t op = ssa[3 * k], a = ssa[3 * k + 1], b = ssa[3 * k + 2];
        if (op == ZC_ASSERT_ZERO) continue;
        if (is_bin(op)) { cone[k] = cone[a] + cone[b] + 1; remat[k] = remat[a] && remat[b] && (cone[k] <= 4 || (cone[k] <= 7 && uses[k] <= 8)); }
        else if (is_un(op)) { cone[k] = cone[a] + 1; remat[k] = remat[a] && (cone[k] <= 4 || (cone[k] <= 7 && uses[k] <= 8)); }
        else remat[k] = 1;                       // LOAD_MAIN / LOAD_PREP / CONST / PUBLIC
    }
    out->clear();
    std::vector<uint32_t> where(n, 0xffffffffu), stack;
    auto push = [&](uint32_t op, uint32_t a, uint32_t b) { out->insert(out->end(), {op, a, b}); return (uint32_t)(out->size() / 3 - 1); };
    // a fresh copy of the cone of a rematerialisable value (at most 7 instructions: recursion depth is bounded)
    std::function<uint32_t(uint32_t)> clone = [&](uint32_t v) -> uint32_t {
        if (!remat[v]) return where[v];
        const uint32_t op = ssa[3 * v], a = ssa[3 * v + 1], b = ssa[3 * v + 2];
        if (is_bin(op)) { const uint32_t x = clone(a), y = clone(b); return push(op, x, y); }
        if (is_un(op)) { const uint32_t x = clone(a); return push(op, x, b); }
        return push(op, a, b);
    };
    for (uint32_t k = 0; k < n; k++) {
        if (remat[k]) continue;                  // emitted where it is used
        const uint32_t op = ssa[3 * k], a = ssa[3 * k + 1], b = ssa[3 * k + 2];
        if (is_bin(op)) { const uint32_t x = clone(a), y = clone(b); where[k] = push(op, x, y); }
        else if (is_un(op)) { const uint32_t x = clone(a); where[k] = push(op, x, b); }
        else where[k] = push(op, a, b);
    }
}

static void schedule_program(const uint32_t* ssa, uint32_t n, uint32_t main_w, int mode, std::vector<uint32_t>* out) {
    std::vector<uint32_t> remat_ssa;
    const bool lazy = mode == 3;
    if (lazy) {
        rematerialize_cheap(ssa, n, &remat_ssa);
        ssa = remat_ssa.data(); n = (uint32_t)(remat_ssa.size() / 3); mode = 1;
    }
    auto is_bin = [](uint32_t op) { return op == ZC_ADD || op == ZC_SUB || op == ZC_MUL; };
    auto is_un = [](uint32_t op) { return op == ZC_NEG || op == ZC_ASSERT_ZERO || zc_is_imm(op); };
    std::vector<uint32_t> asserts, idx_of(n, 0);
    for (uint32_t k = 0; k < n; k++)
        if (ssa[3 * k] == ZC_ASSERT_ZERO) { idx_of[k] = (uint32_t)asserts.size(); asserts.push_back(k); }
    out->clear();
    if (mode == 0) {
        out->assign(ssa, ssa + (size_t)n * 3);
        for (uint32_t k : asserts) (*out)[3 * (size_t)k + 2] = idx_of[k];
        return;
    }
    // first / last column a value depends on (main columns first, then preprocessed)
    std::vector<uint32_t> lo(n, 0xffffffffu), hi(n, 0);
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t op = ssa[3 * k], a = ssa[3 * k + 1], b = ssa[3 * k + 2];
        if (op == ZC_LOAD_MAIN) lo[k] = hi[k] = a + 1;
        else if (op == ZC_LOAD_PREP) lo[k] = hi[k] = main_w + a + 1;
        else if (is_bin(op)) { lo[k] = std::min(lo[a], lo[b]); hi[k] = std::max(hi[a], hi[b]); }
        else if (is_un(op)) { lo[k] = lo[a]; hi[k] = hi[a]; }
    }
    std::vector<uint32_t> order = asserts;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return mode == 1 ? hi[x] < hi[y] : lo[x] < lo[y]; });
    std::vector<uint32_t> renum(n, 0xffffffffu), stack, loads;
    auto emit = [&](uint32_t k) {
        const uint32_t op = ssa[3 * k];
        uint32_t a = ssa[3 * k + 1], b = ssa[3 * k + 2];
        if (is_bin(op)) { a = renum[a]; b = renum[b]; }
        else if (is_un(op)) a = renum[a];
        if (op == ZC_ASSERT_ZERO) b = idx_of[k];
        renum[k] = (uint32_t)(out->size() / 3);
        out->insert(out->end(), {op, a, b});
    };
    std::vector<uint8_t> visited(n, 0);
    for (uint32_t as : order) {
        // 1. the columns this assert still needs, ascending
        loads.clear();
        stack.assign(1, ssa[3 * as + 1]);
        std::vector<uint32_t> seen_here;
        while (!stack.empty()) {
            const uint32_t v = stack.back();
            stack.pop_back();
            if (renum[v] != 0xffffffffu || visited[v]) continue;
            visited[v] = 1;
            seen_here.push_back(v);
            const uint32_t op = ssa[3 * v];
            if (op == ZC_LOAD_MAIN || op == ZC_LOAD_PREP) loads.push_back(v);
            else if (is_bin(op)) { stack.push_back(ssa[3 * v + 1]); stack.push_back(ssa[3 * v + 2]); }
            else if (is_un(op)) stack.push_back(ssa[3 * v + 1]);
        }
        for (uint32_t v : seen_here) visited[v] = 0;
        std::sort(loads.begin(), loads.end(), [&](uint32_t x, uint32_t y) { return lo[x] < lo[y]; });
        if (!lazy) for (uint32_t v : loads) emit(v);
        // 2. the rest of the cone, operands before users (iterative post-order)
        stack.assign(1, ssa[3 * as + 1]);
        while (!stack.empty()) {
            const uint32_t v = stack.back();
            if (renum[v] != 0xffffffffu) { stack.pop_back(); continue; }
            const uint32_t op = ssa[3 * v];
            uint32_t need[2], nn = 0;
            if (is_bin(op)) { need[nn++] = ssa[3 * v + 1]; need[nn++] = ssa[3 * v + 2]; }
            else if (is_un(op)) need[nn++] = ssa[3 * v + 1];
            bool ready = true;
            for (uint32_t j = nn; j-- > 0;)
                if (renum[need[j]] == 0xffffffffu) { stack.push_back(need[j]); ready = false; }
            if (ready) { emit(v); stack.pop_back(); }
        }
        emit(as);
    }
}

// Register allocation of an SSA program (host) -> the interpreter's [op | flags, dst, a, b] words.
//  * last-use allocation into the lowest free register (the LDS file is sized by the highest one used);
//  * operand forwarding: the interpreter keeps the value of the last value-producing instruction in VGPRs (`prev`);
//    an operand that is that value is flagged ZC_A_PREV / ZC_B_PREV (no LDS read), and a value whose every use
//    happens before the next value is produced is flagged ZC_DST_TEMP: it never touches the register file — in the
//    constraint programs of real chips about half of all values are consumed by the very next instruction;
//  * runs of up to 4 LOADs of consecutive columns of one table become ONE instruction (count in bits 16-17) with
//    consecutive destination registers: the kernel issues all their global loads before waiting once, so a row
//    of a wide chip costs a quarter of the memory round trips.
static int allocate_registers(const uint32_t* ssa, uint32_t n, std::vector<uint32_t>* out, uint32_t* n_regs) {
    auto is_bin = [](uint32_t op) { return op == ZC_ADD || op == ZC_SUB || op == ZC_MUL; };
    auto is_un = [](uint32_t op) { return op == ZC_NEG || op == ZC_ASSERT_ZERO || zc_is_imm(op); };
    std::vector<int> last_use(n, -1), next_val(n, -1);
    std::vector<uint32_t> n_uses(n, 0);
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t op = ssa[3 * k], a = ssa[3 * k + 1], b = ssa[3 * k + 2];
        SP1HIP_REQUIRE(op <= ZC_ASSERT_ZERO || zc_is_imm(op), "bad opcode in constraint program");
        if (is_bin(op)) {
            SP1HIP_REQUIRE(a < k && b < k, "constraint program is not in SSA order");
            last_use[a] = (int)k; last_use[b] = (int)k;
            n_uses[a]++; n_uses[b]++;
        } else if (is_un(op)) {
            SP1HIP_REQUIRE(a < k, "constraint program is not in SSA order");
            last_use[a] = (int)k;
            n_uses[a]++;
        }
    }
    // fused[k]: a MULC whose single use is the ADD / SUB (as subtrahend) that is the next value-producing instruction:
    // it is not emitted, its user becomes a MADC
    std::vector<char> fused(n, 0);
    std::vector<int> fused_src(n, -1);         // for the user: the MULC it absorbs
    for (uint32_t k = 0; k + 1 < n; k++) {
        const bool is_mulc = ssa[3 * k] == ZC_MULC;
        const bool is_mul = ssa[3 * k] == ZC_MUL && ssa[3 * k + 1] != ssa[3 * k + 2];
        if (!(is_mulc || is_mul) || n_uses[k] != 1) continue;
        uint32_t u = k + 1;
        while (u < n && ssa[3 * u] == ZC_ASSERT_ZERO) u++;
        if (u >= n || fused_src[u] >= 0) continue;
        const uint32_t uop = ssa[3 * u], ua = ssa[3 * u + 1], ub = ssa[3 * u + 2];
        if (ua == ub) continue;
        if (is_mul) {                      // the other summand must not be one of the factors (it may live in `prev` only)
            const uint32_t other = ua == k ? ub : ua;
            if (other == ssa[3 * k + 1] || other == ssa[3 * k + 2]) continue;
        }
        if ((uop == ZC_ADD && (ua == k || ub == k)) || (uop == ZC_SUB && ub == k)) { fused[k] = 1; fused_src[u] = (int)k; }
    }
    {   // next_val[k]: the first value-producing (emitted) instruction after k
        int nv = -1;
        for (uint32_t k = n; k-- > 0;) { next_val[k] = nv; if (ssa[3 * k] != ZC_ASSERT_ZERO && !fused[k]) nv = (int)k; }
    }
    // load groups: group_len[k] > 0 on the first LOAD of a run, 0 on the merged followers
    std::vector<uint32_t> group_len(n, 1);
    for (uint32_t k = 0; k < n;) {
        const uint32_t op = ssa[3 * k];
        uint32_t m = 1;
        if (op == ZC_LOAD_MAIN || op == ZC_LOAD_PREP)
            while (m < 4 && k + m < n && ssa[3 * (k + m)] == op && ssa[3 * (k + m) + 1] == ssa[3 * k + 1] + m) m++;
        group_len[k] = m;
        for (uint32_t j = 1; j < m; j++) group_len[k + j] = 0;
        k += m;
    }
    // a value is a temporary when it dies before the next value is produced (and it is not inside a load group,
    // whose members all go to the file except that the LAST column stays forwardable)
    auto is_temp = [&](uint32_t k) {
        if (ssa[3 * k] == ZC_ASSERT_ZERO || n_uses[k] == 0) return false;
        if ((ssa[3 * k] == ZC_LOAD_MAIN || ssa[3 * k] == ZC_LOAD_PREP) && !(group_len[k] == 1)) return false;
        return next_val[k] < 0 ? true : last_use[k] <= next_val[k];
    };
    std::vector<char> busy;
    auto take = [&](uint32_t m) {            // lowest run of m free registers
        uint32_t run = 0;
        for (uint32_t r = 0; r < busy.size(); r++) {
            run = busy[r] ? 0 : run + 1;
            if (run == m) { for (uint32_t j = 0; j < m; j++) busy[r - j] = 1; return r + 1 - m; }
        }
        const uint32_t tail = run;             // free registers at the top can be extended
        const uint32_t start = (uint32_t)busy.size() - tail;
        busy.resize(start + m, 1);
        for (uint32_t j = 0; j < m; j++) busy[start + j] = 1;
        return start;
    };
    std::vector<uint32_t> reg_of(n, 0xffffffffu);
    out->clear();
    int last_value = -1;                       // SSA index held in `prev` when the next instruction runs
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t op = ssa[3 * k], a = ssa[3 * k + 1], b = ssa[3 * k + 2];
        if (group_len[k] == 0) continue;       // merged into the group's first LOAD
        if (fused[k]) continue;                // emitted with its user
        uint32_t word = op, ra = a, rb = b;
        if (fused_src[k] >= 0 && ssa[3 * fused_src[k]] == ZC_MUL) {      // acc +- (x * y)  ->  MAD / MSB
            const uint32_t m = (uint32_t)fused_src[k], acc = a == m ? b : a;
            uint32_t fx = ssa[3 * m + 1], fy = ssa[3 * m + 2];
            uint32_t racc = 0, rx = 0, ry = 0;
            word = op == ZC_SUB ? ZC_MSB : ZC_MAD;
            if ((int)acc == last_value) word |= ZC_B_PREV;
            else {
                racc = reg_of[acc];
                if ((int)fy == last_value) std::swap(fx, fy);        // the forwarded factor must be the first one
                if ((int)fx == last_value) word |= ZC_A_PREV;
            }
            if (!(word & ZC_A_PREV)) rx = reg_of[fx];
            ry = reg_of[fy];
            if ((!(word & ZC_A_PREV) && rx == 0xffffffffu) || ry == 0xffffffffu || (!(word & ZC_B_PREV) && racc == 0xffffffffu)) {
                set_error("internal: operand of fused multiply-add %u has no register", k);
                return SP1HIP_ERROR_RUNTIME;
            }
            if (word & ZC_A_PREV) rx = 0;
            for (uint32_t f : {fx, fy})
                if (last_use[f] == (int)m && reg_of[f] != 0xffffffffu) { busy[reg_of[f]] = 0; reg_of[f] = 0xffffffffu; }
            if (last_use[acc] == (int)k && reg_of[acc] != 0xffffffffu) { busy[reg_of[acc]] = 0; reg_of[acc] = 0xffffffffu; }
            uint32_t dst = 0;
            if (is_temp(k) || n_uses[k] == 0) word |= ZC_DST_TEMP;
            else { dst = take(1); reg_of[k] = dst; }
            if (dst > 0xffffu || racc > 0xffffu) { set_error("constraint program needs more than 65536 registers"); return SP1HIP_ERROR_RUNTIME; }
            last_value = (int)k;
            out->insert(out->end(), {word, dst | (racc << 16), rx, ry});
            continue;
        }
        if (fused_src[k] >= 0) {               // acc +- (term * c)  ->  MADC
            const uint32_t m = (uint32_t)fused_src[k], term = ssa[3 * m + 1], acc = a == m ? b : a;
            const uint32_t c = kb::to_monty(ssa[3 * m + 2] % kb::P);
            uint32_t racc = 0;
            word = ZC_MADC;
            if ((int)term == last_value) word |= ZC_A_PREV; else ra = reg_of[term];
            if ((int)acc == last_value) word |= ZC_B_PREV; else racc = reg_of[acc];
            if ((!(word & ZC_A_PREV) && ra == 0xffffffffu) || (!(word & ZC_B_PREV) && racc == 0xffffffffu)) {
                set_error("internal: operand of fused instruction %u has no register", k);
                return SP1HIP_ERROR_RUNTIME;
            }
            if (word & ZC_A_PREV) ra = 0;
            if (last_use[term] == (int)m && reg_of[term] != 0xffffffffu) { busy[reg_of[term]] = 0; reg_of[term] = 0xffffffffu; }
            if (acc != term && last_use[acc] == (int)k && reg_of[acc] != 0xffffffffu) { busy[reg_of[acc]] = 0; reg_of[acc] = 0xffffffffu; }
            uint32_t dst = 0;
            if (is_temp(k) || n_uses[k] == 0) word |= ZC_DST_TEMP;
            else { dst = take(1); reg_of[k] = dst; }
            if (dst > 0xffffu || racc > 0xffffu) { set_error("constraint program needs more than 65536 registers"); return SP1HIP_ERROR_RUNTIME; }
            last_value = (int)k;
            out->insert(out->end(), {word, dst | (racc << 16), ra, op == ZC_SUB ? kb::neg(c) : c});
            continue;
        }
        if (is_bin(op) || is_un(op)) {
            // the interpreter loads operand A into the forwarded value's registers: a forwarded operand must BE operand A
            uint32_t oa = a, ob = b;
            if (is_bin(op) && (int)ob == last_value && (int)oa != last_value) {
                std::swap(oa, ob);
                if (op == ZC_SUB) word = ZC_RSUB;
            }
            ra = oa; rb = ob;
            if ((int)oa == last_value) word |= ZC_A_PREV; else ra = reg_of[oa];
            if (is_bin(op)) { if ((int)ob == last_value) word |= ZC_B_PREV; else rb = reg_of[ob]; }
            if ((!(word & ZC_A_PREV) && ra == 0xffffffffu) || (is_bin(op) && !(word & ZC_B_PREV) && rb == 0xffffffffu)) {
                set_error("internal: operand of instruction %u has no register", k);
                return SP1HIP_ERROR_RUNTIME;
            }
            if (last_use[a] == (int)k && reg_of[a] != 0xffffffffu) { busy[reg_of[a]] = 0; reg_of[a] = 0xffffffffu; }
            if (is_bin(op) && b != a && last_use[b] == (int)k && reg_of[b] != 0xffffffffu) { busy[reg_of[b]] = 0; reg_of[b] = 0xffffffffu; }
        }
        uint32_t dst = 0;
        if (op != ZC_ASSERT_ZERO) {
            const uint32_t m = group_len[k];
            if (m == 1 && (is_temp(k) || n_uses[k] == 0)) {
                word |= ZC_DST_TEMP;           // lives in `prev` only (or is dead)
            } else {
                dst = take(m);
                for (uint32_t j = 0; j < m; j++) {
                    if (n_uses[k + j]) reg_of[k + j] = dst + j; else busy[dst + j] = 0;
                }
            }
            word |= (m - 1) << 16;
            last_value = (int)(k + m - 1);
        }
        if (op == ZC_CONST) ra = kb::to_monty(a % kb::P);
        if (zc_is_imm(op)) rb = kb::to_monty(b % kb::P);
        if (op == ZC_ASSERT_ZERO) rb = b;         // the constraint's index (schedule_program)
        out->insert(out->end(), {word, dst, ra, rb});
    }
    *n_regs = busy.empty() ? 1u : (uint32_t)busy.size();
    return SP1HIP_SUCCESS;
}

// Splits the SSA program into self-contained chunks at assert boundaries (each chunk re-emits the
// dependency cone of its asserts, at most ~`limit` instructions unless a single cone is larger). Chunks
// are independent workgroups on the GPU: wide chips get parallelism across constraints, which is what
// keeps the late, tiny sumcheck rounds from being one wave interpreting thousands of instructions
// serially (cf. the reference's chunked bytecode, /root/reference/sp1-gpu/crates/air/src/ir/bytecode.rs:L27-L110).
static int build_chunks(const uint32_t* ssa, uint32_t n, uint32_t main_w, uint32_t prep_w, uint32_t limit,
                        std::vector<Chunk>* out, uint32_t hard_max = ZC_CHUNK_HARD_MAX, const std::vector<ZcMacro>* macros = nullptr,
                        const std::vector<ZcPoly>* polys = nullptr) {
    std::vector<uint32_t> stamp(n, 0xffffffffu);
    std::vector<uint8_t> cone_seen(n, 0);
    std::vector<uint32_t> members, asserts, stack;
    uint32_t chunk_id = 0, assert_index = 0, first_assert = 0;
    auto flush = [&]() -> int {
        if (asserts.empty()) return SP1HIP_SUCCESS;
        std::sort(members.begin(), members.end());
        std::vector<uint32_t> renum(n, 0), sub;
        // interleave: every member instruction in original order, asserts after their operand exists
        std::vector<std::pair<uint32_t, bool>> order;   // (ssa index, is_assert)
        for (uint32_t m : members) order.push_back({m, false});
        for (uint32_t a : asserts) order.push_back({a, true});
        std::sort(order.begin(), order.end());
        uint32_t next = 0;
        for (auto& o : order) {
            const uint32_t k = o.first, op = ssa[3 * k];
            uint32_t a = ssa[3 * k + 1], b = ssa[3 * k + 2];
            if (op == ZC_ADD || op == ZC_SUB || op == ZC_MUL) { a = renum[a]; b = renum[b]; }
            else if (op == ZC_NEG || op == ZC_ASSERT_ZERO || zc_is_imm(op)) a = renum[a];
            renum[k] = next++;
            sub.insert(sub.end(), {op, a, b});
        }
        Chunk c;
        c.alpha_off = first_assert;
        SP1HIP_TRY(allocate_registers(sub.data(), (uint32_t)(sub.size() / 3), &c.prog, &c.n_regs));
        out->push_back(std::move(c));
        members.clear();
        asserts.clear();
        chunk_id++;
        return SP1HIP_SUCCESS;
    };
    for (uint32_t k = 0; k < n; k++) {
        if (ssa[3 * k] != ZC_ASSERT_ZERO) continue;
        // new nodes this assert would add to the current chunk
        std::vector<uint32_t> fresh;
        stack.assign(1, ssa[3 * k + 1]);
        while (!stack.empty()) {
            const uint32_t v = stack.back();
            stack.pop_back();
            if (stamp[v] == chunk_id) continue;
            stamp[v] = chunk_id;
            fresh.push_back(v);
            const uint32_t op = ssa[3 * v];
            if (op == ZC_ADD || op == ZC_SUB || op == ZC_MUL) { stack.push_back(ssa[3 * v + 1]); stack.push_back(ssa[3 * v + 2]); }
            else if (op == ZC_NEG || zc_is_imm(op)) stack.push_back(ssa[3 * v + 1]);
        }
        if (!asserts.empty() && members.size() + fresh.size() + asserts.size() + 1 > limit) {
            // over the target size. If most of this assert's cone is ALREADY in the chunk (it shares the chunk's
            // intermediate values: the 16 constraints of a Poseidon2 external round share one S-box / linear layer), closing
            // the chunk here would recompute all of it in the next one: keep it, up to a hard cap.
            bool keep = false;
            if (limit != 0xffffffffu && members.size() + fresh.size() + asserts.size() + 1 <= hard_max) {
                size_t cone = 0;
                std::vector<uint32_t> st2(1, ssa[3 * k + 1]);
                std::vector<uint8_t>& seen = cone_seen;
                std::vector<uint32_t> touched;
                while (!st2.empty()) {
                    const uint32_t v = st2.back();
                    st2.pop_back();
                    if (seen[v]) continue;
                    seen[v] = 1; touched.push_back(v); cone++;
                    const uint32_t op = ssa[3 * v];
                    if (op == ZC_ADD || op == ZC_SUB || op == ZC_MUL) { st2.push_back(ssa[3 * v + 1]); st2.push_back(ssa[3 * v + 2]); }
                    else if (op == ZC_NEG || zc_is_imm(op)) st2.push_back(ssa[3 * v + 1]);
                }
                for (uint32_t v : touched) seen[v] = 0;
                keep = 2 * fresh.size() <= cone;
            }
            if (!keep) {
                for (uint32_t v : fresh) stamp[v] = 0xffffffffu;     // undo, close the chunk, retry in a new one
                SP1HIP_TRY(flush());
                k--;
                continue;
            }
        }
        if (asserts.empty()) first_assert = assert_index;
        members.insert(members.end(), fresh.begin(), fresh.end());
        asserts.push_back(k);
        assert_index++;
    }
    SP1HIP_TRY(flush());
    // GKR visits: the first load of each column, in chunk order, carries the flag; columns no constraint
    // reads get TOUCH pseudo-instructions in extra chunks
    std::vector<bool> seen_m(main_w, false), seen_p(prep_w, false);
    if (macros)                                    // the fused pieces of a hinted sub-AIR carry the GKR term of its columns themselves
        for (const ZcMacro& m : *macros) {
            uint32_t lo, cnt;
            m.owned(&lo, &cnt);
            for (uint32_t c = 0; c < cnt; c++) seen_m[lo + c] = true;
            if (m.kind == ZC_HINT_POLY && polys) for (uint32_t c : (*polys)[m.aux0].owned) seen_m[c] = true;
        }
    for (auto& c : *out)
        for (size_t k = 0; k < c.prog.size() / 4; k++) {
            uint32_t* o = c.prog.data() + 4 * k;
            const uint32_t op = o[0] & 0xffu, cnt = ((o[0] >> 16) & 3u) + 1;
            if (op != ZC_LOAD_MAIN && op != ZC_LOAD_PREP) continue;
            std::vector<bool>& seen = op == ZC_LOAD_MAIN ? seen_m : seen_p;
            for (uint32_t j = 0; j < cnt; j++)
                if (!seen[o[2] + j]) { seen[o[2] + j] = true; o[0] |= ZC_GKR_FLAG << j; }
        }
    Chunk touch;
    auto push_touch = [&](uint32_t col, uint32_t is_prep) {
        touch.prog.insert(touch.prog.end(), {ZC_TOUCH, 0u, col, is_prep});
        if (touch.prog.size() / 4 >= limit) { out->push_back(touch); touch.prog.clear(); }
    };
    for (uint32_t c = 0; c < main_w; c++) if (!seen_m[c]) push_touch(c, 0);
    for (uint32_t c = 0; c < prep_w; c++) if (!seen_p[c]) push_touch(c, 1);
    if (!touch.prog.empty()) out->push_back(touch);
    if (out->empty()) { Chunk e; e.prog = {ZC_TOUCH, 0u, 0u, 2u}; out->push_back(e); }   // no constraints, no columns
    return SP1HIP_SUCCESS;
}

// Host interpreter of allocated program words on ONE row (Montgomery words; null row = all zeros): every ASSERT_ZERO hands
// (constraint index, value) to `on_assert`. The same semantics as run_program on the device, in the base field.
template <class F>
static void eval_words_row(const uint32_t* words, size_t n, uint32_t n_regs, const uint32_t* main_row, const uint32_t* prep_row,
                           const uint32_t* publics, F&& on_assert) {
    std::vector<uint32_t> reg(n_regs + 4, 0);
    uint32_t prev = 0;
    for (size_t k = 0; k < n; k++) {
        const uint32_t opw = words[4 * k], op = opw & 0xffu, dst = words[4 * k + 1], x = words[4 * k + 2], y = words[4 * k + 3];
        const uint32_t A = (opw & ZC_A_PREV) ? prev : (op >= ZC_ADD && op != ZC_TOUCH ? reg[x] : 0u);
        const bool bin = (op >= ZC_ADD && op <= ZC_MUL) || op == ZC_RSUB;
        const uint32_t B = (bin && (opw & ZC_B_PREV)) ? prev : (bin ? reg[y] : 0u);
        uint32_t res = 0;
        switch (op) {
            case ZC_LOAD_MAIN: case ZC_LOAD_PREP: {
                const uint32_t* row = op == ZC_LOAD_MAIN ? main_row : prep_row;
                for (uint32_t j = 0; j <= ((opw >> 16) & 3u); j++) {
                    prev = row ? row[x + j] : 0u;
                    if (!(opw & ZC_DST_TEMP)) reg[dst + j] = prev;
                }
                continue;
            }
            case ZC_TOUCH: continue;
            case ZC_CONST: res = x; break;
            case ZC_PUBLIC: res = publics[x]; break;
            case ZC_ADD: res = kb::add(A, B); break;
            case ZC_SUB: res = kb::sub(A, B); break;
            case ZC_MUL: res = kb::mul(A, B); break;
            case ZC_RSUB: res = kb::sub(B, A); break;
            case ZC_NEG: res = kb::neg(A); break;
            case ZC_ADDC: res = kb::add(A, y); break;
            case ZC_SUBC: res = kb::sub(A, y); break;
            case ZC_CSUB: res = kb::sub(y, A); break;
            case ZC_MULC: res = kb::mul(A, y); break;
            case ZC_MADC: res = kb::add((opw & ZC_B_PREV) ? prev : reg[dst >> 16], kb::mul(A, y)); break;
            case ZC_MAD: res = kb::add((opw & ZC_B_PREV) ? prev : reg[dst >> 16], kb::mul(A, reg[y])); break;
            case ZC_MSB: res = kb::sub((opw & ZC_B_PREV) ? prev : reg[dst >> 16], kb::mul(A, reg[y])); break;
            default: on_assert(y, A); continue;
        }
        prev = res;
        if (!(opw & ZC_DST_TEMP)) reg[dst & 0xffffu] = res;
    }
}
// host model of the fused pieces on ONE row of base-field words (the planner's check of a hint, sp1hip_zerocheck_plan_eval)
template <class Sink>
static void macro_eval_row(const ZcMacro& m, const std::vector<ZcPoly>& polys, const uint32_t* main_row, Sink&& sink) {
    static const p2::RoundConstants host_rc = p2::make_round_constants();
    if (m.kind == ZC_HINT_POLY) { zc_poly_eval_row(polys[m.aux0], main_row, sink); return; }
    for (uint32_t q = 0; q < m.n_host_pieces(); q++) {
        if (m.kind == ZC_HINT_POSEIDON2)
            zc_p2_piece<P2Base>(q, &host_rc, [&](uint32_t c, bool) { return main_row[m.base_col + c]; }, sink);
        else if (m.kind == ZC_HINT_KECCAK)
            zc_keccak_piece<P2Base>(q, [&](uint32_t c, bool) { return main_row[m.base_col + c]; }, sink);
        else if (m.kind == ZC_HINT_MUL)
            zc_mul_piece<P2Base>(q, [&](uint32_t c, bool) { return main_row[m.base_col + c]; }, [&](uint32_t c, bool) { return main_row[m.aux0 + c]; }, sink);
        else if (m.kind == ZC_HINT_SEPTIC_CURVE)
            zc_septic_curve_piece<P2Base>([&](uint32_t c, bool) { return main_row[m.base_col + c]; }, sink);
        else
            zc_septic_sum_piece<P2Base>(q, [&](uint32_t c, bool) { return main_row[m.base_col + c]; },
                                        [&](uint32_t c, bool) { return main_row[m.aux0 + c]; }, [&]() { return main_row[m.aux1]; }, sink);
    }
}

static uint32_t asserts_total(const uint32_t* program, uint32_t n) {
    uint32_t a = 0;
    for (uint32_t k = 0; k < n; k++) a += program[3 * k] == ZC_ASSERT_ZERO;
    return a;
}

// The plan of a program (immediates folded, instruction order chosen, registers allocated; chunked, undivided and finely
// cut forms) depends on the program alone: a machine's chips are planned once per process and looked up afterwards (a
// prover proves the same machine shard after shard; planning 33 chips costs ~1.3 ms of host time per proof).
// `rows`: the chip's height in this proof. The MulOperation piece (kind 6) replaces interpreter work that grows with the height by
// one more launch per round: below ZC_MUL_MIN_ROWS rows (SP1HIP_ZC_MUL_MIN_ROWS) that launch sits at its latency floor in every
// round and the hint is ignored — the recorded core shard has 128 Mul rows, a fibonacci shard 1.9 million.
constexpr uint64_t ZC_MUL_MIN_ROWS = 1u << 16;
int zc_get_plan(const uint32_t* program, uint32_t n_instr, uint32_t main_width, uint32_t prep_width, int chip_index,
                std::shared_ptr<const ZcPlan>* out, uint64_t rows) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint32_t v) { h = (h ^ v) * 1099511628211ull; };
    // SP1HIP_ZC_MACRO=0 ignores hints; read per call like the BIVARIATE / FORK switches and part of the cache key
    const bool macros_enabled = env_flag("SP1HIP_ZC_MACRO", true);
    const uint64_t mul_min_rows = env_uint("SP1HIP_ZC_MUL_MIN_ROWS", ZC_MUL_MIN_ROWS);
    static const bool zc_debug = env_flag("SP1HIP_ZC_DEBUG", false);
    const bool mul_enabled = macros_enabled && rows >= mul_min_rows;
    mix(main_width); mix(prep_width); mix(n_instr); mix((macros_enabled ? 1u : 0u) | (mul_enabled ? 2u : 0u));
    for (size_t k = 0; k < (size_t)n_instr * 3; k++) mix(program[k]);
    static std::mutex plan_mutex;
    static std::unordered_map<uint64_t, std::shared_ptr<const ZcPlan>> plan_cache;
    std::shared_ptr<const ZcPlan> plan;
    {
        std::lock_guard<std::mutex> lk(plan_mutex);
        auto it = plan_cache.find(h);
        if (it != plan_cache.end() && it->second->n_instr == n_instr && it->second->main_w == main_width && it->second->prep_w == prep_width &&
            it->second->macros_enabled == macros_enabled && it->second->mul_enabled == mul_enabled && (n_instr == 0 || memcmp(it->second->source.data(), program, (size_t)n_instr * 12) == 0))
            plan = it->second;
    }
    if (!plan) {
        std::shared_ptr<ZcPlan> np(new ZcPlan());
        np->n_instr = n_instr; np->main_w = main_width; np->prep_w = prep_width; np->macros_enabled = macros_enabled; np->mul_enabled = mul_enabled;
        np->source.assign(program, program + (size_t)n_instr * 3);
        // hinted sub-AIRs (zc_poseidon2.hpp): the HINT pseudo-instructions become harmless constants, the hints are CHECKED
        // against the SSA, and the asserts they cover leave the interpreted forms (not the whole program `prog`, which the
        // host still evaluates on the all-zero row)
        std::vector<uint32_t> clean(program, program + (size_t)n_instr * 3);
        {
            uint32_t asserts_before = 0;
            for (uint32_t k = 0; k < n_instr; k++) {
                if (clean[3 * k] == ZC_ASSERT_ZERO) asserts_before++;
                if (clean[3 * k] != ZC_HINT) continue;
                const uint32_t kind = clean[3 * k + 1] & 0xffu, w1 = clean[3 * k + 1] >> 8, w2 = clean[3 * k + 2];
                if (kind == ZC_HINT_POLY) {
                    // a polynomial identity (zc_poly.hpp): the values it names follow as ARG pseudo-instructions. Its forms are taken
                    // from the SSA; values that are not affine in the main columns drop the hint (the interpreter keeps the constraints)
                    const uint32_t n_terms = w1, n_c = w2;
                    SP1HIP_REQUIRE(n_terms <= 80 && n_c >= 1 && n_c < (1u << 16), "polynomial-identity hint: bad header");
                    std::vector<std::vector<uint32_t>> ids(3 * (size_t)n_terms + 1);
                    uint32_t j = k + 1;
                    for (; j < n_instr && clean[3 * j] == ZC_HINT && (clean[3 * j + 1] & 0xffu) == ZC_HINT_POLY_ARG; j++) {
                        const uint32_t code = clean[3 * j + 1] >> 8, id = clean[3 * j + 2];
                        SP1HIP_REQUIRE((code == 255u || code < 3 * n_terms) && id < k, "polynomial-identity hint: bad argument");
                        ids[code == 255u ? 3 * (size_t)n_terms : code].push_back(id);
                    }
                    bool shape = ids.back().size() == n_c;
                    for (uint32_t t = 0; t < n_terms; t++)
                        shape &= !ids[3 * t].empty() && !ids[3 * t + 1].empty() && ids[3 * t].size() + ids[3 * t + 1].size() + std::max<size_t>(ids[3 * t + 2].size(), 1) - 2 <= n_c;
                    SP1HIP_REQUIRE(shape, "polynomial-identity hint: operand counts do not match the number of constraints");
                    for (uint32_t q = k; q < j; q++) { clean[3 * q] = ZC_CONST; clean[3 * q + 1] = 0; clean[3 * q + 2] = 0; }
                    ZcPoly poly;
                    poly.first_constraint = asserts_before; poly.n_c = n_c;
                    bool affine = n_terms <= ZC_POLY_MAX_TERMS;
                    std::vector<uint32_t> all;
                    for (auto& v : ids) all.insert(all.end(), v.begin(), v.end());
                    std::vector<ZcLinForm> forms;
                    affine = affine && zc_poly_extract(clean.data(), n_instr, all, &forms);
                    if (affine) {
                        size_t at = 0;
                        poly.terms.resize(n_terms);
                        for (uint32_t t = 0; t < n_terms; t++)
                            for (int f = 0; f < 3; f++) {
                                poly.terms[t].f[f].assign(forms.begin() + at, forms.begin() + at + ids[3 * t + f].size());
                                at += ids[3 * t + f].size();
                            }
                        poly.rest.assign(forms.begin() + at, forms.end());
                        ZcMacro m{kind, 0u, asserts_before};
                        m.aux0 = (uint32_t)np->polys.size(); m.n_c = n_c;
                        np->polys.push_back(std::move(poly));
                        np->macros.push_back(m);
                    } else if (zc_debug) {
                        fprintf(stderr, "[sp1hip zc] chip %d: polynomial-identity hint at constraint %u dropped (a named value is not affine in the main columns)\n", chip_index, asserts_before);
                    }
                    k = j - 1;
                    continue;
                }
                SP1HIP_REQUIRE(kind != ZC_HINT_POLY_ARG, "polynomial-identity argument without its hint");
                SP1HIP_REQUIRE((kind >= ZC_HINT_POSEIDON2 && kind <= ZC_HINT_SEPTIC_SUM) || kind == ZC_HINT_KECCAK || kind == ZC_HINT_MUL, "unknown hint kind in constraint program");
                ZcMacro m{kind, kind == ZC_HINT_SEPTIC_SUM ? (w2 & 0xffffu) : w2, asserts_before};
                if (kind == ZC_HINT_SEPTIC_SUM) { m.aux0 = w2 >> 16; m.aux1 = w1; }
                if (kind == ZC_HINT_MUL) m.aux0 = w1;                 // the first limb of op_b's value (op_c's: seven columns further)
                SP1HIP_REQUIRE((uint64_t)m.base_col + (kind == ZC_HINT_POSEIDON2 ? ZC_P2_COLUMNS : kind == ZC_HINT_KECCAK ? KK_IS_REAL + 1 : kind == ZC_HINT_MUL ? MUL_COLUMNS : 14u) <= main_width &&
                               (kind != ZC_HINT_SEPTIC_SUM || ((uint64_t)m.aux0 + 28 <= main_width && m.aux1 < main_width)) &&
                               (kind != ZC_HINT_MUL || (uint64_t)m.aux0 + MUL_OPC_FROM_OPB + 4 <= main_width), "hint: columns out of range");
                np->macros.push_back(m);
                clean[3 * k] = ZC_CONST; clean[3 * k + 1] = 0; clean[3 * k + 2] = 0;
            }
            if (!macros_enabled) np->macros.clear();
            if (!mul_enabled) np->macros.erase(std::remove_if(np->macros.begin(), np->macros.end(), [](const ZcMacro& m) { return m.kind == ZC_HINT_MUL; }), np->macros.end());
            // each hint is checked against the SSA on its own (below); two hints that overlap — a duplicated HINT, two sum
            // checkers sharing accumulator columns — would each pass and then count their constraints and the GKR batching
            // term of their columns twice: a silently invalid proof. Constraint ranges and owned columns must be disjoint.
            for (size_t a = 0; a < np->macros.size(); a++)
                for (size_t b = a + 1; b < np->macros.size(); b++) {
                    const ZcMacro &ma = np->macros[a], &mb = np->macros[b];
                    const bool c_overlap = ma.first_constraint < mb.first_constraint + mb.n_constraints() &&
                                           mb.first_constraint < ma.first_constraint + ma.n_constraints();
                    uint32_t alo, an, blo, bn;
                    ma.owned(&alo, &an); mb.owned(&blo, &bn);
                    const bool o_overlap = alo < blo + bn && blo < alo + an;
                    SP1HIP_REQUIRE(!c_overlap, "two fused-kernel hints cover the same constraints");
                    SP1HIP_REQUIRE(!o_overlap, "two fused-kernel hints own the same columns");
                }
        }
        program = clean.data();
        auto hinted = [&](uint32_t idx) {
            for (const ZcMacro& m : np->macros) if (idx >= m.first_constraint && idx < m.first_constraint + m.n_constraints()) return true;
            return false;
        };
        // the columns a polynomial identity OWNS (its piece carries their GKR batching term, the interpreter never loads them): those
        // of its rest form that neither its products, nor another identity, nor any constraint left to the interpreter reads
        if (!np->polys.empty() && std::all_of(np->macros.begin(), np->macros.end(), [](const ZcMacro& m) { return m.kind == ZC_HINT_POLY; })) {
            std::vector<uint8_t> interp(main_width, 0), visited(n_instr, 0);
            std::vector<uint32_t> stack;
            uint32_t idx = 0;
            for (uint32_t k = 0; k < n_instr; k++) {
                if (clean[3 * k] != ZC_ASSERT_ZERO) continue;
                if (!hinted(idx) && clean[3 * k + 1] < n_instr) stack.push_back(clean[3 * k + 1]);
                idx++;
            }
            while (!stack.empty()) {
                const uint32_t v = stack.back();
                stack.pop_back();
                if (visited[v]) continue;
                visited[v] = 1;
                const uint32_t op = clean[3 * v], a = clean[3 * v + 1], b = clean[3 * v + 2];
                if (op == ZC_LOAD_MAIN) { if (a < main_width) interp[a] = 1; }
                else if (op == ZC_ADD || op == ZC_SUB || op == ZC_MUL) { if (a < v) stack.push_back(a); if (b < v) stack.push_back(b); }
                else if (op == ZC_NEG) { if (a < v) stack.push_back(a); }
            }
            std::vector<uint32_t> users(main_width, 0);
            std::vector<std::vector<uint8_t>> in_prod(np->polys.size(), std::vector<uint8_t>(main_width, 0)), in_any = in_prod;
            for (size_t pi = 0; pi < np->polys.size(); pi++) {
                const ZcPoly& pl = np->polys[pi];
                auto mark = [&](const ZcLinForm& f, bool prod) { for (uint32_t c : f.cols) if (c < main_width) { in_any[pi][c] = 1; if (prod) in_prod[pi][c] = 1; } };
                for (const ZcPolyTerm& t : pl.terms) for (int f = 0; f < 3; f++) for (auto& lf : t.f[f]) mark(lf, true);
                for (auto& f : pl.rest) mark(f, false);
                for (uint32_t c = 0; c < main_width; c++) users[c] += in_any[pi][c];
            }
            for (size_t pi = 0; pi < np->polys.size(); pi++)
                for (uint32_t c = 0; c < main_width; c++)
                    if (in_any[pi][c] && !in_prod[pi][c] && !interp[c] && users[c] == 1) np->polys[pi].owned.push_back(c);
        }
        for (const ZcPoly& pl : np->polys) np->poly_segs.push_back(zc_poly_segments(pl));
        auto drop_hinted = [&](std::vector<uint32_t>& sch) {      // asserts carry their constraint index in operand b by now
            if (np->macros.empty()) return;
            for (size_t k = 0; k < sch.size() / 3; k++)
                if (sch[3 * k] == ZC_ASSERT_ZERO && hinted(sch[3 * k + 2])) { sch[3 * k] = ZC_CONST; sch[3 * k + 1] = 0; sch[3 * k + 2] = 0; }
        };
        // fold constants into immediates, then pick the instruction order with the smallest register file
        std::vector<uint32_t> folded, sched;
        fold_immediates(program, n_instr, &folded);
        // mode 3 (rematerialised loads: a ~3x longer program with a much smaller file) only where the file is the problem: when the
        // best of the other orders needs at least ZC_LAZY_MIN_REGS registers (64 = two waves' files per CU). It was
        // 128 while the secp256k1 / uint256 chips (195 - 225) were the only ones above 40; the tower / carry chips that came later
        // (Bn254FpOpAssign 103, Uint256Ops 71, Bn254Fp2AddSubAssign 66: the same FieldOpCols programs) take the same form at 64;
        // every chip with a measured schedule is below 40 and keeps it
        constexpr uint32_t ZC_LAZY_MIN_REGS = 64;
        uint32_t best_regs = 0xffffffffu;
        for (int mode = 0; mode < 4; mode++) {
            if (mode == 3 && best_regs < ZC_LAZY_MIN_REGS) continue;
            std::vector<uint32_t> cand;
            std::vector<Chunk> mono;
            schedule_program(folded.data(), n_instr, main_width, mode, &cand);
            std::vector<uint32_t> cand_f = cand;
            drop_hinted(cand_f);
            SP1HIP_TRY(build_chunks(cand_f.data(), (uint32_t)(cand_f.size() / 3), main_width, prep_width, 0xffffffffu, &mono, ZC_CHUNK_HARD_MAX, &np->macros, &np->polys));
            uint32_t regs = 0;
            for (auto& ck : mono) regs = std::max(regs, ck.n_regs);
            if (regs < best_regs) { best_regs = regs; sched.swap(cand); np->mono.swap(mono); }
        }
        const uint32_t n_sched = (uint32_t)(sched.size() / 3);
        if (zc_debug) {
            size_t mono_instr = 0;
            for (auto& ck : np->mono) mono_instr += ck.prog.size() / 4;
            fprintf(stderr, "[sp1hip zc] chip %d: %u ssa instrs, %u+%u cols -> undivided program %zu words, %u registers\n",
                    chip_index, n_instr, main_width, prep_width, mono_instr, best_regs);
        }
        SP1HIP_TRY(allocate_registers(sched.data(), n_sched, &np->prog, &np->n_regs));
        std::vector<uint32_t> sched_f = sched;
        drop_hinted(sched_f);
        SP1HIP_TRY(build_chunks(sched_f.data(), n_sched, main_width, prep_width, ZC_CHUNK_LIMIT, &np->chunks, ZC_CHUNK_HARD_MAX, &np->macros, &np->polys));
        SP1HIP_TRY(build_chunks(sched_f.data(), n_sched, main_width, prep_width, ZC_FINE_LIMIT, &np->fine, ZC_FINE_LIMIT, &np->macros, &np->polys));
        np->sched = sched;
        // trust, but verify: on a pseudo-random row the fused pieces must give what the caller's SSA gives for the constraints
        // they replace (a hint on the wrong columns, or on constraints that are not the Poseidon2 sub-AIR, is an error here)
        if (!np->macros.empty()) {
            std::vector<uint32_t> row(main_width), prow(std::max<uint32_t>(prep_width, 1u)), want(asserts_total(program, n_instr), 0u);
            uint64_t x = 0x9E3779B97F4A7C15ull ^ h;
            auto rnd = [&]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return (uint32_t)(x % kb::P); };
            for (auto& v : row) v = rnd();
            for (auto& v : prow) v = rnd();
            uint32_t n_pub = 1;
            for (uint32_t k = 0; k < n_instr; k++) if (program[3 * k] == ZC_PUBLIC) n_pub = std::max(n_pub, program[3 * k + 1] + 1);
            std::vector<uint32_t> pub(n_pub, 0u);
            eval_words_row(np->prog.data(), np->prog.size() / 4, np->n_regs, row.data(), prow.data(), pub.data(),
                           [&](uint32_t idx, uint32_t v) { if (idx < want.size()) want[idx] = v; });
            for (const ZcMacro& m : np->macros) {
                bool ok = true;
                uint32_t n_seen = 0;
                macro_eval_row(m, np->polys, row.data(), [&](uint32_t j, uint32_t v) {
                    n_seen++;
                    const bool same = m.first_constraint + j < want.size() && want[m.first_constraint + j] == v;
                    if (!same && zc_debug)
                        fprintf(stderr, "[sp1hip zc] hint kind %u: constraint %u + %u: pieces give %08x, the program %08x\n", m.kind, m.first_constraint, j,
                                v, m.first_constraint + j < want.size() ? want[m.first_constraint + j] : 0u);
                    ok &= same;
                });
                SP1HIP_REQUIRE(ok && n_seen == m.n_constraints(), "a fused-kernel hint does not match the constraints it annotates");
            }
        }
        plan = np;
        std::lock_guard<std::mutex> lk(plan_mutex);
        if (plan_cache.size() > 4096) plan_cache.clear();
        plan_cache[h] = plan;
    }
    *out = plan;
    return SP1HIP_SUCCESS;
}

int zc_plain_pieces(const uint32_t* program, uint32_t n_instr, uint32_t main_width, uint32_t prep_width, uint32_t max_regs,
                    std::vector<Chunk>* pieces) {
    pieces->clear();
    std::vector<uint32_t> clean(program, program + (size_t)n_instr * 3), folded, tagged;
    for (uint32_t k = 0; k < n_instr; k++)                       // a HINT defines no value: a constant nobody reads, as in zc_get_plan
        if (clean[3 * k] == ZC_HINT) { clean[3 * k] = ZC_CONST; clean[3 * k + 1] = 0; clean[3 * k + 2] = 0; }
    fold_immediates(clean.data(), n_instr, &folded);
    schedule_program(folded.data(), n_instr, main_width, 0, &tagged);      // mode 0: the caller's order, asserts tagged with their index
    // the cut: halve the instruction target until every piece's file fits (build_chunks closes a piece at an assert boundary and
    // re-emits the cone of the next one's asserts)
    for (uint32_t limit = 0xffffffffu;;) {
        std::vector<Chunk> cut;
        SP1HIP_TRY(build_chunks(tagged.data(), n_instr, main_width, prep_width, limit, &cut, limit));
        // the GKR bookkeeping of the zerocheck (TOUCH pseudo-chunks for columns no constraint reads) is not the checker's business
        cut.erase(std::remove_if(cut.begin(), cut.end(), [](const Chunk& c) { return c.prog.empty() || (c.prog[0] & 0xffu) == ZC_TOUCH; }), cut.end());
        uint32_t regs = 0;
        for (const Chunk& c : cut) regs = std::max(regs, c.n_regs);
        if (regs <= max_regs) { pieces->swap(cut); return SP1HIP_SUCCESS; }
        limit = (limit == 0xffffffffu ? n_instr : limit) / 2;
        if (limit < 8) {
            set_error("zc_plain_pieces: one constraint alone needs %u registers, more than the budget of %u", regs, max_regs);
            return SP1HIP_ERROR_INVALID_ARGUMENT;
        }
    }
}

Ext zc_eval_zero_row(const ZcPlan& plan, const Ext* alpha_pows, const uint32_t* publics) {
    Ext acc = kb::ext_zero();
    eval_words_row(plan.prog.data(), plan.prog.size() / 4, plan.n_regs, nullptr, nullptr, publics,
                   [&](uint32_t idx, uint32_t v) { acc = acc + kb::ext_mul_base(alpha_pows[idx], v); });
    return acc;
}

}  // namespace sp1hip

using namespace sp1hip;

// Host-only: plans `program` exactly as sp1hip_zerocheck_prove does and interprets the chosen form of it on one row.
extern "C" int sp1hip_zerocheck_plan_eval(const uint32_t* program, uint32_t n_instr, uint32_t main_width, uint32_t prep_width,
                                          const uint32_t* main_row, const uint32_t* prep_row, const uint32_t* publics,
                                          uint32_t n_publics, int form, uint32_t* out_values, uint32_t n_constraints,
                                          uint32_t* out_stats) {
    SP1HIP_REQUIRE(program || n_instr == 0, "null program");
    SP1HIP_REQUIRE(out_values || n_constraints == 0, "null output");
    SP1HIP_REQUIRE(form >= 0 && form <= 3, "form: 0 whole program, 1 chunks, 2 undivided, 3 fine");
    uint32_t asserts = 0;
    for (uint32_t k = 0; k < n_instr; k++) {
        const uint32_t op = program[3 * k], a = program[3 * k + 1];
        SP1HIP_REQUIRE(op <= ZC_ASSERT_ZERO || op == ZC_HINT, "bad opcode in constraint program");
        if (op == ZC_ASSERT_ZERO) asserts++;
        if (op == ZC_LOAD_MAIN) SP1HIP_REQUIRE(a < main_width && main_row, "main column out of range");
        if (op == ZC_LOAD_PREP) SP1HIP_REQUIRE(a < prep_width && prep_row, "preprocessed column out of range");
        if (op == ZC_PUBLIC) SP1HIP_REQUIRE(a < n_publics && publics, "public value index out of range");
    }
    SP1HIP_REQUIRE(asserts == n_constraints, "n_constraints does not match the program");
    std::shared_ptr<const ZcPlan> plan;
    SP1HIP_TRY(zc_get_plan(program, n_instr, main_width, prep_width, -1, &plan));
    std::vector<uint32_t> seen(n_constraints, 0);
    auto on_assert = [&](uint32_t idx, uint32_t v) { if (idx < n_constraints) { out_values[idx] = v; seen[idx]++; } };
    uint32_t words = 0, pieces = 0, regs = 0;
    if (form == 0) {
        eval_words_row(plan->prog.data(), plan->prog.size() / 4, plan->n_regs, main_row, prep_row, publics, on_assert);
        words = (uint32_t)(plan->prog.size() / 4); pieces = 1; regs = plan->n_regs;
    } else {
        const std::vector<Chunk>& cks = form == 1 ? plan->chunks : form == 2 ? plan->mono : plan->fine;
        for (const Chunk& ck : cks) {
            // (every ASSERT carries its chip-wide constraint index, whatever piece it ended up in)
            eval_words_row(ck.prog.data(), ck.prog.size() / 4, ck.n_regs, main_row, prep_row, publics, on_assert);
            words += (uint32_t)(ck.prog.size() / 4); pieces++; regs = std::max(regs, ck.n_regs);
        }
    }
    if (form != 0) {                                  // the forms the GPU runs: hinted constraints come from the fused pieces
        for (const ZcMacro& m : plan->macros) {
            macro_eval_row(m, plan->polys, main_row, [&](uint32_t j, uint32_t v) { on_assert(m.first_constraint + j, v); });
            pieces += m.n_pieces();
        }
    }
    for (uint32_t k = 0; k < n_constraints; k++) SP1HIP_REQUIRE(seen[k] == 1, "a constraint was not evaluated exactly once");
    if (out_stats) { out_stats[0] = words; out_stats[1] = pieces; out_stats[2] = regs; }
    return SP1HIP_SUCCESS;
}

extern "C" int sp1hip_zerocheck_poly_check(const uint32_t* program, uint32_t n_instr, uint32_t main_width, uint32_t prep_width,
                                           const uint32_t* main_row, sp1hip_ext_t alpha_c, sp1hip_ext_t* out_collapsed,
                                           sp1hip_ext_t* out_direct, uint32_t* n_identities) {
    SP1HIP_REQUIRE(program && main_row && out_collapsed && out_direct && n_identities, "null argument");
    for (uint32_t k = 0; k < n_instr; k++) SP1HIP_REQUIRE(program[3 * k] <= ZC_ASSERT_ZERO || program[3 * k] == ZC_HINT, "bad opcode in constraint program");
    std::shared_ptr<const ZcPlan> plan;
    SP1HIP_TRY(zc_get_plan(program, n_instr, main_width, prep_width, -1, &plan));
    const Ext alpha{{alpha_c.c[0], alpha_c.c[1], alpha_c.c[2], alpha_c.c[3]}};
    SP1HIP_REQUIRE(!kb::ext_eq(alpha, kb::ext_zero()), "the batching challenge is zero");
    const uint32_t n_c = asserts_total(program, n_instr);
    std::vector<Ext> pows(n_c);                                   // [alpha^(n-1), ..., alpha, 1] as in the prover (zerocheck.hip)
    { Ext cur = kb::ext_one(); for (uint32_t k = n_c; k-- > 0;) { pows[k] = cur; cur = cur * alpha; } }
    const Ext rho = kb::ext_inv(alpha);
    Ext collapsed = kb::ext_zero(), direct = kb::ext_zero();
    std::vector<kb::Ext> scratch[2];
    uint32_t count = 0;
    for (const ZcMacro& m : plan->macros) {
        if (m.kind != ZC_HINT_POLY) continue;
        count++;
        const ZcPoly& pl = plan->polys[m.aux0];
        std::vector<uint32_t> tb;
        zc_poly_table(pl, plan->poly_segs[m.aux0], pows.data() + m.first_constraint, rho, &tb, scratch);
        // the kernels' evaluation of the table on one row: every segment is an affine form (constant first)
        size_t off = ZC_POLY_HDR;
        auto form = [&](uint32_t n, bool with_const) -> Ext {
            Ext f = kb::ext_zero();
            if (with_const) { f = Ext{{tb[off + 4], tb[off + 5], tb[off + 6], tb[off + 7]}}; off += ZC_POLY_ENTRY; }
            for (uint32_t k = 0; k < n; k++, off += ZC_POLY_ENTRY) f = f + kb::ext_mul_base(Ext{{tb[off + 4], tb[off + 5], tb[off + 6], tb[off + 7]}}, main_row[tb[off]]);
            return f;
        };
        Ext v = kb::ext_zero();
        for (uint32_t t = 0; t < tb[0]; t++) {
            Ext p = form(tb[4 + 3 * t], true) * form(tb[5 + 3 * t], true);
            if (tb[6 + 3 * t] != ZC_POLY_NONE) p = p * form(tb[6 + 3 * t], true);
            v = v + p;
        }
        v = v + form(tb[1], true) + form(tb[2], false);
        collapsed = collapsed + v;
        zc_poly_eval_row(pl, main_row, [&](uint32_t k, uint32_t c) { direct = direct + kb::ext_mul_base(pows[m.first_constraint + k], c); });
    }
    memcpy(out_collapsed->c, collapsed.c, 16);
    memcpy(out_direct->c, direct.c, 16);
    *n_identities = count;
    return SP1HIP_SUCCESS;
}
