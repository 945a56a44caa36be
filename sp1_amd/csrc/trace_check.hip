// sp1_amd/csrc/trace_check.hip — the device trace checker: every constraint of every chip on every row of the column-major tables
// the prover holds, where they are made. What the reference does under cfg(sp1_debug_constraints) inside the function this library
// restates: `ShardProver::prove_shard_with_data` calls `debug_constraints_all_chips`
// (/root/reference/crates/hypercube/src/prover/shard.rs:L711-L720, crates/hypercube/src/debug.rs:L27-L125: "row N failed,
// constraint indices ..., row values ..."). A verifier's return code says that a proof is wrong; this says which chip, which row
// and which constraint.
//
// Mapping: one lane owns one row, lanes of a wave on consecutive rows, so every column load is 64 consecutive words of a
// column-major table. The walk over the program is the same in every lane: instruction words are read at wave-uniform addresses.
// The lane's register file lives in LDS, lane-interleaved (register r of lane l at word r * lanes + l: conflict-free), as in the
// zerocheck interpreter; no scratch, no per-lane array (profiles/trace_check_resource_usage.txt). 256 rows per workgroup unless the
// file forces fewer: the widest of 256 / 128 / 64 whose file fits a compute unit's 160 KB (tc_lanes_for), down to
// one wave at the budget of TC_MAX_REGS = 512 registers. A program that needs more (KeccakPermute: 2,285) is cut at assert
// boundaries into pieces that each fit, values two pieces need recomputed in both (zc_plain_pieces: the zerocheck's allocator and
// cutter on the caller's PLAIN SSA — HINT pseudo-instructions dropped, the caller's order, none of the fused pieces of zc_*.hpp,
// which are what this checks). A lane runs the pieces one after the other over the same file.
//
// Report, per chip, written by the kernel and read back once: failing_rows, first_row (atomic min), fail_count[k] per constraint,
// noncanonical (words >= p, by a streaming kernel of its own). Counters are touched on the failure path only, and a wave's lanes
// become ONE add per counter (ballot + popcount; cf. lc_add_combined of tracegen_lookup.hip). The entry point then fetches
// first_row's words and runs the host form of the same row function over them for the constraint indices failing there.
//
// Buses: `debug_interactions_with_all_chips`, which the reference's LogUp-GKR prover calls under the same cfg
// (/root/reference/crates/hypercube/src/logup_gkr/prover.rs:L99-L135, crates/hypercube/src/lookup/debug.rs:L48-L200), without a
// host-side map of every message. Pass 1: one lane one row, every interaction of the chip (compiled by lc_compile_interactions,
// evaluated by lc_form: tg_lookup_counts.hpp); a message with multiplicity m != 0 is folded into two independent 64-bit hashes of
// (kind, number of values, canonical values) (tc_rows.hpp: ia_message) and m — or m - p when m > p / 2 —, negated for a receive,
// is added with a device-scope 64-bit atomic to one bucket in each of two tables of 2^log_buckets signed sums, lanes of a wave
// that hold the same bucket combined into one add first. Verdict: balanced exactly when every bucket of both tables is 0 mod p.
// The collision argument: a key whose sends and receives cancel adds 0 mod p to its buckets whatever else lands there, so a
// balanced shard is never called unbalanced. A wrong "balanced" needs every non-zero discrepancy to be cancelled inside its bucket in
// the first table AND inside its bucket in the second: with k unbalanced keys some two of them must share a bucket under both
// hashes — probability of order k^2 / 2^(2 log_buckets), 2^-44 per pair at the default 22 — and their discrepancies must then sum
// to 0 mod p in both. Pass 2, a second launch, only when the first table has a non-zero bucket: the messages again, a 4-word record
// (chip, interaction, row, canonical multiplicity) for each one whose bucket of the first table is non-zero, into a buffer of the
// caller's size beside a counter of the records wanted; beyond the buffer `truncated` is set, the verdict stands and an arbitrary
// subset is kept. The exact answer is the caller's: sum the records' messages by key (api.check_interactions); balanced keys that
// merely share a bucket cancel there.
#include <algorithm>
#include <cstring>
#include <memory>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "common.hpp"
#include "tc_rows.hpp"
#include "zc_compile.hpp"

namespace sp1hip {
namespace tc {

constexpr uint32_t TC_COUNTER_HEADER = 4;          // u32 words: [0..1] noncanonical (u64), [2] failing rows, [3] first row; then fail_count[]
constexpr unsigned TC_MAX_BLOCKS = 2048;

// the reports as the ABI lays them out in u64 words (include/sp1hip.h: SP1HIP_CHECK_REPORT_WORDS, SP1HIP_CHECK_BUSES_WORDS)
struct Report {
    uint64_t failing_rows, first_row, noncanonical, fail_count_offset, row_offset, pieces, registers, lanes, n_first, first_constraints[TC_MAX_FIRST];
};
struct BusesReport {
    uint64_t messages, nonzero_buckets[2], records_wanted, records, balanced, truncated, spare;
};
static_assert(sizeof(Report) == 8 * SP1HIP_CHECK_REPORT_WORDS && sizeof(BusesReport) == 8 * SP1HIP_CHECK_BUSES_WORDS, "report layouts");

struct Compiled {
    std::vector<uint32_t> source, words;
    uint32_t main_w = 0, prep_w = 0, max_regs = 0, n_publics = 0;      // n_publics: one past the largest public value read
};

// HINT (16) is a pseudo-instruction of the SSA; everything else must be a value or an assert, in SSA order, inside the tables.
static const char* validate_program(const uint32_t* program, uint32_t n_instr, uint32_t main_w, uint32_t prep_w, uint32_t num_constraints,
                                    uint32_t* n_publics) {
    uint32_t asserts = 0, pub = 0;
    for (uint32_t k = 0; k < n_instr; k++) {
        const uint32_t op = program[3 * k], a = program[3 * k + 1], b = program[3 * k + 2];
        if (op == ZC_HINT) continue;
        if (op > ZC_ASSERT_ZERO) return "bad opcode in constraint program";
        if (op == ZC_LOAD_MAIN && a >= main_w) return "main column out of range";
        if (op == ZC_LOAD_PREP && a >= prep_w) return "preprocessed column out of range";
        if (op == ZC_PUBLIC) { if (a >= (1u << 24)) return "public value index out of range"; pub = a + 1 > pub ? a + 1 : pub; }
        if (op >= ZC_ADD && op <= ZC_MUL && (a >= k || b >= k)) return "constraint program is not in SSA order";
        if ((op == ZC_NEG || op == ZC_ASSERT_ZERO) && a >= k) return "constraint program is not in SSA order";
        if (op >= ZC_ADD && program[3 * a] == ZC_HINT) return "a HINT pseudo-instruction used as a value";
        if (op >= ZC_ADD && op <= ZC_MUL && program[3 * b] == ZC_HINT) return "a HINT pseudo-instruction used as a value";
        if (op >= ZC_ADD && (program[3 * a] == ZC_ASSERT_ZERO || (op <= ZC_MUL && program[3 * b] == ZC_ASSERT_ZERO))) return "an assert used as a value";
        asserts += op == ZC_ASSERT_ZERO;
    }
    if (asserts != num_constraints) return "num_constraints does not match the program";
    *n_publics = pub;
    return nullptr;
}

// The compiled form of a program, made once per process and looked up afterwards (like ZcPlan).
static int get_compiled(const uint32_t* program, uint32_t n_instr, uint32_t main_w, uint32_t prep_w, uint32_t num_constraints, uint32_t max_regs,
                        std::shared_ptr<const Compiled>* out) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint32_t v) { h = (h ^ v) * 1099511628211ull; };
    mix(main_w); mix(prep_w); mix(n_instr); mix(max_regs);
    for (size_t k = 0; k < (size_t)n_instr * 3; k++) mix(program[k]);
    static std::mutex mutex;
    static std::unordered_map<uint64_t, std::shared_ptr<const Compiled>> cache;
    {
        std::lock_guard<std::mutex> lk(mutex);
        auto it = cache.find(h);
        if (it != cache.end() && it->second->main_w == main_w && it->second->prep_w == prep_w && it->second->max_regs == max_regs &&
            it->second->source.size() == (size_t)n_instr * 3 && (n_instr == 0 || memcmp(it->second->source.data(), program, (size_t)n_instr * 12) == 0)) {
            SP1HIP_REQUIRE(it->second->words[3] == num_constraints, "num_constraints does not match the program");
            *out = it->second;
            return SP1HIP_SUCCESS;
        }
    }
    std::shared_ptr<Compiled> c(new Compiled());
    c->main_w = main_w; c->prep_w = prep_w; c->max_regs = max_regs;
    const char* why = validate_program(program, n_instr, main_w, prep_w, num_constraints, &c->n_publics);
    SP1HIP_REQUIRE(why == nullptr, why);
    c->source.assign(program, program + (size_t)n_instr * 3);
    std::vector<Chunk> pieces;
    if (num_constraints) SP1HIP_TRY(zc_plain_pieces(program, n_instr, main_w, prep_w, max_regs, &pieces));
    uint32_t regs = 1;
    for (const Chunk& p : pieces) regs = std::max(regs, p.n_regs);
    c->words.assign(TC_HEADER, 0u);
    for (const Chunk& p : pieces) {
        c->words.push_back((uint32_t)(p.prog.size() / 4));
        c->words.push_back(p.n_regs);
        c->words.insert(c->words.end(), p.prog.begin(), p.prog.end());
    }
    SP1HIP_REQUIRE(c->words.size() < (1ull << 32), "compiled program of 2^32 words or more");
    c->words[0] = (uint32_t)pieces.size(); c->words[1] = regs; c->words[2] = tc_lanes_for(regs); c->words[3] = num_constraints;
    c->words[4] = (uint32_t)c->words.size();
    SP1HIP_REQUIRE(c->words[2] != 0, "internal: a register file that does not fit LDS");
    why = tc_check_words(c->words.data(), c->words.size(), main_w, prep_w, c->n_publics, max_regs);
    if (why) { set_error("internal: %s", why); return SP1HIP_ERROR_RUNTIME; }
    std::lock_guard<std::mutex> lk(mutex);
    if (cache.size() > 4096) cache.clear();
    cache[h] = c;
    *out = c;
    return SP1HIP_SUCCESS;
}

__device__ __forceinline__ void tc_atomic_add(uint32_t* p, uint32_t v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Called by whole waves at every assert: nothing but a ballot unless a lane fails.
struct DeviceSink {
    uint32_t* fail_count;
    bool live;
    bool* failed;
    __device__ __forceinline__ void operator()(uint32_t index, uint32_t value) const {
        const bool bad = live && value != 0;
        const uint64_t who = __ballot(bad);
        if (who) {
            *failed |= bad;
            if (__lane_id() == (uint32_t)__builtin_ctzll(who)) tc_atomic_add(fail_count + index, (uint32_t)__popcll(who));
        }
    }
};

// prog: the compiled words; the file: blockDim.x * registers words of dynamic LDS. rows >= 1; a lane past the end walks the last row
// and reports nothing. No barrier: a lane reads only what it wrote.
__global__ __launch_bounds__(256) void tc_check_kernel(const uint32_t* __restrict__ prog, const uint32_t* __restrict__ main,
                                                       const uint32_t* __restrict__ prep, uint32_t rows, const uint32_t* __restrict__ publics,
                                                       uint32_t* __restrict__ counters) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = row < rows;
    const uint32_t at = live ? row : rows - 1;
    bool failed = false;
    const DeviceSink sink{counters + TC_COUNTER_HEADER, live, &failed};
    const uint32_t n_pieces = prog[0];
    const uint32_t* p = prog + TC_HEADER;
    for (uint32_t piece = 0; piece < n_pieces; piece++) {
        const uint32_t n = p[0];
        tc_run_piece(p + TC_PIECE_HEADER, n, lds + threadIdx.x, blockDim.x, main + at, (size_t)rows, prep + at, (size_t)rows, publics, sink);
        p += TC_PIECE_HEADER + 4 * (size_t)n;
    }
    const uint64_t who = __ballot(failed);
    if (who && __lane_id() == (uint32_t)__builtin_ctzll(who)) {      // the lowest failing lane holds the wave's smallest failing row
        tc_atomic_add(counters + 2, (uint32_t)__popcll(who));
        (void)__hip_atomic_fetch_min(counters + 3, row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Words at or above the modulus in n words: one 64-bit add per wave that found any.
__global__ __launch_bounds__(256) void tc_noncanonical_kernel(const uint32_t* __restrict__ table, uint64_t n, uint32_t* __restrict__ counters) {
    uint32_t mine = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) mine += table[i] >= kb::P;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if (mine && __lane_id() == 0)
        (void)__hip_atomic_fetch_add((unsigned long long*)counters, (unsigned long long)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- buses ---------------------------------------------------------------------------------------------------------------------
// table[bucket] += add for the lanes with `pending`, lanes of one bucket combined into ONE add first (messages are very uneven: a
// fifth of a shard's byte lookups address one cell), as lc_add_combined of tracegen_lookup.hip does. Called by whole waves.
constexpr int IA_COMBINE_ROUNDS = 4;
__device__ __forceinline__ void ia_atomic_add(long long* p, long long v) {
    (void)__hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ia_add_combined(long long* table, bool pending, uint32_t bucket, long long add) {
    const uint32_t lane = __lane_id();
    uint64_t todo = __ballot(pending);
    for (int round = 0; round < IA_COMBINE_ROUNDS && todo; round++) {
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const uint32_t b = __shfl(bucket, leader, 64);
        const long long a0 = __shfl(add, leader, 64);
        const bool same = pending && bucket == b;
        const uint64_t group = __ballot(same);
        long long sum = a0 * (long long)__popcll(group);      // the usual multiplicity is a flag: every lane of the group holds the leader's
        if (__ballot(same && add != a0)) {
            sum = same ? add : 0ll;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
        }
        if (lane == leader) ia_atomic_add(table + b, sum);
        pending = pending && !same;
        todo &= ~group;
        if ((group & (group - 1)) == 0) break;                // nobody shared the leader's bucket: take the rest as they are
    }
    if (pending) ia_atomic_add(table + bucket, add);
}

// Pass 1: one lane one row, grid-stride; every interaction of the chip on the row; tables: [2][1 << log_buckets] signed sums.
// counters[0..1]: messages (u64), one add per wave at the end.
__global__ __launch_bounds__(256) void ia_tally_kernel(const uint32_t* __restrict__ prog, const uint32_t* __restrict__ main,
                                                       const uint32_t* __restrict__ prep, uint32_t rows, long long* __restrict__ tables,
                                                       uint32_t log_buckets, uint32_t* __restrict__ counters) {
    const uint32_t n = prog[0];
    long long* second = tables + ((size_t)1 << log_buckets);
    uint32_t sent = 0;
    for (uint32_t base = blockIdx.x * 256u; base < rows; base += gridDim.x * 256u) {
        const uint32_t row = base + threadIdx.x;
        const bool live = row < rows;
        const uint32_t at = live ? row : rows - 1;         // a lane past the end reads the last row and sends nothing
        const uint32_t* rec = prog + 1;
        for (uint32_t k = 0; k < n; k++, rec += rec[1]) {
            const IaMsg msg = ia_message(rec, main, prep, rows, at);
            const bool has = live && msg.m != 0;
            if (!__ballot(has)) continue;
            sent += has;
            ia_add_combined(tables, has, ia_bucket(msg.ha, log_buckets), (long long)msg.add);
            ia_add_combined(second, has, ia_bucket(msg.hb, log_buckets), (long long)msg.add);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sent += __shfl_xor(sent, d, 64);
    if (sent && __lane_id() == 0)
        (void)__hip_atomic_fetch_add((unsigned long long*)counters, (unsigned long long)sent, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The verdict: buckets that are not 0 mod p, per table -> counters[2 + 2 t .. ] (u64 each).
__global__ __launch_bounds__(256) void ia_verdict_kernel(const long long* __restrict__ tables, uint32_t log_buckets, uint32_t* __restrict__ counters) {
    const uint64_t per = (uint64_t)1 << log_buckets;
    for (uint32_t t = 0; t < 2; t++) {
        uint32_t mine = 0;
        for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < per; i += (uint64_t)gridDim.x * 256u) {
            const long long v = tables[t * per + i];
            mine += v != 0 && v % (long long)kb::P != 0;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
        if (mine && __lane_id() == 0)
            (void)__hip_atomic_fetch_add((unsigned long long*)(counters + 2 + 2 * t), (unsigned long long)mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// Pass 2: the messages again; one whose bucket of the FIRST table is not 0 mod p draws a slot (a returning add, on this path only)
// and, if the slot is inside the buffer, leaves its record. counters[6..7]: records wanted (u64).
__global__ __launch_bounds__(256) void ia_who_kernel(const uint32_t* __restrict__ prog, const uint32_t* __restrict__ main, const uint32_t* __restrict__ prep,
                                                     uint32_t rows, const long long* __restrict__ tables, uint32_t log_buckets, uint32_t chip,
                                                     uint32_t* __restrict__ records, uint64_t cap, uint32_t* __restrict__ counters) {
    const uint32_t n = prog[0];
    for (uint32_t base = blockIdx.x * 256u; base < rows; base += gridDim.x * 256u) {
        const uint32_t row = base + threadIdx.x;
        if (row >= rows) continue;
        const uint32_t* rec = prog + 1;
        for (uint32_t k = 0; k < n; k++, rec += rec[1]) {
            const IaMsg msg = ia_message(rec, main, prep, rows, row);
            if (msg.m == 0) continue;
            const long long v = tables[ia_bucket(msg.ha, log_buckets)];
            if (v == 0 || v % (long long)kb::P == 0) continue;
            const unsigned long long slot = __hip_atomic_fetch_add((unsigned long long*)(counters + 6), 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (slot < cap) {
                uint32_t* out = records + slot * IA_RECORD_WORDS;
                out[0] = chip; out[1] = rec[0]; out[2] = row; out[3] = msg.m;
            }
        }
    }
}

static unsigned blocks_for(uint64_t n) { return (unsigned)((n + 255) / 256 < TC_MAX_BLOCKS ? (n + 255) / 256 : TC_MAX_BLOCKS); }

}  // namespace tc
}  // namespace sp1hip

using namespace sp1hip;

extern "C" {

int sp1hip_trace_check_compile(const uint32_t* program, uint32_t n_instr, uint32_t main_width, uint32_t prep_width, uint32_t num_constraints,
                               uint32_t max_regs, uint32_t* out_words, size_t* n_words) {
    SP1HIP_REQUIRE((program || n_instr == 0) && n_words, "null argument");
    SP1HIP_REQUIRE(n_instr < (1u << 28), "a program of 2^28 instructions or more");
    if (max_regs == 0) max_regs = tc::TC_MAX_REGS;
    SP1HIP_REQUIRE(max_regs >= 8 && tc::tc_lanes_for(max_regs) != 0, "max_regs: between 8 and what one wave's file can hold in LDS (640)");
    std::shared_ptr<const tc::Compiled> c;
    SP1HIP_TRY(tc::get_compiled(program, n_instr, main_width, prep_width, num_constraints, max_regs, &c));
    const size_t have = *n_words;
    *n_words = c->words.size();
    if (!out_words || have < c->words.size()) {
        set_error("%s: the compiled program has %zu words", __func__, c->words.size());
        return SP1HIP_ERROR_BUFFER_TOO_SMALL;
    }
    memcpy(out_words, c->words.data(), c->words.size() * 4);
    return SP1HIP_SUCCESS;
}

int sp1hip_check_constraints(const sp1hip_shard_chip_t* chips, int n_chips, const uint32_t* h_publics, int n_publics,
                             uint64_t* reports_words, uint32_t* h_words, size_t* n_words, sp1hip_stream_t stream) {
    tc::Report* reports = (tc::Report*)reports_words;
    SP1HIP_REQUIRE(n_chips >= 0 && (chips || n_chips == 0) && n_words && n_publics >= 0 && (h_publics || n_publics == 0), "null argument");
    // arguments, then the size protocol, then work
    std::vector<std::shared_ptr<const tc::Compiled>> compiled((size_t)n_chips);
    size_t need = 0;
    for (int i = 0; i < n_chips; i++) {
        const sp1hip_shard_chip_t& c = chips[i];
        SP1HIP_REQUIRE(c.program || c.n_instr == 0, "null program");
        SP1HIP_REQUIRE(c.n_instr < (1u << 28) && c.main_width < (1u << 24) && c.prep_width < (1u << 24), "a program or a table too large");
        SP1HIP_REQUIRE(c.real_rows <= (1ull << 30), "a table taller than 2^30");
        SP1HIP_REQUIRE(c.real_rows == 0 || ((c.d_main || c.main_width == 0) && (c.d_prep || c.prep_width == 0)), "null table");
        SP1HIP_TRY(tc::get_compiled(c.program, c.n_instr, c.main_width, c.prep_width, c.num_constraints, tc::TC_MAX_REGS, &compiled[i]));
        SP1HIP_REQUIRE(compiled[i]->n_publics <= (uint32_t)n_publics, "a constraint program reads a public value that was not given");
        need += (size_t)c.num_constraints + c.main_width + c.prep_width;
    }
    for (int k = 0; k < n_publics; k++) SP1HIP_REQUIRE(h_publics[k] < kb::P, "a public value outside the field");
    const size_t have = *n_words;
    *n_words = need;
    if (have < need || (need && !h_words) || (n_chips && !reports_words)) {
        set_error("%s: the report needs %zu words", __func__, need);
        return SP1HIP_ERROR_BUFFER_TOO_SMALL;
    }
    // one device block: counters of every chip | compiled programs | public values
    std::vector<uint32_t> image;
    std::vector<size_t> counters_at((size_t)n_chips), prog_at((size_t)n_chips);
    for (int i = 0; i < n_chips; i++) {
        counters_at[i] = image.size();
        image.resize(image.size() + ((tc::TC_COUNTER_HEADER + (size_t)chips[i].num_constraints + 1) & ~(size_t)1), 0u);
        image[counters_at[i] + 3] = 0xffffffffu;
    }
    const size_t counter_words = image.size();
    for (int i = 0; i < n_chips; i++) {
        prog_at[i] = image.size();
        image.insert(image.end(), compiled[i]->words.begin(), compiled[i]->words.end());
    }
    const size_t publics_at = image.size();
    image.insert(image.end(), h_publics, h_publics + n_publics);
    image.push_back(0u);
    hipStream_t s = S(stream);
    const size_t bytes = image.size() * 4;
    void* d_block = nullptr;
    SP1HIP_TRY(arena_alloc(&d_block, bytes, s));
    uint32_t* d = (uint32_t*)d_block;
    int status = SP1HIP_SUCCESS;
    auto fail = [&](hipError_t e, const char* what) { if (status == SP1HIP_SUCCESS && e != hipSuccess) status = map_hip_error(e, what); };
    fail(hipMemcpyAsync(d, image.data(), bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync");
    std::unique_ptr<ScopedTimer> kernels_timer(new ScopedTimer("trace_check_constraints", s));      // the kernels of all chips (sp1hip_timers_*)
    for (int i = 0; i < n_chips && status == SP1HIP_SUCCESS; i++) {
        const sp1hip_shard_chip_t& c = chips[i];
        if (c.real_rows == 0) continue;
        const uint32_t rows = (uint32_t)c.real_rows;
        const uint32_t* w = compiled[i]->words.data();
        if (w[0]) {
            const uint32_t lanes = w[2];
            const size_t lds = (size_t)w[1] * 4 * lanes;
            if (lds > 48 * 1024) status = ensure_dynamic_lds((const void*)tc::tc_check_kernel, (int)tc::TC_LDS_CU);
            if (status != SP1HIP_SUCCESS) break;
            hipLaunchKernelGGL(tc::tc_check_kernel, dim3((rows + lanes - 1) / lanes), dim3(lanes), lds, s, (const uint32_t*)(d + prog_at[i]), c.d_main,
                               c.prep_width ? c.d_prep : c.d_main, rows, (const uint32_t*)(d + publics_at), d + counters_at[i]);
            fail(hipGetLastError(), "tc_check_kernel");
        }
        for (int t = 0; t < 2 && status == SP1HIP_SUCCESS; t++) {
            const uint64_t n = (uint64_t)rows * (t ? c.prep_width : c.main_width);
            if (!n) continue;
            hipLaunchKernelGGL(tc::tc_noncanonical_kernel, dim3(tc::blocks_for(n)), dim3(256), 0, s, t ? c.d_prep : c.d_main, n, d + counters_at[i]);
            fail(hipGetLastError(), "tc_noncanonical_kernel");
        }
    }
    kernels_timer.reset();
    std::vector<uint32_t> counters(counter_words);
    if (status == SP1HIP_SUCCESS && counter_words) fail(hipMemcpyAsync(counters.data(), d, counter_words * 4, hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
    if (status == SP1HIP_SUCCESS) fail(hipStreamSynchronize(s), "hipStreamSynchronize");
    // the reports; then the first failing row of every chip that has one, fetched (one strided copy per table) and re-evaluated here
    size_t at = 0;
    for (int i = 0; i < n_chips && status == SP1HIP_SUCCESS; i++) {
        const sp1hip_shard_chip_t& c = chips[i];
        const uint32_t* k = counters.data() + counters_at[i];
        tc::Report& r = reports[i];
        memset(&r, 0, sizeof r);
        memcpy(&r.noncanonical, k, 8);
        r.failing_rows = k[2];
        r.first_row = k[3] == 0xffffffffu ? ~0ull : k[3];
        r.pieces = compiled[i]->words[0]; r.registers = compiled[i]->words[1]; r.lanes = compiled[i]->words[2];
        r.fail_count_offset = at;
        memcpy(h_words + at, k + tc::TC_COUNTER_HEADER, (size_t)c.num_constraints * 4);
        at += c.num_constraints;
        r.row_offset = at;
        uint32_t* row = h_words + at;
        memset(row, 0, ((size_t)c.main_width + c.prep_width) * 4);
        at += (size_t)c.main_width + c.prep_width;
        if (r.failing_rows == 0) continue;
        if (c.main_width)
            fail(hipMemcpy2DAsync(row, 4, c.d_main + r.first_row, (size_t)c.real_rows * 4, 4, c.main_width, hipMemcpyDeviceToHost, s), "hipMemcpy2DAsync");
        if (c.prep_width && status == SP1HIP_SUCCESS)
            fail(hipMemcpy2DAsync(row + c.main_width, 4, c.d_prep + r.first_row, (size_t)c.real_rows * 4, 4, c.prep_width, hipMemcpyDeviceToHost, s), "hipMemcpy2DAsync");
    }
    if (status == SP1HIP_SUCCESS) fail(hipStreamSynchronize(s), "hipStreamSynchronize");
    arena_free(d_block, bytes, s);
    SP1HIP_TRY(status);
    for (int i = 0; i < n_chips; i++) {
        tc::Report& r = reports[i];
        if (r.failing_rows == 0) continue;
        const sp1hip_shard_chip_t& c = chips[i];
        const uint32_t* w = compiled[i]->words.data();
        const uint32_t* row = h_words + r.row_offset;
        std::vector<uint32_t> file(w[1] + 4u, 0u), failing;
        const uint32_t* p = w + tc::TC_HEADER;
        for (uint32_t piece = 0; piece < w[0]; piece++) {
            tc::tc_run_piece(p + tc::TC_PIECE_HEADER, p[0], file.data(), 1u, row, (size_t)1, row + c.main_width, (size_t)1, h_publics,
                             [&](uint32_t index, uint32_t value) { if (value != 0) failing.push_back(index); });
            p += tc::TC_PIECE_HEADER + 4 * (size_t)p[0];
        }
        std::sort(failing.begin(), failing.end());
        r.n_first = std::min<size_t>(failing.size(), tc::TC_MAX_FIRST);
        for (uint64_t k = 0; k < r.n_first; k++) r.first_constraints[k] = failing[k];
    }
    return SP1HIP_SUCCESS;
}

int sp1hip_check_interactions(const sp1hip_shard_chip_t* chips, int n_chips, uint32_t log_buckets, uint64_t* report_words, uint32_t* h_records,
                              uint64_t cap, sp1hip_stream_t stream) {
    SP1HIP_REQUIRE(n_chips >= 0 && (chips || n_chips == 0) && report_words && (h_records || cap == 0), "null argument");
    tc::BusesReport* report = (tc::BusesReport*)report_words;
    SP1HIP_REQUIRE(log_buckets >= 1 && log_buckets <= 26, "log_buckets: 1 to 26");
    SP1HIP_REQUIRE(cap <= (1ull << 28), "more than 2^28 records");
    std::vector<uint32_t> image(8, 0u);                       // the counters, then every chip's compiled interactions
    std::vector<size_t> prog_at((size_t)n_chips);
    for (int i = 0; i < n_chips; i++) {
        const sp1hip_shard_chip_t& c = chips[i];
        SP1HIP_REQUIRE(c.interactions && c.n_words >= 1, "no interaction words");
        SP1HIP_REQUIRE(c.real_rows <= (1ull << 30), "a table taller than 2^30");
        SP1HIP_REQUIRE(c.real_rows == 0 || ((c.d_main || c.main_width == 0) && (c.d_prep || c.prep_width == 0)), "null table");
        std::vector<uint32_t> prog;
        const char* why = tg::lc_compile_interactions(c.interactions, c.n_words, c.main_width, c.prep_width, true, prog);
        SP1HIP_REQUIRE(why == nullptr, why);
        prog_at[i] = image.size();
        image.insert(image.end(), prog.begin(), prog.end());
    }
    memset(report, 0, sizeof *report);
    hipStream_t s = S(stream);
    const size_t image_bytes = image.size() * 4, table_bytes = ((size_t)16) << log_buckets, record_bytes = (size_t)cap * tc::IA_RECORD_WORDS * 4;
    void *d_image = nullptr, *d_tables = nullptr, *d_records = nullptr;
    SP1HIP_TRY(arena_alloc(&d_image, image_bytes, s));
    int status = arena_alloc(&d_tables, table_bytes, s);
    if (status == SP1HIP_SUCCESS && record_bytes) status = arena_alloc(&d_records, record_bytes, s);
    auto fail = [&](hipError_t e, const char* what) { if (status == SP1HIP_SUCCESS && e != hipSuccess) status = map_hip_error(e, what); };
    uint32_t* d = (uint32_t*)d_image;
    if (status == SP1HIP_SUCCESS) fail(hipMemcpyAsync(d, image.data(), image_bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync");
    if (status == SP1HIP_SUCCESS) fail(hipMemsetAsync(d_tables, 0, table_bytes, s), "hipMemsetAsync");
    for (int pass = 0; pass < 2 && status == SP1HIP_SUCCESS; pass++) {
        std::unique_ptr<ScopedTimer> pass_timer(new ScopedTimer(pass ? "trace_check_buses_pass2" : "trace_check_buses_pass1", s));
        for (int i = 0; i < n_chips && status == SP1HIP_SUCCESS; i++) {
            const sp1hip_shard_chip_t& c = chips[i];
            if (c.real_rows == 0 || image[prog_at[i]] == 0) continue;
            const uint32_t rows = (uint32_t)c.real_rows;
            const uint32_t* d_main = c.main_width ? c.d_main : c.d_prep;     // a width of 0 is never read; the pointer is never null
            const uint32_t* d_prep = c.prep_width ? c.d_prep : c.d_main;
            if (pass == 0)
                hipLaunchKernelGGL(tc::ia_tally_kernel, dim3(tc::blocks_for(rows)), dim3(256), 0, s, (const uint32_t*)(d + prog_at[i]), d_main, d_prep, rows,
                                   (long long*)d_tables, log_buckets, d);
            else
                hipLaunchKernelGGL(tc::ia_who_kernel, dim3(tc::blocks_for(rows)), dim3(256), 0, s, (const uint32_t*)(d + prog_at[i]), d_main, d_prep, rows,
                                   (const long long*)d_tables, log_buckets, (uint32_t)i, (uint32_t*)d_records, cap, d);
            fail(hipGetLastError(), pass ? "ia_who_kernel" : "ia_tally_kernel");
        }
        if (pass == 0 && status == SP1HIP_SUCCESS) {
            hipLaunchKernelGGL(tc::ia_verdict_kernel, dim3(tc::blocks_for((uint64_t)1 << log_buckets)), dim3(256), 0, s, (const long long*)d_tables, log_buckets, d);
            fail(hipGetLastError(), "ia_verdict_kernel");
            pass_timer.reset();
            // a balanced shard needs no second pass: the verdict is read first
            uint32_t k[8] = {0};
            fail(hipMemcpyAsync(k, d, sizeof k, hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
            if (status == SP1HIP_SUCCESS) fail(hipStreamSynchronize(s), "hipStreamSynchronize");
            memcpy(&report->messages, k, 8);
            memcpy(&report->nonzero_buckets[0], k + 2, 8);
            memcpy(&report->nonzero_buckets[1], k + 4, 8);
            report->balanced = report->nonzero_buckets[0] == 0 && report->nonzero_buckets[1] == 0;
            if (report->nonzero_buckets[0] == 0) break;
        }
    }
    if (status == SP1HIP_SUCCESS && report->nonzero_buckets[0] != 0) {
        uint64_t wanted = 0;
        fail(hipMemcpyAsync(&wanted, d + 6, 8, hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
        if (status == SP1HIP_SUCCESS) fail(hipStreamSynchronize(s), "hipStreamSynchronize");
        report->records_wanted = wanted;
        report->records = wanted < cap ? wanted : cap;
        report->truncated = wanted > cap;
        if (status == SP1HIP_SUCCESS && report->records) {
            fail(hipMemcpyAsync(h_records, d_records, (size_t)report->records * tc::IA_RECORD_WORDS * 4, hipMemcpyDeviceToHost, s), "hipMemcpyAsync");
            if (status == SP1HIP_SUCCESS) fail(hipStreamSynchronize(s), "hipStreamSynchronize");
        }
    }
    if (d_records) arena_free(d_records, record_bytes, s);
    if (d_tables) arena_free(d_tables, table_bytes, s);
    arena_free(d_image, image_bytes, s);
    return status;
}

}  // extern "C"
