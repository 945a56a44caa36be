/* include/sp1hip.h — C ABI of libsp1hip.so, the MI355X (gfx950) backend for SP1's core-shard
 * commit/open hot path.
 *
 * This is the drop-in boundary: plain `extern "C"` functions, raw device pointers, sizes, no C++ or
 * torch types. It follows the conventions of the reference's own GPU FFI crate `sp1-gpu-sys`
 * (/root/reference/sp1-gpu/crates/sys/src/runtime.rs:L3-L172): the caller owns every buffer,
 * every compute call is asynchronous on the given stream, field elements are u32 words in
 * Montgomery form (R = 2^32) exactly as `KoalaBear` is laid out in Rust memory, extension elements
 * are 4 consecutive words. A Rust crate wraps these the way `sp1-gpu-cudart` wraps `sp1-gpu-sys`
 * (see INTEGRATION.md).
 *
 * Device layouts:
 *   base tensor   [height x width]  COLUMN-major: word (row r, col c) at  c*height + r
 *   ext vector    [len]             4 base columns (SoA): coordinate k of element i at k*len + i
 *   digest        8 words, array-of-structs
 *   Merkle tree   leaf-first layers back to back: 2^h leaf digests, 2^(h-1) parents, ..., root;
 *                 (2^(h+1) - 1) digests in total
 *
 * Every function returns SP1HIP_SUCCESS (0) or a negative sp1hip_status; the message for the
 * calling thread's last failure is sp1hip_last_error(). Nothing throws across this ABI.
 */
#ifndef SP1HIP_H
#define SP1HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    SP1HIP_SUCCESS = 0,
    SP1HIP_ERROR_INVALID_ARGUMENT = -1,
    SP1HIP_ERROR_OUT_OF_MEMORY = -2,   /* cf. CUDA_OUT_OF_MEMORY,       runtime.rs:L3-L15 */
    SP1HIP_ERROR_NOT_READY = -3,       /* cf. CUDA_ERROR_NOT_READY_SLOP, runtime.rs:L3-L15 */
    SP1HIP_ERROR_RUNTIME = -4,         /* any other HIP failure */
    SP1HIP_ERROR_NO_DEVICE = -5,
    SP1HIP_ERROR_BUFFER_TOO_SMALL = -6
} sp1hip_status;

typedef void* sp1hip_stream_t; /* hipStream_t; NULL = the default stream */
typedef void* sp1hip_event_t;  /* hipEvent_t */

/* Extension-field element passed by value (4 Montgomery words). */
typedef struct { uint32_t c[4]; } sp1hip_ext_t;

/* One committed tensor of a `Message<Tensor>`: column-major device data, `width` columns. */
typedef struct {
    const uint32_t* d_data;
    uint32_t width;
} sp1hip_tensor_t;

const char* sp1hip_last_error(void);
const char* sp1hip_version(void);

/* ---------------------------------------------------------------- runtime
 * Replaces sp1-gpu-sys `cuda_malloc[_async]`, `cuda_free[_async]`, `cuda_malloc_host`,
 * `cuda_mem_copy_*`, `cuda_stream_*`, `cuda_event_*`, `cuda_mem_get_info`
 * (/root/reference/sp1-gpu/crates/sys/src/runtime.rs:L16-L172). */
int sp1hip_device_count(int* count);
int sp1hip_set_device(int device);
int sp1hip_get_device(int* device);
int sp1hip_mem_info(size_t* free_bytes, size_t* total_bytes);
/* The library keeps its working buffers (codewords, trees, fold layers) in per-stream free lists so that
 * steady-state proving never calls the driver; this returns every cached block to the driver. */
int sp1hip_mem_trim(size_t* released_bytes);
/* A caller stream that has been passed to this library owns helper streams (the commit's encode stream, the zerocheck's fork
 * streams), their events and the working buffers cached for it and for them. Call this BEFORE destroying such a stream (the
 * prover pool does it for its own slots): it waits for the stream, destroys the helpers and hands every block cached for them
 * and for the stream back to the driver. Without it the helpers outlive the stream, and a later stream that reuses the handle
 * value would inherit them. */
int sp1hip_stream_release(sp1hip_stream_t stream);
/* Host threads (the caller included) the library uses for the arithmetic between device hand-overs: SP1HIP_HOST_THREADS,
 * else min(8, CPUs / (2 x LOCAL_WORLD_SIZE)) with CPUs honouring the cgroup quota. Decided once per process. */
int sp1hip_host_threads(void);
int sp1hip_malloc(void** d_ptr, size_t bytes);
int sp1hip_free(void* d_ptr);
int sp1hip_malloc_async(void** d_ptr, size_t bytes, sp1hip_stream_t stream);
int sp1hip_free_async(void* d_ptr, sp1hip_stream_t stream);
int sp1hip_malloc_host(void** h_ptr, size_t bytes);
int sp1hip_free_host(void* h_ptr);
int sp1hip_memcpy_h2d_async(void* d_dst, const void* h_src, size_t bytes, sp1hip_stream_t stream);
int sp1hip_memcpy_d2h_async(void* h_dst, const void* d_src, size_t bytes, sp1hip_stream_t stream);
int sp1hip_memcpy_d2d_async(void* d_dst, const void* d_src, size_t bytes, sp1hip_stream_t stream);
int sp1hip_memset_async(void* d_dst, int value, size_t bytes, sp1hip_stream_t stream);
int sp1hip_stream_create(sp1hip_stream_t* stream);
int sp1hip_stream_destroy(sp1hip_stream_t stream);     /* releases what the library keeps for the stream first (sp1hip_stream_release) */
int sp1hip_stream_synchronize(sp1hip_stream_t stream);
int sp1hip_stream_query(sp1hip_stream_t stream); /* SP1HIP_ERROR_NOT_READY while work is pending */
int sp1hip_event_create(sp1hip_event_t* event);
int sp1hip_event_destroy(sp1hip_event_t event);
int sp1hip_event_record(sp1hip_event_t event, sp1hip_stream_t stream);
int sp1hip_event_synchronize(sp1hip_event_t event);
int sp1hip_event_elapsed_ms(float* ms, sp1hip_event_t start, sp1hip_event_t stop);
int sp1hip_stream_wait_event(sp1hip_stream_t stream, sp1hip_event_t event);

/* ---------------------------------------------------------------- kernel timers (measurement aid)
 * When enabled, the library brackets its hot kernels with HIP events on the caller's stream
 * (the equivalent of the reference's NVTX ranges + `SP1_GPU_*_TIMING` switches,
 * /root/reference/sp1-gpu/crates/tracing/src/tracer.rs). `sp1hip_timers_read` synchronises the recorded
 * events and returns, for `name` ("leaf_hash", "compress", "ntt_pass", ...), the number of launches and
 * their summed duration since the last `sp1hip_timers_reset`. */
int sp1hip_timers_enable(int on);
int sp1hip_timers_reset(void);
int sp1hip_timers_read(const char* name, uint64_t* launches, double* total_ms);

/* ---------------------------------------------------------------- layout
 * Host traces are row-major `[rows][cols]` (`RowMajorMatrix`, slop Tensor); the device wants
 * column-major. Replaces sp1-gpu's transpose kernels (/root/reference/sp1-gpu/crates/sys/lib/transpose). */
int sp1hip_transpose_to_col_major(uint32_t* d_out, const uint32_t* d_in_row_major, size_t rows, size_t cols,
                                  sp1hip_stream_t stream);
int sp1hip_transpose_to_row_major(uint32_t* d_out, const uint32_t* d_in_col_major, size_t rows, size_t cols,
                                  sp1hip_stream_t stream);
/* Host traces -> device tables in one call (staging half). Replaces the per-chip
 * "copy host trace to device" + `DeviceTensor::transpose` of `device_main_tracegen`
 * (/root/reference/sp1-gpu/crates/jagged_tracegen/src/lib.rs:L819-L835). Table i is `rows x cols` Montgomery
 * words, row-major, at h_data (pinned memory — `sp1hip_malloc_host` / `sp1hip_host_register` — for an
 * asynchronous copy at full PCIe rate; pageable memory works but is copied through the runtime's bounce
 * buffers); d_out[i] receives it column-major (`cols` columns of `rows` words). Chunked copies on a side
 * stream overlap the transposes on `stream`; returns after enqueueing. The host buffers must stay untouched
 * until `stream` has passed this call. */
typedef struct {
    const uint32_t* h_data;
    uint64_t rows;
    uint32_t cols;
} sp1hip_host_table_t;
int sp1hip_stage_tables(const sp1hip_host_table_t* tables, int n_tables, uint32_t* const* d_out, sp1hip_stream_t stream);
/* hipHostRegister / hipHostUnregister on caller-owned memory (the reference's `cuda_host_register`,
 * /root/reference/sp1-gpu/crates/sys/src/runtime.rs:L75-L172). */
int sp1hip_host_register(void* h_ptr, size_t bytes);
int sp1hip_host_unregister(void* h_ptr);
/* canonical <-> Montgomery, in place */
int sp1hip_to_monty(uint32_t* d_data, size_t n, sp1hip_stream_t stream);
int sp1hip_from_monty(uint32_t* d_data, size_t n, sp1hip_stream_t stream);

/* ---------------------------------------------------------------- Reed–Solomon encode (a4)
 * Replaces `Dft::dft(src, log_blowup, DftOrdering::BitReversed, dim = 0)` as called by
 * `CpuDftEncoder::encode_batch` (/root/reference/slop/crates/basefold-prover/src/encoder.rs:L22-L38,
 * /root/reference/slop/crates/dft/src/lib.rs:L17-L71) and sp1-gpu-sys `batch_coset_dft`
 * (/root/reference/sp1-gpu/crates/sys/src/dft.rs:L12-L59).
 * d_in: [2^lg_n x n_cols] column-major coefficients; d_out: [2^(lg_n+lg_blowup) x n_cols]
 * column-major, row j of a column holds f(w_N^{bitrev(j)}). d_out must not alias d_in. */
int sp1hip_rs_encode_batch(uint32_t* d_out, const uint32_t* d_in, int lg_n, int lg_blowup, size_t n_cols,
                           sp1hip_stream_t stream);

/* ---------------------------------------------------------------- Poseidon2 Merkle TCS (a2, a3, a6)
 * Replaces `TensorCsProver::commit_tensors` / `prove_openings_at_indices` and
 * `ComputeTcsOpenings::compute_openings_at_indices`
 * (/root/reference/slop/crates/merkle-tree/src/tcs.rs:L15-L47, p3sync.rs:L40-L238).
 * d_tree: (2^(lg_height+1) - 1) * 8 words. d_root_and_commit: 16 words — the Merkle root followed by
 * the commitment compress(root, hash([lg_height, total_width])). */
int sp1hip_merkle_commit(const sp1hip_tensor_t* tensors, int n_tensors, int lg_height, uint32_t* d_tree,
                         uint32_t* d_root_and_commit, sp1hip_stream_t stream);
/* d_indices: n_idx row indices. d_values: [n_idx][total_width] row-major (tensor order);
 * d_paths: [n_idx][lg_height][8]. Either output may be NULL. */
int sp1hip_merkle_open(const sp1hip_tensor_t* tensors, int n_tensors, int lg_height, const uint32_t* d_tree,
                       const uint32_t* d_indices, size_t n_idx, uint32_t* d_values, uint32_t* d_paths,
                       sp1hip_stream_t stream);
/* Batched permutations / hashes for testing and for small host-side uses:
 * d_states [n][16] permuted in place. */
int sp1hip_poseidon2_permute(uint32_t* d_states, size_t n, sp1hip_stream_t stream);
/* The same permutation in its all-integer formulation (modular-add linear layers, unsigned Montgomery S-box). The
 * production kernels use the exact-fp64 linear layer + signed S-box of sp1_amd/csrc/poseidon2.hpp; this entry point
 * exists so that the two independent formulations can be compared on hundreds of millions of states. */
int sp1hip_poseidon2_permute_integer_form(uint32_t* d_states, size_t n, sp1hip_stream_t stream);
/* The Fiat-Shamir transcript's permutation, on the HOST (no device needed): h_states [n][16] canonical Montgomery
 * words, permuted in place. The transcript is a duplex sponge (`DuplexChallenger<F, Perm, 16, 8>` through
 * `IopCtx::Challenger`, /root/reference/slop/crates/challenger/src/lib.rs:L25-L87): every permutation waits for the
 * one before, and the GPU waits for the transcript, so its latency is proof time. form 0 = what the transcript runs
 * (AVX-512 on CPUs that have it: sp1_amd/csrc/p2_host.cpp; the scalar integer form otherwise), 1 = scalar integer
 * form, 2 = scalar fp64 form; all three return the same words. sp1hip_host_permutation_is_vectorised: 1 if form 0 is
 * the AVX-512 path on this CPU. */
int sp1hip_poseidon2_permute_host(uint32_t* h_states, size_t n, int form);
int sp1hip_host_permutation_is_vectorised(void);
/* Host-only test hooks for the vectorised interaction-variable rounds of LogUp-GKR (sp1_amd/csrc/gkr_host.cpp; the rounds of
 * `InteractionLayer`, /root/reference/crates/hypercube/src/logup_gkr/logup_poly.rs:L240-L316, on coefficient planes): tab = 4 tables
 * (n0, d0, n1, d1) x 4 planes of `stride` words (multiple of 16, >= 2 * pairs rounded up to 8, + 16), eq = 4 planes of eq_stride
 * words. sums: out24 = [x0 | y0 | xh | yh | e0 | es] over the first real_pairs (even, odd) pairs; fold: out[k] = t[2k] +
 * alpha (t[2k+1] - t[2k]). Return 0, or -1 when the CPU has no AVX-512 (the library then runs the scalar rounds) or an
 * argument is malformed. */
int sp1hip_gkr_host_simd_available(void);
int sp1hip_gkr_host_round_sums(const uint32_t* tab, size_t stride, const uint32_t* eq, size_t eq_stride, size_t real_pairs, uint32_t* out24);
int sp1hip_gkr_host_round_fold(const uint32_t* tab, uint32_t* out, size_t stride, size_t real_pairs, const uint32_t* alpha4);

/* ---------------------------------------------------------------- the commit path over BabyBear (BASELINE config 2, "both fields")
 * The second `IopCtx` of the reference (/root/reference/slop/crates/baby-bear/src/baby_bear_poseidon2.rs:L11-L55): p = 2^31 - 2^27 + 1,
 * Montgomery words (R = 2^32), Poseidon2 width 16 with x^7, 8 + 13 rounds, same sponge / compression / commit_tensors and the same
 * layouts as the KoalaBear entry points above. PARITY NOTE: the internal diffusion matrix is not restated in the reference tree
 * (oracle/bb_commit.hpp). sp1hip_bb_commit_mles: d_codewords[k] receives the codeword of mle k (2^(lg_n + lg_blowup) x width,
 * column-major), d_tree the (2^(lg + 1) - 1) digests leaf-first; synchronises the stream to return the commitment. */
int sp1hip_bb_rs_encode_batch(uint32_t* d_out, const uint32_t* d_in, int lg_n, int lg_blowup, size_t n_cols, sp1hip_stream_t stream);
int sp1hip_bb_merkle_commit(const sp1hip_tensor_t* tensors, int n_tensors, int lg_height, uint32_t* d_tree,
                            uint32_t* d_root_and_commit, sp1hip_stream_t stream);
int sp1hip_bb_commit_mles(const sp1hip_tensor_t* mles, int n_mles, int lg_n, int lg_blowup, uint32_t* const* d_codewords,
                          uint32_t* d_tree, uint32_t h_commit[8], sp1hip_stream_t stream);
int sp1hip_bb_poseidon2_permute(uint32_t* d_states, size_t n, sp1hip_stream_t stream);

/* ---------------------------------------------------------------- BaseFold kernels (a13, a14)
 * batch: out[r] = sum_c coeff[c] * col_c[r] over all columns of all tensors (message order)
 *   (`FriCpuProver::batch`, /root/reference/slop/crates/basefold-prover/src/fri.rs:L31-L80).
 *   d_coeffs: [total_cols] ext, array-of-structs (4 words each). d_out: ext vector [2^lg_height]. */
int sp1hip_basefold_batch(const sp1hip_tensor_t* tensors, int n_tensors, int lg_height,
                          const uint32_t* d_coeffs, uint32_t* d_out, sp1hip_stream_t stream);
/* codeword fold (`p3_fri::fold_even_odd` as called at fri.rs:L118): ext vector 2^lg_n -> 2^(lg_n-1) */
int sp1hip_fold_even_odd(const uint32_t* d_codeword, int lg_n, sp1hip_ext_t beta, uint32_t* d_out,
                         sp1hip_stream_t stream);
/* `Mle::fold` (/root/reference/slop/crates/multilinear/src/fold.rs:L12-L26): out[i] = m[2i] + beta m[2i+1] */
int sp1hip_fold_mle(const uint32_t* d_mle, int lg_n, sp1hip_ext_t beta, uint32_t* d_out, sp1hip_stream_t stream);
/* eq(point, .) table (`partial_lagrange`, /root/reference/slop/crates/multilinear/src/lagrange.rs:L19-L45);
 * h_point: dim ext elements on the host; d_out: ext vector [2^dim]. */
int sp1hip_partial_lagrange(const sp1hip_ext_t* h_point, int dim, uint32_t* d_out, sp1hip_stream_t stream);
/* `eval_mle_at_point` for every column (/root/reference/slop/crates/multilinear/src/eval.rs:L9-L21):
 * d_evals[c] = sum_r d_eq[r] * col_c[r]; d_evals: [total_cols] ext array-of-structs. */
int sp1hip_mle_eval_columns(const sp1hip_tensor_t* tensors, int n_tensors, int lg_height, const uint32_t* d_eq,
                            uint32_t* d_evals, sp1hip_stream_t stream);
/* `Mle::fixed_at_zero` for an ext mle (/root/reference/slop/crates/multilinear/src/restrict.rs:L75-L87):
 * d_out[4] = sum_i d_eq[i] * d_mle[2 i]; d_mle ext vector [2^lg_n], d_eq ext vector [2^(lg_n-1)]. */
int sp1hip_ext_fixed_at_zero(const uint32_t* d_mle, int lg_n, const uint32_t* d_eq, uint32_t* d_out,
                             sp1hip_stream_t stream);

/* `mle_fix_last_variable` for a whole table (/root/reference/slop/crates/multilinear/src/restrict.rs:L10-L72; the
 * zerocheck prover's per-round table update, /root/reference/crates/hypercube/src/prover/zerocheck/mod.rs:L156-L171):
 * out[i][c] = x + alpha (y - x), x = row 2i, y = row 2i + 1, or the column's padding value when 2i + 1 == rows.
 * d_in: column-major, `rows x width` base words (in_is_ext == 0) or the extension layout below (in_is_ext != 0).
 * d_out: extension table of ceil(rows / 2) rows in the layout the sumcheck kernels use: word q of column c, row i at
 * d_out[(4 c + q) * out_rows + i]. d_padding: `width` base words (or 4 width words, (c, q) order, for an extension
 * input) in DEVICE memory, or NULL for zero padding. */
int sp1hip_fix_last_variable(const uint32_t* d_in, uint64_t rows, uint32_t width, int in_is_ext, sp1hip_ext_t alpha,
                             const uint32_t* d_padding, uint32_t* d_out, sp1hip_stream_t stream);

/* ---------------------------------------------------------------- transcript (a17)
 * `DuplexChallenger<KoalaBear, KoalaPerm, 16, 8>` (/root/reference/slop/crates/challenger/src/lib.rs:L25-L87).
 * Host object; `grind` runs the witness search on the GPU and returns the SMALLEST valid witness. */
typedef struct sp1hip_challenger_s sp1hip_challenger_t;
int sp1hip_challenger_new(sp1hip_challenger_t** out);
int sp1hip_challenger_clone(const sp1hip_challenger_t* ch, sp1hip_challenger_t** out);
void sp1hip_challenger_free(sp1hip_challenger_t* ch);
int sp1hip_challenger_observe(sp1hip_challenger_t* ch, const uint32_t* felts, size_t n);
int sp1hip_challenger_sample(sp1hip_challenger_t* ch, uint32_t* out);
int sp1hip_challenger_sample_ext(sp1hip_challenger_t* ch, sp1hip_ext_t* out);
int sp1hip_challenger_sample_bits(sp1hip_challenger_t* ch, int bits, uint32_t* out);
int sp1hip_challenger_check_witness(sp1hip_challenger_t* ch, int bits, uint32_t witness, int* ok);
int sp1hip_challenger_grind(sp1hip_challenger_t* ch, int bits, uint32_t* witness, sp1hip_stream_t stream);
/* Proof-of-work witnesses to USE instead of searching, in the order the proof grinds (a shard proof: LogUp-GKR 12 bits,
 * BaseFold batching 5 bits, BaseFold queries `proof_of_work_bits`); canonical words, at most 4. The reference's rayon
 * `find_any` (and its CUDA grind) return ANY valid witness, this library's search the smallest: a caller that replays a
 * Rust-made proof injects that proof's witnesses and gets the same bytes. An injected witness the transcript rejects
 * is an error (SP1HIP_ERROR_INVALID_ARGUMENT). Consumed by grind; cleared with n = 0. */
int sp1hip_challenger_inject_pow_witnesses(sp1hip_challenger_t* ch, const uint32_t* witnesses, int n);
/* 34 words: sponge state[16], n_in, in[8], n_out, out[8] */
int sp1hip_challenger_state(const sp1hip_challenger_t* ch, uint32_t* out34);

/* ---------------------------------------------------------------- BaseFold prover (a15, a16)
 * `BasefoldProver::commit_mles` (/root/reference/slop/crates/basefold-prover/src/prover.rs:L78-L99):
 * RS-encode every mle of one commitment round and Merkle-commit the codewords. The returned
 * handle owns the device codewords + tree (`BasefoldProverData`); the input mles stay caller-owned
 * and must outlive the handle (they are read again by `sp1hip_basefold_prove`). */
typedef struct sp1hip_basefold_data_s sp1hip_basefold_data_t;
int sp1hip_commit_mles(const sp1hip_tensor_t* mles, int n_mles, int lg_n, int lg_blowup, uint32_t h_commit[8],
                       sp1hip_basefold_data_t** out, sp1hip_stream_t stream);
/* Prover data is scratch of the stream it was committed on: freeing it orders the reuse of its blocks behind THAT stream's
 * work. A handle that was also opened on another stream (a proving key shared by provers on their own streams) waits for
 * the device when it is freed; do not free a handle while a prove call that uses it is still running on another thread. */
void sp1hip_basefold_data_free(sp1hip_basefold_data_t* data);
/* accessors for parity tests */
int sp1hip_basefold_data_codeword(const sp1hip_basefold_data_t* data, int mle_index, const uint32_t** d_codeword,
                                  uint32_t* width, int* lg_height);
int sp1hip_basefold_data_tree(const sp1hip_basefold_data_t* data, const uint32_t** d_tree, int* lg_height);

typedef struct {
    int log_blowup;          /* core: 2  (/root/reference/crates/primitives/src/fri_params.rs:L5-L15) */
    int num_queries;         /* core: 124 */
    int proof_of_work_bits;  /* core: 16 */
} sp1hip_fri_config_t;

/* `BasefoldProver::prove_trusted_mle_evaluations` (prover.rs:L102-L243). `rounds[r]` are the handles of the commitment rounds in
 * order; h_claims holds one ext per column flattened round -> mle -> column. Writes the bincode encoding of `BasefoldProof`
 * (/root/reference/slop/crates/basefold/src/verifier.rs:L94-L116) into h_proof (capacity *proof_len on entry, size on return;
 * SP1HIP_ERROR_BUFFER_TOO_SMALL sets the needed size and leaves the challenger untouched). Malformed input (a round of another
 * dimension or blowup, a claims count other than the total width, dim + log_blowup > 24, proof_of_work_bits >= 31) is
 * SP1HIP_ERROR_INVALID_ARGUMENT before any device work and before the size protocol (a too-small buffer does not change that). */
int sp1hip_basefold_prove(const sp1hip_ext_t* h_point, int dim, sp1hip_basefold_data_t* const* rounds, int n_rounds,
                          const sp1hip_ext_t* h_claims, size_t n_claims, sp1hip_fri_config_t config,
                          sp1hip_challenger_t* challenger, uint8_t* h_proof, size_t* proof_len,
                          sp1hip_stream_t stream);
size_t sp1hip_basefold_proof_size(int dim, const uint32_t* round_widths, int n_rounds, sp1hip_fri_config_t config);

/* ---------------------------------------------------------------- stacked + jagged commit (a5, a7, a8)
 * One chip table: column-major [rows x cols] device words (rows = real rows, no padding). */
typedef struct {
    const uint32_t* d_data;
    uint64_t rows;
    uint32_t cols;
} sp1hip_table_t;
typedef struct sp1hip_stacked_data_s sp1hip_stacked_data_t;

/* `StackedPcsProver::commit_multilinears` (/root/reference/slop/crates/stacked/src/prover.rs:L59-L94) with
 * `interleave_multilinears_with_fixed_rate` (/root/reference/slop/crates/stacked/src/fixed_rate.rs:L6-L47):
 * dense column-major concatenation of the tables, zero-padded to a multiple of 2^log_stacking_height
 * (at least one column), cut into batches of `batch_size` stacked columns, BaseFold-committed.
 * The tables are copied; the returned handle owns the dense buffer and the BaseFold data. */
int sp1hip_stacked_commit(const sp1hip_table_t* tables, int n_tables, int log_stacking_height, int batch_size,
                          int lg_blowup, uint32_t h_commit[8], uint64_t* num_added_vals, sp1hip_stacked_data_t** out,
                          sp1hip_stream_t stream);
void sp1hip_stacked_data_free(sp1hip_stacked_data_t* data);
int sp1hip_stacked_data_info(const sp1hip_stacked_data_t* data, sp1hip_basefold_data_t** basefold, int* n_batches,
                             const uint32_t** d_dense, uint64_t* padded_area);
int sp1hip_stacked_batch(const sp1hip_stacked_data_t* data, int k, sp1hip_tensor_t* batch);
/* `JaggedProver::commit_multilinears` (/root/reference/slop/crates/jagged/src/prover.rs:L106-L160), the call made by
 * `ShardProver::commit_traces` (/root/reference/crates/hypercube/src/prover/shard.rs:L462-L468): tables with zero
 * rows are counted but not committed; the result is compress(stacked_commit, hash([n + 2, rows.., cols..]))
 * with the two padding tables appended. */
int sp1hip_jagged_commit(const sp1hip_table_t* tables, int n_tables, int max_log_row_count, int log_stacking_height,
                         int batch_size, int lg_blowup, uint32_t h_commit[8], sp1hip_stacked_data_t** out,
                         sp1hip_stream_t stream);

/* ---------------------------------------------------------------- jagged PCS evaluation proof
 * `JaggedProver::prove_trusted_evaluations` (/root/reference/slop/crates/jagged/src/prover.rs:L162-L328): the jagged
 * sumcheck over the dense vector (`HadamardProduct`, hadamard.rs:L52-L146), the jagged-eval sumcheck
 * (jagged_eval/sumcheck_eval.rs:L185-L243) and the stacked / BaseFold opening of the dense commitments
 * (stacked/src/prover.rs:L107-L152) — everything between the zerocheck point and the end of the shard proof's
 * `evaluation_proof`. rounds[r]: handles returned by sp1hip_jagged_commit, in commitment order (SP1:
 * preprocessed, main); h_z_row: the zerocheck point (max_log_row_count ext); h_claims: the evaluations at z_row
 * of every column of every table of every round (round -> table -> column; no padding columns),
 * claims_per_round[r] of them for round r. Writes bincode(JaggedPcsProof)
 * (/root/reference/slop/crates/jagged/src/verifier.rs:L17-L26) into h_proof (capacity *proof_len on entry, size on
 * return; SP1HIP_ERROR_BUFFER_TOO_SMALL sets the needed size). The challenger is advanced only on success. */
int sp1hip_jagged_prove(const sp1hip_ext_t* h_z_row, int max_log_row_count, sp1hip_stacked_data_t* const* rounds,
                        int n_rounds, const sp1hip_ext_t* h_claims, const size_t* claims_per_round,
                        sp1hip_fri_config_t config, sp1hip_challenger_t* challenger, uint8_t* h_proof,
                        size_t* proof_len, sp1hip_stream_t stream);

/* ---------------------------------------------------------------- LogUp-GKR
 * One chip of the shard for the lookup argument. `interactions`: HOST words describing its sends (first) and
 * receives, the data form of `Interaction { values: Vec<VirtualPairCol>, multiplicity, kind }`
 * (/root/reference/crates/hypercube/src/lookup/interaction.rs:L11-L24):
 *   [n_interactions, then per interaction: is_send, kind, n_values, vcol(multiplicity), vcol(value_0), ...]
 *   vcol = [n_terms, constant (canonical), then n_terms x (is_main, column, weight (canonical))]
 * Traces: column-major device tensors with `real_rows` rows. Chips must be passed in name order (BTreeSet<Chip>). */
typedef struct {
    const char* name;
    const uint32_t* interactions;
    uint32_t n_words;
    uint32_t main_width, prep_width;
    const uint32_t* d_main;
    const uint32_t* d_prep;
    uint64_t real_rows;
} sp1hip_gkr_chip_t;

/* `GkrProverImpl::prove_logup_gkr` (/root/reference/crates/hypercube/src/logup_gkr/prover.rs:L70-L215): 12-bit grind,
 * alpha / beta challenges, the fraction circuit over every (row, interaction) (execution.rs:L112-L382), one degree-3
 * sumcheck per circuit layer (cpu.rs:L146-L226, logup_poly.rs:L70-L553) and the trace-column openings at the
 * final point. Writes bincode(LogupGkrProof) (/root/reference/crates/hypercube/src/logup_gkr/proof.rs:L32-L62): its
 * `logup_evaluations` (point + per-chip openings) are the `h_zeta` / `h_openings` inputs of
 * sp1hip_zerocheck_prove. The challenger is advanced only on success. */
int sp1hip_logup_gkr_prove(const sp1hip_gkr_chip_t* chips, int n_chips, int max_log_row_count,
                           sp1hip_challenger_t* challenger, uint8_t* h_proof, size_t* proof_len,
                           sp1hip_stream_t stream);

/* ---------------------------------------------------------------- zerocheck (a9-a12)
 * One chip of the shard. `program` is a HOST array of n_instr [op, a, b] triples in SSA form
 * (instruction k defines value k): 0 LOAD_MAIN col, 1 LOAD_PREP col, 2 CONST canonical, 3 PUBLIC idx,
 * 4 ADD, 5 SUB, 6 MUL, 7 NEG a, 8 ASSERT_ZERO a — the data form of `Air::eval` over
 * `ConstraintSumcheckFolder` (/root/reference/crates/hypercube/src/folder.rs:L276-L323); single-row constraints.
 * Optional pseudo-instruction 16 HINT kind col (defines no value, asserts nothing): kind 1 = "the next 163 ASSERT_ZEROs are
 * the Poseidon2 permutation sub-AIR — eval_external_round r = 0..7, then eval_internal_rounds,
 * /root/reference/crates/hypercube/src/operations/poseidon2/air.rs:L66-L144 — over main columns [col, col + 179)"; the
 * prover then evaluates those constraints with a fused kernel instead of interpreting them (the hint is verified against the
 * program before it is used; SP1HIP_ZC_MACRO=0 ignores hints; the proof bytes do not depend on it).
 * Traces: column-major device tensors with `real_rows` rows (padding rows are implicit zeros). */
typedef struct {
    const uint32_t* program;
    uint32_t n_instr;
    uint32_t main_width, prep_width, num_constraints;
    const uint32_t* d_main;
    const uint32_t* d_prep;
    uint64_t real_rows;
} sp1hip_zc_chip_t;

/* `ShardProver::zerocheck` (/root/reference/crates/hypercube/src/prover/shard.rs:L474-L646): one sumcheck over all
 * chips (RLC with lambda sampled from the transcript), 2^max_log_row_count rows per chip. h_zeta: the
 * GKR point (max_log_row_count ext); h_openings: per chip, in order, the main then preprocessed column
 * evaluations at zeta; alpha / gkr_batch: the two challenges sampled by the caller before the call.
 * Output: bincode `PartialSumcheckProof<EF>` (/root/reference/slop/crates/sumcheck/src/proof.rs:L10-L14) followed by
 * u64 n_chips and, per chip, Vec<EF> = preprocessed then main column evaluations at the sumcheck point.
 * The challenger ends in the state after the openings have been observed (shard.rs:L609-L640). */
int sp1hip_zerocheck_prove(const sp1hip_zc_chip_t* chips, int n_chips, int max_log_row_count,
                           const sp1hip_ext_t* h_zeta, const sp1hip_ext_t* h_openings, sp1hip_ext_t alpha,
                           sp1hip_ext_t gkr_batch, const uint32_t* h_publics, int n_publics,
                           sp1hip_challenger_t* challenger, uint8_t* h_proof, size_t* proof_len,
                           sp1hip_stream_t stream);

/* Host-only check of the constraint-program compiler (no GPU needed): plans `program` exactly as sp1hip_zerocheck_prove
 * does (immediates folded, instruction order chosen, registers allocated, fused multiply-adds, forwarded operands; the
 * chunked / undivided / finely cut forms) and interprets the chosen form on ONE row (Montgomery words). form: 0 = the whole
 * allocated program, 1 = chunks, 2 = undivided, 3 = fine. out_values[k] = value of constraint k at the row; out_stats
 * (optional) = {instruction words, pieces, registers}. Fails if a constraint is not evaluated exactly once. */
int sp1hip_zerocheck_plan_eval(const uint32_t* program, uint32_t n_instr, uint32_t main_width, uint32_t prep_width,
                               const uint32_t* main_row, const uint32_t* prep_row, const uint32_t* publics,
                               uint32_t n_publics, int form, uint32_t* out_values, uint32_t n_constraints,
                               uint32_t* out_stats);
/* Host-only check of the polynomial-identity pieces (hint kind 7, sp1_amd/csrc/zc_poly.hpp) without a GPU: plans `program`, builds
 * every identity's device table for the batching challenge `alpha` exactly as sp1hip_zerocheck_prove does, and evaluates the
 * tables on ONE main row the way the kernels do (affine forms, then products). out_collapsed = the sum over the identities of
 * their batched value; out_direct = the same sum taken constraint by constraint, sum_k alpha^(n - 1 - k) C_k(row) over the
 * constraints the identities cover (n = num constraints of the program); *n_identities = how many hints the planner accepted.
 * Equal for every row and alpha, or the pieces are wrong. */
int sp1hip_zerocheck_poly_check(const uint32_t* program, uint32_t n_instr, uint32_t main_width, uint32_t prep_width,
                                const uint32_t* main_row, sp1hip_ext_t alpha, sp1hip_ext_t* out_collapsed, sp1hip_ext_t* out_direct,
                                uint32_t* n_identities);
/* Host-only: the bilinear extension of a column's row quad (r00, r01, r10, r11 = rows 4q .. 4q + 3, Montgomery words) at node
 * `node` (0 .. 11) of the bivariate grid the fused first two zerocheck rounds evaluate — the same function the kernels call
 * (zc_biv_interp: one 36-bit accumulation and its reduction); for tests of its edge cases without a GPU. */
int sp1hip_zerocheck_biv_interp_host(uint32_t r00, uint32_t r01, uint32_t r10, uint32_t r11, uint32_t node, uint32_t* out);

/* ---------------------------------------------------------------- one whole shard proof
 * A chip of the shard with everything the stages need: constraint program (zerocheck, see sp1hip_zc_chip_t),
 * interaction program (LogUp-GKR, see sp1hip_gkr_chip_t) and its device traces. Chips in name order. */
typedef struct {
    const char* name;
    const uint32_t* program;        /* [n_instr][3] constraint program (host) */
    uint32_t n_instr, num_constraints;
    const uint32_t* interactions;   /* interaction program words (host) */
    uint32_t n_words;
    uint32_t main_width, prep_width;
    const uint32_t* d_main;
    const uint32_t* d_prep;
    uint64_t real_rows;
} sp1hip_shard_chip_t;

typedef struct {
    int max_log_row_count;          /* core: 22 */
    int log_stacking_height;        /* core: 21 */
    int batch_size;                 /* stacked columns per BaseFold batch */
    sp1hip_fri_config_t fri;
} sp1hip_shard_params_t;

/* `ShardProver::prove_shard_with_data` (/root/reference/crates/hypercube/src/prover/shard.rs:L650-L792) — the body of
 * `AirProver::prove_shard_with_pk`, the seam a proving backend plugs into. `preprocessed`: the proving key's
 * preprocessed commitment round (sp1hip_jagged_commit over the preprocessed traces of the chips that have one, in
 * chip order, done once at setup). The challenger must already have absorbed the verifying key
 * (`vk.observe_into`). Commits the main traces, runs LogUp-GKR, zerocheck and the jagged evaluation proof in the
 * reference's transcript order and writes bincode(ShardProof)
 * (/root/reference/crates/hypercube/src/verifier/proof.rs:L47-L94). Size protocol and transcript commit-on-success as
 * for the stage entry points. */
int sp1hip_prove_shard(const sp1hip_shard_chip_t* chips, int n_chips, const uint32_t* h_publics, int n_publics,
                       sp1hip_stacked_data_t* preprocessed, sp1hip_shard_params_t params, sp1hip_challenger_t* challenger,
                       uint8_t* h_proof, size_t* proof_len, sp1hip_stream_t stream);

/* ---------------------------------------------------------------- device trace generation (recursion machine)
 * `CudaTracegenAir::generate_trace_device` of the recursion chips
 * (/root/reference/sp1-gpu/crates/tracegen/src/recursion/{alu_base,alu_ext,select,poseidon2_wide,prefix_sum_checks}.rs, mod.rs):
 * d_events = the execution record's event array copied to the device as is (Montgomery words in the `#[repr(C)]` layout
 * of /root/reference/crates/recursion/executor/src/lib.rs: BaseAluIo 3 words, ExtAluIo<Block> 12, SelectIo 5, MemEvent 4,
 * PrefixSumChecksEvent 20, Poseidon2Event 32 = input[16] | output[16]); d_trace = the chip's main trace, column-major
 * [width][height] (widths 3, 12, 5, 8, 15, 179), rows past the events are the reference's padding rows (zeros; for
 * Poseidon2 the permutation trace of the zero state). height >= the number of event rows (MemoryVar: 2 events per row). */
int sp1hip_tracegen_recursion_base_alu(uint32_t* d_trace, uint64_t height, const uint32_t* d_events, uint64_t n_events,
                                       sp1hip_stream_t stream);
int sp1hip_tracegen_recursion_ext_alu(uint32_t* d_trace, uint64_t height, const uint32_t* d_events, uint64_t n_events,
                                      sp1hip_stream_t stream);
int sp1hip_tracegen_recursion_select(uint32_t* d_trace, uint64_t height, const uint32_t* d_events, uint64_t n_events,
                                     sp1hip_stream_t stream);
int sp1hip_tracegen_recursion_memory_var(uint32_t* d_trace, uint64_t height, const uint32_t* d_events, uint64_t n_events,
                                         sp1hip_stream_t stream);
int sp1hip_tracegen_recursion_prefix_sum_checks(uint32_t* d_trace, uint64_t height, const uint32_t* d_events, uint64_t n_events,
                                                sp1hip_stream_t stream);
int sp1hip_tracegen_recursion_poseidon2_wide(uint32_t* d_trace, uint64_t height, const uint32_t* d_events, uint64_t n_events,
                                             sp1hip_stream_t stream);

/* Device trace generation for the RISC-V machine's Global chip (`CudaTracegenAir for GlobalChip`,
 * /root/reference/sp1-gpu/crates/sys/lib/tracegen/riscv/global.cu:L1-L252; CPU definition
 * /root/reference/crates/core/machine/src/global/mod.rs:L131-L260): events = `GlobalInteractionEvent { message: [u32; 8],
 * is_receive: bool, kind: u8 }` as 9 u32 words each (word 8 = is_receive | kind << 8, the `#[repr(C)]` image); writes the
 * column-major [241][height] table: message, limbs, the Poseidon2 permutation's 179 columns, the lifted curve point, the running
 * digest sum (a scan over the septic curve's group law) and the reference's padding rows. Synchronises the stream before it
 * returns (it reports an event without a curve point as an error). */
int sp1hip_tracegen_riscv_global(uint32_t* d_trace, uint64_t height, const uint32_t* d_events, uint64_t n_events,
                                 sp1hip_stream_t stream);

/* Device trace generation for the RISC-V instruction chips of a core shard (round 6): Add, Addi, Sub, Addw, Subw, Mul, ShiftRight,
 * Branch, Bitwise, Lt, ShiftLeft, UType, Jal, Jalr — `generate_trace_into` / `event_to_row` of
 * /root/reference/crates/core/machine/src/alu/{add_sub,addw,subw,mul,sr,bitwise,lt,sll}/, utype/ and control_flow/{branch,jal,jalr}/,
 * the R / I / ALU / J register adapters and CPUState they share (adapter/{state,register}, memory/consistency/trace.rs).
 * The reference fills these tables on the host and copies them (sp1-gpu/crates/jagged_tracegen/src/lib.rs:L819-L835); here a row
 * is made from an 88-byte event on the device. An event is the instruction's `AluEvent` / `BranchEvent` with its register access
 * records (core/executor/src/events/{alu,branch,memory}.rs), flattened:
 *   ops  = opcode | op_a << 8 | op_b << 16 | op_c << 24 | imm_b << 32 | imm_c << 33   (register numbers; Opcode as in opcode.rs)
 *   a / b / c = the operand values (a: the value written; c: the immediate when imm_c), a_prev = the value op_a held before
 *   (for a branch: the value of rs1), *_pts = the timestamp of the register's previous access, aux = next_pc (branches).
 *   An instruction whose operand b is an immediate (JAL, LUI, AUIPC: imm_b set) carries that immediate as b, and 0 as op_b; its
 *   op_c_imm is the same immediate for LUI / AUIPC and zero for JAL, so c is not read.
 * Writes the column-major [width][height] table in Montgomery words, rows >= n_events as the chip's padding rows. Clock carries
 * across 2^24 (MemoryBump / StateBump rows) stay with the caller: they are a handful of rows per shard. */
typedef struct { uint64_t pc, clk, ops, a, b, c, a_prev, a_pts, b_pts, c_pts, aux; } sp1hip_rv64_alu_event_t;
typedef enum { SP1HIP_RV64_CHIP_ADD = 0, SP1HIP_RV64_CHIP_ADDI = 1, SP1HIP_RV64_CHIP_SUB = 2, SP1HIP_RV64_CHIP_ADDW = 3, SP1HIP_RV64_CHIP_SUBW = 4,
               SP1HIP_RV64_CHIP_MUL = 5, SP1HIP_RV64_CHIP_SHIFT_RIGHT = 6, SP1HIP_RV64_CHIP_BRANCH = 7, SP1HIP_RV64_CHIP_BITWISE = 8,
               SP1HIP_RV64_CHIP_LT = 9, SP1HIP_RV64_CHIP_SHIFT_LEFT = 10, SP1HIP_RV64_CHIP_UTYPE = 11, SP1HIP_RV64_CHIP_JAL = 12,
               SP1HIP_RV64_CHIP_JALR = 13 } sp1hip_rv64_chip;
int sp1hip_tracegen_riscv_alu_width(int chip);       /* columns of the chip's table; -1 for an unknown chip */
int sp1hip_tracegen_riscv_alu(int chip, uint32_t* d_table, uint32_t height, const sp1hip_rv64_alu_event_t* d_events, uint32_t n_events,
                              sp1hip_stream_t stream);

/* Device trace generation for the nine load and store chips of a core shard: LoadByte, LoadHalf, LoadWord, LoadDouble, LoadX0 (a
 * load whose destination is x0), StoreByte, StoreHalf, StoreWord, StoreDouble — `event_to_row` of the reference's
 * crates/core/machine/src/memory/instructions/{load,store}/ with CPUState, the I register adapter, AddressOperation
 * (operations/address.rs) and MemoryAccessCols (memory/consistency/{columns,trace}.rs). An event is the instruction's
 * `MemInstrEvent` with its register access records and its memory record, flattened to twelve words (96 bytes; a row is 156-200):
 *   ops    = opcode | op_a << 8 | op_b << 16   (register numbers; Opcode as in opcode.rs), as in sp1hip_rv64_alu_event_t
 *   b      = the value of the base register, imm = the I-type immediate (op_c_imm), sign-extended
 *   a_prev = the value op_a held before (for a store: the value stored), a_pts / b_pts = the registers' previous timestamps
 *   m_addr = the byte address b + imm; m_pts / m_prev = the timestamp and content of its 8-byte word's previous access;
 *   m_new  = the word's content afterwards (= m_prev for a load). These three travel as the executor recorded them: the device
 *            does not re-derive what the instruction does to memory.
 * The memory access stands at clk + 1, the accesses of op_b and op_a at clk + 3 and clk + 4. Writes the column-major
 * [width][height] table in Montgomery words; rows >= n_events are zero rows, the padding of all nine chips. A register access across
 * a 2^24 clock boundary compares against 0 as above (its MemoryBump row stays with the caller); the memory access itself needs no
 * such row. */
typedef struct { uint64_t pc, clk, ops, b, imm, a_prev, a_pts, b_pts, m_addr, m_pts, m_prev, m_new; } /* 96 bytes */ sp1hip_rv64_mem_event_t;
typedef enum { SP1HIP_RV64_MEM_CHIP_LOAD_BYTE = 0, SP1HIP_RV64_MEM_CHIP_LOAD_HALF = 1, SP1HIP_RV64_MEM_CHIP_LOAD_WORD = 2,
               SP1HIP_RV64_MEM_CHIP_LOAD_DOUBLE = 3, SP1HIP_RV64_MEM_CHIP_LOAD_X0 = 4, SP1HIP_RV64_MEM_CHIP_STORE_BYTE = 5,
               SP1HIP_RV64_MEM_CHIP_STORE_HALF = 6, SP1HIP_RV64_MEM_CHIP_STORE_WORD = 7, SP1HIP_RV64_MEM_CHIP_STORE_DOUBLE = 8 } sp1hip_rv64_mem_chip;
int sp1hip_tracegen_riscv_mem_width(int chip);       /* columns of the chip's table; -1 for an unknown chip */
int sp1hip_tracegen_riscv_mem(int chip, uint32_t* d_table, uint32_t height, const sp1hip_rv64_mem_event_t* d_events, uint32_t n_events,
                              sp1hip_stream_t stream);

/* Device trace generation for three more tables of a core shard — DivRem, AluX0, MemoryLocal — and, with MemoryLocal, the events of
 * the shard's Global table. They have entry points of their own: the chip numbers above stay as they are.
 *   sp1hip_tracegen_riscv_divrem        DivRem, width 246 (`event_to_row` of crates/core/machine/src/alu/divrem/mod.rs): CPUState, the R
 *       adapter, quotient and remainder of DIV / DIVU / REM / REMU and their W forms (division by zero, signed overflow, the W forms'
 *       extension of their low halves), the three IsZeroWordOperations with their field inverses, the absolute values, the unsigned
 *       compare |remainder| < max(|c|, 1) when c != 0, c * quotient through one MulOperation (W forms) or two, and the 8 carries. Events
 *       are sp1hip_rv64_alu_event_t records as above. A padding row is the reference's "0 / 1" row: is_divu, c = abs_c = max_abs_c_or_1 =
 *       op_c's prev_value = 1, b_not_neg_not_overflow, is_c_0 of [1, 0, 0, 0].
 *   sp1hip_tracegen_riscv_alu_x0        AluX0, width 34 (alu/alu_x0.rs): CPUState, the ALU adapter, opcode, is_real — every ALU
 *       instruction whose destination is x0. The same records. Padding rows are zero.
 *   sp1hip_tracegen_riscv_memory_local  MemoryLocal, width 20 (memory/local.rs): one row per address the shard touched, from n_records
 *       x 5 u64 { addr, initial clk, initial value, final clk, final value }. Padding rows are zero. When d_global_events is not null it
 *       receives the rows' Global events in the form sp1hip_tracegen_riscv_global reads, [2 n_records][9] words: record i's initial state
 *       (a receive) at row 2 i and its final state (a send) at row 2 i + 1, message = clk_high, clk_low, addr[3], value[0] + lower * 2^16,
 *       value[1] + upper * 2^16, value[3], kind Memory. The buffer may be larger: what lies behind row 2 n_records is not touched.
 * Output: column-major [width][height] Montgomery words. Needs n <= height. All argument checks come before any launch; a null
 * pointer is accepted only with nothing to read or write (d_global_events: always); height == 0 succeeds without a launch. The calls
 * enqueue and return: they do not synchronise. */
int sp1hip_tracegen_riscv_divrem_width(void);          /* 246 */
int sp1hip_tracegen_riscv_alu_x0_width(void);          /* 34 */
int sp1hip_tracegen_riscv_memory_local_width(void);    /* 20 */
int sp1hip_tracegen_riscv_divrem(uint32_t* d_table, uint32_t height, const sp1hip_rv64_alu_event_t* d_events, uint32_t n_events, sp1hip_stream_t stream);
int sp1hip_tracegen_riscv_alu_x0(uint32_t* d_table, uint32_t height, const sp1hip_rv64_alu_event_t* d_events, uint32_t n_events, sp1hip_stream_t stream);
int sp1hip_tracegen_riscv_memory_local(uint32_t* d_table, uint32_t height, const uint64_t* d_records, uint32_t n_records, int32_t* d_global_events,
                                       sp1hip_stream_t stream);

/* A stable partition of a core shard's executed instructions on the device: from the executor's records as sp1hip_rv64_events
 * yields them (n_events x 20 u64 in device memory: pc, clk, opcode, op_a, op_b, op_c, flags (1: b is an immediate, 2: c is), a, b, c,
 * a_prev, a_pts, b_pts, c_pts, m_addr, m_pts, m_prev, m_new, next_pc, spare) to one record stream per BIN, in execution order inside
 * each bin, packed as the chips' kernels read them — what the tracing executor's emit_alu_event / emit_mem_instr_event do with an
 * instruction (core/executor/src/tracing.rs:L1096-L1228), and the selection of the StateBump and MemoryBump rows.
 *   bins  0..13  the chips of sp1hip_rv64_chip, same numbers            sp1hip_rv64_alu_event_t (11 words)
 *   bins 14..22  14 + sp1hip_rv64_mem_chip                              sp1hip_rv64_mem_event_t (12 words)
 *   bins 23, 24  DivRem, AluX0                                          sp1hip_rv64_alu_event_t
 *   bin  25      SyscallInstrs: every ECALL                             sp1hip_rv64_alu_event_t (a_prev = the syscall code)
 *   bin  26      SyscallCore: an ECALL with (code >> 8 & 0xFF) == 1     sp1hip_rv64_alu_event_t, the same record
 *   bin  27      StateBump: the clock step (8; 8 + 256 for an ECALL) carries out of the low 24 bits of clk, or pc + 4 out of the low
 *                16 bits of pc — not for branches, JAL, JALR and HALT   4 words: clk, pc, next_pc, clock step | pc_carry << 32
 *   bin  28      MemoryBump: one record per REGISTER ACCESS whose previous timestamp lies in another 2^24 window than the access
 *                (slot A at clk + 4, B at clk + 3, C at clk + 2; the slots the chip's adapter reads: A, B, C for Add, Sub, Subw, Mul,
 *                DivRem, SyscallInstrs; A, B for Addi, Branch, Jalr, loads and stores; A, B and a register C for Addw, ShiftRight,
 *                Bitwise, Lt, ShiftLeft, AluX0; A for UType, Jal)       4 words: register, previous timestamp, value,
 *                                                                       (access timestamp >> 24) << 24
 * A destination x0 sends an ALU opcode to AluX0 and a load to LoadX0. An event adds one record to exactly one of the bins 0..25, at
 * most one to bin 26 and to bin 27, and 0 to 3 to bin 28, there in the order A, B, C. EBREAK, UNIMP and numbers that are no opcode
 * add nothing. The record arena is one array of u64 words: bin b starts at the sum of the earlier bins' count x words.
 *   sp1hip_rv64_partition_scratch_bytes  the size of d_scratch for n_events: 32 u32 counters per workgroup of
 *                                        SP1HIP_RV64_PARTITION_WORKGROUP events (at least one row)
 *   sp1hip_rv64_partition_count          fills d_scratch and writes the SP1HIP_RV64_BINS record counts to d_counts (u32 each). The
 *                                        counts decide every table height, so the caller reads them back — 116 bytes — and sizes the
 *                                        arena exactly
 *   sp1hip_rv64_partition_scatter        packs and stores every record; d_scratch and d_counts as the first call left them. A record
 *                                        that would not fit into records_words words is not written
 * Bit-reproducible: no atomics, no workgroup waits on another. d_events is 16-byte aligned. At most 2^30 events. All argument checks
 * come before any launch; n_events == 0 succeeds without a launch and writes nothing (the counts are the caller's zeros). The calls
 * enqueue and return: they do not synchronise. */
#define SP1HIP_RV64_BINS 29
#define SP1HIP_RV64_PARTITION_WORKGROUP 256
#define SP1HIP_RV64_PARTITION_SCAN_SLICES 32        /* the scan gives each of its 32 lane-slices ceil(workgroups / 32) workgroups */
/* (DivRem's and AluX0's bins are spelt DIVIDE and X0: no constant of this header names those two chips as the chip enums would — they
 * have entry points of their own and no chip number, and tests/test_tracegen_riscv_core_abi.py keeps it so. csrc says BIN_DIVREM, BIN_ALU_X0.) */
typedef enum { SP1HIP_RV64_BIN_ALU = 0, SP1HIP_RV64_BIN_MEM = 14, SP1HIP_RV64_BIN_DIVIDE = 23 /* DivRem */, SP1HIP_RV64_BIN_X0 = 24 /* AluX0 */,
               SP1HIP_RV64_BIN_SYSCALL_INSTRS = 25, SP1HIP_RV64_BIN_SYSCALL_CORE = 26, SP1HIP_RV64_BIN_STATE_BUMP = 27,
               SP1HIP_RV64_BIN_MEMORY_BUMP = 28 } sp1hip_rv64_bin;
uint64_t sp1hip_rv64_partition_scratch_bytes(uint64_t n_events);
int sp1hip_rv64_partition_count(const uint64_t* d_events, uint64_t n_events, uint32_t* d_scratch, uint32_t* d_counts, sp1hip_stream_t stream);
int sp1hip_rv64_partition_scatter(const uint64_t* d_events, uint64_t n_events, const uint32_t* d_scratch, const uint32_t* d_counts,
                                  uint64_t* d_records, uint64_t records_words, sp1hip_stream_t stream);

/* Device trace generation for the four small chips of a core shard, from the records of the bins 25..28 above:
 *   sp1hip_tracegen_riscv_syscall_instrs  SyscallInstrs, width 65 (syscall/instructions/trace.rs event_to_row): CPUState, the R adapter,
 *       next_pc NOT normalised (limb 0 = pc[0] + 4; HALT: 1, 0, 0), is_halt, op_a_value, the low bytes of the code's limbs, the IsZero
 *       operations (inverse, result) of syscall_id - 0x03, 0xF0, 0x00, 0x10, 0x1A, the index bitmap of op_b & 7 and the digest bytes of
 *       op_c for COMMIT (bitmap only for COMMIT_DEFERRED_PROOFS), op_b_range_check = HALT and op_b's limb 1 < (p - 1) >> 16,
 *       op_c_range_check = COMMIT_DEFERRED_PROOFS and the same of op_c, is_real
 *   sp1hip_tracegen_riscv_syscall_core    SyscallCore, width 10 (syscall/chip.rs): clk_high, clk_low, syscall_id, arg1[3], arg2[3],
 *       is_real. When d_global_events is not null it receives the rows' Global events in the form sp1hip_tracegen_riscv_global reads,
 *       [n_events][9] words: message = clk_high, clk_low, syscall_id + arg1[0] * 2^8, arg1[1], arg1[2], arg2[3]; word 8 = kind Syscall
 *       << 8 (a send). Point it behind MemoryLocal's events
 *   sp1hip_tracegen_riscv_state_bump      StateBump, width 14 (adapter/bump.rs): the limbs of clk + step, clk_high, clk_low + step, next_pc,
 *       the pc the instruction's row sent (pc with limb 0 + 4 after a pc carry, else next_pc), is_clk, is_real
 *   sp1hip_tracegen_riscv_memory_bump     MemoryBump, width 15 (memory/bump.rs): prev_value[4], prev_high, prev_low, compare_low = 0, the
 *       two limbs of window - prev_high - 1, the window's clk limbs, the register, is_real
 * Output: column-major [width][height] Montgomery words, zero padding rows. Needs n <= height. All argument checks come before any
 * launch; a null pointer is accepted only with nothing to read or write (d_global_events: always); height == 0 succeeds without a
 * launch. The calls enqueue and return: they do not synchronise. */
int sp1hip_tracegen_riscv_syscall_instrs_width(void);  /* 65 */
int sp1hip_tracegen_riscv_syscall_core_width(void);    /* 10 */
int sp1hip_tracegen_riscv_state_bump_width(void);      /* 14 */
int sp1hip_tracegen_riscv_memory_bump_width(void);     /* 15 */
int sp1hip_tracegen_riscv_syscall_instrs(uint32_t* d_table, uint32_t height, const sp1hip_rv64_alu_event_t* d_events, uint32_t n_events,
                                         sp1hip_stream_t stream);
int sp1hip_tracegen_riscv_syscall_core(uint32_t* d_table, uint32_t height, const sp1hip_rv64_alu_event_t* d_events, uint32_t n_events,
                                       int32_t* d_global_events, sp1hip_stream_t stream);
int sp1hip_tracegen_riscv_state_bump(uint32_t* d_table, uint32_t height, const uint64_t* d_records, uint32_t n_records, sp1hip_stream_t stream);
int sp1hip_tracegen_riscv_memory_bump(uint32_t* d_table, uint32_t height, const uint64_t* d_records, uint32_t n_records, sp1hip_stream_t stream);

/* Device trace generation for the chips that close the shards WITHOUT instructions — a memory shard's two chips, and the three
 * chips every precompile shard has around its own — so that those shards are made on the device from the executor's records, as a
 * core shard is. The reference fills all of them on the host.
 *   sp1hip_tracegen_riscv_memory_global  MemoryGlobalInit (finalize = 0) / MemoryGlobalFinalize (finalize = 1), width 30, one layout
 *       for both (`generate_trace_into` of crates/core/machine/src/memory/global.rs): one row per address, from n_records x 3 u64
 *       { addr, value, timestamp } in strictly increasing address order. Row i holds clk_high, clk_low, index = i, prev_addr[3] (record
 *       i - 1's address; previous_addr for row 0: the last address of the previous memory shard, 0 for the first), addr[3], value[4],
 *       value_lower / value_upper (bytes 4 and 5), is_real, is_comp = prev != 0 or i != 0, prev_valid = 1 - (prev == 0 and i != 0), the
 *       IsZero operations (inverse, result) of prev_addr's limb sum and of the index, and lt_cols of prev < addr over four 16-bit limbs
 *       (bit, u16_flags[4]: the most significant limb that differs, not_eq_inv, comparison_limbs[2]), all times is_comp. The order of
 *       the addresses is not checked: a list that does not increase makes a row whose constraints fail. When d_global_events is not
 *       null it receives the rows' Global events in the form sp1hip_tracegen_riscv_global reads, [n_records][9] words: message = 0, 0
 *       (Init: timestamp zero whatever the clk columns hold) or clk_high, clk_low (Finalize), addr[3], value[0] + lower * 2^16, value[1] +
 *       upper * 2^16, value[3]; word 8 = kind Memory << 8 (Init: a send) or 1 | kind Memory << 8 (Finalize: a receive).
 *   sp1hip_tracegen_riscv_syscall_precompile  SyscallPrecompile, width 10 (syscall/chip.rs): clk_high, clk_low, syscall_id, arg1[3],
 *       arg2[3], is_real — one row per call, from a precompile's event records as the executor leaves them (n_events x words_per_event
 *       u64: word 0 the clk, word 1 the first pointer, word arg2_word the second, arg2_word = -1 for none). When d_global_events is not
 *       null it receives [n_events][9] words: message = clk_high, clk_low, syscall_id + arg1[0] * 2^8, arg1[1], arg1[2], arg2[3]; word 8 =
 *       1 | kind Syscall << 8 — the RECEIVE of what sp1hip_tracegen_riscv_syscall_core sends. Point it behind MemoryLocal's events.
 *   sp1hip_precompile_local_records      the MemoryLocal records { addr, initial clk, initial value, final clk, final value } of the
 *       words the calls touched, one per word of each call (not merged across calls), ready for sp1hip_tracegen_riscv_memory_local.
 *       `segments`: a HOST array of n_segments (1 to 4) x 5 u32 { ptr_word, count, pairs_word, final_word or 0xFFFFFFFF, final_clk_delta },
 *       read before the call returns. Word i < count of event e in segment s becomes record base_s + e * count_s + i, base_s = the sum
 *       of n_events * count over the earlier segments: addr = ev[ptr_word] + 8 i, initial clk = ev[pairs_word + 2 i], initial value =
 *       ev[pairs_word + 2 i + 1], final clk = ev[0] + final_clk_delta, final value = ev[final_word + i], or the initial value for
 *       0xFFFFFFFF (words only read). Keccak: 77 words, { 1, 25, 2, 52, 1 }; secp256k1 add: 43 words, { 1, 8, 3, 35, 1 } and
 *       { 2, 8, 19, none, 0 }; secp256k1 double: 26 words, { 1, 8, 2, 18, 0 }. d_records holds records_capacity records; the sum of
 *       n_events * count are written. Every segment must lie inside the event record.
 * Tables: column-major [width][height] Montgomery words, zero padding rows. Needs n <= height. All argument checks come before any
 * launch; a null pointer is accepted only with nothing to read or write (d_global_events: always); height == 0 (no records) succeeds
 * without a launch. The calls enqueue and return: they do not synchronise. */
int sp1hip_tracegen_riscv_memory_global_width(void);       /* 30 */
int sp1hip_tracegen_riscv_syscall_precompile_width(void);  /* 10 */
int sp1hip_tracegen_riscv_memory_global(int finalize, uint32_t* d_table, uint32_t height, const uint64_t* d_records, uint32_t n_records,
                                        uint64_t previous_addr, int32_t* d_global_events, sp1hip_stream_t stream);
int sp1hip_tracegen_riscv_syscall_precompile(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, uint32_t words_per_event,
                                             uint32_t syscall_id, int32_t arg2_word, int32_t* d_global_events, sp1hip_stream_t stream);
/* The same for a shard that mixes system calls (FpOpAssign, Fp2AddSubAssign): each row's syscall id is the low byte of its own event
 * word code_word (code_word < words_per_event) instead of one id per call. */
int sp1hip_tracegen_riscv_syscall_precompile_coded(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events,
                                                   uint32_t words_per_event, uint32_t code_word, int32_t arg2_word, int32_t* d_global_events,
                                                   sp1hip_stream_t stream);
int sp1hip_precompile_local_records(uint64_t* d_records, uint64_t records_capacity, const uint64_t* d_events, uint32_t n_events, uint32_t words_per_event,
                                    const uint32_t* segments, uint32_t n_segments, sp1hip_stream_t stream);

/* Device trace generation for the two chips of a KECCAK_PERMUTE precompile shard, from the executor's event records as they are
 * (sp1hip_rv64_keccak_events below: n_events x 77 u64 on the device — [0] clk, [1] state pointer, [2 + 2i] / [3 + 2i] the previous
 * timestamp and the word read of state word i < 25, [52 + i] the word written). The reference fills both tables on the host
 * (crates/core/machine/src/syscall/precompiles/keccak256/trace.rs:L63-L162, controller.rs:L155-L237) and has no device filler
 * for them; a call's rows are ~253 KB of table for a 616-byte event. Output as above: column-major [width][height] Montgomery words.
 *   sp1hip_tracegen_riscv_keccak          KeccakPermute, width 2640: row 24 e + r is round r of event e — KeccakCols (step_flags[24],
 *       export, preimage, a, c, c_prime, a_prime, a_prime_prime, a_prime_prime_0_0_bits, a_prime_prime_prime_0_0_limbs), clk_high,
 *       clk_low, state_addr[3], index, is_real. The permutation is computed from the words read. A padding row q >= 24 n_events is
 *       round q mod 24 of the permutation of the zero state with clk, state_addr, index and is_real zero. Needs 24 n_events <= height.
 *   sp1hip_tracegen_riscv_keccak_control  KeccakPermuteControl, width 634: one row per event — clk_high, clk_low, SyscallAddrOperation,
 *       25 AddrAddOperation values, is_real, 25 initial and 25 final MemoryAccessCols (reads at clk against the previous timestamps,
 *       writes at clk + 1 against clk), final_value from the words written. Padding rows are zero. Needs n_events <= height.
 * A null pointer is accepted only with a zero count / height; height == 0 succeeds without a launch. */
int sp1hip_tracegen_riscv_keccak_width(void);            /* 2640 */
int sp1hip_tracegen_riscv_keccak_control_width(void);    /* 634 */
int sp1hip_tracegen_riscv_keccak(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream);
int sp1hip_tracegen_riscv_keccak_control(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events,
                                         sp1hip_stream_t stream);

/* Device trace generation for the secp256k1 point-addition and point-doubling precompile chips, from the executor's event records as
 * they are (sp1hip_rv64_secp256k1_add_events: n_events x 43 u64 on the device — [0] clk, [1] p_ptr, [2] q_ptr, [3 + 2i] / [4 + 2i] the
 * previous timestamp and the word read of p word i < 8, [19 + 2i] / [20 + 2i] the same of q, [35 + i] the word written;
 * sp1hip_rv64_secp256k1_double_events: 26 u64 — [0] clk, [1] p_ptr, [2 + 2i] / [3 + 2i] of p word i, [18 + i] the word written). The
 * reference fills both tables on the host (crates/core/machine/src/syscall/precompiles/weierstrass/weierstrass_add.rs:L246-L330,
 * weierstrass_double.rs:L262-L380) and has no device filler for them. Output as above: column-major [width][height] Montgomery words,
 * one row per event.
 *   sp1hip_tracegen_riscv_secp256k1_add     Secp256k1AddAssign, width 1599: is_real, clk_high, clk_low, two SyscallAddrOperation, 8 + 8
 *       AddrAddOperation values, 8 + 8 MemoryAccessColsU8 (q read at clk, p rewritten at clk + 1), ten FieldOpCols in the order of
 *       populate_field_ops (L95-L165) and the FieldLtCols of x3 and y3. x3 and y3 are computed from the words read.
 *   sp1hip_tracegen_riscv_secp256k1_double  Secp256k1DoubleAssign, width 1591: the same with one pointer, 8 accesses (p rewritten in
 *       place at clk) and eleven FieldOpCols (weierstrass_double.rs:L89-L160; a = 0, the constants 3 and 2 as operands).
 * A padding row (row >= n_events) is the reference's dummy row: the field operations on p = (0, 0), q = (1, 1) (doubling: p = (0, 1)),
 * the dummy access record in q_access[0] and q_access[4] (doubling: p_access[4]), zero elsewhere. Needs n_events <= height.
 * Precondition, which the executor enforces before it records an event: the coordinates are reduced modulo the field's prime,
 * q.x != p.x for an addition, p.y != 0 for a doubling. An event that breaks it neither faults nor spins — the inverse of 0 comes out
 * as 0 — but its row satisfies no constraint system. All argument checks come before any launch; a null pointer is accepted only with
 * a zero count / height; height == 0 succeeds without a launch. The calls enqueue and return: they do not synchronise. */
int sp1hip_tracegen_riscv_secp256k1_add_width(void);      /* 1599 */
int sp1hip_tracegen_riscv_secp256k1_double_width(void);   /* 1591 */
int sp1hip_tracegen_riscv_secp256k1_add(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream);
int sp1hip_tracegen_riscv_secp256k1_double(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events,
                                           sp1hip_stream_t stream);

/* Device trace generation for the Weierstrass and Fp / Fp2 precompile chips of SP1HIP_RV64_FAMILY_* 0..11 (below), from the executor's
 * event records as sp1hip_rv64_precompile_events gives them (n_events x words u64 on the device): [0] clk, [1] arg1, [2] arg2, [3] the
 * system-call code — a FOUR-word head —, then per word i < W of the first operand [4 + 2i] / [5 + 2i] the previous timestamp and the
 * word read, the same of the second operand at [4 + 2W + 2i] (additions and the tower chips), then the W words written.
 *   family 0..5   Secp256r1 / Bn254 / Bls12381 AddAssign, DoubleAssign   W = 8, 8, 12    width 1599 / 1591, 1599 / 1591, 2399 / 2391
 *   family 6, 7   Bn254 / Bls12381 FpOpAssign                           W = 4, 6        width 306, 450
 *   family 8, 9   Bn254 / Bls12381 Fp2AddSubAssign                      W = 8, 12       width 592, 880
 *   family 10, 11 Bn254 / Bls12381 Fp2MulAssign                         W = 8, 12       width 1095, 1639
 * The reference fills these tables on the host (crates/core/machine/src/syscall/precompiles/weierstrass, fptower) and has no device
 * filler for them. Output: column-major [width][height] Montgomery words, one row per event. An FpOpAssign / Fp2AddSubAssign row takes
 * its operation from the low byte of word 3, so one call may mix ADD, SUB (and MUL). A padding row is the reference's dummy row: an
 * addition's field operations on p = (0, 0), q = (1, 1) with the dummy access record in q_access[0] and q_access[W / 2]; a doubling's on
 * p = (0, 1) with the record in p_access[W / 2]; a tower chip's operation on zero operands as an addition (is_add = 1).
 * The table is made in two launches through a work buffer of ops x (3 N + 1) x height u32 (N = 8 or 12 limbs of a field element;
 * ops = 10 / 11 / 1 / 2 / 6 FieldOpCols per row), which the call allocates and releases itself in stream order (hipMallocAsync /
 * hipFreeAsync on `stream`): the caller passes no scratch. Operands must be reduced, q.x != p.x for an addition, p.y != 0 for a
 * doubling, which the executor guarantees; an event that breaks it neither faults nor spins but its row satisfies no constraint
 * system. Families 12..14 (EdAddAssign, EdDecompress, Uint256Ops) and anything larger are refused with
 * SP1HIP_ERROR_INVALID_ARGUMENT and a message that names the family; the width query returns -1 for them. The other argument checks
 * are those above: n_events <= height, a null pointer only with a zero count / height, height == 0 succeeds without a launch. The
 * call enqueues and returns: it does not synchronise. */
int sp1hip_tracegen_riscv_field_chip_width(uint32_t family);   /* -1: no device filler */
int sp1hip_tracegen_riscv_field_chip(uint32_t family, uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events,
                                     sp1hip_stream_t stream);

/* Device trace generation for the last three chips behind sp1hip_rv64_precompile_events, SP1HIP_RV64_FAMILY_* 12..14, from the
 * executor's event records as they are (layouts below, at the family constants): EdAddAssign (ED_ADD, 44 u64 per event, width 1347),
 * EdDecompress (ED_DECOMPRESS, 24 u64, width 1123) and Uint256Ops (UINT256_ADD_CARRY and UINT256_MUL_CARRY, which one call may mix: the
 * row's operation is the low byte of word 3; 58 u64, width 477). The reference fills these tables on the host
 * (crates/core/machine/src/syscall/precompiles/edwards, uint256_ops) and has no device filler for them. Output: column-major
 * [width][height] Montgomery words, one row per event. A padding row is the reference's dummy row: EdAddAssign's field operations on
 * four zero coordinates and EdDecompress' on y = 0, both with a zero head; Uint256Ops zero except the 63 witness columns, which hold
 * the offset. The two Edwards tables are made in two launches through a work buffer of 8 x 40 (EdAddAssign) or 7 x 25 (EdDecompress)
 * u32 per row, which the call allocates and releases itself in stream order (hipMallocAsync / hipFreeAsync on `stream`): the caller
 * passes no scratch. Uint256Ops is one launch. Operands must be reduced, ED_ADD's denominators 1 +- d x1 x2 y1 y2 must not vanish and
 * ED_DECOMPRESS' (y^2 - 1) / (d y^2 + 1) must be a square, which the executor guarantees; an event that breaks it neither faults nor
 * takes longer, but its row satisfies no constraint system. All argument checks come before any launch: n_events <= height, a null
 * pointer only with a zero count / height; height == 0 succeeds without a launch. The calls enqueue and return: they do not
 * synchronise. */
int sp1hip_tracegen_riscv_ed_add_width(void);          /* 1347 */
int sp1hip_tracegen_riscv_ed_decompress_width(void);   /* 1123 */
int sp1hip_tracegen_riscv_uint256_ops_width(void);     /* 477 */
int sp1hip_tracegen_riscv_ed_add(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream);
int sp1hip_tracegen_riscv_ed_decompress(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream);
int sp1hip_tracegen_riscv_uint256_ops(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream);
/* The MemoryLocal records { addr, initial clk, initial value, final clk, final value } of the words the calls of an ED_DECOMPRESS or
 * a UINT256 carry shard touched, which the four segments of sp1hip_precompile_local_records cannot state (a pointer plus an offset;
 * a register's constant address with its value and timestamp in separate words; six runs). family = SP1HIP_RV64_FAMILY_ED_DECOMPRESS
 * or SP1HIP_RV64_FAMILY_UINT256_OPS, anything else is SP1HIP_ERROR_INVALID_ARGUMENT (ED_ADD is two plain segments). d_events:
 * n_events x 24 / 58 u64. Records: n_events x 8 / 23, run after run, event by event inside each run —
 *   ED_DECOMPRESS   the 4 x words at ptr + 8 i (pairs at event words 4 + 2 i, final clk + 1, final value word 20 + i), then the 4 y
 *                   words at ptr + 32 + 8 i (pairs at 12 + 2 i, final clk, value unchanged);
 *   UINT256 carry   registers 12, 13, 14 (addr = the register number, value word 4 + j, initial clk word 7 + j, final clk, value
 *                   unchanged), then the blocks a, b, c, d, e of 4 words (pointers at event words 1, 2, 4, 5, 6; pairs at
 *                   10 + 8 j + 2 i; final clk + j; a, b, c unchanged, d takes words 50..53, e words 54..57).
 * records_capacity: the records d_records has room for; too few, more than 2^31 - 1 records, or a null pointer with records to write
 * or events to read is SP1HIP_ERROR_INVALID_ARGUMENT before any launch. No events: success without a launch. */
int sp1hip_precompile_touched_records(uint64_t* d_records, uint64_t records_capacity, const uint64_t* d_events, uint32_t n_events, uint32_t family,
                                      sp1hip_stream_t stream);

/* Device trace generation for the four chips of the SHA_EXTEND and SHA_COMPRESS precompile shards, from the executor's event records
 * as they are (sp1hip_rv64_sha_extend_events: n_events x 786 u64 on the device — [0] clk, [1] w_ptr, [2 + 11 r ..] step r < 48: four
 * (previous timestamp, word read) pairs for w[i-15], w[i-2], w[i-16], w[i-7], then w[i]'s previous timestamp, previous value and new
 * value, [530 + 4 k ..] word k < 64 of w: initial timestamp, initial value, final timestamp, final value;
 * sp1hip_rv64_sha_compress_events: 155 u64 — [0] clk, [1] w_ptr, [2] h_ptr, [3 + 2 q] / [4 + 2 q] the previous timestamp and the word
 * read of h word q < 8, [19 + 2 t] / [20 + 2 t] the same of w word t < 64, [147 + q] the h word written). The reference fills the four
 * tables on the host (crates/core/machine/src/syscall/precompiles/sha256/extend/{trace,controller}.rs, compress/{trace,controller}.rs)
 * and has no device filler for them. Output as above: column-major [width][height] Montgomery words.
 *   sp1hip_tracegen_riscv_sha_extend            ShaExtend, width 128: row 48 e + r is step i = 16 + r of event e, at clk + 1 + r — clk_high,
 *       clk_low + 1, next_clk, w_ptr[3], five AddrAddOperation values, i, the accesses of w[i-15], w[i-2], w[i-16], w[i-7] and w[i], the
 *       fixed rotates and shifts of w[i-15] and w[i-2], s0, s1 with their intermediates, s2, is_real. Padding rows are zero. Needs
 *       48 n_events <= height.
 *   sp1hip_tracegen_riscv_sha_extend_control    ShaExtendControl, width 18: one row per event; zero padding rows.
 *   sp1hip_tracegen_riscv_sha_compress          ShaCompress, width 206: row 80 e + j of event e — j < 8 reads h[j] at clk, 8 <= j < 72 is
 *       round j - 8 and reads w[j - 8] at clk + 1, j >= 72 writes h[j - 72] at clk + 2. The working state entering the row is computed
 *       from the h and w words read. The compression column groups are zero off the compression rows, the finalise groups off the
 *       finalise rows. A PADDING ROW IS NOT ZERO: octet, octet_num, index and k cycle by row mod 80 on every row of the table; every
 *       other column of a padding row is zero. Needs 80 n_events <= height.
 *   sp1hip_tracegen_riscv_sha_compress_control  ShaCompressControl, width 53: one row per event — clk, two SyscallAddrOperation, the two
 *       slice ends, is_real, the state read and the state after the 64 rounds; zero padding rows.
 * The MemoryLocal records of the touched words: sp1hip_precompile_local_records with { 2, 8, 3, 147, 2 } and { 1, 64, 19, none, 1 } for
 * SHA_COMPRESS (155 words; arg2_word 2) and with the QUAD form { 1, 64, 530, 0xFFFFFFFE, 0 } for SHA_EXTEND (786 words): final_word =
 * 0xFFFFFFFE reads word i's initial clk, initial value, final clk and final value from ev[pairs_word + 4 i .. + 4 i + 3] — the words
 * of one SHA_EXTEND call end at different timestamps — and needs pairs_word + 4 count <= words_per_event; final_clk_delta is not read.
 * All argument checks come before any launch; a null pointer is accepted only with a zero count / height; height == 0 succeeds
 * without a launch. The calls enqueue and return: they do not synchronise. */
int sp1hip_tracegen_riscv_sha_extend_width(void);            /* 128 */
int sp1hip_tracegen_riscv_sha_extend_control_width(void);    /* 18 */
int sp1hip_tracegen_riscv_sha_compress_width(void);          /* 206 */
int sp1hip_tracegen_riscv_sha_compress_control_width(void);  /* 53 */
int sp1hip_tracegen_riscv_sha_extend(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream);
int sp1hip_tracegen_riscv_sha_extend_control(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events,
                                             sp1hip_stream_t stream);
int sp1hip_tracegen_riscv_sha_compress(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream);
int sp1hip_tracegen_riscv_sha_compress_control(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events,
                                               sp1hip_stream_t stream);

/* Device trace generation for the chips of the POSEIDON2 and UINT256_MUL precompile shards, from the executor's event records as they
 * are (sp1hip_rv64_poseidon2_events: n_events x 26 u64 on the device — [0] clk, [1] ptr, [2 + 2 i] / [3 + 2 i] the previous timestamp
 * and the word read of word i < 8, [18 + i] the word written; sp1hip_rv64_uint256_events: 31 u64 — [0] clk, [1] x_ptr, [2] y_ptr,
 * [3 + 2 i] / [4 + 2 i] the previous timestamp and the word read of x word i < 4, [11 + 2 i] / [12 + 2 i] the same of y word i < 4 and,
 * for 4 <= i < 8, of modulus word i - 4, [27 + i] the x word written). The reference fills both tables on the host
 * (crates/core/machine/src/syscall/precompiles/poseidon2/air.rs:L107-L290, uint256/air.rs:L118-L290) and has no device filler for
 * them. Output as above: column-major [width][height] Montgomery words, one row per event.
 *   sp1hip_tracegen_riscv_poseidon2     Poseidon2, width 348: clk_high, clk_low, the SyscallAddrOperation of ptr, 8 AddrAddOperation
 *       values, 8 MemoryAccessCols (the words are rewritten in place at clk), the 8 words written as 16-bit limbs, the 16 + 16
 *       SP1FieldWordRangeChecker bits of the words written and read, the permutation's 179 columns — computed from the sixteen halves
 *       of the words READ, low half first, each reduced mod p — and is_real. A padding row (row >= n_events) is zero except for its
 *       permutation columns, which are those of the zero state.
 *   sp1hip_tracegen_riscv_uint256_mul   Uint256MulMod, width 371: clk_high, clk_low, two SyscallAddrOperation, 4 + 8 AddrAddOperation
 *       values, 4 + 4 + 4 MemoryAccessColsU8 (x rewritten at clk + 1; y and the modulus read at clk), the IsZero of the modulus' byte
 *       sum, modulus_is_not_zero, the FieldOpCols of x y = result + carry m' (result[32], carry[32], witness[63]; m' = m, or 2^256 when
 *       m = 0: a modulus of 33 byte limbs), the FieldLtCols of result < m (zero when m = 0) and is_real. result and carry are computed
 *       from the words read, by a 512-step division that is correct for every m, odd or even. A padding row is zero except for its 63
 *       witness columns, which hold the offset 2^14.
 * Precondition of the Uint256MulMod row, which holds for every event of a reduced x or y: x y / m' < 2^256. An event beyond it neither
 * faults nor takes longer — the carry columns take the quotient's low 256 bits and the witness wraps — but its row satisfies no
 * constraint system. The MemoryLocal records of the touched words: sp1hip_precompile_local_records with { 1, 8, 2, 18, 0 } for
 * POSEIDON2 (26 words; no second pointer) and with { 1, 4, 3, 27, 1 } and { 2, 8, 11, none, 0 } for UINT256_MUL (31 words; arg2_word
 * 2). Needs n_events <= height. All argument checks come before any launch; a null pointer is accepted only with a zero count /
 * height; height == 0 succeeds without a launch. The calls enqueue and return: they do not synchronise. */
int sp1hip_tracegen_riscv_poseidon2_width(void);      /* 348 */
int sp1hip_tracegen_riscv_uint256_mul_width(void);    /* 371 */
int sp1hip_tracegen_riscv_poseidon2(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream);
int sp1hip_tracegen_riscv_uint256_mul(uint32_t* d_table, uint32_t height, const uint64_t* d_events, uint32_t n_events, sp1hip_stream_t stream);

/* The Byte, Range and Program multiplicities of a shard, counted on the device from the tables that send: the receive side of the
 * byte lookup argument, which the reference computes in `generate_dependencies` of its Byte and Range chips
 * (crates/core/machine/src/bytes/trace.rs:L50-L66, range/trace.rs:L54-L95), and the Program chip's count of executed pcs. Generic over
 * the chip: `interactions` are the words `sp1hip_gkr_chip_t.interactions` takes (host memory), of which the sends of kind 5 (Byte)
 * are evaluated — [opcode, a, b, c] and a multiplicity m, affine forms of the row — on ALL `rows` rows of the chip's column-major
 * Montgomery tables (padding rows send with multiplicity 0, as the proof requires of them). Count arrays are u32 words, zeroed by the
 * caller once and added to by any number of calls:
 *   d_byte_counts   6 x 65536: opcode 0..5 (AND, OR, XOR, U8Range, LTU, MSB) adds m to cell opcode * 65536 + b * 256 + c — Byte's main
 *                   table [6][65536] as it stands
 *   d_range_counts  131072: opcode 6 adds m to cell (1 << b) + a (`a` has `b` bits) — Range's main table [1][131072]
 *   d_status        8 words, zeroed by the caller: [0] the number of bad messages, [1] 1 message / 2 pc / 3 count, [2] the interaction
 *                   index and [3] the row (or pc index, or cell) of the first, [4] the `tag` of the call that found it
 * A message with m == 0 is none. One with m != 0 is checked before its cell is formed — b <= 16, a < 2^b, c == 0 for a range; b, c <
 * 256, opcode < 6, a the table's answer, c == 0 for MSB; m < 2^16 (a negative multiplicity arrives as p - k) — and one that fails is
 * counted in d_status and moves no count. A malformed description (a column outside its table's width, a byte message with other than
 * 4 values, a truncated or overlong word list, a constant or weight outside the field) is SP1HIP_ERROR_INVALID_ARGUMENT before any
 * launch. rows == 0 succeeds without a launch; a null table pointer is accepted only with zero width or zero rows.
 *   sp1hip_lookup_count_program  adds 1 to d_program_counts[(pc - pc_base) >> 2] for the n executed pcs d_pcs[i * stride_words] (u64
 *                   words: stride 20 reads column 0 of the executor's event matrix, 11 and 12 the packed ALU and memory records); a pc
 *                   below pc_base, off the 4-byte grid or at or beyond n_instructions is counted in d_status instead.
 *   sp1hip_lookup_counts_finish  turns n_cells counts into Montgomery words, in place or into d_table_or_null, then SYNCHRONISES the
 *                   stream and returns SP1HIP_ERROR_INVALID_ARGUMENT with a message that names the first bad (send, row) when
 *                   d_status[0] != 0 (a count at or above the modulus is such an error too). The two count calls only enqueue.
 * Counts are u32 and a cell that wraps past 2^32 is NOT detected: the caller keeps the sum of the multiplicities sent to one cell
 * between zeroing and finish below 2^32 (every m is below 2^16, so any 2^16 messages per cell are safe; a shard of 2^22-row tables
 * would need 43 sends per row, all of multiplicity 2^16 - 1 and all to one cell, to reach it). */
int sp1hip_lookup_count_sends(const uint32_t* interactions, uint64_t n_words, uint32_t main_width, uint32_t prep_width, const uint32_t* d_main,
                              const uint32_t* d_prep, uint32_t rows, uint32_t* d_byte_counts, uint32_t* d_range_counts, uint32_t* d_status, uint32_t tag,
                              sp1hip_stream_t stream);
int sp1hip_lookup_count_program(const uint64_t* d_pcs, uint64_t stride_words, uint32_t n, uint64_t pc_base, uint32_t n_instructions,
                                uint32_t* d_program_counts, uint32_t* d_status, uint32_t tag, sp1hip_stream_t stream);
int sp1hip_lookup_counts_finish(uint32_t* d_counts, uint64_t n_cells, uint32_t* d_table_or_null, uint32_t* d_status, sp1hip_stream_t stream);

/* ---------------------------------------------------------------- device trace checker (sp1_amd/csrc/trace_check.hip)
 * Every constraint of every chip on every real row of the device tables a shard proof is about to be made from: what the reference
 * does under cfg(sp1_debug_constraints) in `prove_shard_with_data` (`debug_constraints_all_chips`,
 * /root/reference/crates/hypercube/src/prover/shard.rs:L711-L720, crates/hypercube/src/debug.rs:L27-L125). A call of its own: no
 * prover path reads it and nothing switches it on inside one.
 *
 * sp1hip_check_constraints takes the chip array of sp1hip_prove_shard (program, widths, d_main, d_prep, real_rows of each chip;
 * names and interaction words are not read) and the public values as Montgomery words, evaluates the caller's plain SSA — HINT
 * pseudo-instructions dropped, none of the zerocheck's fused pieces — one row per lane, and fills one report per chip,
 * SP1HIP_CHECK_REPORT_WORDS u64 words each in `reports`, in this order: failing_rows, first_row, noncanonical, fail_count_offset,
 * row_offset, pieces, registers, lanes, n_first, first_constraints[64]. What they hold:
 *   failing_rows        rows on which at least one constraint is non-zero
 *   first_row           the smallest of them; UINT64_MAX when there is none
 *   noncanonical        main and preprocessed words that are >= p (no field element's stored form; constraint values of a table
 *                       that holds one mean nothing)
 *   n_first, first_constraints   the constraints that are non-zero on first_row, ascending, at most 64 of them
 *   pieces, registers, lanes     how the program ran: the pieces it was cut into (1 unless it needs more than 512 registers), the
 *                       largest piece's register count, rows per workgroup
 *   fail_count_offset   where in h_words the chip's num_constraints words start: fail_count[k] = rows on which constraint k is non-zero
 *   row_offset          where in h_words the main_width + prep_width Montgomery words of first_row start (main, then
 *                       preprocessed; zeros when no row fails)
 * A chip with no rows or no constraints reports zeros. h_words / *n_words: the size protocol of the other entry points (too small,
 * or NULL: SP1HIP_ERROR_BUFFER_TOO_SMALL and *n_words = the sum over the chips of num_constraints + main_width + prep_width, before
 * any device work). A malformed program (an opcode, an operand that is not an earlier value, a column outside its table, a public
 * value index at or above n_publics, num_constraints other than the number of asserts) is SP1HIP_ERROR_INVALID_ARGUMENT before any
 * launch. The call synchronises the stream.
 *
 * sp1hip_trace_check_compile (host only): the compiled form the kernel and the host loop of tests/native/trace_check.hip run
 * (layout: sp1_amd/csrc/tc_rows.hpp), cut for a budget of max_regs registers (0: the default, 512). Size protocol on
 * out_words / *n_words. */
#define SP1HIP_CHECK_REPORT_WORDS 73   /* u64 words per chip: nine fields, then first_constraints[64] (the order is given above) */
int sp1hip_check_constraints(const sp1hip_shard_chip_t* chips, int n_chips, const uint32_t* h_publics, int n_publics,
                             uint64_t* reports, uint32_t* h_words, size_t* n_words, sp1hip_stream_t stream);
int sp1hip_trace_check_compile(const uint32_t* program, uint32_t n_instr, uint32_t main_width, uint32_t prep_width, uint32_t num_constraints,
                               uint32_t max_regs, uint32_t* out_words, size_t* n_words);

/* Every bus of the shard: do the sends and receives of all chips cancel as a multiset of (kind, values)? The reference's
 * `debug_interactions_with_all_chips` (/root/reference/crates/hypercube/src/logup_gkr/prover.rs:L99-L135,
 * crates/hypercube/src/lookup/debug.rs:L48-L200) without a host copy of any table. chips: the same array (interaction words, widths,
 * d_main, d_prep, real_rows are read); the caller appends the machine's eval_public_values as one more chip with a one-row table
 * that holds the public values.
 *   Pass 1 evaluates every interaction on every row, one row per lane. A message with a non-zero multiplicity m is folded into two
 *   independent 64-bit hashes of (kind, number of values, canonical values), and m — or m - p when m > p / 2 —, negated for a
 *   receive, is added (device-scope 64-bit atomic adds, lanes of a wave that hold one bucket combined into one add first) to one
 *   bucket in each of two tables of 2^log_buckets signed sums (log_buckets 1..26; 22 is the library's usual value: 64 MB).
 *   Verdict: balanced = every bucket of both tables is 0 mod p. A balanced shard is never called unbalanced. A wrong "balanced" needs
 *   the discrepancies of the unbalanced keys to cancel bucket by bucket in BOTH tables: with k unbalanced keys, some pair must share
 *   a bucket in each (two independent hashes: of order k^2 / 2^(2 log_buckets)) and their discrepancies must then sum to 0 mod p.
 *   Pass 2 (only when the first table has a non-zero bucket) evaluates the messages again and writes a 4-word record — chip index,
 *   interaction index, row, canonical multiplicity — for every message whose bucket of the first table is non-zero: every message
 *   of an unbalanced key, and whatever balanced messages share such a bucket (the caller's exact tally cancels those). `cap`
 *   records fit h_records; records_wanted counts them all, records = min(records_wanted, cap) were written, truncated says that
 *   some were left out (an arbitrary subset is kept; the verdict stands).
 * A malformed description is SP1HIP_ERROR_INVALID_ARGUMENT before any launch, by the parser sp1hip_lookup_count_sends uses. The call
 * synchronises the stream. */
#define SP1HIP_CHECK_BUSES_WORDS 8      /* u64 words of `report`: messages, nonzero buckets of the first and of the second table,
                                         * records_wanted, records, balanced (0 / 1), truncated (0 / 1), one spare */
int sp1hip_check_interactions(const sp1hip_shard_chip_t* chips, int n_chips, uint32_t log_buckets, uint64_t* report,
                              uint32_t* h_records, uint64_t cap, sp1hip_stream_t stream);

/* ---------------------------------------------------------------- guest execution (host code, no device work)
 * An rv64im executor for SP1 guest ELFs: what `MinimalExecutor` + `TracingVM` do for the core prover
 * (/root/reference/crates/core/executor/src/minimal.rs, tracing.rs:L57-L147, vm.rs:L139-L431; the controller's shard loop is
 * /root/reference/crates/prover/src/worker/controller/core.rs:L231). It runs the program one shard of at most `max_cycles`
 * instructions at a time and hands back the events the chips' trace generation starts from:
 *   events        [n_events][SP1HIP_RV64_EVENT_WORDS] u64 per executed instruction: pc, clk, opcode (the reference's `Opcode`
 *                 discriminant), op_a, op_b, op_c, flags (1 imm_b | 2 imm_c | 4 memory access), a, b, c, previous value of op_a,
 *                 previous timestamps of the op_a / op_b / op_c register accesses, memory address, previous timestamp and value of
 *                 the memory word, its new value, next pc, one spare word
 *   local memory  [n_local][5] u64 per address touched in the shard (registers are addresses 0..31): address, timestamp and
 *                 value before the shard's first access, timestamp and value after its last (`MemoryLocalEvent`,
 *                 events/memory.rs)
 *   keccak        [n_keccak][SP1HIP_RV64_KECCAK_WORDS] u64 per KECCAK_PERMUTE call: clk, state pointer, 25 x (previous timestamp,
 *                 word read), the 25 words written
 *   poseidon2     [n_poseidon2][SP1HIP_RV64_POSEIDON2_WORDS] u64 per POSEIDON2 call: clk, pointer, 8 x (previous timestamp, word
 *                 read), the 8 words written (at clk)
 *   sha_extend    [n][SP1HIP_RV64_SHA_EXTEND_WORDS]: clk, w_ptr, 48 steps x (4 x (previous timestamp, word read) for w[i-15], w[i-2],
 *                 w[i-16], w[i-7]; previous timestamp and value of w[i]; w[i] written), then 64 x (timestamp, value) before and after
 *   sha_compress  [n][SP1HIP_RV64_SHA_COMPRESS_WORDS]: clk, w_ptr, h_ptr, 8 x (previous timestamp, h word), 64 x (previous timestamp, w
 *                 word), the 8 h words written
 *   uint256       [n][SP1HIP_RV64_UINT256_WORDS]: clk, x_ptr, y_ptr, 4 x (previous timestamp, x word), 8 x (previous timestamp, y /
 *                 modulus word), the 4 x words written (x * y mod modulus; a zero modulus means 2^256)
 * After the program halts, sp1hip_rv64_global_memory lists every address the run touched as (address, initial value, final value,
 * final timestamp): the `MemoryGlobalInit` / `MemoryGlobalFinalize` events. Supervisor mode only; system calls: HALT, WRITE,
 * ENTER / EXIT_UNCONSTRAINED, COMMIT, COMMIT_DEFERRED_PROOFS, HINT_LEN, HINT_READ, KECCAK_PERMUTE, POSEIDON2, SHA_EXTEND, SHA_COMPRESS, UINT256_MUL, SECP256K1_ADD, SECP256K1_DOUBLE, and the families of sp1hip_rv64_precompile_events (any other stops the run with
 * SP1HIP_ERROR_RUNTIME and a message naming it). The pointers stay valid until the next call on the same handle. */
#define SP1HIP_RV64_EVENT_WORDS 20
#define SP1HIP_RV64_KECCAK_WORDS 77
#define SP1HIP_RV64_POSEIDON2_WORDS 26
#define SP1HIP_RV64_SHA_EXTEND_WORDS 786
#define SP1HIP_RV64_SHA_COMPRESS_WORDS 155
#define SP1HIP_RV64_UINT256_WORDS 31
#define SP1HIP_RV64_SECP_ADD_WORDS 43
#define SP1HIP_RV64_SECP_DOUBLE_WORDS 26
/* The other field / curve precompiles, one family per chip that proves them (sp1hip_rv64_precompile_events). Every event starts
 * [clk, first argument, second argument, system-call code]; then
 *   two-operand calls (curve additions, ED_ADD, Fp / Fp2 operations): n x (previous timestamp, x word), n x (previous timestamp,
 *     y word), the n x words written at clk + 1 (y is read at clk) — n = 8 / 12 words for a secp256r1 / bn254 / ed25519 or a
 *     bls12-381 point or Fp2 element, 4 / 6 for an Fp element;
 *   doublings: n x (previous timestamp, word), the n words written (at clk);
 *   ED_DECOMPRESS (second argument = the sign bit): 4 x (previous timestamp, x word before), 4 x (previous timestamp, y word read
 *     at pointer + 32), the 4 x words written at clk + 1;
 *   UINT256_ADD_CARRY / UINT256_MUL_CARRY: the pointers c, d, e (registers x12, x13, x14), those registers' previous timestamps,
 *     4 x (previous timestamp, word before) for each of a, b, c (read at clk, clk + 1, clk + 2), d, e (rewritten at clk + 3,
 *     clk + 4), the 4 d and 4 e words written (low and high half of a + b + c or a * b + c).
 * Operands must be reduced field elements; the affine formulas have no special cases (equal x in an addition, y = 0 in a
 * doubling and points off the curve whose denominators vanish stop the run with SP1HIP_ERROR_RUNTIME). */
#define SP1HIP_RV64_FAMILY_SECP256R1_ADD 0
#define SP1HIP_RV64_FAMILY_SECP256R1_DOUBLE 1
#define SP1HIP_RV64_FAMILY_BN254_ADD 2
#define SP1HIP_RV64_FAMILY_BN254_DOUBLE 3
#define SP1HIP_RV64_FAMILY_BLS12381_ADD 4
#define SP1HIP_RV64_FAMILY_BLS12381_DOUBLE 5
#define SP1HIP_RV64_FAMILY_BN254_FP 6
#define SP1HIP_RV64_FAMILY_BLS12381_FP 7
#define SP1HIP_RV64_FAMILY_BN254_FP2_ADDSUB 8
#define SP1HIP_RV64_FAMILY_BLS12381_FP2_ADDSUB 9
#define SP1HIP_RV64_FAMILY_BN254_FP2_MUL 10
#define SP1HIP_RV64_FAMILY_BLS12381_FP2_MUL 11
#define SP1HIP_RV64_FAMILY_ED_ADD 12
#define SP1HIP_RV64_FAMILY_ED_DECOMPRESS 13
#define SP1HIP_RV64_FAMILY_UINT256_OPS 14
#define SP1HIP_RV64_FAMILIES 15
typedef void* sp1hip_rv64_vm_t;
typedef struct {
    uint64_t shard;                      /* index of this shard in the run */
    uint64_t n_cycles;                   /* instructions executed in this shard */
    uint64_t n_events, n_local, n_keccak, n_poseidon2, n_sha_extend, n_sha_compress, n_uint256, n_secp256k1_add, n_secp256k1_double; /* n_events = n_cycles, or 0 when recording is off */
    uint64_t pc_start, next_pc;          /* `PublicValues::pc_start / next_pc` (HALT_PC = 1 after HALT) */
    uint64_t clk_start, clk_end;         /* `initial_timestamp / last_timestamp` */
    uint32_t halted, exit_code;
    uint32_t commit_syscall, commit_deferred_syscall;
    uint32_t committed_value_digest[8];  /* as set by COMMIT so far */
    uint32_t deferred_proofs_digest[8];
    uint64_t estimated_area, estimated_max_height;   /* the shard-cutting estimator's totals (0 without sp1hip_rv64_set_shard_limits) */
} sp1hip_rv64_shard_info_t;

/* Shard cutting by trace area, as the reference's executor does it (`ShapeChecker`, crates/core/executor/src/vm/shapes.rs:L27-L245;
 * thresholds `ShardingThreshold`, opts.rs:L12-L14, less the HALT allowance of splicing.rs:L413-L428): after every instruction
 * the estimate grows by the cost (columns) of the instruction's chip, by memory_local_cost + 2 global_cost per address first
 * touched in the shard, by syscall_core_cost + global_cost per call sent to a precompile shard, by 32 memory_bump_cost +
 * state_bump_cost when the clock's high limb moves; a shard ends when the estimate reaches element_threshold or a table
 * height_threshold rows — never between a COMMIT and the HALT. opcode_cost / opcode_chip are indexed by the opcode numbers of
 * sp1hip_rv64_events (chip: any numbering < 64 that groups the opcodes of one table); ALU / load instructions into x0 go to the
 * AluX0 / LoadX0 tables. fixed_area = the preprocessed tables (Program, Byte, Range). The caller owns the cost model: this
 * library does not know the chips. */
typedef struct {
    uint64_t element_threshold, height_threshold, fixed_area;
    uint64_t opcode_cost[64];
    uint32_t opcode_chip[64];
    uint64_t alu_x0_cost, load_x0_cost, memory_local_cost, global_cost, syscall_core_cost, memory_bump_cost, state_bump_cost;
} sp1hip_rv64_shard_limits_t;
int sp1hip_rv64_create(const uint8_t* elf, uint64_t elf_len, sp1hip_rv64_vm_t* out);
void sp1hip_rv64_destroy(sp1hip_rv64_vm_t vm);
/* One entry of the input stream (`SP1Stdin::write_slice`): what the guest's next HINT_LEN / HINT_READ pair consumes. */
int sp1hip_rv64_write_stdin(sp1hip_rv64_vm_t vm, const uint8_t* data, uint64_t len);
int sp1hip_rv64_run_shard(sp1hip_rv64_vm_t vm, uint64_t max_cycles, sp1hip_rv64_shard_info_t* info);
/* on = 0: the following shards run without keeping their instruction events (a rank that proves shard r of an execution runs
 * shards 0..r-1 this way); memory state, local memory events and public values are kept as always. */
int sp1hip_rv64_set_recording(sp1hip_rv64_vm_t vm, int on);
/* limits != NULL: sp1hip_rv64_run_shard also ends a shard where the estimator above says so (max_cycles still bounds it);
 * NULL: cycle counts only (the default). */
int sp1hip_rv64_set_shard_limits(sp1hip_rv64_vm_t vm, const sp1hip_rv64_shard_limits_t* limits);
const uint64_t* sp1hip_rv64_events(sp1hip_rv64_vm_t vm);
const uint64_t* sp1hip_rv64_local_memory(sp1hip_rv64_vm_t vm);
const uint64_t* sp1hip_rv64_keccak_events(sp1hip_rv64_vm_t vm);
const uint64_t* sp1hip_rv64_poseidon2_events(sp1hip_rv64_vm_t vm);
const uint64_t* sp1hip_rv64_sha_extend_events(sp1hip_rv64_vm_t vm);
const uint64_t* sp1hip_rv64_sha_compress_events(sp1hip_rv64_vm_t vm);
const uint64_t* sp1hip_rv64_uint256_events(sp1hip_rv64_vm_t vm);
const uint64_t* sp1hip_rv64_secp256k1_add_events(sp1hip_rv64_vm_t vm);     /* [n][43]: clk, p_ptr, q_ptr, 8 x (ts, p word), 8 x (ts, q word), 8 p words written */
const uint64_t* sp1hip_rv64_secp256k1_double_events(sp1hip_rv64_vm_t vm);  /* [n][26]: clk, p_ptr, 8 x (ts, p word), 8 p words written */
/* The shard's events of one SP1HIP_RV64_FAMILY_*: [n_events][words_per_event] u64, layouts above. */
int sp1hip_rv64_precompile_events(sp1hip_rv64_vm_t vm, uint32_t family, uint64_t* n_events, uint64_t* words_per_event, const uint64_t** data);
/* The transpiled program (`Program::instructions`): [n][6] u64 = opcode, op_a, op_b, op_c, imm_b, imm_c; instruction i sits at
 * pc_base + 4 i. */
int sp1hip_rv64_program(sp1hip_rv64_vm_t vm, uint64_t* pc_base, uint64_t* n_instructions, const uint64_t** table);
int sp1hip_rv64_global_memory(sp1hip_rv64_vm_t vm, uint64_t* n, const uint64_t** table);
/* The program's memory image (`Program::memory_image`, /root/reference/crates/core/executor/src/disassembler/elf.rs:L320-L353):
 * [n][2] u64 = (address, value) of every 8-byte word of the ELF's PT_LOAD segments, file bytes and zero fill alike, by ascending
 * address. The reference initialises these words through the verifying key (`initial_global_cumulative_sum`,
 * core/executor/src/program.rs:L170-L199: no MemoryGlobalInit row) and finalises every one of them, touched or not
 * (prover/src/worker/controller/global.rs:L145-L300). */
int sp1hip_rv64_memory_image(sp1hip_rv64_vm_t vm, uint64_t* n, const uint64_t** table);
/* which = 0: the bytes written to the public-values descriptor; 1: stdout / stderr. */
int sp1hip_rv64_output(sp1hip_rv64_vm_t vm, int which, const uint8_t** data, uint64_t* len);

/* ---------------------------------------------------------------- the AirProver slot: setup / proving key
 * `MachineVerifyingKey` (/root/reference/crates/hypercube/src/verifier/config.rs:L71-L81), Montgomery words. The
 * septic digest is x[7] then y[7]. */
typedef struct {
    uint32_t pc_start[3];
    uint32_t initial_global_cumulative_sum[14];
    uint32_t preprocessed_commit[8];
    uint32_t enable_untrusted_programs;
} sp1hip_vk_t;
typedef struct sp1hip_pk_s sp1hip_pk_t;

/* `ShardProver::setup_from_preprocessed_data_and_traces` (/root/reference/crates/hypercube/src/prover/shard.rs:L406-L429),
 * the body of `AirProver::setup_from_vk` once the preprocessed traces exist: commits them (one jagged round) and returns
 * the proving key = that commitment round (`PreprocessedData`) + the verifying key it defines. `preprocessed_tables`:
 * the column-major device tables of the chips that have preprocessed columns, in chip (name) order; they stay
 * caller-owned and must outlive the key. */
int sp1hip_setup(const sp1hip_table_t* preprocessed_tables, int n_tables, const uint32_t pc_start[3],
                 const uint32_t initial_global_cumulative_sum[14], uint32_t enable_untrusted_programs,
                 sp1hip_shard_params_t params, sp1hip_pk_t** out, sp1hip_stream_t stream);
void sp1hip_pk_free(sp1hip_pk_t* pk);
int sp1hip_pk_vk(const sp1hip_pk_t* pk, sp1hip_vk_t* out);
/* `MachineVerifyingKey::observe_into` (config.rs:L97-L112): commit, pc_start, septic x / y, untrusted flag, 6 zeros. */
int sp1hip_vk_observe_into(const sp1hip_vk_t* vk, sp1hip_challenger_t* challenger);
/* `AirProver::prove_shard_with_pk` (shard.rs:L321-L345) from the generated traces on: a default challenger absorbs the
 * verifying key, then `sp1hip_prove_shard`. `pow_witnesses` (canonical words, may be NULL / 0): see
 * sp1hip_challenger_inject_pow_witnesses. */
int sp1hip_prove_shard_with_pk(const sp1hip_pk_t* pk, const sp1hip_shard_chip_t* chips, int n_chips, const uint32_t* h_publics,
                               int n_publics, const uint32_t* pow_witnesses, int n_pow_witnesses, uint8_t* h_proof, size_t* proof_len,
                               sp1hip_stream_t stream);

/* ---------------------------------------------------------------- prover pool: N shard proofs in flight per GPU
 * The library-side counterpart of the reference's `ProverSemaphore`
 * (/root/reference/crates/hypercube/src/prover/permits.rs:L36-L66; its GPU worker builder takes ONE permit,
 * /root/reference/sp1-gpu/crates/prover_components/src/builder.rs:L107) plus the pinned `trace_buffers` queue of its shard
 * prover: `n_slots` prover slots (a host thread + a stream each) prove shards concurrently and fill each other's
 * transcript hand-over gaps, while one stager thread uploads the host traces of the next shards
 * (`sp1hip_stage_tables`). Tickets are served in submission order. */
typedef struct sp1hip_pool_s sp1hip_pool_t;
typedef uint64_t sp1hip_ticket_t;

/* One chip of a shard for the pool: sp1hip_shard_chip_t with the main trace EITHER on the host (`h_main`: row-major
 * [real_rows][main_width] Montgomery words — pinned memory for a full-rate asynchronous copy — which the pool stages into
 * a column-major device table it owns) OR already resident (`d_main`, column-major). `d_prep`: the chip's preprocessed
 * device table (the one the proving key was set up from), or NULL. Everything the struct points to stays caller-owned and
 * must remain valid and unchanged until the ticket has been waited for. */
typedef struct {
    const char* name;
    const uint32_t* program;
    uint32_t n_instr, num_constraints;
    const uint32_t* interactions;
    uint32_t n_words;
    uint32_t main_width, prep_width;
    const uint32_t* h_main;
    const uint32_t* d_main;
    const uint32_t* d_prep;
    uint64_t real_rows;
} sp1hip_pool_chip_t;

/* Where a ticket spent its time (milliseconds) and which slot proved it. */
typedef struct {
    double staging_ms;  /* submit -> host traces enqueued for upload (includes waiting for a staging buffer) */
    double queued_ms;   /* staged -> a prover slot took it */
    double proving_ms;  /* sp1hip_prove_shard_with_pk on the slot's stream */
    int slot;
} sp1hip_pool_times_t;

int sp1hip_pool_create(int device, int n_slots, sp1hip_pool_t** out);
/* Finishes every submitted shard, then stops the threads and destroys the streams (the slots' helper streams, their events and
   every arena block cached for them included). Like any destructor of this ABI it must not run concurrently with another
   call on the same pool: a thread blocked in sp1hip_pool_wait holds a pointer into it. */
void sp1hip_pool_destroy(sp1hip_pool_t* pool);
/* Queue one shard: `AirProver::prove_shard_with_pk` (/root/reference/crates/hypercube/src/prover/shard.rs:L321-L345) from
 * the generated traces on. Returns at once. */
int sp1hip_pool_submit(sp1hip_pool_t* pool, const sp1hip_pk_t* pk, const sp1hip_pool_chip_t* chips, int n_chips,
                       const uint32_t* h_publics, int n_publics, sp1hip_ticket_t* ticket);
/* Block until the ticket's proof exists and copy bincode(ShardProof) out (size protocol as sp1hip_prove_shard:
 * SP1HIP_ERROR_BUFFER_TOO_SMALL sets *proof_len and leaves the ticket claimable). A failed proof returns its status and
 * message here. `times` may be NULL. A ticket can be collected once. */
int sp1hip_pool_wait(sp1hip_pool_t* pool, sp1hip_ticket_t ticket, uint8_t* h_proof, size_t* proof_len, sp1hip_pool_times_t* times);
/* The same without blocking: SP1HIP_ERROR_NOT_READY while the shard is in flight. */
int sp1hip_pool_try_wait(sp1hip_pool_t* pool, sp1hip_ticket_t ticket, uint8_t* h_proof, size_t* proof_len, sp1hip_pool_times_t* times);

/* ---------------------------------------------------------------- outer (BN254) commitments and transcript
 * The commitment scheme and transcript of the wrap proof (the reference's `SP1OuterGlobalContext`,
 * /root/reference/slop/crates/bn254/src/lib.rs:L24-L90): Poseidon2 over the BN254 scalar field (width 3, x^5, 8 + 56 rounds),
 * the sponge MultiField32PaddingFreeSponge<KB, Fr, Perm, 3, 16, 1> (16 KoalaBear elements per block, 8 packed into each of
 * lanes 0 and 1 by reduce_31 = sum canonical(v_i) 2^(31 i)), compress = permute([l, r, 0])[0], and the transcript
 * MultiField32Challenger<KB, Fr, Perm, 3, 2>. Every BN254 value that crosses this ABI is 8 little-endian u32 words in
 * Montgomery form (R = 2^256, the Rust layout of Bn254Fr); KoalaBear words are Montgomery words (R = 2^32) as everywhere.
 * PARITY: the permutation is pinned by its published test vectors; the sponge, packing, compress, commitment cap, challenger and
 * the 40-byte digest encoding by the reference's one real outer proof (crates/prover/wrapped_proof.bin), whose Merkle openings
 * and whole transcript replay under tests/outer_model.py (tests/golden/make_outer_golden.py, tests/test_outer_golden.py). */
/* d_states [n][3][8] permuted in place (device); h_states the same on the host. */
int sp1hip_outer_poseidon2_permute(uint32_t* d_states, size_t n, sp1hip_stream_t stream);
int sp1hip_outer_poseidon2_permute_host(uint32_t* h_states, size_t n);
/* d_tree: (2^(lg_height+1) - 1) x 8 words, one digest per node, leaf layer first (indexed like sp1hip_merkle_commit's tree).
 * d_root_and_commit: 16 words, the root followed by compress(root, hash([lg_height, total_width])). */
int sp1hip_outer_merkle_commit(const sp1hip_tensor_t* tensors, int n_tensors, int lg_height, uint32_t* d_tree,
                               uint32_t* d_root_and_commit, sp1hip_stream_t stream);
/* d_values: [n_idx][total_width] row-major (tensor order); d_paths: [n_idx][lg_height][8] sibling digests, leaf level first.
 * Either output may be NULL. */
int sp1hip_outer_merkle_open(const sp1hip_tensor_t* tensors, int n_tensors, int lg_height, const uint32_t* d_tree,
                             const uint32_t* d_indices, size_t n_idx, uint32_t* d_values, uint32_t* d_paths,
                             sp1hip_stream_t stream);
/* KoalaBear RS encode (sp1hip_rs_encode_batch) of every mle into d_codewords[k] (2^(lg_n + lg_blowup) x width, column-major),
 * then the outer tree over the codewords into d_tree; synchronises the stream to return the commitment (8 words). */
int sp1hip_outer_commit_mles(const sp1hip_tensor_t* mles, int n_mles, int lg_n, int lg_blowup, uint32_t* const* d_codewords,
                             uint32_t* d_tree, uint32_t h_commit[8], sp1hip_stream_t stream);
/* The outer transcript (host). observe_commitment: the 8-word digest, observed as its four 64-bit chunks reduced into
 * KoalaBear. grind: the SMALLEST witness w (canonical order) with check_witness(bits, w), searched on the device; returns it
 * as a Montgomery word and leaves the challenger as check_witness would. state: out50 = sponge [3][8] Montgomery words,
 * input length, input [16], output length, output [8] (the split form, popped from the end; unused entries zero). */
typedef struct sp1hip_outer_challenger_s sp1hip_outer_challenger_t;
int sp1hip_outer_challenger_new(sp1hip_outer_challenger_t** out);
int sp1hip_outer_challenger_clone(const sp1hip_outer_challenger_t* ch, sp1hip_outer_challenger_t** out);
void sp1hip_outer_challenger_free(sp1hip_outer_challenger_t* ch);
int sp1hip_outer_challenger_observe(sp1hip_outer_challenger_t* ch, const uint32_t* felts, size_t n);
int sp1hip_outer_challenger_observe_commitment(sp1hip_outer_challenger_t* ch, const uint32_t* digest8);
int sp1hip_outer_challenger_sample(sp1hip_outer_challenger_t* ch, uint32_t* out);
int sp1hip_outer_challenger_sample_ext(sp1hip_outer_challenger_t* ch, sp1hip_ext_t* out);
int sp1hip_outer_challenger_sample_bits(sp1hip_outer_challenger_t* ch, int bits, uint32_t* out);
int sp1hip_outer_challenger_check_witness(sp1hip_outer_challenger_t* ch, int bits, uint32_t witness, int* ok);
int sp1hip_outer_challenger_grind(sp1hip_outer_challenger_t* ch, int bits, uint32_t* witness, sp1hip_stream_t stream);
int sp1hip_outer_challenger_state(const sp1hip_outer_challenger_t* ch, uint32_t* out50);

/* ---------------------------------------------------------------- outer (BN254) BaseFold opening
 * The outer counterpart of sp1hip_commit_mles / sp1hip_basefold_prove: `BasefoldProver` under SP1OuterGlobalContext. The field
 * work (batching, RS encode, folds, query gathers) is the inner prover's; trees are Poseidon2-BN254, the transcript the
 * MultiField32Challenger (digests enter it through observe_commitment). commit_mles_data owns the codewords and the tree;
 * h_commit receives the 8 Montgomery words of the commitment. The proof is bincode(BasefoldProof<SP1OuterGlobalContext>): the
 * inner layout with every digest (fri_commitments, merkle_root, path entries) as u64(32) followed by the 32 little-endian
 * bytes of the CANONICAL BN254 value (40 bytes; the serde form of Hash<KoalaBear, Bn254Fr, 1>). Size protocol and
 * commit-on-success rule as sp1hip_basefold_prove: a NULL or too-small buffer sets *proof_len, returns
 * SP1HIP_ERROR_BUFFER_TOO_SMALL and leaves the challenger untouched. Malformed input (a round of another dimension or blowup, a
 * claims count other than the total width, dim + log_blowup > 24) is SP1HIP_ERROR_INVALID_ARGUMENT before any device work. */
typedef struct sp1hip_outer_basefold_data_s sp1hip_outer_basefold_data_t;
int sp1hip_outer_commit_mles_data(const sp1hip_tensor_t* mles, int n_mles, int lg_n, int lg_blowup, uint32_t h_commit[8],
                                  sp1hip_outer_basefold_data_t** out, sp1hip_stream_t stream);
void sp1hip_outer_basefold_data_free(sp1hip_outer_basefold_data_t* data);
size_t sp1hip_outer_basefold_proof_size(int dim, const uint32_t* round_widths, int n_rounds, sp1hip_fri_config_t config);
int sp1hip_outer_basefold_prove(const sp1hip_ext_t* h_point, int dim, sp1hip_outer_basefold_data_t* const* rounds, int n_rounds,
                                const sp1hip_ext_t* h_claims, size_t n_claims, sp1hip_fri_config_t config,
                                sp1hip_outer_challenger_t* challenger, uint8_t* h_proof, size_t* proof_len, sp1hip_stream_t stream);

/* ---------------------------------------------------------------- outer (BN254) stacked + jagged PCS
 * The outer counterparts of sp1hip_stacked_commit / sp1hip_jagged_commit / sp1hip_jagged_prove, argument for argument: what a
 * wrap-shard prover calls for `commit_traces`, the verifying key's `preprocessed_commit` and the shard proof's
 * `evaluation_proof`. The dense stacking and the whole evaluation-proof round loop are the inner prover's; the stacked batches
 * are committed with sp1hip_outer_commit_mles_data, the transcript is the MultiField32Challenger and the proof ends in
 * sp1hip_outer_basefold_prove.
 * jagged commitment = compress(stacked commitment, hash([n + 2, rows.., cols..])) under the outer sponge (the counts as
 * KoalaBear elements, reduce_31 chunks of 8, 16 per permutation) — the rule that reproduces `main_commitment` and the vk's
 * `preprocessed_commit` of the reference's real wrap proof (tests/test_outer_jagged_model.py).
 * A commitment without any table value is refused (the outer tree has no zero-width leaf).
 * The proof is bincode(JaggedPcsProof<SP1OuterGlobalContext>) in the reference's field order: the BaseFold proof
 * (sp1hip_outer_basefold_prove's bytes), batch evaluations, the jagged and the jagged-eval sumcheck, row / column counts,
 * `merkle_tree_commitments` (the STACKED commitments, one 40-byte digest per round), `expected_eval`, `max_log_row_count`,
 * `log_m`. Size protocol, commit-on-success rule and argument checks as sp1hip_jagged_prove. */
typedef struct sp1hip_outer_stacked_data_s sp1hip_outer_stacked_data_t;
int sp1hip_outer_stacked_commit(const sp1hip_table_t* tables, int n_tables, int log_stacking_height, int batch_size, int lg_blowup,
                                uint32_t h_commit[8], uint64_t* num_added_vals, sp1hip_outer_stacked_data_t** out,
                                sp1hip_stream_t stream);
int sp1hip_outer_jagged_commit(const sp1hip_table_t* tables, int n_tables, int max_log_row_count, int log_stacking_height,
                               int batch_size, int lg_blowup, uint32_t h_commit[8], sp1hip_outer_stacked_data_t** out,
                               sp1hip_stream_t stream);
void sp1hip_outer_stacked_data_free(sp1hip_outer_stacked_data_t* data);
/* Every output may be NULL. jagged_commit needs a handle from sp1hip_outer_jagged_commit; row_counts / column_counts receive
 * *n_tables entries each (the two padding tables included) and need counts_capacity >= that. */
int sp1hip_outer_stacked_data_info(const sp1hip_outer_stacked_data_t* data, sp1hip_outer_basefold_data_t** basefold, int* n_batches,
                                   const uint32_t** d_dense, uint64_t* padded_area, uint32_t stacked_commit[8],
                                   uint32_t jagged_commit[8], size_t* n_tables, uint64_t* row_counts, uint64_t* column_counts,
                                   size_t counts_capacity);
int sp1hip_outer_stacked_batch(const sp1hip_outer_stacked_data_t* data, int k, sp1hip_tensor_t* batch);
/* 0 for rounds that are not jagged commitments. */
size_t sp1hip_outer_jagged_proof_size(sp1hip_outer_stacked_data_t* const* rounds, int n_rounds, sp1hip_fri_config_t config);
int sp1hip_outer_jagged_prove(const sp1hip_ext_t* h_z_row, int max_log_row_count, sp1hip_outer_stacked_data_t* const* rounds,
                              int n_rounds, const sp1hip_ext_t* h_claims, const size_t* claims_per_round,
                              sp1hip_fri_config_t config, sp1hip_outer_challenger_t* challenger, uint8_t* h_proof,
                              size_t* proof_len, sp1hip_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SP1HIP_H */
