// sp1_amd/csrc/stacked_data.hpp — the prover data behind sp1hip_stacked_data_t and sp1hip_outer_stacked_data_t, shared by
// stacked.hip / outer_jagged.hip (commit) and jagged.hip (evaluation proof): `StackedBasefoldProverData`
// (/root/reference/slop/crates/stacked/src/prover.rs:L20-L31) plus, when it came from a jagged commit, the
// `JaggedProverData` fields (/root/reference/slop/crates/jagged/src/prover.rs:L36-L46).
//
// StackedCore is everything that does not depend on the hash: the dense buffer, its batches and the jagged counts. The two
// handles add their BaseFold data and their commitments (8 KoalaBear words inside, one BN254 element = 8 words outside).
#pragma once
#include <atomic>
#include <functional>
#include <vector>

#include "common.hpp"

namespace sp1hip {

struct StackedCore {
    void* d_dense = nullptr;             // dense column-major concatenation of the tables, zero-padded
    hipStream_t stream = nullptr;
    std::vector<sp1hip_tensor_t> batches;    // slices of d_dense: [2^lsh x w] stacked batches
    uint64_t area = 0, padded = 0;
    int log_stacking_height = 0;
    // jagged wrapper
    bool jagged = false;
    int max_log_row_count = 0;
    std::vector<uint64_t> row_counts, column_counts;   // per table, the two padding tables appended
    uint64_t padding_column_count = 0;
    std::atomic<bool> foreign_use{false};            // read on a stream other than `stream` (see BasefoldData, basefold_host.hpp)
    ~StackedCore() { arena_free(d_dense, padded * 4, stream); }      // (after the derived handle released its BaseFold data)
};

// ---- the hash-free halves of the two commits (stacked.hip)
// fill_batch(b, on): enqueue the copy of the table slices of stacked batch b into the dense buffer on stream `on`
using FillBatch = std::function<int(int, hipStream_t)>;
// `StackedPcsProver::commit_multilinears` up to the BaseFold commit: validates, allocates and lays out sd (dense buffer, zero
// tail, batches) and calls `commit(fill_batch)`, which must have every batch filled before it encodes it.
int stacked_commit_dense(const sp1hip_table_t* tables, int n_tables, int log_stacking_height, int batch_size, int lg_blowup,
                         StackedCore* sd, uint64_t* num_added_vals, hipStream_t s, const std::function<int(const FillBatch&)>& commit);
// `JaggedProver::commit_multilinears` around it: the tables with real rows (the ones that are committed) and every table's counts
struct JaggedTables { std::vector<sp1hip_table_t> dense; std::vector<uint64_t> rows, cols; };
int jagged_select_tables(const sp1hip_table_t* tables, int n_tables, int max_log_row_count, JaggedTables* out);
// appends the two padding tables that account for `added` zero values, records JaggedProverData in sd and returns the words
// the wrap hashes, [n + 2, rows.., cols..] (plain integers)
std::vector<uint32_t> jagged_finish_counts(uint64_t added, int max_log_row_count, JaggedTables&& t, StackedCore* sd);

}  // namespace sp1hip

struct sp1hip_stacked_data_s : sp1hip::StackedCore {
    sp1hip_basefold_data_t* basefold = nullptr;
    uint32_t commit[8];                  // stacked (inner) commitment = JaggedProverData.original_commitment
    uint32_t jagged_commit[8];
    ~sp1hip_stacked_data_s() {
        if (foreign_use) (void)hipDeviceSynchronize();
        if (basefold) sp1hip_basefold_data_free(basefold);
    }
};

struct sp1hip_outer_stacked_data_s : sp1hip::StackedCore {
    sp1hip_outer_basefold_data_t* basefold = nullptr;
    uint32_t commit[8];                  // stacked commitment, BN254 Montgomery words
    uint32_t jagged_commit[8];
    ~sp1hip_outer_stacked_data_s() {
        if (foreign_use) (void)hipDeviceSynchronize();
        if (basefold) sp1hip_outer_basefold_data_free(basefold);
    }
};
