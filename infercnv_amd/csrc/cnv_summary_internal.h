// Internal declarations of K14 (include/icnv.h "per-cell CNV features and run-length segmentation"): cnv_summary_kernels.hip
// holds the kernels and their launches, cnv_summary_api.hip the C ABI.  DESIGN.md section 4 K14.
#pragma once
#include "icnv_internal.h"

namespace icnv {

constexpr int CNVSUM_TILE_GENES = 128;     // genes of 64 columns staged through LDS at a time
constexpr int CNVSUM_CHUNK_GENES = 1024;   // genes of one workgroup of the counting pass (whole tiles)
constexpr int CNVSUM_MAX_K = 7;            // the packed-byte compares need every valid state in three bits

struct CnvSumArgs {
    const uint8_t *st;          // element (gene g, column c) at st[c * ld + g]
    int64_t ld;
    int32_t G;
    int64_t C;                  // columns of the matrix
    const int32_t *chr_start;   // device, n_chr + 1
    int32_t n_chr;
    int32_t K;                  // states 1 .. K are valid; 0: every byte is taken as it is (the segmentation only)
    int32_t neutral;            // the centre state s0; 0 (the segmentation only): no state is neutral
    int32_t *counts;            // [n_chr][C][4] n_loss, n_gain, d_loss, d_gain; zeroed by the launch; null: run counts only
    int32_t *run_counts;        // [C][2] runs of every state, runs of a non-neutral state; zeroed by the launch
    int32_t *bad;               // one word, set when a byte is outside 1 .. K; zeroed by the launch
};
int launch_cnvsum_count(const CnvSumArgs &a, hipStream_t stream);

// exclusive scan, in list order, of the two run counts of the listed columns: rec_off[i] = records before list position i,
// ord_off[i] = runs (of every state) before it; totals[0] = records, totals[1] = runs.  All device pointers.
int launch_cnvsum_scan(const int32_t *run_counts, const int32_t *col_idx, int64_t n_cols, int64_t *rec_off, int64_t *ord_off,
                       int64_t *totals, hipStream_t stream);

struct CnvRunsArgs {
    const uint8_t *st;
    int64_t ld;
    int32_t G;
    const int32_t *chr_start;   // device
    int32_t n_chr;
    const int32_t *col_idx;     // device, nullable: list position -> column
    int64_t n_cols;             // list positions
    int32_t neutral;
    const int64_t *rec_off, *ord_off;
    int64_t capacity;           // records the six arrays hold: nothing is written at or beyond it
    int32_t *rec;               // [6][capacity]: col, chr, gene_first, gene_last, state, ordinal
};
int launch_cnvsum_runs(const CnvRunsArgs &a, hipStream_t stream);

}  // namespace icnv
