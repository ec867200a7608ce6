// Shared between table_text_api.hip (validation, chunk planning, the host formatting of flagged elements, the row scan) and
// table_text_kernels.hip (K20, plot_cnv's matrix files as text: digits pass, lengths, emit pass).  DESIGN.md section 4 K20.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "table_text_digits.h"

namespace icnv {

constexpr int TT_NT = 256;                 // lanes of a workgroup
constexpr int TT_SEG = 256;                // fields of one segment of a file row: one per lane of the emit pass
constexpr int TT_TILE = 64;                // gene rows: the digits pass transposes 64 genes x 64 cells through LDS
constexpr int TT_FLAG_CAP = 1 << 16;       // flagged elements one round hands to the host

constexpr int TT_GENE_ROWS = 0, TT_CELL_ROWS = 1;   // ICNV_TABLE_GENE_ROWS / ICNV_TABLE_CELL_ROWS

struct TtFlagged {                         // a flagged element: its record index and its bits
    int64_t idx;
    uint64_t bits;
};

struct TtArgs {
    const double *x;                       // element (g, c) at x[c * ld + g]
    int64_t ld;
    int32_t orientation;
    int64_t row0;                          // gene rows: the gene of local row 0 (cell rows: cells[] is already cut to the range)
    int64_t n_rows;                        // local rows of this call
    int64_t n_fields;                      // gene rows: the cell list's length; cell rows: G
    const int32_t *cells;                  // device.  gene rows: [n_fields], the cell of field j; cell rows: [n_rows], the cell of local row r
    uint64_t *rec;                         // [n_rows * n_fields], file order
    uint16_t *meta;
    TtFlagged *flagged;                    // [TT_FLAG_CAP]
    uint32_t *n_flagged;                   // every flagged element counts, listed or not
    // lengths
    int64_t n_seg;                         // segments of a row
    uint32_t *seg_sum;                     // [n_rows * n_seg] bytes of a segment's fields, their separators / newline included
    int64_t *seg_off;                      // [n_rows * n_seg] the segment's first byte, counted from the row's first byte
    int64_t *row_bytes;                    // [n_rows]
    const int64_t *lab_off;                // device [n_rows + 1] or null: the label of local row r is lab[lab_off[r] .. lab_off[r + 1])
    const uint8_t *lab;
    // emit
    const int64_t *row_off;                // device [n_rows + 1]
    uint8_t *out;
    uint8_t sep;
};

int launch_tt_digits(const TtArgs &a, hipStream_t s);
int launch_tt_collect(const TtArgs &a, hipStream_t s);
int launch_tt_patch(const TtArgs &a, const int64_t *idx, const uint64_t *rec, const uint16_t *meta, int32_t n, hipStream_t s);
int launch_tt_lengths(const TtArgs &a, hipStream_t s);
int launch_tt_emit(const TtArgs &a, int64_t n_rows_fit, hipStream_t s);

}  // namespace icnv
