// Shared between table_parse_api.hip (validation, the host's strtod path, the error text) and table_parse_kernels.hip
// (K21, count matrices from text: structure, index, rows, parse, transpose; the matrix gather).  DESIGN.md section 4 K21.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "table_parse_num.h"

namespace icnv {

constexpr int TP_NT = 256;                 // lanes of a workgroup
constexpr int TP_BYTES = 16;               // text positions of one lane of the structure passes
constexpr int TP_SEG = TP_NT * TP_BYTES;   // text positions of one workgroup: a segment
constexpr int TP_TILE = 64;                // the transpose moves 64 rows x 64 columns through LDS
constexpr int TP_FLAG_CAP = 1 << 16;       // uncertified fields one round hands to the host
constexpr uint64_t TP_PENDING = 0x7FF4000000000001ull;   // staged in place of an uncertified field: no parse gives these bits
constexpr uint64_t TP_NO_ERROR = ~0ull;

struct TpFlagged {                         // an uncertified field: its slot in the staged values and its first byte
    int64_t slot;
    int64_t pos;
};

struct TpArgs {
    const uint8_t *text;                   // device, 16-byte aligned, n bytes
    int64_t n;                             // 1 .. 2^31 - 2
    uint8_t sep;
    int64_t n_cols;
    int64_t n_seg;                         // segments covering the positions 0 .. n
    uint32_t *seg_count;                   // [n_seg] row starts << 16 | field starts
    uint32_t *seg_row_off, *seg_field_off; // [n_seg] exclusive scans
    uint32_t *totals;                      // [2] rows, fields
    // index (the totals are known on the host by then)
    int64_t n_rows, n_fields;
    uint32_t *field_pos;                   // [n_fields] first byte of field f
    uint32_t *field_row;                   // [n_fields]
    uint32_t *row_pos;                     // [n_rows] first byte of row r
    uint32_t *row_field0;                  // [n_rows] the row's first field
    int32_t *label_range;                  // [2 n_rows] begin, end of the row's first field
    unsigned long long *error;             // offset << 8 | code, the smallest wins; TP_NO_ERROR
    // parse
    uint64_t *vals;                        // [n_rows * n_cols] file order
    TpFlagged *flagged;                    // [TP_FLAG_CAP]
    uint32_t *n_flagged;                   // every uncertified field counts, listed or not
    // transpose
    double *out;                           // row i, column c of the chunk at out[c * ld + row0 + i]
    int64_t ld, row0;
};

int launch_tp_structure(const TpArgs &a, hipStream_t s);     // seg_count, the scans, totals
int launch_tp_index(const TpArgs &a, hipStream_t s);         // field_pos, field_row, row_pos, row_field0; then the rows' checks and label ranges
int launch_tp_parse(const TpArgs &a, hipStream_t s);
int launch_tp_collect(const TpArgs &a, hipStream_t s);
int launch_tp_patch(const TpArgs &a, const int64_t *slot, const uint64_t *bits, int32_t n, hipStream_t s);
int launch_tp_transpose(const TpArgs &a, hipStream_t s);
int launch_gather_matrix(const double *in, int64_t ld_in, const int32_t *genes, int64_t n_genes, const int32_t *cells, int64_t n_cells,
                         double *out, int64_t ld_out, hipStream_t s);

}  // namespace icnv
