// Shared between table_parse_api.hip (the one host driver of the plain and the column-selected table entries: validation, the
// host's strtod path, the error text), table_parse_kernels.hip (K21, count matrices from text: structure, index, rows, parse,
// transpose; the matrix gather) and table_cols_kernels.hip (K26: index, parse and collect of selected columns).
// DESIGN.md section 4 K21, K26.
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

// ---- device helpers shared by table_parse_kernels.hip and table_cols_kernels.hip ----------------------------------------
// Position p of the text (0 .. n; n is a position because a last line without '\n' may end in a separator) is
//   a row start    when it begins a line (p == 0 or text[p - 1] == '\n') that is not blank (tp_at_line_end(p) is false);
//   a field start  when it is a row start or text[p - 1] is the separator.
// A lane looks at TP_BYTES positions from `base`: b[k] is the byte at base - 1 + k, '\n' on either side of the text, which
// makes position 0 a line start and keeps every position beyond n from being anything.  Bit j of the masks is position base + j.
__device__ inline void tp_masks(const TpArgs &a, int64_t base, uint32_t &rows, uint32_t &fields) {
    uint8_t b[TP_BYTES + 2];
    b[0] = (base > 0 && base - 1 < a.n) ? a.text[base - 1] : (uint8_t)'\n';
    if (base + TP_BYTES <= a.n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(a.text + base);
        const uint32_t word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < TP_BYTES; ++j) b[1 + j] = (uint8_t)(word[j >> 2] >> (8 * (j & 3)));
    } else {
#pragma unroll
        for (int j = 0; j < TP_BYTES; ++j) b[1 + j] = base + j < a.n ? a.text[base + j] : (uint8_t)'\n';
    }
    b[TP_BYTES + 1] = base + TP_BYTES < a.n ? a.text[base + TP_BYTES] : (uint8_t)'\n';
    rows = 0;
    fields = 0;
#pragma unroll
    for (int j = 0; j < TP_BYTES; ++j) {
        const int k = j + 1;
        const bool line_start = b[k - 1] == '\n';
        const bool line_end = b[k] == '\n' || (b[k] == '\r' && b[k + 1] == '\n');
        const bool row = line_start && !line_end;
        rows |= (uint32_t)row << j;
        fields |= (uint32_t)(row || b[k - 1] == a.sep) << j;
    }
}

__device__ inline uint32_t tp_packed_counts(uint32_t rows, uint32_t fields) { return ((uint32_t)__popc(rows) << 16) | (uint32_t)__popc(fields); }

// Inclusive scan of one word per lane over the workgroup (s_scan: TP_NT words).
__device__ inline uint32_t tp_block_scan(uint32_t v, uint32_t *s_scan) {
    const int tid = threadIdx.x;
    s_scan[tid] = v;
    __syncthreads();
    for (int d = 1; d < TP_NT; d <<= 1) {
        const uint32_t add = tid >= d ? s_scan[tid - d] : 0u;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    return s_scan[tid];
}

__device__ inline void tp_refuse(const TpArgs &a, int64_t offset, int code) {
    atomicMin(a.error, ((unsigned long long)offset << 8) | (unsigned long long)code);
}

__device__ inline void tp_flag(const TpArgs &a, int64_t slot, int64_t pos) {
    const uint32_t t = atomicAdd(a.n_flagged, 1u);
    if (t < (uint32_t)TP_FLAG_CAP) a.flagged[t] = TpFlagged{slot, pos};
}

// The index pass of one lane: the first byte and first field of every row that starts in the lane's positions and, with
// LIST_FIELDS (K21), the first byte and the row of every field.  K26 lists no fields: it keeps positions of selected ones only.
template <bool LIST_FIELDS>
__device__ inline void tp_index_starts(const TpArgs &a, uint32_t *s_scan) {
    const int64_t base = ((int64_t)blockIdx.x * TP_NT + threadIdx.x) * TP_BYTES;
    uint32_t rows, fields;
    tp_masks(a, base, rows, fields);
    const uint32_t mine = tp_packed_counts(rows, fields), excl = tp_block_scan(mine, s_scan) - mine;
    int64_t r = (int64_t)a.seg_row_off[blockIdx.x] + (excl >> 16), f = (int64_t)a.seg_field_off[blockIdx.x] + (excl & 0xffffu);
    while (fields) {
        const int j = __ffs((int)fields) - 1;
        fields &= fields - 1;
        if ((rows >> j) & 1u) {
            if (r < a.n_rows) {
                a.row_pos[r] = (uint32_t)(base + j);
                a.row_field0[r] = (uint32_t)f;
            }
            ++r;
        }
        if (LIST_FIELDS && f < a.n_fields && r >= 1 && r <= a.n_rows) {
            a.field_pos[f] = (uint32_t)(base + j);
            a.field_row[f] = (uint32_t)(r - 1);
        }
        ++f;
    }
}

// The field that starts at p, converted and staged at vals[slot]: its value where the scan certifies one, else TP_PENDING --
// with the field flagged for the host's strtod, or the chunk refused where the field is no number at all.
__device__ inline void tp_stage_field(const TpArgs &a, int64_t p, int64_t slot) {
    int64_t end = p;
    while (end - p <= TP_MAX_SCAN && !tp_at_line_end(a.text, a.n, end) && a.text[end] != a.sep) ++end;
    uint64_t bits = TP_PENDING, w;
    int q;
    bool neg;
    int kind = TP_HOST;
    if (end - p <= TP_MAX_SCAN) kind = tp_scan_number(a.text + p, end - p, bits, w, q, neg);
    if (kind == TP_DECIMAL) kind = tp_convert(w, q, neg, bits) ? TP_VALUE : TP_HOST;
    if (kind == TP_BAD) tp_refuse(a, p, 2 /* TP_E_NUMBER */);
    if (kind != TP_VALUE) bits = TP_PENDING;
    if (kind == TP_HOST) tp_flag(a, slot, p);
    a.vals[slot] = bits;
}

int tp_grid(int64_t blocks, unsigned &grid, const char *who);   // blocks as a grid size, or ICNV_ERR_UNSUPPORTED "<who>: the chunk needs ..."
int launch_tp_structure(const TpArgs &a, hipStream_t s);     // seg_count, the scans, totals
int launch_tp_index(const TpArgs &a, hipStream_t s);         // field_pos, field_row, row_pos, row_field0; then the rows' checks and label ranges
int launch_tp_rows(const TpArgs &a, hipStream_t s);          // the rows' checks and label ranges alone, timed as table_cols_rows (K26: needs row_pos, row_field0 only)
int launch_tp_parse(const TpArgs &a, hipStream_t s);
int launch_tp_collect(const TpArgs &a, hipStream_t s);
int launch_tp_patch(const TpArgs &a, const int64_t *slot, const uint64_t *bits, int32_t n, hipStream_t s);
int launch_tp_transpose(const TpArgs &a, hipStream_t s);
// K26, the column-selected entry: its launches (table_cols_kernels.hip)
struct TcArgs {
    TpArgs tp;                             // n_cols: the file's; vals: [n_rows * n_cols_out], row r, output column k at r * n_cols_out + k
    const int32_t *col_map;                // [tp.n_cols] output column of a file column, or -1
    int64_t n_cols_out;
    uint32_t *sel_pos;                     // [n_rows * n_cols_out] first byte of the field staged at that slot; TC_ABSENT: a ragged row lacks it
};
constexpr uint32_t TC_ABSENT = 0xffffffffu;
int launch_tc_index(const TcArgs &a, hipStream_t s);         // row_pos, row_field0; the rows' checks; sel_pos
int launch_tc_parse(const TcArgs &a, hipStream_t s);
int launch_tc_collect(const TcArgs &a, hipStream_t s);

int launch_gather_matrix(const double *in, int64_t ld_in, const int32_t *genes, int64_t n_genes, const int32_t *cells, int64_t n_cells,
                         double *out, int64_t ld_out, hipStream_t s);

}  // namespace icnv
