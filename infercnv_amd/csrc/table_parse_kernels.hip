// K21: a chunk of a text table to doubles in the library's layout (include/icnv.h "count matrices from text").  Passes over a
// chunk of whole lines: structure (row and field starts counted per segment, scanned), index (the lists of field and row
// starts), rows (field counts, labels), parse (one lane per field), transpose (file order to cell-major through LDS).  The
// host side -- validation, strtod for the fields the parse does not certify, the error text -- is table_parse_api.hip.
// DESIGN.md section 4 K21.
#include "icnv_internal.h"
#include "table_parse_internal.h"

namespace icnv {

namespace {

// ---- structure (tp_masks, tp_block_scan: table_parse_internal.h) ---------------------------------------------------------
__global__ __launch_bounds__(TP_NT) void tp_count_kernel(TpArgs a) {
    __shared__ uint32_t s_part[TP_NT / 64];
    uint32_t rows, fields;
    tp_masks(a, ((int64_t)blockIdx.x * TP_NT + threadIdx.x) * TP_BYTES, rows, fields);
    uint32_t v = tp_packed_counts(rows, fields);             // at most 4096 of either in a segment: the halves do not meet
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) a.seg_count[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// One workgroup: the exclusive scans of the segments' row and field counts, and the totals.
__global__ __launch_bounds__(TP_NT) void tp_scan_kernel(TpArgs a) {
    __shared__ uint32_t s_scan[TP_NT];
    uint32_t carry_r = 0, carry_f = 0;
    for (int64_t i0 = 0; i0 < a.n_seg; i0 += TP_NT) {
        const int64_t i = i0 + threadIdx.x;
        const uint32_t c = i < a.n_seg ? a.seg_count[i] : 0u, r = c >> 16, f = c & 0xffffu;
        const uint32_t inc_r = tp_block_scan(r, s_scan), tot_r = s_scan[TP_NT - 1];
        __syncthreads();
        const uint32_t inc_f = tp_block_scan(f, s_scan), tot_f = s_scan[TP_NT - 1];
        __syncthreads();
        if (i < a.n_seg) {
            a.seg_row_off[i] = carry_r + inc_r - r;
            a.seg_field_off[i] = carry_f + inc_f - f;
        }
        carry_r += tot_r;
        carry_f += tot_f;
    }
    if (threadIdx.x == 0) {
        a.totals[0] = carry_r;
        a.totals[1] = carry_f;
    }
}

// ---- index ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TP_NT) void tp_index_kernel(TpArgs a) {
    __shared__ uint32_t s_scan[TP_NT];
    tp_index_starts<true>(a, s_scan);
}

// One lane per row: the field count, the label's range and its quotes.
__global__ __launch_bounds__(TP_NT) void tp_rows_kernel(TpArgs a) {
    const int64_t r = (int64_t)blockIdx.x * TP_NT + threadIdx.x;
    if (r >= a.n_rows) return;
    const int64_t f0 = a.row_field0[r], f1 = r + 1 < a.n_rows ? (int64_t)a.row_field0[r + 1] : a.n_fields, p0 = a.row_pos[r];
    if (f1 - f0 != a.n_cols + 1) tp_refuse(a, p0, 1 /* TP_E_RAGGED */);
    const int64_t e = tp_field_end(a.text, a.n, p0, a.sep);
    const bool quoted = e - p0 >= 2 && a.text[p0] == '"' && a.text[e - 1] == '"';
    for (int64_t i = p0; i < e; ++i)
        if (a.text[i] == '"' && !(quoted && (i == p0 || i == e - 1))) {
            tp_refuse(a, i, 3 /* TP_E_LABEL */);
            break;
        }
    a.label_range[2 * r] = (int32_t)p0;
    a.label_range[2 * r + 1] = (int32_t)e;
}

// ---- parse ----------------------------------------------------------------------------------------------------------------
// One lane per field start.  The label (field 0) and the fields of a ragged row beyond n_cols are left alone; the rows pass
// refuses such a chunk.  The values are staged in file order: row r, column c at vals[r * n_cols + c].
__global__ __launch_bounds__(TP_NT) void tp_parse_kernel(TpArgs a) {
    const int64_t f = (int64_t)blockIdx.x * TP_NT + threadIdx.x;
    if (f >= a.n_fields) return;
    const int64_t p = a.field_pos[f], r = a.field_row[f];
    if (p > a.n || r >= a.n_rows) return;                      // cannot happen: the index pass wrote every entry from the same masks
    const int64_t c = f - (int64_t)a.row_field0[r];
    if (c < 1 || c > a.n_cols) return;
    const int64_t slot = r * a.n_cols + c - 1;
    tp_stage_field(a, p, slot);
}

// More than TP_FLAG_CAP uncertified fields: list (up to the capacity) those that are still pending.  Runs only on a chunk
// whose rows all have n_cols + 1 fields.
__global__ __launch_bounds__(TP_NT) void tp_collect_kernel(TpArgs a) {
    const int64_t n = a.n_rows * a.n_cols;
    for (int64_t i = (int64_t)blockIdx.x * TP_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * TP_NT) {
        if (a.vals[i] != TP_PENDING) continue;
        const int64_t r = i / a.n_cols, c = i % a.n_cols;
        tp_flag(a, i, a.field_pos[(int64_t)a.row_field0[r] + c + 1]);
    }
}

__global__ __launch_bounds__(TP_NT) void tp_patch_kernel(uint64_t *vals, const int64_t *slot, const uint64_t *bits, int32_t n) {
    const int i = blockIdx.x * TP_NT + threadIdx.x;
    if (i < n) vals[slot[i]] = bits[i];
}

// ---- transpose ------------------------------------------------------------------------------------------------------------
// A 64 rows x 64 columns tile: the reads run along the columns of one file row (contiguous in vals), the stores along the rows
// of one column (contiguous in out).  The padded LDS row keeps both sides free of bank conflicts.
__global__ __launch_bounds__(TP_NT) void tp_transpose_kernel(TpArgs a) {
    __shared__ uint64_t s_tile[TP_TILE][TP_TILE + 1];
    const int64_t tiles_c = (a.n_cols + TP_TILE - 1) / TP_TILE;
    const int64_t r_base = ((int64_t)blockIdx.x / tiles_c) * TP_TILE, c_base = ((int64_t)blockIdx.x % tiles_c) * TP_TILE;
    const int tx = threadIdx.x & (TP_TILE - 1), ty = threadIdx.x >> 6;
    for (int rr = ty; rr < TP_TILE; rr += TP_NT / TP_TILE) {
        const int64_t r = r_base + rr, c = c_base + tx;
        if (r < a.n_rows && c < a.n_cols) s_tile[rr][tx] = a.vals[r * a.n_cols + c];
    }
    __syncthreads();
    for (int cc = ty; cc < TP_TILE; cc += TP_NT / TP_TILE) {
        const int64_t r = r_base + tx, c = c_base + cc;
        if (r < a.n_rows && c < a.n_cols) a.out[c * a.ld + a.row0 + r] = __longlong_as_double((long long)s_tile[tx][cc]);
    }
}

// ---- gather ---------------------------------------------------------------------------------------------------------------
// out[j * ld_out + i] = in[cells[j] * ld_in + genes[i]]; a null list is the identity.  One workgroup per (cell, 256 genes).
__global__ __launch_bounds__(TP_NT) void gather_matrix_kernel(const double *in, int64_t ld_in, const int32_t *genes, int64_t n_genes,
                                                              const int32_t *cells, int64_t gene_blocks, double *out, int64_t ld_out) {
    const int64_t j = (int64_t)blockIdx.x / gene_blocks, i = ((int64_t)blockIdx.x % gene_blocks) * TP_NT + threadIdx.x;
    if (i >= n_genes) return;
    const int64_t c = cells ? (int64_t)cells[j] : j, g = genes ? (int64_t)genes[i] : i;
    out[j * ld_out + i] = in[c * ld_in + g];
}

// The rows pass without a timer of its own: launch_tp_index and launch_tp_rows each run it under theirs.
int tp_rows_untimed(const TpArgs &a, hipStream_t s) {
    unsigned grid;
    int rc;
    if ((rc = tp_grid((a.n_rows + TP_NT - 1) / TP_NT, grid, "parse_table"))) return rc;
    hipLaunchKernelGGL(tp_rows_kernel, dim3(grid), dim3(TP_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace

int tp_grid(int64_t blocks, unsigned &grid, const char *who) {
    if (blocks < 1 || blocks > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, std::string(who) + ": the chunk needs more than 2^31 - 1 workgroups");
    grid = (unsigned)blocks;
    return ICNV_OK;
}

int launch_tp_structure(const TpArgs &a, hipStream_t s) {
    KernelTimer kt("table_parse_structure", s);
    unsigned grid;
    int rc;
    if ((rc = tp_grid(a.n_seg, grid, "parse_table"))) return rc;
    hipLaunchKernelGGL(tp_count_kernel, dim3(grid), dim3(TP_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    hipLaunchKernelGGL(tp_scan_kernel, dim3(1), dim3(TP_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_tp_index(const TpArgs &a, hipStream_t s) {
    KernelTimer kt("table_parse_index", s);
    unsigned grid;
    int rc;
    if ((rc = tp_grid(a.n_seg, grid, "parse_table"))) return rc;
    hipLaunchKernelGGL(tp_index_kernel, dim3(grid), dim3(TP_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return tp_rows_untimed(a, s);
}

int launch_tp_rows(const TpArgs &a, hipStream_t s) {
    KernelTimer kt("table_cols_rows", s);
    return tp_rows_untimed(a, s);
}

int launch_tp_parse(const TpArgs &a, hipStream_t s) {
    KernelTimer kt("table_parse_fields", s);
    unsigned grid;
    int rc;
    if ((rc = tp_grid((a.n_fields + TP_NT - 1) / TP_NT, grid, "parse_table"))) return rc;
    hipLaunchKernelGGL(tp_parse_kernel, dim3(grid), dim3(TP_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_tp_collect(const TpArgs &a, hipStream_t s) {
    KernelTimer kt("table_parse_collect", s);
    const int64_t blocks = (a.n_rows * a.n_cols + TP_NT - 1) / TP_NT, cap = (int64_t)num_cus() * 8;
    hipLaunchKernelGGL(tp_collect_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(TP_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_tp_patch(const TpArgs &a, const int64_t *slot, const uint64_t *bits, int32_t n, hipStream_t s) {
    hipLaunchKernelGGL(tp_patch_kernel, dim3((unsigned)((n + TP_NT - 1) / TP_NT)), dim3(TP_NT), 0, s, a.vals, slot, bits, n);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_tp_transpose(const TpArgs &a, hipStream_t s) {
    KernelTimer kt("table_parse_transpose", s);
    unsigned grid;
    int rc;
    if ((rc = tp_grid(((a.n_rows + TP_TILE - 1) / TP_TILE) * ((a.n_cols + TP_TILE - 1) / TP_TILE), grid, "parse_table"))) return rc;
    hipLaunchKernelGGL(tp_transpose_kernel, dim3(grid), dim3(TP_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_gather_matrix(const double *in, int64_t ld_in, const int32_t *genes, int64_t n_genes, const int32_t *cells, int64_t n_cells,
                         double *out, int64_t ld_out, hipStream_t s) {
    KernelTimer kt("gather_matrix", s);
    const int64_t gene_blocks = (n_genes + TP_NT - 1) / TP_NT;
    unsigned grid;
    int rc;
    if ((rc = tp_grid(gene_blocks * n_cells, grid, "parse_table"))) return rc;
    hipLaunchKernelGGL(gather_matrix_kernel, dim3(grid), dim3(TP_NT), 0, s, in, ld_in, genes, n_genes, cells, gene_blocks, out, ld_out);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
