// K26: the columns a rank owns out of a chunk of a text table (include/icnv.h "reading a selection of columns").  The check of
// a column map, shared with the triplet flavour (triplets_cols_kernels.hip); then, after K21's structure pass over the whole
// chunk: index (the rows' starts; the rows' checks of K21; the first byte of every SELECTED field), parse (one lane per
// selected field), collect.  The staged values are n_cols_out wide and go through K21's transpose.  The host side is
// the driver K21 and K26 share in table_parse_api.hip; the index pass and the conversion of a field are K21's device functions
// (table_parse_internal.h).  DESIGN.md section 4 K26.
#include "icnv_internal.h"
#include "col_map_internal.h"
#include "table_parse_internal.h"

namespace icnv {

namespace {

// ---- column map -----------------------------------------------------------------------------------------------------------
// error word: kind << 62 | index << 8 | kind, the smallest wins: an entry out of range before a repeat before an unhit column.
// inv[k] starts at CM_UNHIT and ends as the smallest file column that maps to k.
__global__ __launch_bounds__(TP_NT) void cm_range_kernel(const int32_t *col_map, int64_t n_cols, int64_t n_cols_out, int32_t *inv,
                                                         unsigned long long *error) {
    const int64_t c = (int64_t)blockIdx.x * TP_NT + threadIdx.x;
    if (c >= n_cols) return;
    const int64_t k = col_map[c];
    if (k < -1 || k >= n_cols_out) atomicMin(error, ((unsigned long long)c << 8) | (unsigned long long)CM_E_RANGE);
    else if (k >= 0) atomicMin(&inv[k], (int32_t)c);
}

__global__ __launch_bounds__(TP_NT) void cm_hits_kernel(const int32_t *col_map, int64_t n_cols, int64_t n_cols_out, const int32_t *inv,
                                                        unsigned long long *error) {
    const int64_t c = (int64_t)blockIdx.x * TP_NT + threadIdx.x;
    if (c < n_cols) {
        const int64_t k = col_map[c];
        if (k >= 0 && k < n_cols_out && inv[k] != (int32_t)c)
            atomicMin(error, (1ull << 62) | ((unsigned long long)c << 8) | (unsigned long long)CM_E_REPEAT);
    }
    if (c < n_cols_out && inv[c] == CM_UNHIT) atomicMin(error, (2ull << 62) | ((unsigned long long)c << 8) | (unsigned long long)CM_E_UNHIT);
}

// ---- index ----------------------------------------------------------------------------------------------------------------
// K21's index pass without the field lists: the rows' first bytes and first fields only.
__global__ __launch_bounds__(TP_NT) void tc_index_rows_kernel(TpArgs a) {
    __shared__ uint32_t s_scan[TP_NT];
    tp_index_starts<false>(a, s_scan);
}

// Runs after tc_index_rows_kernel: the field start f of row r is file column f - row_field0[r] - 1; where the map selects it,
// its first byte goes to the slot of (r, output column).  A field beyond n_cols of a ragged row is left alone.
__global__ __launch_bounds__(TP_NT) void tc_index_fields_kernel(TcArgs t) {
    __shared__ uint32_t s_scan[TP_NT];
    const TpArgs &a = t.tp;
    const int64_t base = ((int64_t)blockIdx.x * TP_NT + threadIdx.x) * TP_BYTES;
    uint32_t rows, fields;
    tp_masks(a, base, rows, fields);
    const uint32_t mine = tp_packed_counts(rows, fields), excl = tp_block_scan(mine, s_scan) - mine;
    int64_t r = (int64_t)a.seg_row_off[blockIdx.x] + (excl >> 16), f = (int64_t)a.seg_field_off[blockIdx.x] + (excl & 0xffffu);
    while (fields) {
        const int j = __ffs((int)fields) - 1;
        fields &= fields - 1;
        if ((rows >> j) & 1u) ++r;
        if (r >= 1 && r <= a.n_rows) {
            const int64_t c = f - (int64_t)a.row_field0[r - 1] - 1;
            if (c >= 0 && c < a.n_cols) {
                const int64_t k = t.col_map[c];
                if (k >= 0 && k < t.n_cols_out) t.sel_pos[(r - 1) * t.n_cols_out + k] = (uint32_t)(base + j);
            }
        }
        ++f;
    }
}

// ---- parse ----------------------------------------------------------------------------------------------------------------
// One lane per selected field; the conversion is tp_parse_kernel's.  The fields of skipped columns have no lane.
__global__ __launch_bounds__(TP_NT) void tc_parse_kernel(TcArgs t) {
    const TpArgs &a = t.tp;
    const int64_t slot = (int64_t)blockIdx.x * TP_NT + threadIdx.x;
    if (slot >= a.n_rows * t.n_cols_out) return;
    const uint32_t at = t.sel_pos[slot];
    if (at == TC_ABSENT || (int64_t)at > a.n) return;          // a ragged row without this field: the rows pass refuses the chunk
    tp_stage_field(a, at, slot);
}

// More than TP_FLAG_CAP uncertified fields: list (up to the capacity) those that are still pending.  Runs only on a chunk
// whose rows all have n_cols + 1 fields, so every slot has its position.
__global__ __launch_bounds__(TP_NT) void tc_collect_kernel(TcArgs t) {
    const TpArgs &a = t.tp;
    const int64_t n = a.n_rows * t.n_cols_out;
    for (int64_t i = (int64_t)blockIdx.x * TP_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * TP_NT)
        if (a.vals[i] == TP_PENDING && t.sel_pos[i] != TC_ABSENT) tp_flag(a, i, t.sel_pos[i]);
}

}  // namespace

int check_col_map(const int32_t *col_map_dev, int64_t n_cols, int64_t n_cols_out, const char *who, hipStream_t s) {
    if (n_cols_out < 1 || n_cols_out > n_cols) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": n_cols_out must be 1 .. n_cols");
    DevBuf d_inv, d_word;
    int rc;
    if ((rc = d_inv.alloc((size_t)n_cols_out * sizeof(int32_t))) || (rc = d_word.alloc(sizeof(unsigned long long)))) return rc;
    const unsigned long long none = ~0ull;
    unsigned long long word = 0;
    {
        KernelTimer kt("col_map_check", s);
        ICNV_HIP(hipMemsetAsync(d_inv.p, 0x7f, (size_t)n_cols_out * sizeof(int32_t), s));      // CM_UNHIT in every element
        ICNV_HIP(hipMemcpyAsync(d_word.p, &none, sizeof none, hipMemcpyHostToDevice, s));
        const unsigned grid = (unsigned)((n_cols + TP_NT - 1) / TP_NT);                        // n_cols <= 2^31 - 1
        hipLaunchKernelGGL(cm_range_kernel, dim3(grid), dim3(TP_NT), 0, s, col_map_dev, n_cols, n_cols_out, d_inv.as<int32_t>(),
                           d_word.as<unsigned long long>());
        ICNV_HIP(hipGetLastError());
        hipLaunchKernelGGL(cm_hits_kernel, dim3(grid), dim3(TP_NT), 0, s, col_map_dev, n_cols, n_cols_out, d_inv.as<int32_t>(),
                           d_word.as<unsigned long long>());
        ICNV_HIP(hipGetLastError());
    }
    ICNV_HIP(hipMemcpyAsync(&word, d_word.p, sizeof word, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (word == none) return ICNV_OK;
    const std::string at = std::to_string((word & ~(3ull << 62)) >> 8);
    switch ((int)(word & 0xff)) {
    case CM_E_RANGE: ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": entry " + at + " of the column map is outside -1 .. n_cols_out - 1");
    case CM_E_REPEAT: ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": entry " + at + " of the column map names an output column a second time");
    default: ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": output column " + at + " is hit by no entry of the column map");
    }
}

int launch_tc_index(const TcArgs &t, hipStream_t s) {
    unsigned grid;
    int rc;
    if ((rc = tp_grid(t.tp.n_seg, grid, "parse_table_cols"))) return rc;
    {
        KernelTimer kt("table_cols_index", s);
        hipLaunchKernelGGL(tc_index_rows_kernel, dim3(grid), dim3(TP_NT), 0, s, t.tp);
        ICNV_HIP(hipGetLastError());
    }
    if ((rc = launch_tp_rows(t.tp, s))) return rc;
    KernelTimer kt("table_cols_index", s);
    ICNV_HIP(hipMemsetAsync(t.sel_pos, 0xff, (size_t)(t.tp.n_rows * t.n_cols_out) * sizeof(uint32_t), s));   // TC_ABSENT
    hipLaunchKernelGGL(tc_index_fields_kernel, dim3(grid), dim3(TP_NT), 0, s, t);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_tc_parse(const TcArgs &t, hipStream_t s) {
    KernelTimer kt("table_cols_fields", s);
    unsigned grid;
    int rc;
    if ((rc = tp_grid((t.tp.n_rows * t.n_cols_out + TP_NT - 1) / TP_NT, grid, "parse_table_cols"))) return rc;
    hipLaunchKernelGGL(tc_parse_kernel, dim3(grid), dim3(TP_NT), 0, s, t);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_tc_collect(const TcArgs &t, hipStream_t s) {
    KernelTimer kt("table_cols_collect", s);
    const int64_t blocks = (t.tp.n_rows * t.n_cols_out + TP_NT - 1) / TP_NT, cap = (int64_t)num_cus() * 8;
    hipLaunchKernelGGL(tc_collect_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(TP_NT), 0, s, t);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
