// K20: plot_cnv's matrix files as text (include/icnv.h "matrix files of plot_cnv").  Three passes over a chunk of whole file
// rows: digits (one record per element), lengths (segment and row byte counts), emit (the characters).  The host side --
// validation, the host formatting of flagged elements, the scan of the row byte counts -- is table_text_api.hip.
// DESIGN.md section 4 K20.
#include "icnv_internal.h"
#include "table_text_internal.h"

namespace icnv {

namespace {

// ---- digits (the arithmetic and its certification: table_text_digits.h) ---------------------------------------------------
__device__ inline void tt_flag(const TtArgs &a, int64_t idx, uint64_t bits) {
    const uint32_t slot = atomicAdd(a.n_flagged, 1u);
    if (slot < (uint32_t)TT_FLAG_CAP) a.flagged[slot] = TtFlagged{idx, bits};
}

// Gene rows: a 64 genes x 64 fields tile.  Reads run along the genes of one cell (contiguous), the records leave in file
// order (along the fields of one gene) after a transpose through LDS.
__global__ __launch_bounds__(TT_NT) void tt_digits_gene_rows_kernel(TtArgs a) {
    __shared__ uint64_t s_rec[TT_TILE][TT_TILE + 1];
    __shared__ uint16_t s_meta[TT_TILE][TT_TILE + 2];
    const int64_t tiles_f = (a.n_fields + TT_TILE - 1) / TT_TILE;
    const int64_t r_base = ((int64_t)blockIdx.x / tiles_f) * TT_TILE, j_base = ((int64_t)blockIdx.x % tiles_f) * TT_TILE;
    const int tx = threadIdx.x & (TT_TILE - 1), ty = threadIdx.x >> 6;
    for (int cc = ty; cc < TT_TILE; cc += TT_NT / TT_TILE) {
        const int64_t r = r_base + tx, j = j_base + cc;
        if (r < a.n_rows && j < a.n_fields) {
            const uint64_t bits = (uint64_t)__double_as_longlong(a.x[(int64_t)a.cells[j] * a.ld + a.row0 + r]);
            uint64_t rec;
            uint16_t meta;
            tt_digits(bits, rec, meta);
            if (rec & TT_FLAG_BIT) tt_flag(a, r * a.n_fields + j, bits);
            s_rec[cc][tx] = rec;
            s_meta[cc][tx] = meta;
        }
    }
    __syncthreads();
    for (int rr = ty; rr < TT_TILE; rr += TT_NT / TT_TILE) {
        const int64_t r = r_base + rr, j = j_base + tx;
        if (r < a.n_rows && j < a.n_fields) {
            a.rec[r * a.n_fields + j] = s_rec[tx][rr];
            a.meta[r * a.n_fields + j] = s_meta[tx][rr];
        }
    }
}

// Cell rows: file order is memory order; one workgroup per (row, segment).
__global__ __launch_bounds__(TT_NT) void tt_digits_cell_rows_kernel(TtArgs a) {
    const int64_t r = (int64_t)blockIdx.x / a.n_seg, j = ((int64_t)blockIdx.x % a.n_seg) * TT_SEG + threadIdx.x;
    if (r >= a.n_rows || j >= a.n_fields) return;
    const uint64_t bits = (uint64_t)__double_as_longlong(a.x[(int64_t)a.cells[r] * a.ld + j]);
    uint64_t rec;
    uint16_t meta;
    tt_digits(bits, rec, meta);
    if (rec & TT_FLAG_BIT) tt_flag(a, r * a.n_fields + j, bits);
    a.rec[r * a.n_fields + j] = rec;
    a.meta[r * a.n_fields + j] = meta;
}

// More than TT_FLAG_CAP flagged elements: list (up to the capacity) those that still carry the bit.
__global__ __launch_bounds__(TT_NT) void tt_collect_kernel(TtArgs a) {
    const int64_t n = a.n_rows * a.n_fields;
    for (int64_t i = (int64_t)blockIdx.x * TT_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * TT_NT) {
        if (!(a.rec[i] & TT_FLAG_BIT)) continue;
        const int64_t r = i / a.n_fields, j = i % a.n_fields;
        const double v = a.orientation == TT_GENE_ROWS ? a.x[(int64_t)a.cells[j] * a.ld + a.row0 + r] : a.x[(int64_t)a.cells[r] * a.ld + j];
        tt_flag(a, i, (uint64_t)__double_as_longlong(v));
    }
}

__global__ __launch_bounds__(TT_NT) void tt_patch_kernel(uint64_t *rec, uint16_t *meta, const int64_t *idx, const uint64_t *new_rec,
                                                         const uint16_t *new_meta, int32_t n) {
    const int i = blockIdx.x * TT_NT + threadIdx.x;
    if (i < n) {
        rec[idx[i]] = new_rec[i];
        meta[idx[i]] = new_meta[i];
    }
}

// ---- lengths --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TT_NT) void tt_seg_sum_kernel(TtArgs a) {
    __shared__ uint32_t s_part[TT_NT / 64];
    const int64_t r = (int64_t)blockIdx.x / a.n_seg, seg = (int64_t)blockIdx.x % a.n_seg, j = seg * TT_SEG + threadIdx.x;
    uint32_t v = (r < a.n_rows && j < a.n_fields) ? (uint32_t)(a.meta[r * a.n_fields + j] >> 10) + 1u : 0u;   // + separator / newline
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0 && r < a.n_rows) a.seg_sum[r * a.n_seg + seg] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

__global__ __launch_bounds__(TT_NT) void tt_row_bytes_kernel(TtArgs a) {
    const int64_t r = (int64_t)blockIdx.x * TT_NT + threadIdx.x;
    if (r >= a.n_rows) return;
    int64_t acc = a.lab_off ? a.lab_off[r + 1] - a.lab_off[r] + 1 : 0;    // the label and its separator
    for (int64_t s = 0; s < a.n_seg; ++s) {
        a.seg_off[r * a.n_seg + s] = acc;
        acc += a.seg_sum[r * a.n_seg + s];
    }
    a.row_bytes[r] = acc;
}

// ---- emit -----------------------------------------------------------------------------------------------------------------
// One workgroup per (row, segment): a lane per field.  The text of the segment is assembled in LDS at the byte offset that
// its first byte has within a 16-byte word of the output, so LDS words and output words line up: whole words leave as 16-byte
// stores, the ragged ends byte by byte.  No byte of the output is written by two workgroups.
constexpr int TT_TXT_WORDS = (TT_SEG * (TT_MAX_FIELD + 1) + 15) / 16 + 1;
__global__ __launch_bounds__(TT_NT) void tt_emit_kernel(TtArgs a) {
    __shared__ uint4 s_txt4[TT_TXT_WORDS];
    __shared__ int s_scan[TT_NT];
    uint8_t *s_txt = reinterpret_cast<uint8_t *>(s_txt4);
    const int tid = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x / a.n_seg, seg = (int64_t)blockIdx.x % a.n_seg, j = seg * TT_SEG + tid;
    const bool live = j < a.n_fields;
    uint64_t rec = 0;
    int len = 0, E = 0;
    if (live) {
        rec = a.rec[r * a.n_fields + j];
        const uint16_t meta = a.meta[r * a.n_fields + j];
        len = meta >> 10;
        E = (int)(meta & 1023) - TT_E_BIAS;
    }
    const int mine = live ? len + 1 : 0;
    s_scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < TT_NT; d <<= 1) {
        const int add = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    const int total = s_scan[TT_NT - 1], at = s_scan[tid] - mine;
    const int64_t row_at = a.row_off[r];
    if (seg == 0 && a.lab_off) {                               // the label and its separator
        const int64_t l0 = a.lab_off[r], ln = a.lab_off[r + 1] - l0;
        for (int64_t i = tid; i <= ln; i += TT_NT) a.out[row_at + i] = i < ln ? a.lab[l0 + i] : a.sep;
    }
    uint8_t *dst = a.out + row_at + a.seg_off[r * a.n_seg + seg];
    const int shift = (int)(reinterpret_cast<uintptr_t>(dst) & 15);
    if (live) {
        uint8_t *w = s_txt + shift + at;
        for (int p = 0; p < len; ++p) w[p] = tt_char(p, rec, E, len);
        w[len] = j == a.n_fields - 1 ? (uint8_t)'\n' : a.sep;
    }
    __syncthreads();
    uint8_t *base = dst - shift;                               // 16-byte aligned
    const int end = shift + total;
    for (int w = tid; w * 16 < end; w += TT_NT) {
        const int lo = w * 16, hi = lo + 16;
        if (lo >= shift && hi <= end) reinterpret_cast<uint4 *>(base)[w] = s_txt4[w];
        else
            for (int b = lo > shift ? lo : shift; b < (hi < end ? hi : end); ++b) base[b] = s_txt[b];
    }
}

int tt_grid(int64_t blocks, unsigned &grid) {
    if (blocks < 1 || blocks > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "format_table: the chunk needs more than 2^31 - 1 workgroups");
    grid = (unsigned)blocks;
    return ICNV_OK;
}

}  // namespace

int launch_tt_digits(const TtArgs &a, hipStream_t s) {
    KernelTimer kt("table_text_digits", s);
    unsigned grid;
    int rc;
    if (a.orientation == TT_GENE_ROWS) {
        const int64_t tiles = ((a.n_rows + TT_TILE - 1) / TT_TILE) * ((a.n_fields + TT_TILE - 1) / TT_TILE);
        if ((rc = tt_grid(tiles, grid))) return rc;
        hipLaunchKernelGGL(tt_digits_gene_rows_kernel, dim3(grid), dim3(TT_NT), 0, s, a);
    } else {
        if ((rc = tt_grid(a.n_rows * a.n_seg, grid))) return rc;
        hipLaunchKernelGGL(tt_digits_cell_rows_kernel, dim3(grid), dim3(TT_NT), 0, s, a);
    }
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_tt_collect(const TtArgs &a, hipStream_t s) {
    KernelTimer kt("table_text_collect", s);
    const int64_t blocks = (a.n_rows * a.n_fields + TT_NT - 1) / TT_NT, cap = (int64_t)num_cus() * 8;
    hipLaunchKernelGGL(tt_collect_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(TT_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_tt_patch(const TtArgs &a, const int64_t *idx, const uint64_t *rec, const uint16_t *meta, int32_t n, hipStream_t s) {
    hipLaunchKernelGGL(tt_patch_kernel, dim3((unsigned)((n + TT_NT - 1) / TT_NT)), dim3(TT_NT), 0, s, a.rec, a.meta, idx, rec, meta, n);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_tt_lengths(const TtArgs &a, hipStream_t s) {
    KernelTimer kt("table_text_lengths", s);
    unsigned grid;
    int rc;
    if ((rc = tt_grid(a.n_rows * a.n_seg, grid))) return rc;
    hipLaunchKernelGGL(tt_seg_sum_kernel, dim3(grid), dim3(TT_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    hipLaunchKernelGGL(tt_row_bytes_kernel, dim3((unsigned)((a.n_rows + TT_NT - 1) / TT_NT)), dim3(TT_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_tt_emit(const TtArgs &a, int64_t n_rows_fit, hipStream_t s) {
    KernelTimer kt("table_text_emit", s);
    unsigned grid;
    int rc;
    if ((rc = tt_grid(n_rows_fit * a.n_seg, grid))) return rc;
    hipLaunchKernelGGL(tt_emit_kernel, dim3(grid), dim3(TT_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
