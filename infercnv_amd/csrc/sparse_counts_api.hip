// C ABI of K22 (include/icnv.h "sparse count matrices"): validation, the order of the passes, the text of a refusal.
// Kernels: sparse_counts_kernels.hip.  DESIGN.md section 4 K22.
#include <string>

#include "icnv_internal.h"
#include "sparse_counts_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

extern "C" {

int icnv_parse_triplets_dev(const uint8_t *text_dev, const uint8_t *text_host, int64_t n_bytes, int32_t field, int64_t n_rows, int64_t n_cols,
                            int64_t line0, int32_t *row_dev, int32_t *col_dev, int32_t *val_dev, int64_t capacity, int64_t *n_entries,
                            void *stream) {
    if (!text_dev || !n_entries) ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: null argument");
    if (n_bytes < 1 || n_bytes > 0x7ffffffe) ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: a chunk has 1 .. 2^31 - 2 bytes");
    if (reinterpret_cast<uintptr_t>(text_dev) & 15) ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: the device text must start on a 16-byte boundary");
    if (field != ICNV_MM_INTEGER && field != ICNV_MM_REAL && field != ICNV_MM_PATTERN)
        ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: field must be ICNV_MM_INTEGER, ICNV_MM_REAL or ICNV_MM_PATTERN");
    if (n_rows < 1 || n_rows > 0x7fffffff || n_cols < 1 || n_cols > 0x7fffffff)
        ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: n_rows and n_cols must be 1 .. 2^31 - 1");
    if (line0 < 1) ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: line0 counts from 1");
    if (capacity < 0 || (capacity > 0 && (!row_dev || !col_dev || !val_dev)))
        ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: capacity must be >= 0 and the output arrays must be given");
    hipStream_t s = (hipStream_t)stream;
    int rc;

    ScParseArgs a{};
    a.text = text_dev; a.n = n_bytes; a.field = field; a.G = n_rows; a.C = n_cols;
    a.n_seg = (n_bytes + SC_SEG - 1) / SC_SEG;
    DevBuf d_seg, d_small;
    if ((rc = d_seg.alloc((size_t)a.n_seg * 2 * sizeof(uint32_t))) || (rc = d_small.alloc(2 * sizeof(uint64_t)))) return rc;
    a.seg_count = d_seg.as<uint32_t>(); a.seg_off = a.seg_count + a.n_seg;
    a.error = d_small.as<unsigned long long>();                       // word 0: the error; word 1: the total
    a.total = reinterpret_cast<uint32_t *>(a.error + 1);
    const uint64_t init[2] = {SC_NO_ERROR, 0};
    ICNV_HIP(hipMemcpyAsync(d_small.p, init, sizeof init, hipMemcpyHostToDevice, s));

    // structure: how many entries
    if ((rc = launch_sc_structure(a, s))) return rc;
    uint32_t total = 0;
    ICNV_HIP(hipMemcpyAsync(&total, a.total, sizeof total, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    a.n_entries = total;
    if (a.n_entries > capacity)
        ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: the chunk has " + std::to_string(a.n_entries) + " entries, capacity is " + std::to_string(capacity));
    if (a.n_entries == 0) {                                             // blank lines only
        *n_entries = 0;
        return ICNV_OK;
    }

    // index, parse into staged arrays; the caller's arrays are written only when nothing was refused
    DevBuf d_pos, d_stage;
    if ((rc = d_pos.alloc((size_t)a.n_entries * sizeof(uint32_t))) || (rc = d_stage.alloc((size_t)a.n_entries * 3 * sizeof(int32_t)))) return rc;
    a.line_pos = d_pos.as<uint32_t>();
    a.row = d_stage.as<int32_t>(); a.col = a.row + a.n_entries; a.val = a.col + a.n_entries;
    if ((rc = launch_sc_index(a, s)) || (rc = launch_sc_parse(a, s))) return rc;
    uint64_t word = 0;
    ICNV_HIP(hipMemcpyAsync(&word, a.error, sizeof word, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (word != SC_NO_ERROR) {
        if ((int64_t)(word >> 8) >= n_bytes) ICNV_FAIL(ICNV_ERR_HIP, "parse_triplets: a refusal lies outside the chunk (internal error)");
        HostText host{text_host, text_dev, n_bytes, s, {}};
        const uint8_t *text = nullptr;
        if ((rc = host.get(text))) return rc;
        ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: " + sc_describe(text, n_bytes, word, field, n_rows, n_cols, line0));
    }
    const size_t bytes = (size_t)a.n_entries * sizeof(int32_t);
    ICNV_HIP(hipMemcpyAsync(row_dev, a.row, bytes, hipMemcpyDeviceToDevice, s));
    ICNV_HIP(hipMemcpyAsync(col_dev, a.col, bytes, hipMemcpyDeviceToDevice, s));
    ICNV_HIP(hipMemcpyAsync(val_dev, a.val, bytes, hipMemcpyDeviceToDevice, s));
    ICNV_HIP(hipStreamSynchronize(s));                                  // the staged arrays go back to the pool
    *n_entries = a.n_entries;
    return ICNV_OK;
}

int icnv_csc_from_sorted_triplets_dev(const int32_t *row_dev, const int32_t *col_dev, int64_t nnz, int64_t G, int64_t C, int64_t *colptr_dev,
                                      int64_t *first_violation, int32_t *violation_kind, void *stream) {
    if (!colptr_dev || !first_violation || !violation_kind) ICNV_FAIL(ICNV_ERR_ARG, "csc_from_sorted_triplets: null argument");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "csc_from_sorted_triplets: G and C must be 1 .. 2^31 - 1");
    if (nnz < 0 || (nnz > 0 && (!row_dev || !col_dev))) ICNV_FAIL(ICNV_ERR_ARG, "csc_from_sorted_triplets: nnz must be >= 0 and the arrays must be given");
    hipStream_t s = (hipStream_t)stream;
    *first_violation = -1;
    *violation_kind = ICNV_CSC_SORTED;
    if (nnz == 0) {                                                     // an empty matrix: no launch
        ICNV_HIP(hipMemsetAsync(colptr_dev, 0, (size_t)(C + 1) * sizeof(int64_t), s));
        ICNV_HIP(hipStreamSynchronize(s));
        return ICNV_OK;
    }
    DevBuf d_word;
    int rc;
    if ((rc = d_word.alloc(2 * sizeof(unsigned long long)))) return rc;
    if ((rc = launch_sc_build(row_dev, col_dev, nnz, G, C, d_word.as<unsigned long long>(), nullptr, false, s))) return rc;
    unsigned long long word[2] = {0, 0};
    ICNV_HIP(hipMemcpyAsync(word, d_word.p, sizeof word, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (word[1] != SC_NO_VIOLATION)
        ICNV_FAIL(ICNV_ERR_ARG, "csc_from_sorted_triplets: entry " + std::to_string(word[1]) + " lies outside the matrix");
    if (word[0] != SC_NO_VIOLATION) {
        *first_violation = (int64_t)(word[0] >> 2);
        *violation_kind = (word[0] & 3) == 1 ? ICNV_CSC_DUPLICATE : ICNV_CSC_DESCENT;
        return ICNV_OK;
    }
    if ((rc = launch_sc_build(row_dev, col_dev, nnz, G, C, nullptr, colptr_dev, true, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));
    return ICNV_OK;
}

int icnv_csc_select_dev(const icnv_counts *cnt, int64_t G, int64_t C, const int32_t *gene_map_dev, int64_t n_genes_out, const int32_t *cells_dev,
                        int64_t n_cells, int64_t *colptr_out, int32_t *rowidx_out, int32_t *vals_out, int64_t capacity, int64_t *nnz_out,
                        void *stream) {
    if (!cnt || !gene_map_dev || !cells_dev || !colptr_out || !nnz_out) ICNV_FAIL(ICNV_ERR_ARG, "csc_select: null argument");
    if (cnt->dense || !cnt->colptr) ICNV_FAIL(ICNV_ERR_ARG, "csc_select: the counts must be in CSC form");
    if (cnt->nnz < 0 || (cnt->nnz > 0 && (!cnt->rowidx || !cnt->vals))) ICNV_FAIL(ICNV_ERR_ARG, "csc_select: CSC row indices / values missing");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "csc_select: G and C must be 1 .. 2^31 - 1");
    if (n_genes_out < 0 || n_genes_out > 0x7fffffff || n_cells < 1 || n_cells > 0x7fffffff)
        ICNV_FAIL(ICNV_ERR_ARG, "csc_select: n_genes_out must be 0 .. 2^31 - 1 and n_cells 1 .. 2^31 - 1");
    const bool fill = rowidx_out != nullptr;
    if (fill && (!vals_out || capacity < 0)) ICNV_FAIL(ICNV_ERR_ARG, "csc_select: rowidx_out comes with vals_out and a capacity");
    hipStream_t s = (hipStream_t)stream;
    int rc;

    ScSelectArgs a{};
    a.colptr = cnt->colptr; a.rowidx = cnt->rowidx; a.vals = cnt->vals; a.G = G; a.C = C; a.nnz = cnt->nnz;
    a.gene_map = gene_map_dev; a.n_genes_out = n_genes_out; a.cells = cells_dev; a.n_cells = n_cells;
    const int64_t n_tiles = (n_cells + SC_SCAN_TILE - 1) / SC_SCAN_TILE;
    DevBuf d_counts, d_tiles, d_word, d_colptr;
    if ((rc = d_counts.alloc((size_t)n_cells * sizeof(int64_t))) || (rc = d_tiles.alloc((size_t)n_tiles * sizeof(int64_t))) ||
        (rc = d_word.alloc(sizeof(unsigned long long))) || (rc = d_colptr.alloc((size_t)(n_cells + 1) * sizeof(int64_t))))
        return rc;
    a.counts = d_counts.as<int64_t>(); a.tile_sum = d_tiles.as<int64_t>(); a.error = d_word.as<unsigned long long>();
    a.colptr_out = d_colptr.as<int64_t>();                              // staged: the caller's arrays are written when nothing is refused
    a.rowidx_out = rowidx_out; a.vals_out = vals_out;
    const unsigned long long none = SC_NO_ERROR;
    ICNV_HIP(hipMemcpyAsync(d_word.p, &none, sizeof none, hipMemcpyHostToDevice, s));
    if ((rc = launch_sc_check_maps(a, s))) return rc;
    unsigned long long word = 0;
    ICNV_HIP(hipMemcpyAsync(&word, d_word.p, sizeof word, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (word != SC_NO_ERROR) {
        const std::string at = std::to_string(word >> 8);
        if ((word & 0xff) == SC_E_CELL) ICNV_FAIL(ICNV_ERR_ARG, "csc_select: entry " + at + " of the cell list is not a column of the matrix");
        ICNV_FAIL(ICNV_ERR_ARG, "csc_select: entry " + at + " of the gene map is outside -1 .. n_genes_out - 1");
    }
    if ((rc = launch_sc_select_count(a, s))) return rc;
    int64_t total = 0;
    ICNV_HIP(hipMemcpyAsync(&total, a.colptr_out + n_cells, sizeof total, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (fill && capacity < total)
        ICNV_FAIL(ICNV_ERR_ARG, "csc_select: " + std::to_string(total) + " entries are kept, capacity is " + std::to_string(capacity));
    if (fill && total > 0 && (rc = launch_sc_select_fill(a, s))) return rc;
    ICNV_HIP(hipMemcpyAsync(colptr_out, a.colptr_out, (size_t)(n_cells + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    ICNV_HIP(hipStreamSynchronize(s));                                  // the scratch goes back to the pool
    *nnz_out = total;
    return ICNV_OK;
}

}  // extern "C"
