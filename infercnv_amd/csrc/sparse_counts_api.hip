// C ABI of K22 (include/icnv.h "sparse count matrices") and of the sparse half of K26 ("reading a selection of columns"):
// validation, the order of the passes, the text of a refusal.  The plain and the column-selected triplet entry share the half
// that stages a chunk's entries.  Kernels: sparse_counts_kernels.hip, triplets_cols_kernels.hip; the map check is
// table_cols_kernels.hip's.  DESIGN.md section 4 K22, K26.
#include <cstdint>
#include <string>

#include "icnv_internal.h"
#include "col_map_internal.h"
#include "sparse_counts_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

namespace {

// What the two triplet entries check alike, after each one's own null-argument check.
int sc_validate(const uint8_t *text_dev, int64_t n_bytes, int32_t field, int64_t n_rows, int64_t n_cols, int64_t line0, const int32_t *row_dev,
                const int32_t *col_dev, const int32_t *val_dev, int64_t capacity) {
    if (n_bytes < 1 || n_bytes > 0x7ffffffe) ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: a chunk has 1 .. 2^31 - 2 bytes");
    if (reinterpret_cast<uintptr_t>(text_dev) & 15) ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: the device text must start on a 16-byte boundary");
    if (field != ICNV_MM_INTEGER && field != ICNV_MM_REAL && field != ICNV_MM_PATTERN)
        ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: field must be ICNV_MM_INTEGER, ICNV_MM_REAL or ICNV_MM_PATTERN");
    if (n_rows < 1 || n_rows > 0x7fffffff || n_cols < 1 || n_cols > 0x7fffffff)
        ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: n_rows and n_cols must be 1 .. 2^31 - 1");
    if (line0 < 1) ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: line0 counts from 1");
    if (capacity < 0 || (capacity > 0 && (!row_dev || !col_dev || !val_dev)))
        ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: capacity must be >= 0 and the output arrays must be given");
    return ICNV_OK;
}

struct ScStaged {                          // the entries of a chunk as sc_stage leaves them; the buffers live as long as it does
    ScParseArgs a{};                       // n_entries; row | col | val staged; total: a device word the caller may reuse
    DevBuf d_seg, d_small, d_pos, d_stage;
};

// The half the two entries share: the structure, index and parse passes over every entry of the chunk, into staged arrays, and
// the text of a refusal.  st.a.n_entries == 0 (blank lines only): nothing else of st is set.  A chunk with more than
// max_entries entries is refused before the index pass (the plain entry's capacity).
int sc_stage(const uint8_t *text_dev, const uint8_t *text_host, int64_t n_bytes, int32_t field, int64_t n_rows, int64_t n_cols, int64_t line0,
             int64_t max_entries, ScStaged &st, hipStream_t s) {
    int rc;
    ScParseArgs &a = st.a;
    a.text = text_dev; a.n = n_bytes; a.field = field; a.G = n_rows; a.C = n_cols;
    a.n_seg = (n_bytes + SC_SEG - 1) / SC_SEG;
    if ((rc = st.d_seg.alloc((size_t)a.n_seg * 2 * sizeof(uint32_t))) || (rc = st.d_small.alloc(2 * sizeof(uint64_t)))) return rc;
    a.seg_count = st.d_seg.as<uint32_t>(); a.seg_off = a.seg_count + a.n_seg;
    a.error = st.d_small.as<unsigned long long>();                    // word 0: the error; word 1: the total (K26: then the kept total)
    a.total = reinterpret_cast<uint32_t *>(a.error + 1);
    const uint64_t init[2] = {SC_NO_ERROR, 0};
    ICNV_HIP(hipMemcpyAsync(st.d_small.p, init, sizeof init, hipMemcpyHostToDevice, s));

    // structure: how many entries
    if ((rc = launch_sc_structure(a, s))) return rc;
    uint32_t total = 0;
    ICNV_HIP(hipMemcpyAsync(&total, a.total, sizeof total, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    a.n_entries = total;
    if (a.n_entries > max_entries)
        ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: the chunk has " + std::to_string(a.n_entries) + " entries, capacity is " + std::to_string(max_entries));
    if (a.n_entries == 0) return ICNV_OK;                               // blank lines only

    // index, parse: every entry of the chunk, into staged arrays; the caller's arrays are written only when nothing was refused
    if ((rc = st.d_pos.alloc((size_t)a.n_entries * sizeof(uint32_t))) || (rc = st.d_stage.alloc((size_t)a.n_entries * 3 * sizeof(int32_t)))) return rc;
    a.line_pos = st.d_pos.as<uint32_t>();
    a.row = st.d_stage.as<int32_t>(); a.col = a.row + a.n_entries; a.val = a.col + a.n_entries;
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
    return ICNV_OK;
}

}  // namespace

extern "C" {

int icnv_parse_triplets_dev(const uint8_t *text_dev, const uint8_t *text_host, int64_t n_bytes, int32_t field, int64_t n_rows, int64_t n_cols,
                            int64_t line0, int32_t *row_dev, int32_t *col_dev, int32_t *val_dev, int64_t capacity, int64_t *n_entries,
                            void *stream) {
    if (!text_dev || !n_entries) ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: null argument");
    int rc;
    if ((rc = sc_validate(text_dev, n_bytes, field, n_rows, n_cols, line0, row_dev, col_dev, val_dev, capacity))) return rc;
    hipStream_t s = (hipStream_t)stream;
    ScStaged st;
    if ((rc = sc_stage(text_dev, text_host, n_bytes, field, n_rows, n_cols, line0, capacity, st, s))) return rc;
    const ScParseArgs &a = st.a;
    if (a.n_entries == 0) {                                             // blank lines only
        *n_entries = 0;
        return ICNV_OK;
    }
    const size_t bytes = (size_t)a.n_entries * sizeof(int32_t);
    ICNV_HIP(hipMemcpyAsync(row_dev, a.row, bytes, hipMemcpyDeviceToDevice, s));
    ICNV_HIP(hipMemcpyAsync(col_dev, a.col, bytes, hipMemcpyDeviceToDevice, s));
    ICNV_HIP(hipMemcpyAsync(val_dev, a.val, bytes, hipMemcpyDeviceToDevice, s));
    ICNV_HIP(hipStreamSynchronize(s));                                  // the staged arrays go back to the pool
    *n_entries = a.n_entries;
    return ICNV_OK;
}

// K26: every entry is parsed and validated as above; the kept ones are compacted in file order (triplets_cols_kernels.hip)
int icnv_parse_triplets_cols_dev(const uint8_t *text_dev, const uint8_t *text_host, int64_t n_bytes, int32_t field, int64_t n_rows, int64_t n_cols,
                                 int64_t line0, int32_t *row_dev, int32_t *col_dev, int32_t *val_dev, int64_t capacity, int64_t *n_entries,
                                 const int32_t *col_map_dev, int64_t n_cols_out, int64_t *n_seen, void *stream) {
    if (!text_dev || !n_entries || !col_map_dev || !n_seen) ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: null argument");
    int rc;
    if ((rc = sc_validate(text_dev, n_bytes, field, n_rows, n_cols, line0, row_dev, col_dev, val_dev, capacity))) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = check_col_map(col_map_dev, n_cols, n_cols_out, "parse_triplets_cols", s))) return rc;
    ScStaged st;                                                        // no limit here: the capacity is for the kept entries
    if ((rc = sc_stage(text_dev, text_host, n_bytes, field, n_rows, n_cols, line0, INT64_MAX, st, s))) return rc;
    const ScParseArgs &a = st.a;
    if (a.n_entries == 0) {                                             // blank lines only
        *n_entries = 0;
        *n_seen = 0;
        return ICNV_OK;
    }

    // the kept entries, in file order; the caller's arrays are written only when they hold them all
    ScKeepArgs k{};
    k.row = a.row; k.col = a.col; k.val = a.val; k.n_entries = a.n_entries; k.col_map = col_map_dev; k.C = n_cols;
    const int64_t n_blocks = (a.n_entries + SC_KEEP_TILE - 1) / SC_KEEP_TILE;
    DevBuf d_blocks;
    if ((rc = d_blocks.alloc((size_t)n_blocks * 2 * sizeof(uint32_t)))) return rc;
    k.block_count = d_blocks.as<uint32_t>(); k.block_off = k.block_count + n_blocks;
    k.total = a.total;
    k.row_out = row_dev; k.col_out = col_dev; k.val_out = val_dev;
    if ((rc = launch_sc_keep_count(k, s))) return rc;
    uint32_t kept = 0;
    ICNV_HIP(hipMemcpyAsync(&kept, k.total, sizeof kept, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if ((int64_t)kept > capacity)
        ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets_cols: " + std::to_string(kept) + " entries are kept, capacity is " + std::to_string(capacity));
    if (kept && (rc = launch_sc_keep_fill(k, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));                                  // the staged arrays go back to the pool
    *n_entries = kept;
    *n_seen = a.n_entries;
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
