// C ABI of the sparse half of K26 (include/icnv.h "reading a selection of columns"): icnv_parse_triplets_cols_dev.  Every entry
// is parsed and validated by K22's passes, with K22's refusal text; the kept ones are compacted in file order.
// Kernels: sparse_counts_kernels.hip, triplets_cols_kernels.hip; the map check is table_cols_kernels.hip's.  DESIGN.md section 4 K26.
#include <string>

#include "icnv_internal.h"
#include "col_map_internal.h"
#include "sparse_counts_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

extern "C" {

int icnv_parse_triplets_cols_dev(const uint8_t *text_dev, const uint8_t *text_host, int64_t n_bytes, int32_t field, int64_t n_rows, int64_t n_cols,
                                 int64_t line0, int32_t *row_dev, int32_t *col_dev, int32_t *val_dev, int64_t capacity, int64_t *n_entries,
                                 const int32_t *col_map_dev, int64_t n_cols_out, int64_t *n_seen, void *stream) {
    if (!text_dev || !n_entries || !col_map_dev || !n_seen) ICNV_FAIL(ICNV_ERR_ARG, "parse_triplets: null argument");
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
    if ((rc = check_col_map(col_map_dev, n_cols, n_cols_out, "parse_triplets_cols", s))) return rc;

    ScParseArgs a{};
    a.text = text_dev; a.n = n_bytes; a.field = field; a.G = n_rows; a.C = n_cols;
    a.n_seg = (n_bytes + SC_SEG - 1) / SC_SEG;
    DevBuf d_seg, d_small;
    if ((rc = d_seg.alloc((size_t)a.n_seg * 2 * sizeof(uint32_t))) || (rc = d_small.alloc(2 * sizeof(uint64_t)))) return rc;
    a.seg_count = d_seg.as<uint32_t>(); a.seg_off = a.seg_count + a.n_seg;
    a.error = d_small.as<unsigned long long>();                       // word 0: the error; word 1: the total, then the kept total
    a.total = reinterpret_cast<uint32_t *>(a.error + 1);
    const uint64_t init[2] = {SC_NO_ERROR, 0};
    ICNV_HIP(hipMemcpyAsync(d_small.p, init, sizeof init, hipMemcpyHostToDevice, s));

    // structure: how many entries
    if ((rc = launch_sc_structure(a, s))) return rc;
    uint32_t total = 0;
    ICNV_HIP(hipMemcpyAsync(&total, a.total, sizeof total, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    a.n_entries = total;
    if (a.n_entries == 0) {                                             // blank lines only
        *n_entries = 0;
        *n_seen = 0;
        return ICNV_OK;
    }

    // index, parse: every entry of the chunk, into staged arrays
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

}  // extern "C"
