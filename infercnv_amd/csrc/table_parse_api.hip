// C ABI of K21 (include/icnv.h "count matrices from text") and of the dense half of K26 ("reading a selection of columns"):
// validation, the order of the passes over a chunk of whole lines, strtod for the fields the parse pass does not certify, the
// text of a refusal -- one driver for the plain and the column-selected entry; and the matrix gather of CreateInfercnvObject.
// Kernels: table_parse_kernels.hip, table_cols_kernels.hip.  DESIGN.md section 4 K21, K26.
#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <vector>

#include "icnv_internal.h"
#include "col_map_internal.h"
#include "table_parse_host.h"
#include "table_parse_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

namespace {

std::atomic<int64_t> g_tp[7];   // calls, rows, fields, fields parsed on the host, bytes, collect rounds, wall microseconds

int tp_validate(const void *text_dev, const uint8_t *text_host, int64_t n_bytes, const char *sep, int64_t n_cols, int64_t line0,
                const void *out, int64_t ld, int64_t row0, int64_t max_rows, const int64_t *label_ranges, const int64_t *n_rows) {
    if (!text_dev || !sep || !out || !label_ranges || !n_rows) ICNV_FAIL(ICNV_ERR_ARG, "parse_table: null argument");
    if (n_bytes < 1 || n_bytes > 0x7ffffffe) ICNV_FAIL(ICNV_ERR_ARG, "parse_table: a chunk has 1 .. 2^31 - 2 bytes");
    if (std::strlen(sep) != 1 || sep[0] == '\n' || sep[0] == '\r' || sep[0] == '"')
        ICNV_FAIL(ICNV_ERR_ARG, "parse_table: sep must be one byte other than a line end or a quote");
    if (n_cols < 1 || n_cols > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "parse_table: n_cols must be 1 .. 2^31 - 1");
    if (line0 < 1) ICNV_FAIL(ICNV_ERR_ARG, "parse_table: line0 counts from 1");
    if (row0 < 0 || max_rows < 1 || ld < 1 || row0 > ld - max_rows) ICNV_FAIL(ICNV_ERR_ARG, "parse_table: rows row0 .. row0 + max_rows - 1 must lie below ld");
    return ICNV_OK;
}

int tp_refused(const uint8_t *text_host, int64_t n, uint64_t word, uint8_t sep, int64_t line0, int64_t n_cols) {
    ICNV_FAIL(ICNV_ERR_ARG, "parse_table: " + tp_describe(text_host, n, (int64_t)(word >> 8), (int)(word & 0xff), sep, line0, n_cols));
}

// The arguments of the two device entries: tp_validate and the alignment of the device text.
int tp_check_dev(const void *text_dev, const uint8_t *text_host, int64_t n_bytes, const char *sep, int64_t n_cols, int64_t line0, const void *out,
                 int64_t ld, int64_t row0, int64_t max_rows, const int64_t *label_ranges, const int64_t *n_rows) {
    int rc;
    if ((rc = tp_validate(text_dev, text_host, n_bytes, sep, n_cols, line0, out, ld, row0, max_rows, label_ranges, n_rows))) return rc;
    if (reinterpret_cast<uintptr_t>(text_dev) & 15) ICNV_FAIL(ICNV_ERR_ARG, "parse_table: the device text must start on a 16-byte boundary");
    return ICNV_OK;
}

// The driver of icnv_parse_table_dev (col_map null; n_cols_out unused) and of icnv_parse_table_cols_dev (K26: the staged values
// are n_cols_out wide and only the selected fields are indexed, parsed and collected).  The arguments are checked by the entry.
int tp_parse_chunk(const uint8_t *text_dev, const uint8_t *text_host, int64_t n_bytes, const char *sep, int64_t n_cols, int64_t line0, double *out,
                   int64_t ld, int64_t row0, int64_t max_rows, int64_t *label_ranges, int64_t *n_rows, const int32_t *col_map, int64_t n_cols_out,
                   void *stream) {
    int rc;
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = (hipStream_t)stream;
    if (col_map && (rc = check_col_map(col_map, n_cols, n_cols_out, "parse_table_cols", s))) return rc;

    TcArgs t{};                                                         // t.tp is all the plain entry uses
    TpArgs &a = t.tp;
    t.col_map = col_map; t.n_cols_out = n_cols_out;
    a.text = text_dev; a.n = n_bytes; a.sep = (uint8_t)sep[0]; a.n_cols = n_cols;
    a.n_seg = (n_bytes + 1 + TP_SEG - 1) / TP_SEG;
    a.out = out; a.ld = ld; a.row0 = row0;
    DevBuf d_seg, d_small;
    if ((rc = d_seg.alloc((size_t)a.n_seg * 3 * sizeof(uint32_t))) || (rc = d_small.alloc(4 * sizeof(uint64_t)))) return rc;
    a.seg_count = d_seg.as<uint32_t>(); a.seg_row_off = a.seg_count + a.n_seg; a.seg_field_off = a.seg_row_off + a.n_seg;
    a.error = d_small.as<unsigned long long>();                       // word 0: the error; word 1: n_flagged; word 2: totals
    a.n_flagged = reinterpret_cast<uint32_t *>(a.error + 1);
    a.totals = reinterpret_cast<uint32_t *>(a.error + 2);
    const uint64_t init[4] = {TP_NO_ERROR, 0, 0, 0};
    ICNV_HIP(hipMemcpyAsync(d_small.p, init, sizeof init, hipMemcpyHostToDevice, s));

    // structure: how many rows and fields, over the whole chunk
    if ((rc = launch_tp_structure(a, s))) return rc;
    uint32_t totals[2] = {0, 0};
    ICNV_HIP(hipMemcpyAsync(totals, a.totals, sizeof totals, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    a.n_rows = totals[0]; a.n_fields = totals[1];
    if (a.n_rows > max_rows)
        ICNV_FAIL(ICNV_ERR_ARG, "parse_table: the chunk has " + std::to_string(a.n_rows) + " rows, max_rows is " + std::to_string(max_rows));
    if (a.n_rows == 0) {                                                // blank lines only
        *n_rows = 0;
        g_tp[0] += 1; g_tp[4] += n_bytes;
        g_tp[6] += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
        return ICNV_OK;
    }
    const int64_t n_vals = a.n_rows * (col_map ? n_cols_out : n_cols);

    // index, rows, parse: the list of all fields, or (K26) only the positions of the selected ones
    DevBuf d_row, d_vals, d_flag, d_field, d_sel;
    if ((rc = d_row.alloc((size_t)a.n_rows * 4 * sizeof(uint32_t))) || (rc = d_vals.alloc((size_t)n_vals * sizeof(uint64_t))) ||
        (rc = d_flag.alloc((size_t)TP_FLAG_CAP * sizeof(TpFlagged))))
        return rc;
    a.row_pos = d_row.as<uint32_t>(); a.row_field0 = a.row_pos + a.n_rows;
    a.label_range = reinterpret_cast<int32_t *>(a.row_field0 + a.n_rows);
    a.vals = d_vals.as<uint64_t>(); a.flagged = d_flag.as<TpFlagged>();
    if (col_map) {
        if ((rc = d_sel.alloc((size_t)n_vals * sizeof(uint32_t)))) return rc;
        t.sel_pos = d_sel.as<uint32_t>();
        if ((rc = launch_tc_index(t, s)) || (rc = launch_tc_parse(t, s))) return rc;
    } else {
        if ((rc = d_field.alloc((size_t)a.n_fields * 2 * sizeof(uint32_t)))) return rc;
        a.field_pos = d_field.as<uint32_t>(); a.field_row = a.field_pos + a.n_fields;
        if ((rc = launch_tp_index(a, s)) || (rc = launch_tp_parse(a, s))) return rc;
    }

    // the fields the parse pass did not certify, at most TP_FLAG_CAP per round: strtod here, the staged value replaced
    int64_t n_host = 0, rounds = 0;
    HostText host{text_host, text_dev, n_bytes, s, {}};
    for (;;) {
        uint64_t words[2] = {0, 0};                                    // the error word, n_flagged
        ICNV_HIP(hipMemcpyAsync(words, a.error, sizeof words, hipMemcpyDeviceToHost, s));
        ICNV_HIP(hipStreamSynchronize(s));
        const uint32_t count = (uint32_t)words[1];
        if (!count && words[0] == TP_NO_ERROR) break;
        const size_t n = count < (uint32_t)TP_FLAG_CAP ? count : (size_t)TP_FLAG_CAP;
        std::vector<TpFlagged> fl(n);
        if (n) {
            ICNV_HIP(hipMemcpyAsync(fl.data(), a.flagged, n * sizeof(TpFlagged), hipMemcpyDeviceToHost, s));
            ICNV_HIP(hipStreamSynchronize(s));
        }
        std::vector<int64_t> slot(n);
        std::vector<uint64_t> bits(n);
        uint64_t worst = words[0];                                     // the device's refusal, if any: the smallest offset wins
        const uint8_t *text = nullptr;                                 // a flagged field or a refusal: the host copy is needed
        if ((rc = host.get(text))) return rc;
        for (size_t i = 0; i < n; ++i) {
            if (fl[i].slot < 0 || fl[i].slot >= n_vals || fl[i].pos < 0 || fl[i].pos > n_bytes)
                ICNV_FAIL(ICNV_ERR_HIP, std::string(col_map ? "parse_table_cols" : "parse_table") + ": a flagged field lies outside the chunk (internal error)");
            slot[i] = fl[i].slot;
            if (tp_host_field(text, n_bytes, fl[i].pos, a.sep, bits[i]) != TP_VALUE) {
                const uint64_t word = ((uint64_t)fl[i].pos << 8) | (uint64_t)TP_E_NUMBER;
                if (word < worst) worst = word;
            }
        }
        if (worst != TP_NO_ERROR) return tp_refused(text, n_bytes, worst, a.sep, line0, n_cols);
        DevBuf d_slot, d_bits;
        if ((rc = upload(d_slot, slot.data(), n, s)) || (rc = upload(d_bits, bits.data(), n, s)) ||
            (rc = launch_tp_patch(a, d_slot.as<int64_t>(), d_bits.as<uint64_t>(), (int32_t)n, s)))
            return rc;
        n_host += (int64_t)n;
        ICNV_HIP(hipMemsetAsync(a.n_flagged, 0, sizeof(uint64_t), s));
        if (count > (uint32_t)TP_FLAG_CAP) {                          // some were counted but not listed: look for what is still pending
            ++rounds;
            if ((rc = col_map ? launch_tc_collect(t, s) : launch_tp_collect(a, s))) return rc;
        }
        ICNV_HIP(hipStreamSynchronize(s));                              // the uploads' pool blocks outlive the patch
    }

    // every value is known and nothing was refused: only now is the matrix written, by the transpose of a table that is as wide
    // as the staged values
    std::vector<int32_t> ranges((size_t)a.n_rows * 2);
    TpArgs staged = a;
    if (col_map) staged.n_cols = n_cols_out;
    if ((rc = launch_tp_transpose(staged, s))) return rc;
    ICNV_HIP(hipMemcpyAsync(ranges.data(), a.label_range, ranges.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    for (int64_t r = 0; r < a.n_rows; ++r) {
        int64_t b = ranges[(size_t)(2 * r)], e = ranges[(size_t)(2 * r + 1)];
        if (text_host) tp_label_slice(text_host, b, e);                // (no host copy: the caller slices the labels it fetches)
        label_ranges[2 * r] = b;
        label_ranges[2 * r + 1] = e;
    }
    *n_rows = a.n_rows;
    g_tp[0] += 1; g_tp[1] += a.n_rows; g_tp[2] += n_vals; g_tp[3] += n_host; g_tp[4] += n_bytes; g_tp[5] += rounds;
    g_tp[6] += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return ICNV_OK;
}

}  // namespace

extern "C" {

int icnv_parse_table_dev(const uint8_t *text_dev, const uint8_t *text_host, int64_t n_bytes, const char *sep, int64_t n_cols, int64_t line0,
                         double *out, int64_t ld, int64_t row0, int64_t max_rows, int64_t *label_ranges, int64_t *n_rows, void *stream) {
    int rc;
    if ((rc = tp_check_dev(text_dev, text_host, n_bytes, sep, n_cols, line0, out, ld, row0, max_rows, label_ranges, n_rows))) return rc;
    return tp_parse_chunk(text_dev, text_host, n_bytes, sep, n_cols, line0, out, ld, row0, max_rows, label_ranges, n_rows, nullptr, 0, stream);
}

int icnv_parse_table_cols_dev(const uint8_t *text_dev, const uint8_t *text_host, int64_t n_bytes, const char *sep, int64_t n_cols, int64_t line0,
                              double *out, int64_t ld, int64_t row0, int64_t max_rows, int64_t *label_ranges, int64_t *n_rows,
                              const int32_t *col_map_dev, int64_t n_cols_out, void *stream) {
    int rc;
    if ((rc = tp_check_dev(text_dev, text_host, n_bytes, sep, n_cols, line0, out, ld, row0, max_rows, label_ranges, n_rows))) return rc;
    if (!col_map_dev) ICNV_FAIL(ICNV_ERR_ARG, "parse_table_cols: null column map");
    return tp_parse_chunk(text_dev, text_host, n_bytes, sep, n_cols, line0, out, ld, row0, max_rows, label_ranges, n_rows, col_map_dev, n_cols_out,
                          stream);
}

int icnv_parse_table(const uint8_t *text, int64_t n_bytes, const char *sep, int64_t n_cols, int64_t line0, double *out, int64_t ld,
                     int64_t row0, int64_t max_rows, int64_t *label_ranges, int64_t *n_rows) {
    int rc;
    if ((rc = tp_validate(text, text, n_bytes, sep, n_cols, line0, out, ld, row0, max_rows, label_ranges, n_rows))) return rc;
    DevBuf d_text, d_out;
    if ((rc = d_text.alloc((size_t)n_bytes)) || (rc = d_out.alloc((size_t)(n_cols * max_rows) * sizeof(double)))) return rc;
    ICNV_HIP(hipMemcpy(d_text.p, text, (size_t)n_bytes, hipMemcpyHostToDevice));
    int64_t rows = 0;
    if ((rc = icnv_parse_table_dev(d_text.as<uint8_t>(), text, n_bytes, sep, n_cols, line0, d_out.as<double>(), max_rows, 0, max_rows,
                                   label_ranges, &rows, nullptr)))
        return rc;
    if (rows) {
        std::vector<double> tmp((size_t)(n_cols * max_rows));
        ICNV_HIP(hipMemcpy(tmp.data(), d_out.p, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (int64_t c = 0; c < n_cols; ++c) std::memcpy(out + c * ld + row0, tmp.data() + c * max_rows, (size_t)rows * sizeof(double));
    }
    *n_rows = rows;
    return ICNV_OK;
}

int icnv_table_parse_stats(int64_t *out, int32_t n) {
    if (!out || n < 1) ICNV_FAIL(ICNV_ERR_ARG, "bad argument");
    for (int i = 0; i < n && i < 7; ++i) out[i] = g_tp[i].load();
    return ICNV_OK;
}

void icnv_table_parse_stats_reset(void) {
    for (auto &c : g_tp) c.store(0);
}

int icnv_gather_matrix_dev(const double *in, int64_t ld_in, int64_t G_in, int64_t C_in, const int32_t *genes, int64_t n_genes,
                           const int32_t *cells, int64_t n_cells, double *out, int64_t ld_out, void *stream) {
    if (!in || !out) ICNV_FAIL(ICNV_ERR_ARG, "gather_matrix: null argument");
    if (G_in < 1 || G_in > 0x7fffffff || C_in < 1 || C_in > 0x7fffffff || ld_in < G_in) ICNV_FAIL(ICNV_ERR_ARG, "gather_matrix: bad matrix dimensions");
    if (!genes) n_genes = G_in;
    if (!cells) n_cells = C_in;
    if (n_genes < 1 || n_genes > 0x7fffffff || n_cells < 1 || n_cells > 0x7fffffff || ld_out < n_genes)
        ICNV_FAIL(ICNV_ERR_ARG, "gather_matrix: the lists must have 1 .. 2^31 - 1 entries and ld_out must hold a gene list");
    for (int64_t i = 0; genes && i < n_genes; ++i)
        if (genes[i] < 0 || genes[i] >= G_in) ICNV_FAIL(ICNV_ERR_ARG, "gather_matrix: entry " + std::to_string(i) + " of the gene list is not a gene");
    for (int64_t j = 0; cells && j < n_cells; ++j)
        if (cells[j] < 0 || cells[j] >= C_in) ICNV_FAIL(ICNV_ERR_ARG, "gather_matrix: entry " + std::to_string(j) + " of the cell list is not a cell");
    hipStream_t s = (hipStream_t)stream;
    DevBuf d_genes, d_cells;
    int rc;
    if (genes && (rc = upload(d_genes, genes, (size_t)n_genes, s))) return rc;
    if (cells && (rc = upload(d_cells, cells, (size_t)n_cells, s))) return rc;
    if ((rc = launch_gather_matrix(in, ld_in, genes ? d_genes.as<int32_t>() : nullptr, n_genes, cells ? d_cells.as<int32_t>() : nullptr, n_cells,
                                   out, ld_out, s)))
        return rc;
    ICNV_HIP(hipStreamSynchronize(s));                                  // the lists' pool blocks outlive the launch
    return ICNV_OK;
}

}  // extern "C"
