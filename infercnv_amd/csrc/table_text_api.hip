// C ABI of K20 (include/icnv.h "matrix files of plot_cnv"): validation, the plan of a chunk of whole rows, the host
// formatting of the elements the digits pass could not certify, the scan of the row byte counts.
// Kernels: table_text_kernels.hip.  DESIGN.md section 4 K20.
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "icnv_internal.h"
#include "table_text_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

namespace {

std::atomic<int64_t> g_tt[7];   // calls, rows, elements, elements formatted on the host, bytes, collect rounds, wall microseconds

struct TtPlan {
    int64_t n_total_rows, n_fields;
};

// Everything that can be refused before a launch.
int tt_validate(const double *x, int64_t ld, int64_t G, int64_t C, int32_t orientation, int64_t row0, int64_t n_rows,
                const int32_t *cells, int64_t n_cells, const uint8_t *labels, const int64_t *label_off, const char *sep,
                const void *out, int64_t capacity, const int64_t *rows_done, const int64_t *n_bytes, TtPlan &p) {
    if (!x || !cells || !sep || !out || !rows_done || !n_bytes) ICNV_FAIL(ICNV_ERR_ARG, "format_table: null argument");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff || ld < G) ICNV_FAIL(ICNV_ERR_ARG, "format_table: bad matrix dimensions");
    if (orientation != TT_GENE_ROWS && orientation != TT_CELL_ROWS) ICNV_FAIL(ICNV_ERR_ARG, "format_table: unknown orientation");
    if (n_cells < 1 || n_cells > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "format_table: the cell list must have 1 .. 2^31 - 1 entries");
    for (int64_t i = 0; i < n_cells; ++i)
        if (cells[i] < 0 || cells[i] >= C) ICNV_FAIL(ICNV_ERR_ARG, "format_table: entry " + std::to_string(i) + " of the cell list is not a cell");
    p.n_total_rows = orientation == TT_GENE_ROWS ? G : n_cells;
    p.n_fields = orientation == TT_GENE_ROWS ? n_cells : G;
    if (row0 < 0 || n_rows < 1 || row0 > p.n_total_rows - n_rows) ICNV_FAIL(ICNV_ERR_ARG, "format_table: the row range is empty or leaves the table");
    if (std::strlen(sep) != 1) ICNV_FAIL(ICNV_ERR_ARG, "format_table: sep must be one byte");
    if (!label_off && labels) ICNV_FAIL(ICNV_ERR_ARG, "format_table: label bytes without label offsets");
    if (label_off) {
        if (label_off[0] != 0) ICNV_FAIL(ICNV_ERR_ARG, "format_table: the label offsets must start at 0");
        for (int64_t i = 0; i < n_rows; ++i)
            if (label_off[i + 1] < label_off[i]) ICNV_FAIL(ICNV_ERR_ARG, "format_table: the label offsets must not descend");
        if (label_off[n_rows] > 0 && !labels) ICNV_FAIL(ICNV_ERR_ARG, "format_table: label offsets without label bytes");
    }
    const int64_t least = (label_off ? label_off[1] + 1 : 0) + 2 * p.n_fields;   // one-byte fields
    if (capacity < least) ICNV_FAIL(ICNV_ERR_ARG, "format_table: the capacity is below the shortest possible row");
    return ICNV_OK;
}

}  // namespace

extern "C" {

int icnv_format_table_dev(const double *x, int64_t ld, int64_t G, int64_t C, int32_t orientation, int64_t row0, int64_t n_rows,
                          const int32_t *cells, int64_t n_cells, const uint8_t *labels, const int64_t *label_off, const char *sep,
                          uint8_t *out, int64_t capacity, int64_t *row_offsets, int64_t *rows_done, int64_t *n_bytes, void *stream) {
    TtPlan p{};
    int rc;
    if ((rc = tt_validate(x, ld, G, C, orientation, row0, n_rows, cells, n_cells, labels, label_off, sep, out, capacity, rows_done,
                          n_bytes, p)))
        return rc;
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = (hipStream_t)stream;
    const int64_t nf = p.n_fields;

    // rows to attempt: as many as fit when every field takes its 22 bytes (at least one)
    int64_t R = 0, worst = 0;
    for (; R < n_rows; ++R) {
        worst += (label_off ? label_off[R + 1] - label_off[R] + 1 : 0) + nf * (TT_MAX_FIELD + 1);
        if (worst > capacity) break;
    }
    if (R < 1) R = 1;
    const int64_t n_elem = R * nf;
    if (n_elem > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "format_table: more than 2^31 - 1 elements in one chunk");

    TtArgs a{};
    a.x = x; a.ld = ld; a.orientation = orientation; a.row0 = row0; a.n_rows = R; a.n_fields = nf;
    a.n_seg = (nf + TT_SEG - 1) / TT_SEG;
    a.sep = (uint8_t)sep[0];
    DevBuf d_cells, d_rec, d_meta, d_flag, d_seg_sum, d_seg_off, d_row_bytes, d_row_off, d_lab_off, d_lab;
    const int32_t *cell_src = orientation == TT_GENE_ROWS ? cells : cells + row0;
    const size_t n_cell_up = orientation == TT_GENE_ROWS ? (size_t)n_cells : (size_t)R;
    if ((rc = upload(d_cells, cell_src, n_cell_up, s)) || (rc = d_rec.alloc((size_t)n_elem * sizeof(uint64_t))) ||
        (rc = d_meta.alloc((size_t)n_elem * sizeof(uint16_t))) ||
        (rc = d_flag.alloc((size_t)TT_FLAG_CAP * sizeof(TtFlagged) + sizeof(uint64_t))) ||
        (rc = d_seg_sum.alloc((size_t)(R * a.n_seg) * sizeof(uint32_t))) || (rc = d_seg_off.alloc((size_t)(R * a.n_seg) * sizeof(int64_t))) ||
        (rc = d_row_bytes.alloc((size_t)R * sizeof(int64_t))) || (rc = d_row_off.alloc((size_t)(R + 1) * sizeof(int64_t))))
        return rc;
    if (label_off && ((rc = upload(d_lab_off, label_off, (size_t)R + 1, s)) || (rc = upload(d_lab, labels, (size_t)label_off[R], s)))) return rc;
    a.cells = d_cells.as<int32_t>();
    a.rec = d_rec.as<uint64_t>(); a.meta = d_meta.as<uint16_t>();
    a.flagged = d_flag.as<TtFlagged>();
    a.n_flagged = reinterpret_cast<uint32_t *>(a.flagged + TT_FLAG_CAP);
    a.seg_sum = d_seg_sum.as<uint32_t>(); a.seg_off = d_seg_off.as<int64_t>(); a.row_bytes = d_row_bytes.as<int64_t>();
    a.row_off = d_row_off.as<int64_t>();
    a.lab_off = label_off ? d_lab_off.as<int64_t>() : nullptr;
    a.lab = label_off ? d_lab.as<uint8_t>() : nullptr;
    a.out = out;

    // digits; then the flagged elements, at most TT_FLAG_CAP per round, are formatted here and their records replaced
    ICNV_HIP(hipMemsetAsync(a.n_flagged, 0, sizeof(uint64_t), s));
    if ((rc = launch_tt_digits(a, s))) return rc;
    int64_t n_host = 0, rounds = 0;
    for (;;) {
        uint32_t count = 0;
        ICNV_HIP(hipMemcpyAsync(&count, a.n_flagged, sizeof(count), hipMemcpyDeviceToHost, s));
        ICNV_HIP(hipStreamSynchronize(s));
        if (!count) break;
        const size_t n = count < (uint32_t)TT_FLAG_CAP ? count : (size_t)TT_FLAG_CAP;
        std::vector<TtFlagged> fl(n);
        ICNV_HIP(hipMemcpyAsync(fl.data(), a.flagged, n * sizeof(TtFlagged), hipMemcpyDeviceToHost, s));
        ICNV_HIP(hipStreamSynchronize(s));
        std::vector<int64_t> idx(n);
        std::vector<uint64_t> rec(n);
        std::vector<uint16_t> meta(n);
        for (size_t i = 0; i < n; ++i) {
            if (fl[i].idx < 0 || fl[i].idx >= n_elem) ICNV_FAIL(ICNV_ERR_HIP, "format_table: a flagged element lies outside the chunk (internal error)");
            idx[i] = fl[i].idx;
            tt_host_record(fl[i].bits, rec[i], meta[i]);
        }
        DevBuf d_idx, d_nrec, d_nmeta;
        if ((rc = upload(d_idx, idx.data(), n, s)) || (rc = upload(d_nrec, rec.data(), n, s)) || (rc = upload(d_nmeta, meta.data(), n, s)) ||
            (rc = launch_tt_patch(a, d_idx.as<int64_t>(), d_nrec.as<uint64_t>(), d_nmeta.as<uint16_t>(), (int32_t)n, s)))
            return rc;
        n_host += (int64_t)n;
        ICNV_HIP(hipMemsetAsync(a.n_flagged, 0, sizeof(uint64_t), s));
        if (count > (uint32_t)TT_FLAG_CAP) {                  // some were counted but not listed: look for the bit that is left
            ++rounds;
            if ((rc = launch_tt_collect(a, s))) return rc;
        }
        ICNV_HIP(hipStreamSynchronize(s));                      // the uploads' pool blocks outlive the patch
    }

    // lengths: segment sums and row byte counts on the device, the scan over rows here (the caller wants the offsets anyway)
    if ((rc = launch_tt_lengths(a, s))) return rc;
    std::vector<int64_t> off((size_t)R + 1);
    ICNV_HIP(hipMemcpyAsync(off.data() + 1, a.row_bytes, (size_t)R * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    off[0] = 0;
    int64_t fit = 0;
    for (int64_t r = 0; r < R; ++r) {
        off[(size_t)r + 1] += off[(size_t)r];
        if (off[(size_t)r + 1] <= capacity) fit = r + 1;
        else break;
    }
    if (fit < 1) ICNV_FAIL(ICNV_ERR_ARG, "format_table: the capacity is below the first row (" + std::to_string(off[1]) + " bytes)");
    ICNV_HIP(hipMemcpyAsync(d_row_off.p, off.data(), (size_t)(fit + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if ((rc = launch_tt_emit(a, fit, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));

    if (row_offsets) std::memcpy(row_offsets, off.data(), (size_t)(fit + 1) * sizeof(int64_t));
    *rows_done = fit;
    *n_bytes = off[(size_t)fit];
    g_tt[0] += 1; g_tt[1] += fit; g_tt[2] += n_elem; g_tt[3] += n_host; g_tt[4] += off[(size_t)fit]; g_tt[5] += rounds;
    g_tt[6] += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return ICNV_OK;
}

int icnv_format_table(const double *x, int64_t G, int64_t C, int32_t orientation, int64_t row0, int64_t n_rows, const int32_t *cells,
                      int64_t n_cells, const uint8_t *labels, const int64_t *label_off, const char *sep, uint8_t *out, int64_t capacity,
                      int64_t *row_offsets, int64_t *rows_done, int64_t *n_bytes) {
    TtPlan p{};
    int rc;
    if ((rc = tt_validate(x, G, G, C, orientation, row0, n_rows, cells, n_cells, labels, label_off, sep, out, capacity, rows_done, n_bytes,
                          p)))
        return rc;
    MatrixLease in;
    DevBuf d_out;
    int64_t done = 0, bytes = 0;
    if ((rc = acquire_input(x, G * C, nullptr, in)) || (rc = d_out.alloc((size_t)capacity))) return rc;
    if ((rc = icnv_format_table_dev(in.dev, G, G, C, orientation, row0, n_rows, cells, n_cells, labels, label_off, sep, d_out.as<uint8_t>(),
                                    capacity, row_offsets, &done, &bytes, nullptr)))
        return rc;
    ICNV_HIP(hipMemcpy(out, d_out.p, (size_t)bytes, hipMemcpyDeviceToHost));
    *rows_done = done;
    *n_bytes = bytes;
    return ICNV_OK;
}

int icnv_table_text_stats(int64_t *out, int32_t n) {
    if (!out || n < 1) ICNV_FAIL(ICNV_ERR_ARG, "bad argument");
    for (int i = 0; i < n && i < 7; ++i) out[i] = g_tt[i].load();
    return ICNV_OK;
}

void icnv_table_text_stats_reset(void) {
    for (auto &c : g_tt) c.store(0);
}

}  // extern "C"
