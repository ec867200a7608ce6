// C ABI of the dense half of K26 (include/icnv.h "reading a selection of columns"): icnv_parse_table_cols_dev.  The checks, the
// refusal text and the counters are icnv_parse_table_dev's (table_parse_api.hip); the order of the passes and the strtod path
// for uncertified fields are restated here for staging that is n_cols_out wide.  Kernels: table_cols_kernels.hip, and K21's
// structure, rows, patch and transpose launches.  DESIGN.md section 4 K26.
#include <chrono>
#include <string>
#include <vector>

#include "icnv_internal.h"
#include "col_map_internal.h"
#include "table_parse_host.h"
#include "table_parse_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

extern "C" {

int icnv_parse_table_cols_dev(const uint8_t *text_dev, const uint8_t *text_host, int64_t n_bytes, const char *sep, int64_t n_cols, int64_t line0,
                              double *out, int64_t ld, int64_t row0, int64_t max_rows, int64_t *label_ranges, int64_t *n_rows,
                              const int32_t *col_map_dev, int64_t n_cols_out, void *stream) {
    int rc;
    if ((rc = tp_check_args(text_dev, text_host, n_bytes, sep, n_cols, line0, out, ld, row0, max_rows, label_ranges, n_rows))) return rc;
    if (!col_map_dev) ICNV_FAIL(ICNV_ERR_ARG, "parse_table_cols: null column map");
    const auto t0 = std::chrono::steady_clock::now();
    hipStream_t s = (hipStream_t)stream;
    if ((rc = check_col_map(col_map_dev, n_cols, n_cols_out, "parse_table_cols", s))) return rc;

    TcArgs t{};
    TpArgs &a = t.tp;
    t.col_map = col_map_dev; t.n_cols_out = n_cols_out;
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
        tp_count_call(0, 0, 0, n_bytes, 0, std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
        return ICNV_OK;
    }
    const int64_t n_vals = a.n_rows * n_cols_out;

    // index, rows, parse: no list of all fields, only the positions and values of the selected ones
    DevBuf d_row, d_sel, d_vals, d_flag;
    if ((rc = d_row.alloc((size_t)a.n_rows * 4 * sizeof(uint32_t))) || (rc = d_sel.alloc((size_t)n_vals * sizeof(uint32_t))) ||
        (rc = d_vals.alloc((size_t)n_vals * sizeof(uint64_t))) || (rc = d_flag.alloc((size_t)TP_FLAG_CAP * sizeof(TpFlagged))))
        return rc;
    a.row_pos = d_row.as<uint32_t>(); a.row_field0 = a.row_pos + a.n_rows;
    a.label_range = reinterpret_cast<int32_t *>(a.row_field0 + a.n_rows);
    t.sel_pos = d_sel.as<uint32_t>();
    a.vals = d_vals.as<uint64_t>(); a.flagged = d_flag.as<TpFlagged>();
    if ((rc = launch_tc_index(t, s)) || (rc = launch_tc_parse(t, s))) return rc;

    // the selected fields the parse pass did not certify, at most TP_FLAG_CAP per round: strtod here, the staged value replaced
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
                ICNV_FAIL(ICNV_ERR_HIP, "parse_table_cols: a flagged field lies outside the chunk (internal error)");
            slot[i] = fl[i].slot;
            if (tp_host_field(text, n_bytes, fl[i].pos, a.sep, bits[i]) != TP_VALUE) {
                const uint64_t word = ((uint64_t)fl[i].pos << 8) | (uint64_t)TP_E_NUMBER;
                if (word < worst) worst = word;
            }
        }
        if (worst != TP_NO_ERROR) return tp_refusal(text, n_bytes, worst, a.sep, line0, n_cols);
        DevBuf d_slot, d_bits;
        if ((rc = upload(d_slot, slot.data(), n, s)) || (rc = upload(d_bits, bits.data(), n, s)) ||
            (rc = launch_tp_patch(a, d_slot.as<int64_t>(), d_bits.as<uint64_t>(), (int32_t)n, s)))
            return rc;
        n_host += (int64_t)n;
        ICNV_HIP(hipMemsetAsync(a.n_flagged, 0, sizeof(uint64_t), s));
        if (count > (uint32_t)TP_FLAG_CAP) {                          // some were counted but not listed: look for what is still pending
            ++rounds;
            if ((rc = launch_tc_collect(t, s))) return rc;
        }
        ICNV_HIP(hipStreamSynchronize(s));                              // the uploads' pool blocks outlive the patch
    }

    // every selected value is known and nothing was refused: K21's transpose of a table that is n_cols_out wide
    std::vector<int32_t> ranges((size_t)a.n_rows * 2);
    TpArgs narrow = a;
    narrow.n_cols = n_cols_out;
    if ((rc = launch_tp_transpose(narrow, s))) return rc;
    ICNV_HIP(hipMemcpyAsync(ranges.data(), a.label_range, ranges.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    for (int64_t r = 0; r < a.n_rows; ++r) {
        int64_t b = ranges[(size_t)(2 * r)], e = ranges[(size_t)(2 * r + 1)];
        if (text_host) tp_label_slice(text_host, b, e);                // (no host copy: the caller slices the labels it fetches)
        label_ranges[2 * r] = b;
        label_ranges[2 * r + 1] = e;
    }
    *n_rows = a.n_rows;
    tp_count_call(a.n_rows, n_vals, n_host, n_bytes, rounds,
                  std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count());
    return ICNV_OK;
}

}  // extern "C"
