// C ABI of K14 (include/icnv.h "per-cell CNV features and run-length segmentation"): validation, the counting pass, the scan of
// the run counts in list order and the segmentation pass.  Kernels: cnv_summary_kernels.hip.  DESIGN.md section 4 K14.
#include <algorithm>
#include <string>
#include <vector>

#include "cnv_summary_internal.h"

using namespace icnv;

namespace {

int check_matrix(const char *who, const void *states, int64_t G, int64_t C, int64_t ld, const int32_t *chr_start, int32_t n_chr) {
    const std::string w(who);
    if (!states || !chr_start) ICNV_FAIL(ICNV_ERR_ARG, w + ": null argument");
    if (G < 1 || G > 0x7fffffff - 2 * CNVSUM_CHUNK_GENES || C < 0 || C > 0x7fffffff || ld < G)
        ICNV_FAIL(ICNV_ERR_ARG, w + ": bad matrix dimensions");
    if (n_chr < 1 || chr_start[0] != 0 || chr_start[n_chr] != G) ICNV_FAIL(ICNV_ERR_ARG, w + ": chr_start must run from 0 to G");
    for (int32_t k = 0; k < n_chr; ++k)
        if (chr_start[k + 1] < chr_start[k]) ICNV_FAIL(ICNV_ERR_ARG, w + ": chr_start must be non-decreasing");
    return ICNV_OK;
}

int read_bad(const char *who, const DevBuf &d_bad, int32_t K, hipStream_t s) {
    int32_t bad = 0;
    ICNV_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (bad) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": a state outside 1 .. " + std::to_string(K));
    return ICNV_OK;
}

}  // namespace

extern "C" {

int icnv_cnv_features_dev(const uint8_t *states, int64_t G, int64_t C, int64_t ld, const int32_t *chr_start, int32_t n_chr, int32_t K,
                          int32_t s0, int32_t *counts, int32_t *run_counts, void *stream) {
    int rc = check_matrix("cnv_features", states, G, C, ld, chr_start, n_chr);
    if (rc) return rc;
    if (!counts) ICNV_FAIL(ICNV_ERR_ARG, "cnv_features: null argument");
    if (reinterpret_cast<uintptr_t>(counts) & 15u) ICNV_FAIL(ICNV_ERR_ARG, "cnv_features: counts must be 16-byte aligned");
    if (K < 2 || s0 < 1 || s0 > K) ICNV_FAIL(ICNV_ERR_ARG, "cnv_features: K >= 2 and 1 <= s0 <= K");
    if (K > CNVSUM_MAX_K) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "cnv_features: K > " + std::to_string(CNVSUM_MAX_K));
    if (C == 0) return ICNV_OK;
    hipStream_t s = (hipStream_t)stream;
    DevBuf d_cs, d_bad, d_rc;
    if ((rc = upload(d_cs, chr_start, (size_t)n_chr + 1, s)) || (rc = d_bad.alloc(sizeof(int32_t)))) return rc;
    if (!run_counts) {
        if ((rc = d_rc.alloc((size_t)C * 2 * sizeof(int32_t)))) return rc;
        run_counts = d_rc.as<int32_t>();
    }
    CnvSumArgs a{states, ld, (int32_t)G, C, d_cs.as<int32_t>(), n_chr, K, s0, counts, run_counts, d_bad.as<int32_t>()};
    if ((rc = launch_cnvsum_count(a, s))) return rc;
    return read_bad("cnv_features", d_bad, K, s);
}

int icnv_cnv_features(const uint8_t *states, int64_t G, int64_t C, const int32_t *chr_start, int32_t n_chr, int32_t K, int32_t s0,
                      int32_t *counts, int32_t *run_counts) {
    int rc = check_matrix("cnv_features", states, G, C, G, chr_start, n_chr);
    if (rc) return rc;
    if (!counts) ICNV_FAIL(ICNV_ERR_ARG, "cnv_features: null argument");
    if (C == 0) return ICNV_OK;
    const size_t n = (size_t)G * (size_t)C, n_counts = (size_t)n_chr * (size_t)C * 4;
    DevBuf ds, dc, dr;
    if ((rc = ds.alloc(n)) || (rc = dc.alloc(n_counts * sizeof(int32_t))) || (rc = dr.alloc((size_t)C * 2 * sizeof(int32_t)))) return rc;
    ICNV_HIP(hipMemcpy(ds.p, states, n, hipMemcpyHostToDevice));
    if ((rc = icnv_cnv_features_dev(ds.as<uint8_t>(), G, C, G, chr_start, n_chr, K, s0, dc.as<int32_t>(), dr.as<int32_t>(), nullptr)))
        return rc;
    ICNV_HIP(hipMemcpy(counts, dc.p, n_counts * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (run_counts) ICNV_HIP(hipMemcpy(run_counts, dr.p, (size_t)C * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ICNV_OK;
}

int icnv_cnv_runs_dev(const uint8_t *states, int64_t G, int64_t C, int64_t ld, const int32_t *chr_start, int32_t n_chr,
                      const int32_t *col_idx, int64_t n_cols, int32_t K, int32_t neutral, int32_t *run_counts, int32_t counts_valid,
                      int64_t capacity, int32_t *records, int64_t *n_records, int64_t *n_runs, void *stream) {
    int rc = check_matrix("cnv_runs", states, G, C, ld, chr_start, n_chr);
    if (rc) return rc;
    if (!n_records || capacity < 0 || (capacity > 0 && !records)) ICNV_FAIL(ICNV_ERR_ARG, "cnv_runs: null argument");
    if (K < 0 || neutral < 0 || neutral > 255 || (K > 0 && neutral > K)) ICNV_FAIL(ICNV_ERR_ARG, "cnv_runs: bad K / neutral state");
    if (K > CNVSUM_MAX_K) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "cnv_runs: K > " + std::to_string(CNVSUM_MAX_K));
    if (counts_valid && !run_counts) ICNV_FAIL(ICNV_ERR_ARG, "cnv_runs: counts_valid without run_counts");
    if (!col_idx) n_cols = C;
    if (n_cols < 0 || n_cols > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "cnv_runs: bad column list");
    for (int64_t i = 0; col_idx && i < n_cols; ++i)
        if (col_idx[i] < 0 || col_idx[i] >= C) ICNV_FAIL(ICNV_ERR_ARG, "cnv_runs: column index out of range");
    *n_records = 0;
    if (n_runs) *n_runs = 0;
    if (C == 0 || n_cols == 0) return ICNV_OK;
    hipStream_t s = (hipStream_t)stream;
    DevBuf d_cs, d_bad, d_rc, d_idx, d_off, d_tot;
    if ((rc = upload(d_cs, chr_start, (size_t)n_chr + 1, s)) || (rc = d_bad.alloc(sizeof(int32_t))) ||
        (rc = d_off.alloc((size_t)n_cols * 2 * sizeof(int64_t))) || (rc = d_tot.alloc(2 * sizeof(int64_t))))
        return rc;
    if (col_idx && (rc = upload(d_idx, col_idx, (size_t)n_cols, s))) return rc;
    if (!run_counts) {
        if ((rc = d_rc.alloc((size_t)C * 2 * sizeof(int32_t)))) return rc;
        run_counts = d_rc.as<int32_t>();
    }
    if (!counts_valid) {
        CnvSumArgs a{states, ld, (int32_t)G, C, d_cs.as<int32_t>(), n_chr, K, neutral, nullptr, run_counts, d_bad.as<int32_t>()};
        if ((rc = launch_cnvsum_count(a, s))) return rc;
        if (K > 0 && (rc = read_bad("cnv_runs", d_bad, K, s))) return rc;
    }
    int64_t *rec_off = d_off.as<int64_t>(), *ord_off = rec_off + n_cols;
    if ((rc = launch_cnvsum_scan(run_counts, col_idx ? d_idx.as<int32_t>() : nullptr, n_cols, rec_off, ord_off, d_tot.as<int64_t>(), s)))
        return rc;
    int64_t tot[2] = {0, 0};
    ICNV_HIP(hipMemcpyAsync(tot, d_tot.p, sizeof(tot), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    *n_records = tot[0];
    if (n_runs) *n_runs = tot[1];
    if (tot[1] > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "cnv_runs: more than 2^31 - 1 runs: the ordinal does not fit an int32");
    if (!records) return ICNV_OK;                      // the count-only call
    if (tot[0] > capacity) ICNV_FAIL(ICNV_ERR_ARG, "cnv_runs: " + std::to_string(tot[0]) + " records, capacity " + std::to_string(capacity));
    CnvRunsArgs r{states, ld, (int32_t)G, d_cs.as<int32_t>(), n_chr, col_idx ? d_idx.as<int32_t>() : nullptr, n_cols, neutral,
                  rec_off, ord_off, capacity, records};
    if ((rc = launch_cnvsum_runs(r, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));                 // the workspace goes back to the pool when this returns
    return ICNV_OK;
}

int icnv_cnv_runs(const uint8_t *states, int64_t G, int64_t C, const int32_t *chr_start, int32_t n_chr, const int32_t *col_idx,
                  int64_t n_cols, int32_t K, int32_t neutral, int64_t capacity, int32_t *records, int64_t *n_records, int64_t *n_runs) {
    int rc = check_matrix("cnv_runs", states, G, C, G, chr_start, n_chr);
    if (rc) return rc;
    if (!n_records || capacity < 0 || (capacity > 0 && !records)) ICNV_FAIL(ICNV_ERR_ARG, "cnv_runs: null argument");
    const size_t n = (size_t)G * (size_t)C;
    DevBuf ds, dr;
    if ((rc = ds.alloc(std::max<size_t>(n, 1)))) return rc;
    if (records && (rc = dr.alloc((size_t)capacity * 6 * sizeof(int32_t)))) return rc;
    if (n) ICNV_HIP(hipMemcpy(ds.p, states, n, hipMemcpyHostToDevice));
    if ((rc = icnv_cnv_runs_dev(ds.as<uint8_t>(), G, C, G, chr_start, n_chr, col_idx, n_cols, K, neutral, nullptr, 0, capacity,
                                records ? dr.as<int32_t>() : nullptr, n_records, n_runs, nullptr)))
        return rc;
    if (records) ICNV_HIP(hipMemcpy(records, dr.p, (size_t)capacity * 6 * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ICNV_OK;
}

}  // extern "C"
