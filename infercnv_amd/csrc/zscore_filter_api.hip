// C ABI of K32 (include/icnv.h "reference z-score gene filter"): validation, the upload of the cell list, the three passes and
// the download of {mean, sd}.  Kernels: zscore_filter_kernels.hip.  DESIGN.md section 4 K32.
#include <string>

#include "icnv_internal.h"
#include "zscore_filter_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

extern "C" {

int icnv_zscore_gene_filter_dev(const double *x, int64_t ld, int64_t G, int64_t C, const int32_t *ref_cells, int64_t n_ref, double *mean_sd,
                                double *row_mean, void *stream) {
    if (!x || !ref_cells || !mean_sd || !row_mean) ICNV_FAIL(ICNV_ERR_ARG, "zscore_gene_filter: null argument");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff || ld < G) ICNV_FAIL(ICNV_ERR_ARG, "zscore_gene_filter: bad matrix dimensions");
    if (n_ref < 1 || n_ref > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "zscore_gene_filter: the reference cell list must have 1 .. 2^31 - 1 entries");
    for (int64_t j = 0; j < n_ref; ++j)
        if (ref_cells[j] < 0 || ref_cells[j] >= C)
            ICNV_FAIL(ICNV_ERR_ARG, "zscore_gene_filter: entry " + std::to_string(j) + " of the reference cell list is not a cell");
    const int64_t n_chunks = zs_chunks(n_ref);
    if (n_chunks > 65535) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "zscore_gene_filter: more than 65535 * 256 reference cells");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    DevBuf d_rows, d_part, d_params;
    if ((rc = upload(d_rows, ref_cells, (size_t)n_ref, s))) return rc;
    const int64_t n_part = n_chunks * G;
    if ((rc = d_part.alloc((size_t)n_part * 3 * sizeof(double)))) return rc;
    if ((rc = d_params.alloc(4 * sizeof(double)))) return rc;
    double *hi = d_part.as<double>(), *lo = hi + n_part, *mx = lo + n_part, *params = d_params.as<double>();
    const int32_t *rows = d_rows.as<int32_t>();
    const int64_t n_values = n_ref * G;
    ICNV_HIP(hipMemsetAsync(params, 0, 4 * sizeof(double), s));
    if ((rc = launch_zscore_pass(ZS_SUM, x, ld, G, rows, n_ref, params, hi, lo, mx, s))) return rc;
    if ((rc = launch_zscore_finish_total(ZS_SUM, hi, lo, mx, n_part, n_values, params, s))) return rc;
    if ((rc = launch_zscore_pass(ZS_SQUARES, x, ld, G, rows, n_ref, params, hi, lo, mx, s))) return rc;
    if ((rc = launch_zscore_finish_total(ZS_SQUARES, hi, lo, mx, n_part, n_values, params, s))) return rc;
    if ((rc = launch_zscore_pass(ZS_ABS_Z, x, ld, G, rows, n_ref, params, hi, lo, mx, s))) return rc;
    if ((rc = launch_zscore_finish_genes(hi, lo, G, n_chunks, n_ref, row_mean, s))) return rc;
    double out[2];
    ICNV_HIP(hipMemcpyAsync(out, params, sizeof out, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));                                  // the pool blocks outlive the launches
    mean_sd[0] = out[0];
    mean_sd[1] = out[1];
    return ICNV_OK;
}

}  // extern "C"
