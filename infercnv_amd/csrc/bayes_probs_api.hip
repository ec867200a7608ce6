// C ABI of K33 (include/icnv.h "Probability heatmaps and tables of the Bayesian filter"): the refusals, the device-side index
// check of the paint and its launches, the box statistics' launch.  Kernels: bayes_probs_kernels.hip.  DESIGN.md section 4 K33.
#include <string>

#include "icnv_internal.h"
#include "bayes_probs_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

extern "C" {

int icnv_paint_regions_dev(double *out, int64_t G, int64_t C, int64_t ld, int32_t n_regions, const int32_t *gene_first,
                           const int32_t *gene_count, const int64_t *cell_off, const int32_t *cell_idx, int64_t n_idx,
                           const double *value, void *stream) {
    if (!out) ICNV_FAIL(ICNV_ERR_ARG, "paint_regions: null argument");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff || ld < G) ICNV_FAIL(ICNV_ERR_ARG, "paint_regions: bad matrix dimensions");
    if (n_regions < 0 || n_idx < 0 || (n_idx > 0 && !cell_idx)) ICNV_FAIL(ICNV_ERR_ARG, "paint_regions: bad region arrays");
    if (n_regions > 0 && (!gene_first || !gene_count || !cell_off || !value)) ICNV_FAIL(ICNV_ERR_ARG, "paint_regions: null argument");
    hipStream_t s = (hipStream_t)stream;
    PaintRegions a{out, G, C, ld, n_regions, gene_first, gene_count, cell_off, cell_idx, n_idx, value};
    int64_t verdict[4] = {0, 0, 0, 0};
    if (n_regions > 0) {
        DevBuf d_verdict;
        int rc = d_verdict.alloc(4 * sizeof(int64_t));
        if (rc) return rc;
        ICNV_HIP(hipMemsetAsync(d_verdict.p, 0, 4 * sizeof(int64_t), s));
        if ((rc = launch_paint_check(a, d_verdict.as<int64_t>(), s))) return rc;
        ICNV_HIP(hipMemcpyAsync(verdict, d_verdict.p, sizeof(verdict), hipMemcpyDeviceToHost, s));
        ICNV_HIP(hipStreamSynchronize(s));
        if (verdict[0] == 1) ICNV_FAIL(ICNV_ERR_ARG, "paint_regions: cell_off must start at 0, be monotone and end within cell_idx");
        if (verdict[0] == 2) ICNV_FAIL(ICNV_ERR_ARG, "paint_regions: gene run out of range");
        if (verdict[0] == 3) ICNV_FAIL(ICNV_ERR_ARG, "paint_regions: cell index out of range");
    }
    return launch_paint(a, verdict[1], verdict[2], verdict[3] == 0, s);
}

int icnv_theta_box_dev(const double *theta_samples, int32_t n_regions, int32_t n_chains, int32_t n_keep, int32_t K, double *box,
                       void *stream) {
    if (!theta_samples || !box) ICNV_FAIL(ICNV_ERR_ARG, "theta_box: null argument");
    if (n_regions < 0 || n_keep < 1) ICNV_FAIL(ICNV_ERR_ARG, "theta_box: n_regions must be >= 0 and n_keep >= 1");
    if (K < MCMC_MIN_CHAINS || K > MCMC_MAX_CHAINS || n_chains < MCMC_MIN_CHAINS || n_chains > MCMC_MAX_CHAINS)
        ICNV_FAIL(ICNV_ERR_ARG, "theta_box: K and n_chains must be 2 .. 8");
    if ((int64_t)n_chains * n_keep > MCMC_MAX_POOLED)
        ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "theta_box: n_chains * n_keep = " + std::to_string((int64_t)n_chains * n_keep) +
                                            " exceeds 8192 (the pooled draws are sorted in LDS)");
    if ((int64_t)n_regions * K > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "theta_box: too many (region, state) pairs for one call");
    if (n_regions == 0) return ICNV_OK;
    hipStream_t s = (hipStream_t)stream;
    ThetaBoxArgs a{};
    a.samples = theta_samples; a.box = box; a.n_regions = n_regions; a.K = K; a.N = n_chains * n_keep;
    a.n_pad = 64;
    while (a.n_pad < a.N) a.n_pad <<= 1;
    if (int rc = launch_theta_box(a, s)) return rc;
    ICNV_HIP(hipStreamSynchronize(s));
    return ICNV_OK;
}

}  // extern "C"
