// C ABI of K31 (include/icnv.h "MCMC convergence diagnostics"): the refusals, the windows and AR orders of the schedule, the
// launch, and the host-buffer twin.  Kernel: mcmc_diag_kernels.hip.  DESIGN.md section 4 K31.
#include <string>

#include "icnv_internal.h"
#include "mcmc_diag_internal.h"

using namespace icnv;

namespace {

int mcmc_validate(const void *samples, int32_t n_regions, int32_t n_chains, int32_t n_keep, int32_t K, const void *chain_stats,
                  const void *pooled) {
    if (!samples || !chain_stats || !pooled) ICNV_FAIL(ICNV_ERR_ARG, "mcmc_diag: null argument");
    if (n_regions < 1) ICNV_FAIL(ICNV_ERR_ARG, "mcmc_diag: n_regions must be >= 1");
    if (K < MCMC_MIN_CHAINS || K > MCMC_MAX_CHAINS || n_chains < MCMC_MIN_CHAINS || n_chains > MCMC_MAX_CHAINS)
        ICNV_FAIL(ICNV_ERR_ARG, "mcmc_diag: K and n_chains must be 2 .. 8");
    if (n_keep < MCMC_MIN_KEEP) ICNV_FAIL(ICNV_ERR_ARG, "mcmc_diag: n_keep must be >= 20 (the Geweke windows need it)");
    if ((int64_t)n_chains * n_keep > MCMC_MAX_POOLED)
        ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "mcmc_diag: n_chains * n_keep = " + std::to_string((int64_t)n_chains * n_keep) +
                                            " exceeds 8192 (the pooled draws are sorted in LDS)");
    if ((int64_t)n_regions * K > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "mcmc_diag: too many (region, state) pairs for one call");
    return ICNV_OK;
}

}  // namespace

extern "C" {

int icnv_mcmc_diag_dev(const double *theta_samples, int32_t n_regions, int32_t n_chains, int32_t n_keep, int32_t K, double *chain_stats,
                       double *pooled, void *stream) {
    int rc = mcmc_validate(theta_samples, n_regions, n_chains, n_keep, K, chain_stats, pooled);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    McmcDiagArgs a{};
    a.samples = theta_samples; a.chain_stats = chain_stats; a.pooled = pooled;
    a.n_regions = n_regions; a.K = K; a.n_chains = n_chains; a.n_keep = n_keep;
    a.n_pad = 64;
    while (a.n_pad < n_chains * n_keep) a.n_pad <<= 1;
    mcmc_windows(n_keep, a.win);
    if ((rc = launch_mcmc_diag(a, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));
    return ICNV_OK;
}

int icnv_mcmc_diag(const double *theta_samples, int32_t n_regions, int32_t n_chains, int32_t n_keep, int32_t K, double *chain_stats,
                   double *pooled) {
    int rc = mcmc_validate(theta_samples, n_regions, n_chains, n_keep, K, chain_stats, pooled);
    if (rc) return rc;
    const size_t n_cs = (size_t)n_regions * K * n_chains * MCMC_CHAIN_FIELDS, n_po = (size_t)n_regions * K * MCMC_POOLED_FIELDS;
    DevBuf d_in, d_cs, d_po;
    if ((rc = upload(d_in, theta_samples, (size_t)n_regions * n_chains * n_keep * K, nullptr)) ||
        (rc = d_cs.alloc(n_cs * sizeof(double))) || (rc = d_po.alloc(n_po * sizeof(double))))
        return rc;
    if ((rc = icnv_mcmc_diag_dev(d_in.as<double>(), n_regions, n_chains, n_keep, K, d_cs.as<double>(), d_po.as<double>(), nullptr))) return rc;
    ICNV_HIP(hipMemcpy(chain_stats, d_cs.p, n_cs * sizeof(double), hipMemcpyDeviceToHost));
    ICNV_HIP(hipMemcpy(pooled, d_po.p, n_po * sizeof(double), hipMemcpyDeviceToHost));
    return ICNV_OK;
}

}  // extern "C"
