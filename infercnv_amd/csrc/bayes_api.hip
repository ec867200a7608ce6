// C ABI of K13 (include/icnv.h "Bayesian filter of the predicted CNV regions"): validation, the 64-cell tiles of the likelihood
// pass, the LDS-resident, the streaming and the packed class (K25) of the sampler, stats.  Kernels: bayes_kernels.hip.
// DESIGN.md section 4 K13, K25.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <string>
#include <vector>

#include "icnv_internal.h"
#include "bayes_internal.h"

using namespace icnv;

namespace {

std::atomic<int64_t> g_bayes[9];   // sample calls, regions, cells, undecided cells, LDS regions, streamed regions, sample us, loglik us, packed regions

int check_offsets(const char *who, const int64_t *cell_off, int32_t n_regions, int32_t K) {
    if (n_regions < 1) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": n_regions must be >= 1");
    if (K < 2) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": K must be >= 2");
    if (K > BAYES_MAX_K) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, std::string(who) + ": K > " + std::to_string(BAYES_MAX_K));
    if (cell_off[0] != 0) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": offsets must start at 0");
    for (int32_t r = 0; r < n_regions; ++r) {
        if (cell_off[r + 1] < cell_off[r]) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": offsets must be monotone");
        if (cell_off[r + 1] - cell_off[r] > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": region too large");
    }
    if (cell_off[n_regions] * K > ((int64_t)1 << 40)) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, std::string(who) + ": too many (region, cell) rows");
    return ICNV_OK;
}

bool skip_decided() {   // ICNV_BAYES_DECIDED=0: every cell is sampled in every iteration (the output is the same)
    const char *e = std::getenv("ICNV_BAYES_DECIDED");
    return !(e && *e == '0');
}

bool packed_enabled() {   // ICNV_BAYES_PACKED=0: the regions of <= 8 undecided cells take the LDS path (the output is the same)
    const char *e = std::getenv("ICNV_BAYES_PACKED");
    return !(e && *e == '0');
}

int loglik_validate(const double *expr, int64_t G, int64_t C, int64_t ld, const int32_t *gene_start, const int32_t *gene_count,
                    const int32_t *cell_idx, const int64_t *cell_off, int32_t n_regions, int32_t K, const double *mu, const double *tau,
                    const void *ll, const void *L) {
    if (!expr || !gene_start || !gene_count || !cell_off || !mu || !tau || !ll || !L) ICNV_FAIL(ICNV_ERR_ARG, "bayes_loglik: null argument");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff || ld < G) ICNV_FAIL(ICNV_ERR_ARG, "bayes_loglik: bad matrix dimensions");
    int rc = check_offsets("bayes_loglik", cell_off, n_regions, K);
    if (rc) return rc;
    if (cell_off[n_regions] > 0 && !cell_idx) ICNV_FAIL(ICNV_ERR_ARG, "bayes_loglik: null argument");
    for (int32_t r = 0; r < n_regions; ++r)
        if (gene_count[r] < 1 || gene_start[r] < 0 || (int64_t)gene_start[r] + gene_count[r] > G)
            ICNV_FAIL(ICNV_ERR_ARG, "bayes_loglik: region " + std::to_string(r) + ": gene run out of range");
    for (int64_t i = 0; i < cell_off[n_regions]; ++i)
        if (cell_idx[i] < 0 || cell_idx[i] >= C) ICNV_FAIL(ICNV_ERR_ARG, "bayes_loglik: cell index out of range");
    for (int32_t k = 0; k < K; ++k)
        if (!std::isfinite(mu[k]) || !std::isfinite(tau[k]) || !(tau[k] > 0)) ICNV_FAIL(ICNV_ERR_ARG, "bayes_loglik: mu must be finite, tau finite and > 0");
    return ICNV_OK;
}

int sample_validate(const double *L, const int64_t *cell_off, const uint64_t *token, int32_t n_regions, int32_t K, int32_t n_adapt,
                    int32_t n_burn, int32_t n_keep, const void *theta_sum, const void *freq) {
    if (!L || !cell_off || !token || !theta_sum || !freq) ICNV_FAIL(ICNV_ERR_ARG, "bayes_sample: null argument");
    int rc = check_offsets("bayes_sample", cell_off, n_regions, K);
    if (rc) return rc;
    if (n_adapt < 0 || n_burn < 0 || n_keep < 1) ICNV_FAIL(ICNV_ERR_ARG, "bayes_sample: n_adapt, n_burn >= 0 and n_keep >= 1");
    if ((int64_t)n_adapt + n_burn + n_keep > 0x7fffffff || (int64_t)K * n_keep > 0x7fffffff)
        ICNV_FAIL(ICNV_ERR_ARG, "bayes_sample: too many iterations");
    return ICNV_OK;
}

}  // namespace

extern "C" {

int icnv_bayes_loglik_dev(const double *expr, int64_t G, int64_t C, int64_t ld, const int32_t *gene_start, const int32_t *gene_count,
                          const int32_t *cell_idx, const int64_t *cell_off, int32_t n_regions, int32_t K, const double *mu,
                          const double *tau, double *ll, double *L, void *stream) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc = loglik_validate(expr, G, C, ld, gene_start, gene_count, cell_idx, cell_off, n_regions, K, mu, tau, ll, L);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    std::vector<BayesRegion> regs((size_t)n_regions);
    std::vector<int64_t> tile_off((size_t)n_regions + 1, 0);
    for (int32_t r = 0; r < n_regions; ++r) {
        regs[r] = BayesRegion{cell_off[r], (int32_t)(cell_off[r + 1] - cell_off[r]), gene_start[r], gene_count[r], 0, 0};
        tile_off[r + 1] = tile_off[r] + (regs[r].n_cells + 63) / 64;
    }
    if (tile_off[n_regions] > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "bayes_loglik: too many cell tiles");
    std::vector<double> mt((size_t)2 * K);
    for (int32_t k = 0; k < K; ++k) { mt[k] = mu[k]; mt[K + k] = tau[k]; }
    DevBuf d_regs, d_tile, d_cidx, d_mt;
    if ((rc = upload(d_regs, regs.data(), regs.size(), s)) || (rc = upload(d_tile, tile_off.data(), tile_off.size(), s)) ||
        (rc = upload(d_cidx, cell_idx, (size_t)cell_off[n_regions], s)) || (rc = upload(d_mt, mt.data(), mt.size(), s)))
        return rc;
    BayesLoglik a{};
    a.x = expr; a.ld = ld; a.cell_idx = d_cidx.as<int32_t>(); a.regions = d_regs.as<BayesRegion>(); a.tile_off = d_tile.as<int64_t>();
    a.n_regions = n_regions; a.K = K; a.mu_tau = d_mt.as<double>(); a.ll = ll; a.L = L;
    if ((rc = launch_bayes_loglik(a, tile_off[n_regions], s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));
    g_bayes[7] += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return ICNV_OK;
}

int icnv_bayes_loglik(const double *expr, int64_t G, int64_t C, const int32_t *gene_start, const int32_t *gene_count,
                      const int32_t *cell_idx, const int64_t *cell_off, int32_t n_regions, int32_t K, const double *mu, const double *tau,
                      double *ll, double *L) {
    int rc = loglik_validate(expr, G, C, G, gene_start, gene_count, cell_idx, cell_off, n_regions, K, mu, tau, ll, L);
    if (rc) return rc;
    const size_t n = (size_t)cell_off[n_regions] * K;
    MatrixLease in;
    DevBuf d_ll, d_L;
    if ((rc = acquire_input(expr, G * C, nullptr, in)) || (rc = d_ll.alloc(std::max<size_t>(n, 1) * sizeof(double))) ||
        (rc = d_L.alloc(std::max<size_t>(n, 1) * sizeof(double))))
        return rc;
    if ((rc = icnv_bayes_loglik_dev(in.dev, G, C, G, gene_start, gene_count, cell_idx, cell_off, n_regions, K, mu, tau, d_ll.as<double>(),
                                    d_L.as<double>(), nullptr)))
        return rc;
    if (n) {
        ICNV_HIP(hipMemcpy(ll, d_ll.p, n * sizeof(double), hipMemcpyDeviceToHost));
        ICNV_HIP(hipMemcpy(L, d_L.p, n * sizeof(double), hipMemcpyDeviceToHost));
    }
    return ICNV_OK;
}

int icnv_bayes_sample_dev(const double *L, const int64_t *cell_off, const uint64_t *token, int32_t n_regions, int32_t K, int32_t n_adapt,
                          int32_t n_burn, int32_t n_keep, uint64_t seed, double *theta_sum, double *theta_samples, int32_t *freq,
                          void *stream) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc = sample_validate(L, cell_off, token, n_regions, K, n_adapt, n_burn, n_keep, theta_sum, freq);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t rows = cell_off[n_regions];
    std::vector<BayesRegion> regs((size_t)n_regions);
    for (int32_t r = 0; r < n_regions; ++r)
        regs[r] = BayesRegion{cell_off[r], (int32_t)(cell_off[r + 1] - cell_off[r]), 0, 0, 0, token[r]};
    DevBuf d_regs, d_und, d_nund, d_nfix;
    if ((rc = upload(d_regs, regs.data(), regs.size(), s)) || (rc = d_und.alloc((size_t)std::max<int64_t>(rows, 1) * sizeof(int32_t))) ||
        (rc = d_nund.alloc((size_t)n_regions * sizeof(int32_t))) || (rc = d_nfix.alloc((size_t)n_regions * BAYES_MAX_K * sizeof(int32_t))))
        return rc;
    if (rows) ICNV_HIP(hipMemsetAsync(freq, 0, (size_t)rows * K * sizeof(int32_t), s));
    if ((rc = launch_bayes_prep(L, d_regs.as<BayesRegion>(), n_regions, K, skip_decided() ? 1 : 0, n_keep, d_und.as<int32_t>(),
                                d_nund.as<int32_t>(), d_nfix.as<int32_t>(), freq, s)))
        return rc;
    std::vector<int32_t> n_und((size_t)n_regions);
    ICNV_HIP(hipMemcpyAsync(n_und.data(), d_nund.p, (size_t)n_regions * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));

    // three classes: the regions whose undecided cells fit LDS, the others, and the regions of a handful of undecided cells
    std::vector<int32_t> list[3];
    int32_t lds_cells = 0;
    int64_t und_total = 0;
    const bool packed = packed_enabled();
    for (int32_t r = 0; r < n_regions; ++r) {
        und_total += n_und[r];
        if (packed && regs[r].n_cells > 0 && n_und[r] <= BAYES_PACKED_CELLS) list[2].push_back(r);
        else if (n_und[r] <= BAYES_LDS_CELLS) { list[0].push_back(r); lds_cells = std::max(lds_cells, n_und[r]); }
        else list[1].push_back(r);
    }
    DevBuf d_list[3];
    for (int q = 0; q < 3; ++q) {
        if (list[q].empty()) continue;
        if ((int64_t)list[q].size() * K > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "bayes_sample: too many regions");
        if ((rc = upload(d_list[q], list[q].data(), list[q].size(), s))) return rc;
        BayesSample a{};
        a.L = L; a.regions = d_regs.as<BayesRegion>(); a.list = d_list[q].as<int32_t>(); a.n_list = (int32_t)list[q].size(); a.K = K;
        a.n_discard = n_adapt + n_burn; a.n_keep = n_keep; a.seed = seed; a.und = d_und.as<int32_t>(); a.n_und = d_nund.as<int32_t>();
        a.nfix = d_nfix.as<int32_t>(); a.theta_sum = theta_sum; a.theta_samples = theta_samples; a.freq = freq;
        if ((rc = q == 2 ? launch_bayes_sample_packed(a, s) : launch_bayes_sample(a, q == 0 ? lds_cells : 0, s))) return rc;
    }
    ICNV_HIP(hipStreamSynchronize(s));
    g_bayes[0] += 1;
    g_bayes[1] += n_regions;
    g_bayes[2] += rows;
    g_bayes[3] += und_total;
    g_bayes[4] += (int64_t)list[0].size() + (int64_t)list[2].size();
    g_bayes[5] += (int64_t)list[1].size();
    g_bayes[8] += (int64_t)list[2].size();
    g_bayes[6] += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return ICNV_OK;
}

int icnv_bayes_sample(const double *L, const int64_t *cell_off, const uint64_t *token, int32_t n_regions, int32_t K, int32_t n_adapt,
                      int32_t n_burn, int32_t n_keep, uint64_t seed, double *theta_sum, double *theta_samples, int32_t *freq) {
    int rc = sample_validate(L, cell_off, token, n_regions, K, n_adapt, n_burn, n_keep, theta_sum, freq);
    if (rc) return rc;
    const size_t rows = (size_t)cell_off[n_regions];
    const size_t n_sum = (size_t)n_regions * K * K, n_samp = n_sum * (size_t)n_keep;
    DevBuf d_L, d_sum, d_samp, d_freq;
    if ((rc = upload(d_L, L, rows * K, nullptr)) || (rc = d_sum.alloc(n_sum * sizeof(double))) ||
        (rc = d_freq.alloc(std::max<size_t>(rows * K, 1) * sizeof(int32_t))))
        return rc;
    if (theta_samples && (rc = d_samp.alloc(n_samp * sizeof(double)))) return rc;
    if ((rc = icnv_bayes_sample_dev(d_L.as<double>(), cell_off, token, n_regions, K, n_adapt, n_burn, n_keep, seed, d_sum.as<double>(),
                                    theta_samples ? d_samp.as<double>() : nullptr, d_freq.as<int32_t>(), nullptr)))
        return rc;
    ICNV_HIP(hipMemcpy(theta_sum, d_sum.p, n_sum * sizeof(double), hipMemcpyDeviceToHost));
    if (theta_samples) ICNV_HIP(hipMemcpy(theta_samples, d_samp.p, n_samp * sizeof(double), hipMemcpyDeviceToHost));
    if (rows) ICNV_HIP(hipMemcpy(freq, d_freq.p, rows * K * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ICNV_OK;
}

int icnv_bayes_stats(int64_t *out, int32_t n) {
    if (!out || n < 1) ICNV_FAIL(ICNV_ERR_ARG, "bad argument");
    for (int i = 0; i < n && i < 9; ++i) out[i] = g_bayes[i].load();
    return ICNV_OK;
}

void icnv_bayes_stats_reset(void) {
    for (auto &c : g_bayes) c.store(0);
}

}  // extern "C"
