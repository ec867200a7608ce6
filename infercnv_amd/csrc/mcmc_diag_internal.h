// K31: convergence diagnostics of the Bayesian filter's chains (include/icnv.h "MCMC convergence diagnostics").  The per-series
// routines are __host__ __device__ code in this header: the kernel (mcmc_diag_kernels.hip) deals them to lanes, the host program
// mcmc_diag_host_check.cpp runs them one after the other under the sanitizers, and both must give the bits of
// tests/mcmc_diag_restate.py.  Every value is an individually rounded IEEE-754 double operation in the documented order: every
// unit that includes this header is built with -ffp-contract=off.  The table log comes in as a functor (lib_log of lib_math.h
// on the device, the same operation sequence on the host), so this header needs neither HIP nor the table.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MCMC_HD __host__ __device__
#else
#define MCMC_HD
#endif

namespace icnv {

constexpr int MCMC_MIN_CHAINS = 2, MCMC_MAX_CHAINS = 8;      // also the range of K
constexpr int MCMC_MIN_KEEP = 20;                            // the Geweke windows need it
constexpr int MCMC_MAX_POOLED = 8192;                        // n_chains * n_keep: the pooled draws are sorted in LDS
constexpr int MCMC_MAX_ORDER = 36;                           // floor(10 log10(4096)): n_keep <= 8192 / 2
constexpr int MCMC_CHAIN_FIELDS = 9, MCMC_POOLED_FIELDS = 7;
constexpr int MCMC_FAR_LAG = 50;                             // coda's autocorr lags are 1, 5, 10, 50: the only one beyond the AR fit's

// A window of a series: the draws lo .. lo + m - 1 and the largest AR order P = min(m - 1, floor(10 log10 m)) fitted on it.
struct McmcWindow { int32_t lo, m, P; };
enum { MCMC_FULL = 0, MCMC_GEWEKE_A = 1, MCMC_GEWEKE_B = 2 };

// floor(10 log10 m) in integers: the largest p with 10^p <= m^10 (m <= 4096: both sides stay below 2^120)
inline int mcmc_max_order(int m) {
    unsigned __int128 m10 = 1, pw = 1;
    for (int i = 0; i < 10; ++i) m10 *= (unsigned)m;
    int p = 0;
    while (pw * 10 <= m10) { pw *= 10; ++p; }
    return p < m - 1 ? p : m - 1;
}

// the three windows of a series of n draws: all of it, t in [0, ceil((n - 1) / 10)], t in [floor((n - 1) / 2), n - 1]
inline void mcmc_windows(int n, McmcWindow w[3]) {
    const int a_end = (n - 1 + 9) / 10, b_lo = (n - 1) / 2;
    w[MCMC_FULL] = McmcWindow{0, n, mcmc_max_order(n)};
    w[MCMC_GEWEKE_A] = McmcWindow{0, a_end + 1, mcmc_max_order(a_end + 1)};
    w[MCMC_GEWEKE_B] = McmcWindow{b_lo, n - b_lo, mcmc_max_order(n - b_lo)};
}

MCMC_HD inline double mcmc_nan() { return __builtin_nan(""); }

// s = 0; for t in order: s = s + x[lo + t]; s / m
MCMC_HD inline double mcmc_mean(const double *x, int lo, int m) {
    double s = 0.0;
    for (int t = 0; t < m; ++t) s = s + x[lo + t];
    return s / (double)m;
}

// s = 0; for t = 0 .. m - lag - 1: s = s + (x[lo + t] - mean) * (x[lo + t + lag] - mean).  lag >= m: the empty sum.
MCMC_HD inline double mcmc_cross_sum(const double *x, int lo, int m, double mean, int lag) {
    double s = 0.0;
    for (int t = 0; t + lag < m; ++t) s = s + (x[lo + t] - mean) * (x[lo + t + lag] - mean);
    return s;
}

// Yule-Walker fits of the orders 0 .. P by Levinson-Durbin on the autocovariances c[0 .. P] of a window of m draws, the order with
// the smallest m log_lib(v_p) + 2 p (the first on ties), and spec0 = (v_p m / (m - (p + 1))) / (1 - sum phi)^2 of that order.
// phi[0 .. P] is work space; the coefficients of an order are updated in place, pair by pair (every one is still ONE rounded
// a - k * b of the previous order's values).  c[0] == 0 (a constant window): spec0 = 0, order 0, nothing fitted.  c[0] NaN: NaN.
template <class LogF>
MCMC_HD inline void mcmc_ar_spec0(const double *c, int P, int m, double *phi, LogF log_lib, double *spec0, double *order) {
    const double c0 = c[0];
    if (!(c0 > 0.0)) {
        *spec0 = *order = c0 == 0.0 ? 0.0 : mcmc_nan();
        return;
    }
    const double md = (double)m;
    double v = c0;
    int best = 0;
    double best_crit = md * log_lib(v) + 0.0, best_v = v, best_sum = 0.0;
    for (int p = 1; p <= P; ++p) {
        double acc = c[p];
        for (int j = 1; j < p; ++j) acc = acc - phi[j] * c[p - j];
        const double k = acc / v;
        for (int j = 1; 2 * j < p; ++j) {
            const double a = phi[j], b = phi[p - j];
            phi[j] = a - k * b;
            phi[p - j] = b - k * a;
        }
        if ((p & 1) == 0) {
            const double a = phi[p >> 1];
            phi[p >> 1] = a - k * a;
        }
        phi[p] = k;
        v = v * (1.0 - k * k);
        const double crit = md * log_lib(v) + 2.0 * (double)p;
        if (crit < best_crit) {
            double sum = 0.0;
            for (int j = 1; j <= p; ++j) sum = sum + phi[j];
            best = p; best_crit = crit; best_v = v; best_sum = sum;
        }
    }
    const double var_pred = (best_v * md) / (md - (double)(best + 1));
    const double d = 1.0 - best_sum;
    *spec0 = var_pred / (d * d);
    *order = (double)best;
}

MCMC_HD inline double mcmc_geweke(double mean_a, double spec_a, int m_a, double mean_b, double spec_b, int m_b) {
    return (mean_a - mean_b) / sqrt(spec_a / (double)m_a + spec_b / (double)m_b);
}

// Gelman-Rubin's point estimate with coda's degrees-of-freedom adjustment from the m chain means and variances of n draws each
MCMC_HD inline double mcmc_psrf(const double *mean, const double *var, int m, int n) {
    const double md = (double)m, nd = (double)n, m1 = md - 1.0, n1 = nd - 1.0;
    double s = 0.0;
    for (int i = 0; i < m; ++i) s = s + var[i];
    const double W = s / md;
    if (!(W > 0.0)) return mcmc_nan();
    s = 0.0;
    for (int i = 0; i < m; ++i) s = s + mean[i];
    const double mu = s / md;
    s = 0.0;
    for (int i = 0; i < m; ++i) { const double d = mean[i] - mu; s = s + d * d; }
    const double B = nd * (s / m1);
    s = 0.0;
    for (int i = 0; i < m; ++i) { const double d = var[i] - W; s = s + d * d; }
    const double var_w = (s / m1) / md;
    const double var_b = (2.0 * (B * B)) / m1;
    s = 0.0;
    for (int i = 0; i < m; ++i) s = s + mean[i] * mean[i];
    const double q = s / md;
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < m; ++i) {
        const double dv = var[i] - W;
        s1 = s1 + dv * (mean[i] * mean[i] - q);
        s2 = s2 + dv * (mean[i] - mu);
    }
    const double cov_wb = (nd / md) * (s1 / m1 - (2.0 * mu) * (s2 / m1));
    const double f = 1.0 + 1.0 / md;
    const double V = (n1 * W) / nd + (f * B) / nd;
    const double var_V = (((n1 * n1) * var_w + (f * f) * var_b) + ((2.0 * n1) * f) * cov_wb) / (nd * nd);
    const double df = (2.0 * (V * V)) / var_V;
    const double adj = (df + 3.0) / (df + 1.0);
    const double R2 = n1 / nd + (f * (1.0 / nd)) * (B / W);
    return sqrt(adj * R2);
}

// sum over the chains of (n var) / spec0; a chain with spec0 == 0 contributes 0
MCMC_HD inline double mcmc_ess(const double *var, const double *spec0, int m, int n) {
    double s = 0.0;
    for (int i = 0; i < m; ++i) s = s + (spec0[i] == 0.0 ? 0.0 : ((double)n * var[i]) / spec0[i]);
    return s;
}

// quantile(, type = 7) of N ascending values in the operation order of icnv_quantiles_excluding (K17)
MCMC_HD inline double mcmc_quantile7(const double *sorted, int N, double p) {
    const double index = (double)(N - 1) * p;
    const double lo = floor(index), hi = ceil(index);
    const double xl = sorted[(int)lo], xh = sorted[(int)hi];
    if (index == lo || xh == xl) return xl;
    const double h = index - lo;
    return (1.0 - h) * xl + h * xh;
}

// One chain's nine fields from its n draws x[0 .. n - 1], sequentially: what a chain's wavefront computes lane by lane.
// c, phi: work space of MCMC_MAX_ORDER + 1 doubles each.
template <class LogF>
MCMC_HD inline void mcmc_chain_stats(const double *x, int n, const McmcWindow *w, LogF log_lib, double *c, double *phi, double *out) {
    double mean[3], spec[3], order[3], c0_full = 0.0, acf[3] = {0.0, 0.0, 0.0}, var = 0.0;
    for (int q = 0; q < 3; ++q) {
        mean[q] = mcmc_mean(x, w[q].lo, w[q].m);
        for (int l = 0; l <= w[q].P; ++l) c[l] = mcmc_cross_sum(x, w[q].lo, w[q].m, mean[q], l) / (double)w[q].m;
        if (q == MCMC_FULL) {
            var = mcmc_cross_sum(x, 0, n, mean[q], 0) / (double)(n - 1);
            c0_full = c[0];
            acf[0] = c[1] / c[0];
            acf[1] = c[5] / c[0];
            acf[2] = c[10] / c[0];
        }
        mcmc_ar_spec0(c, w[q].P, w[q].m, phi, log_lib, &spec[q], &order[q]);
    }
    out[0] = mean[MCMC_FULL];
    out[1] = var;
    out[2] = spec[MCMC_FULL];
    out[3] = order[MCMC_FULL];
    out[4] = mcmc_geweke(mean[MCMC_GEWEKE_A], spec[MCMC_GEWEKE_A], w[MCMC_GEWEKE_A].m, mean[MCMC_GEWEKE_B], spec[MCMC_GEWEKE_B],
                         w[MCMC_GEWEKE_B].m);
    out[5] = acf[0];
    out[6] = acf[1];
    out[7] = acf[2];
    out[8] = MCMC_FAR_LAG < n ? (mcmc_cross_sum(x, 0, n, mean[MCMC_FULL], MCMC_FAR_LAG) / (double)n) / c0_full : mcmc_nan();
}

// The seven pooled fields of one (region, state) from its chains' fields and the pooled draws: x[ch * n + t] in (chain, t) order,
// sorted[0 .. m n - 1] the same values ascending with -0.0 as +0.0 (read only when no draw is NaN).
MCMC_HD inline void mcmc_pooled_stats(const double *x, const double *sorted, bool any_nan, const double *chain_stats, int m, int n,
                                      double *out) {
    const int N = m * n;
    double mean[MCMC_MAX_CHAINS], var[MCMC_MAX_CHAINS], spec[MCMC_MAX_CHAINS];
    for (int ch = 0; ch < m; ++ch) {
        mean[ch] = chain_stats[ch * MCMC_CHAIN_FIELDS + 0];
        var[ch] = chain_stats[ch * MCMC_CHAIN_FIELDS + 1];
        spec[ch] = chain_stats[ch * MCMC_CHAIN_FIELDS + 2];
    }
    const double pm = mcmc_mean(x, 0, N);
    out[0] = pm;
    out[1] = sqrt(mcmc_cross_sum(x, 0, N, pm, 0) / (double)(N - 1));
    out[2] = any_nan ? mcmc_nan() : mcmc_quantile7(sorted, N, 0.025);
    out[3] = any_nan ? mcmc_nan() : mcmc_quantile7(sorted, N, 0.5);
    out[4] = any_nan ? mcmc_nan() : mcmc_quantile7(sorted, N, 0.975);
    out[5] = mcmc_psrf(mean, var, m, n);
    out[6] = mcmc_ess(var, spec, m, n);
}

#if defined(__HIPCC__)
// The LDS sort of the pooled draws, shared by the diagnostics (K31) and the box statistics (K33): buf[0 .. N - 1] become
// ascending with -0.0 as +0.0, buf[N .. n_pad - 1] (n_pad a power of two >= N) +inf.  Bitonic, in place; every thread of the
// workgroup calls it (tid of nt), after a barrier that made buf visible; it ends on a barrier.  No draw may be NaN.
__device__ inline void mcmc_lds_sort(double *buf, int N, int n_pad, int tid, int nt) {
    for (int q = tid; q < n_pad; q += nt) {
        if (q >= N) buf[q] = __builtin_inf();
        else if (buf[q] == 0.0) buf[q] = 0.0;
    }
    __syncthreads();
    for (int kk = 2; kk <= n_pad; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < (n_pad >> 1); p += nt) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i | j;
                const double u = buf[i], v = buf[l];
                if (((i & kk) == 0) ? (u > v) : (u < v)) { buf[i] = v; buf[l] = u; }
            }
            __syncthreads();
        }
}

struct McmcDiagArgs {
    const double *samples;     // [n_regions, n_chains, n_keep, K]
    double *chain_stats;       // [n_regions, K, n_chains, 9]
    double *pooled;            // [n_regions, K, 7]
    int32_t n_regions, K, n_chains, n_keep;
    int32_t n_pad;             // n_chains * n_keep rounded up to a power of two: the sorted length
    McmcWindow win[3];
};
size_t mcmc_diag_lds_bytes(int32_t n_chains, int32_t n_pad);
int launch_mcmc_diag(const McmcDiagArgs &a, hipStream_t s);
#endif

}  // namespace icnv
