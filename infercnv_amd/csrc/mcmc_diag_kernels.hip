// K31: convergence diagnostics of the Bayesian filter's chains for every (region, state) of a batch at once.  DESIGN.md
// section 4 K31; the contract is in include/icnv.h and restated in tests/mcmc_diag_restate.py.
//
//   mcmc_diag_kernel   one workgroup per (region, state), n_chains + 1 wavefronts.  The state's n_chains series are gathered from
//                      the strided samples into LDS ([chain][t], 48 KB at the defaults).  Wavefront ch serves chain ch: three
//                      lanes take the means of the three windows (the whole series and Geweke's two), then a lane per
//                      (window, lag) takes one autocovariance -- ONE lane's sequential sum, so the result does not depend on how
//                      the lags are dealt to lanes --, then three lanes run Levinson-Durbin, one per window.  The last wavefront's
//                      first lane takes the pooled mean and sd, sequential in (chain, t) order, beside them: with 6 000 draws it
//                      is the longest chain of additions in the workgroup.  Then the pooled draws are sorted in place (bitonic,
//                      padded with +inf to a power of two) for the quantiles, and one lane forms psrf and ess.
// The arithmetic is the __host__ __device__ code of mcmc_diag_internal.h.  Every load is bounded by the series' own range; the
// sizes are refused on the host (mcmc_diag_api.hip) before any launch.
// Every value is an individually rounded IEEE-754 double operation in the documented order: -ffp-contract=off.
#include "icnv_internal.h"
#include "lib_math.h"
#include "mcmc_diag_internal.h"

#pragma clang fp contract(off)

namespace icnv {

namespace {

constexpr int MCMC_NT_MAX = (MCMC_MAX_CHAINS + 1) * 64;
constexpr int MCMC_LAGS = MCMC_MAX_ORDER + 1;
// a chain's work space in LDS, in doubles
constexpr int W_C = 0, W_PHI = 3 * MCMC_LAGS, W_MEAN = 6 * MCMC_LAGS, W_SPEC = W_MEAN + 3, W_ORD = W_SPEC + 3, W_VAR = W_ORD + 1,
              W_FAR = W_VAR + 1, MCMC_WORK = (W_FAR + 1 + 1) & ~1;
// the workgroup's: pooled mean and sd, the chains' nine fields
constexpr int S_POOL = 0, S_CHAIN = 2, MCMC_COMMON = S_CHAIN + MCMC_MAX_CHAINS * MCMC_CHAIN_FIELDS + 2;
static_assert(3 * MCMC_LAGS + 1 <= 128, "a chain's (window, lag) tasks take at most two rounds of its wavefront");
static_assert(MCMC_WORK % 2 == 0 && MCMC_COMMON % 2 == 0, "the carve offsets stay 16-byte aligned");

struct LibLog {
    __device__ double operator()(double x) const { return lib_log(x); }
};

__global__ void __launch_bounds__(MCMC_NT_MAX) mcmc_diag_kernel(McmcDiagArgs a) {
    extern __shared__ __attribute__((aligned(16))) double mcmc_lds[];
    const int m = a.n_chains, n = a.n_keep, N = m * n, K = a.K;
    double *buf = mcmc_lds;                               // [n_pad]: the draws in (chain, t) order, later sorted
    double *common = buf + a.n_pad;
    const int r = blockIdx.x / K, k = blockIdx.x - r * K;
    const int tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, lane = tid & 63;
    const bool chain_wave = wave < m;
    double *w = common + MCMC_COMMON + (chain_wave ? wave : 0) * MCMC_WORK;
    const double *x = buf + (chain_wave ? wave : 0) * n;
    const auto window = [&](int q) {
        return q == MCMC_FULL ? a.win[MCMC_FULL] : (q == MCMC_GEWEKE_A ? a.win[MCMC_GEWEKE_A] : a.win[MCMC_GEWEKE_B]);
    };

    const double *src = a.samples + (int64_t)r * N * K + k;
    int nan = 0;
    for (int q = tid; q < N; q += nt) {
        const double v = src[(int64_t)q * K];
        buf[q] = v;
        nan |= v != v;
    }
    const bool any_nan = __syncthreads_or(nan) != 0;

    // the means: a lane per window; the pooled mean beside them
    if (chain_wave) {
        if (lane < 3) {
            const McmcWindow ww = window(lane);
            w[W_MEAN + lane] = mcmc_mean(x, ww.lo, ww.m);
        }
    } else if (lane == 0) {
        common[S_POOL] = mcmc_mean(buf, 0, N);
    }
    __syncthreads();

    // the autocovariances: a lane per (window, lag), the longest windows first; the pooled sum of squares beside them
    if (chain_wave) {
        const int P0 = a.win[MCMC_FULL].P, PA = a.win[MCMC_GEWEKE_A].P, PB = a.win[MCMC_GEWEKE_B].P;
        const int n_tasks = P0 + PB + PA + 4;
        for (int q = lane; q < n_tasks; q += 64) {
            const bool far = q == P0 + 1;
            int win, lag;
            if (q <= P0) { win = MCMC_FULL; lag = q; }
            else if (far) { win = MCMC_FULL; lag = MCMC_FAR_LAG; }
            else if (q <= P0 + 2 + PB) { win = MCMC_GEWEKE_B; lag = q - P0 - 2; }
            else { win = MCMC_GEWEKE_A; lag = q - P0 - PB - 3; }
            const McmcWindow ww = window(win);
            const double s = mcmc_cross_sum(x, ww.lo, ww.m, w[W_MEAN + win], lag);
            if (far) {
                w[W_FAR] = s / (double)n;
            } else {
                w[W_C + win * MCMC_LAGS + lag] = s / (double)ww.m;
                if (q == 0) w[W_VAR] = s / (double)(n - 1);
            }
        }
    } else if (lane == 0) {
        common[S_POOL + 1] = sqrt(mcmc_cross_sum(buf, 0, N, common[S_POOL], 0) / (double)(N - 1));
    }
    __syncthreads();

    // the AR fits: a lane per window
    if (chain_wave && lane < 3) {
        const McmcWindow ww = window(lane);
        double order;
        mcmc_ar_spec0(w + W_C + lane * MCMC_LAGS, ww.P, ww.m, w + W_PHI + lane * MCMC_LAGS, LibLog{}, &w[W_SPEC + lane], &order);
        if (lane == MCMC_FULL) w[W_ORD] = order;
    }
    __syncthreads();

    if (chain_wave && lane == 0) {
        double *cs = common + S_CHAIN + wave * MCMC_CHAIN_FIELDS;
        const double c0 = w[W_C];
        cs[0] = w[W_MEAN + MCMC_FULL];
        cs[1] = w[W_VAR];
        cs[2] = w[W_SPEC + MCMC_FULL];
        cs[3] = w[W_ORD];
        cs[4] = mcmc_geweke(w[W_MEAN + MCMC_GEWEKE_A], w[W_SPEC + MCMC_GEWEKE_A], a.win[MCMC_GEWEKE_A].m, w[W_MEAN + MCMC_GEWEKE_B],
                            w[W_SPEC + MCMC_GEWEKE_B], a.win[MCMC_GEWEKE_B].m);
        cs[5] = w[W_C + 1] / c0;
        cs[6] = w[W_C + 5] / c0;
        cs[7] = w[W_C + 10] / c0;
        cs[8] = MCMC_FAR_LAG < n ? w[W_FAR] / c0 : mcmc_nan();
        double *out = a.chain_stats + (((int64_t)r * K + k) * m + wave) * MCMC_CHAIN_FIELDS;
        for (int i = 0; i < MCMC_CHAIN_FIELDS; ++i) out[i] = cs[i];
    }

    // the pooled draws ascending, -0.0 as +0.0 (a NaN among them: no order, the quantiles are NaN)
    if (!any_nan) {
        mcmc_lds_sort(buf, N, a.n_pad, tid, nt);
    } else {
        __syncthreads();
    }

    if (tid == 0) {
        double mean[MCMC_MAX_CHAINS], var[MCMC_MAX_CHAINS], spec[MCMC_MAX_CHAINS];
#pragma unroll
        for (int ch = 0; ch < MCMC_MAX_CHAINS; ++ch) {
            const double *cs = common + S_CHAIN + (ch < m ? ch : 0) * MCMC_CHAIN_FIELDS;
            mean[ch] = cs[0]; var[ch] = cs[1]; spec[ch] = cs[2];
        }
        double *out = a.pooled + ((int64_t)r * K + k) * MCMC_POOLED_FIELDS;
        out[0] = common[S_POOL];
        out[1] = common[S_POOL + 1];
        out[2] = any_nan ? mcmc_nan() : mcmc_quantile7(buf, N, 0.025);
        out[3] = any_nan ? mcmc_nan() : mcmc_quantile7(buf, N, 0.5);
        out[4] = any_nan ? mcmc_nan() : mcmc_quantile7(buf, N, 0.975);
        out[5] = mcmc_psrf(mean, var, m, n);
        out[6] = mcmc_ess(var, spec, m, n);
    }
}

}  // namespace

size_t mcmc_diag_lds_bytes(int32_t n_chains, int32_t n_pad) {
    return ((size_t)n_pad + MCMC_COMMON + (size_t)n_chains * MCMC_WORK) * sizeof(double);
}

int launch_mcmc_diag(const McmcDiagArgs &a, hipStream_t s) {
    KernelTimer kt("mcmc_diag", s);
    static DeviceOnce once;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(mcmc_diag_kernel),
                                    (int)mcmc_diag_lds_bytes(MCMC_MAX_CHAINS, MCMC_MAX_POOLED), once))
        return rc;
    const int64_t grid = (int64_t)a.n_regions * a.K;
    hipLaunchKernelGGL(mcmc_diag_kernel, dim3((unsigned)grid), dim3((unsigned)((a.n_chains + 1) * 64)),
                       mcmc_diag_lds_bytes(a.n_chains, a.n_pad), s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
