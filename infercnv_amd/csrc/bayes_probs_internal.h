// K33: the numbers under the Bayesian filter's probability plots (include/icnv.h "Probability heatmaps and tables of the
// Bayesian filter").  The box statistics of one (region, state) are __host__ __device__ code in this header: the kernel
// (bayes_probs_kernels.hip) runs them on the draws it sorted in LDS, the host program bayes_probs_host_check.cpp on std::sort's,
// and both must give the bits of tests/bayes_probs_restate.py.  Every value is an individually rounded IEEE-754 double
// operation: every unit that includes this header is built with -ffp-contract=off.
#pragma once
#include "mcmc_diag_internal.h"

namespace icnv {

constexpr int BOX_FIELDS = 7;                                // ymin, lower, middle, upper, ymax, n_low, n_high

// the first index i of sorted[0 .. N - 1] (ascending, no NaN) with !(sorted[i] < x): #{y < x}.  x NaN: 0.
MCMC_HD inline int box_count_below(const double *sorted, int N, double x) {
    int lo = 0, hi = N;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sorted[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// #{y > x} the same way.  x NaN: 0.
MCMC_HD inline int box_count_above(const double *sorted, int N, double x) {
    int lo = 0, hi = N;                                      // the first index with sorted[i] > x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sorted[mid] > x) hi = mid; else lo = mid + 1;
    }
    return N - lo;
}

// The seven fields from the N pooled draws of one (region, state), ascending with -0.0 as +0.0 (read only when no draw is NaN).
MCMC_HD inline void box_stats(const double *sorted, int N, bool any_nan, double *out) {
    if (any_nan) {
        for (int i = 0; i < BOX_FIELDS; ++i) out[i] = mcmc_nan();
        return;
    }
    const double lower = mcmc_quantile7(sorted, N, 0.25), middle = mcmc_quantile7(sorted, N, 0.5), upper = mcmc_quantile7(sorted, N, 0.75);
    const double iqr = upper - lower;
    const double reach = 1.5 * iqr;
    const double lo = lower - reach, hi = upper + reach;
    const int n_low = box_count_below(sorted, N, lo), n_high = box_count_above(sorted, N, hi);
    const bool none = n_low + n_high >= N;                   // (only with infinite draws: no draw inside the fences)
    out[0] = none ? mcmc_nan() : sorted[n_low];
    out[1] = lower;
    out[2] = middle;
    out[3] = upper;
    out[4] = none ? mcmc_nan() : sorted[N - 1 - n_high];
    out[5] = (double)n_low;
    out[6] = (double)n_high;
}

#if defined(__HIPCC__)
struct ThetaBoxArgs {
    const double *samples;     // [n_regions, n_chains, n_keep, K]
    double *box;               // [n_regions, K, 7]
    int32_t n_regions, K, N;   // N = n_chains * n_keep
    int32_t n_pad;             // N rounded up to a power of two (>= 64): the sorted length
};
int launch_theta_box(const ThetaBoxArgs &a, hipStream_t s);

struct PaintRegions {
    double *out;
    int64_t G, C, ld;
    int32_t n_regions;
    const int32_t *gene_first, *gene_count;
    const int64_t *cell_off;
    const int32_t *cell_idx;
    int64_t n_idx;
    const double *value;
};
// verdict (DEVICE, 4 x int64, zeroed): [0] 0 or the kind of fault, [1] cell_off[n_regions], [2] the longest gene run,
// [3] 1 when some region is not exactly the one cell at its own position
int launch_paint_check(const PaintRegions &a, int64_t *verdict, hipStream_t s);
int launch_paint(const PaintRegions &a, int64_t rows, int64_t longest, bool one_cell, hipStream_t s);
#endif

}  // namespace icnv
