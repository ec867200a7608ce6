// K15: the hidden spike-in of the i6 HMM (.build_and_add_hspike, R/inferCNV_hidden_spike.R:3-165).  DESIGN.md section 4 K15;
// the contract is in include/icnv.h and restated in tests/hspike_restate.py.
//
// group gene tables (.get_mean_var_table / .get_mean_vs_p0_table), one lane per gene, one workgroup per (chunk of <= HS_CHUNK
// cells of one group, 256 genes):
//   hs_sum_kernel    double-double sum, plain sum and zero count of the chunk        (first read of the group's cells)
//   hs_mean_kernel   per (group, gene): the chunks in order, mean = (hi + lo) / n correctly rounded, nzero
//   hs_ss_kernel     double-double sum of round(round(x - mean)^2) of the chunk      (second read)
//   hs_var_kernel    per (group, gene): var = round(hi + lo) / (n - 1)
// simulation (.get_simulated_cell_matrix_using_meanvar_trend_helper + .apply_dropout): hs_simulate_kernel, one lane per gene
// row, one wavefront per workgroup, grid (gene blocks x matrices); pass 1 writes the values, pass 2 re-reads the lane's own
// values and applies the dropout.
// Every value is an individually rounded IEEE-754 double operation in the documented order: -ffp-contract=off.
#include <algorithm>

#include "icnv_internal.h"
#include "lib_math.h"
#include "random_trees_internal.h"
#include "hspike_internal.h"
#include "../../include/icnv.h"

#pragma clang fp contract(off)

namespace icnv {

namespace {

__device__ inline void dd_add(double &hi, double &lo, double x) {
    const double s = hi + x;
    const double bb = s - hi;
    lo += (hi - (s - bb)) + (x - bb);
    hi = s;
}
// (hi + lo) / n, correctly rounded (viterbi_kernels.hip group_means_finish_kernel, de_kernels.hip dd_div)
__device__ inline double dd_div(double hi, double lo, double n) {
    const double s = hi + lo;
    const double e = lo - (s - hi);
    const double q0 = s / n;
    const double r = __builtin_fma(-q0, n, s);
    return q0 + (r + e) / n;
}

__global__ void __launch_bounds__(256) hs_sum_kernel(HsTables a) {
    const int64_t tiles = (a.G + 255) / 256;
    const int64_t ch = blockIdx.x / tiles;
    const int64_t g = (blockIdx.x - ch * tiles) * 256 + threadIdx.x;
    if (g >= a.G) return;
    const HsChunk c = a.chunks[ch];
    const int32_t *idx = a.cell_idx;
    const double *x = a.x + g;
    // two interleaved double-double accumulators, four loads in flight: each chain stays sequential
    double h0 = 0.0, l0 = 0.0, h1 = 0.0, l1 = 0.0, p0 = 0.0, p1 = 0.0;
    int nz = 0;
    int64_t i = c.begin;
    for (; i + 4 <= c.end; i += 4) {
        const double v0 = x[(int64_t)idx[i] * a.ld], v1 = x[(int64_t)idx[i + 1] * a.ld];
        const double v2 = x[(int64_t)idx[i + 2] * a.ld], v3 = x[(int64_t)idx[i + 3] * a.ld];
        dd_add(h0, l0, v0); dd_add(h1, l1, v1);
        dd_add(h0, l0, v2); dd_add(h1, l1, v3);
        p0 += v0 + v2; p1 += v1 + v3;
        nz += (v0 == 0.0) + (v1 == 0.0) + (v2 == 0.0) + (v3 == 0.0);
    }
    for (; i < c.end; ++i) {
        const double v0 = x[(int64_t)idx[i] * a.ld];
        dd_add(h0, l0, v0);
        p0 += v0;
        nz += v0 == 0.0;
    }
    dd_add(h0, l0, h1);
    l0 += l1;
    double *dst = a.part + ch * 3 * a.G + g;
    dst[0] = h0;
    dst[a.G] = l0;
    dst[2 * (int64_t)a.G] = p0 + p1;
    a.part_nz[ch * a.G + g] = nz;
}

__global__ void __launch_bounds__(256) hs_mean_kernel(HsTables a) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.G) return;
    const int q = blockIdx.y;
    double hi = 0.0, lo = 0.0, plain = 0.0;
    int nz = 0;
    for (int64_t ch = a.chunk_off[q]; ch < a.chunk_off[q + 1]; ++ch) {
        const double *src = a.part + ch * 3 * a.G + g;
        dd_add(hi, lo, src[0]);
        lo += src[a.G];
        plain += src[2 * (int64_t)a.G];
        nz += a.part_nz[ch * a.G + g];
    }
    const double n = (double)(a.cell_off[q + 1] - a.cell_off[q]);
    const double m = dd_div(hi, lo, n);
    a.m[(int64_t)q * a.G + g] = (m == m && fabs(m) <= 1.7976931348623157e308) ? m : plain / n;
    a.nzero[(int64_t)q * a.G + g] = nz;
}

__global__ void __launch_bounds__(256) hs_ss_kernel(HsTables a) {
    const int64_t tiles = (a.G + 255) / 256;
    const int64_t ch = blockIdx.x / tiles;
    const int64_t g = (blockIdx.x - ch * tiles) * 256 + threadIdx.x;
    if (g >= a.G) return;
    const HsChunk c = a.chunks[ch];
    const int32_t *idx = a.cell_idx;
    const double *x = a.x + g;
    const double m = a.m[(int64_t)c.q * a.G + g];
    double h0 = 0.0, l0 = 0.0, h1 = 0.0, l1 = 0.0;
    int64_t i = c.begin;
    for (; i + 4 <= c.end; i += 4) {
        const double d0 = x[(int64_t)idx[i] * a.ld] - m, d1 = x[(int64_t)idx[i + 1] * a.ld] - m;
        const double d2 = x[(int64_t)idx[i + 2] * a.ld] - m, d3 = x[(int64_t)idx[i + 3] * a.ld] - m;
        dd_add(h0, l0, d0 * d0); dd_add(h1, l1, d1 * d1);
        dd_add(h0, l0, d2 * d2); dd_add(h1, l1, d3 * d3);
    }
    for (; i < c.end; ++i) {
        const double d0 = x[(int64_t)idx[i] * a.ld] - m;
        dd_add(h0, l0, d0 * d0);
    }
    dd_add(h0, l0, h1);
    l0 += l1;
    double *dst = a.part + ch * 3 * a.G + g;
    dst[0] = h0;
    dst[a.G] = l0;
}

__global__ void __launch_bounds__(256) hs_var_kernel(HsTables a) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.G) return;
    const int q = blockIdx.y;
    double hi = 0.0, lo = 0.0;
    for (int64_t ch = a.chunk_off[q]; ch < a.chunk_off[q + 1]; ++ch) {
        const double *src = a.part + ch * 3 * a.G + g;
        dd_add(hi, lo, src[0]);
        lo += src[a.G];
    }
    const double n = (double)(a.cell_off[q + 1] - a.cell_off[q]);
    a.v[(int64_t)q * a.G + g] = (hi + lo) / (n - 1.0);   // n = 1: 0 / 0 = NaN, as R's var
}

// S(x) of a cubic B-spline on [0, 1] (scaled abscissa), nk coefficients, knots [nk + 4] with knots[0..3] = 0 and
// knots[nk..nk+3] = 1 (include/icnv.h "spline evaluation")
__device__ inline double hs_spline(const HsSpline &s, double x) {
    const double *k = s.knots, *c = s.coef;
    const int nk = s.nk;
    const double t = (x - s.xmin) / s.range;
    if (t < 0.0) return c[0] + ((3.0 * (c[1] - c[0])) / (k[4] - k[3])) * t;
    if (t > 1.0) return c[nk - 1] + ((3.0 * (c[nk - 1] - c[nk - 2])) / (k[nk] - k[nk - 1])) * (t - 1.0);
    int lo = 3, hi = nk;                      // knots[lo] <= t < knots[hi], or t = 1 in the last interval
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (k[mid] <= t) lo = mid; else hi = mid;
    }
    double d0 = c[lo - 3], d1 = c[lo - 2], d2 = c[lo - 1], d3 = c[lo];
    double al;
    // de Boor, r = 1: j = 3, 2, 1
    al = (t - k[lo]) / (k[lo + 3] - k[lo]);          d3 = (1.0 - al) * d2 + al * d3;
    al = (t - k[lo - 1]) / (k[lo + 2] - k[lo - 1]);  d2 = (1.0 - al) * d1 + al * d2;
    al = (t - k[lo - 2]) / (k[lo + 1] - k[lo - 2]);  d1 = (1.0 - al) * d0 + al * d1;
    // r = 2: j = 3, 2
    al = (t - k[lo]) / (k[lo + 2] - k[lo]);          d3 = (1.0 - al) * d2 + al * d3;
    al = (t - k[lo - 1]) / (k[lo + 1] - k[lo - 1]);  d2 = (1.0 - al) * d1 + al * d2;
    // r = 3: j = 3
    al = (t - k[lo]) / (k[lo + 1] - k[lo]);          d3 = (1.0 - al) * d2 + al * d3;
    return d3;
}

__global__ void __launch_bounds__(HS_SIM_BLOCK) hs_simulate_kernel(HsSim a) {
    const int64_t g = (int64_t)blockIdx.x * HS_SIM_BLOCK + threadIdx.x;
    if (g >= a.n_genes) return;
    const int k = blockIdx.y;
    const uint64_t token = a.tokens[k];
    const double m = a.means[(int64_t)k * a.n_genes + g];
    const int n = a.num_cells;
    double *out = a.out + (int64_t)k * n * a.n_genes + g;
    if (!(m > 0.0)) {
        for (int c = 0; c < n; ++c) out[(int64_t)c * a.n_genes] = 0.0;
        return;
    }
    const double logm = lib_log(m + 1.0);
    double var = lib_exp(hs_spline(a.var, logm)) - 1.0;
    var = var > 0.0 ? var : 0.0;
    const double sd = sqrt(var);
    double sum = 0.0;
    int nz = 0;
    for (int c = 0; c < n; ++c) {
        RtPhilox ph(a.seed, token, (uint64_t)g, (uint64_t)c);
        const double u1 = ph.random();
        const double u2 = ph.random();
        const double z = lib_qnorm((floor(134217728.0 * u1) + u2) / 134217728.0);
        double v = m + sd * z;
        v = v > 0.0 ? v : 0.0;
        v = rint(v);
        out[(int64_t)c * a.n_genes] = v;
        sum += v;
        nz += v == 0.0;
    }
    if (nz == n) return;   // an all-zero row stays as it is (R divides by zero there)
    const double nd = (double)n, nzd = (double)nz;
    const double p = hs_spline(a.p0, lib_log(sum / nd));
    const double padj = (p * nd - nzd) / (nd - nzd);
    if (!(padj > 0.0)) return;
    for (int c = 0; c < n; ++c) {
        RtPhilox ph(a.seed, token, (uint64_t)g, (uint64_t)c);
        ph.c0 = 1;         // counter = [1, g, c, 0]
        if (ph.random() <= padj) out[(int64_t)c * a.n_genes] = 0.0;
    }
}

}  // namespace

#define HS_LAUNCH_CHECK() ICNV_HIP(hipGetLastError())

int launch_hs_tables(const HsTables &a, hipStream_t s) {
    const int64_t tiles = (a.G + 255) / 256;
    const dim3 work((unsigned)(tiles * a.n_chunks)), per_group((unsigned)tiles, (unsigned)a.n_grp);
    hipLaunchKernelGGL(hs_sum_kernel, work, dim3(256), 0, s, a);
    HS_LAUNCH_CHECK();
    hipLaunchKernelGGL(hs_mean_kernel, per_group, dim3(256), 0, s, a);
    HS_LAUNCH_CHECK();
    hipLaunchKernelGGL(hs_ss_kernel, work, dim3(256), 0, s, a);
    HS_LAUNCH_CHECK();
    hipLaunchKernelGGL(hs_var_kernel, per_group, dim3(256), 0, s, a);
    HS_LAUNCH_CHECK();
    return ICNV_OK;
}

int launch_hs_simulate(const HsSim &a, hipStream_t s) {
    const dim3 grid((unsigned)((a.n_genes + HS_SIM_BLOCK - 1) / HS_SIM_BLOCK), (unsigned)a.n_mat);
    hipLaunchKernelGGL(hs_simulate_kernel, grid, dim3(HS_SIM_BLOCK), 0, s, a);
    HS_LAUNCH_CHECK();
    return ICNV_OK;
}

}  // namespace icnv
