// K13: the mixture model of the HMM-predicted CNV regions (inferCNVBayesNet, R/inferCNV_BayesNet.R:1054-1107) for every
// region of a run at once.  DESIGN.md section 4 K13; the contract is in include/icnv.h and restated in tests/bayes_restate.py.
//
//   bayes_loglik_kernel   per (region, 64 cells): 64-cell x 32-gene tiles of the region's rectangle go through LDS (reads coalesced along
//                         a cell's genes), every (cell, state) keeps ONE sequential sum of squares in gene order; then ll and
//                         L = exp_lib(ll - max ll) per cell
//   bayes_prep_kernel     per region: the cells with exactly one non-zero L (their state never depends on theta) are counted
//                         once, the others listed
//   bayes_sample_kernel   per (region, chain) ONE workgroup runs every iteration: K lanes draw the gammas of theta, the
//                         undecided cells go over the lanes, the only cross-lane work is the K-bin count (LDS atomics on
//                         integers).  L rows, the cell list and the kept-state counts of a region with <= BAYES_LDS_CELLS
//                         undecided cells stay in LDS; larger regions stream them from L2 / HBM.
//   bayes_sample_packed_kernel   regions with <= BAYES_PACKED_CELLS undecided cells (K25, the per-cell reports): an 8-lane
//                         group per (region, chain), eight of them in a wavefront, registers and shuffles only.
// Every draw has its own Philox counter, so nothing depends on which lane or in which order it is taken.
// Every value is an individually rounded IEEE-754 double operation in the documented order: -ffp-contract=off.
#include "icnv_internal.h"
#include "random_trees_internal.h"
#include "lib_math.h"
#include "bayes_internal.h"
#include "../../include/icnv.h"

#pragma clang fp contract(off)

namespace icnv {

namespace {

__device__ inline int find_region(const int64_t *off, int n, int64_t b) {   // off[r] <= b < off[r + 1]
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (off[m] <= b) lo = m; else hi = m;
    }
    return lo;
}

constexpr int LL_CELLS = 64, LL_GENES = 32;   // one tile: 17 KiB of LDS, so eight workgroups share a CU and one's loads overlap another's sums

__global__ void __launch_bounds__(256) bayes_loglik_kernel(BayesLoglik a) {
    __shared__ double tile[LL_CELLS][LL_GENES + 1];
    __shared__ double s_ll[LL_CELLS][BAYES_MAX_K];
    const int64_t b = blockIdx.x;
    const int r = find_region(a.tile_off, a.n_regions, b);
    const BayesRegion reg = a.regions[r];
    const int64_t ct = b - a.tile_off[r];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;          // second phase: cell tx, states ty and ty + 4
    const int lx = threadIdx.x & (LL_GENES - 1), ly = threadIdx.x / LL_GENES;   // load phase: gene lx of the cells ly, ly + 8, ..
    const int K = a.K;
    const int k0 = ty, k1 = ty + 4;
    const double mu0 = k0 < K ? a.mu_tau[k0] : 0.0, mu1 = k1 < K ? a.mu_tau[k1] : 0.0;
    const int64_t i = ct * LL_CELLS + tx;
    double acc0 = 0.0, acc1 = 0.0;
    for (int64_t g = 0; g < reg.ng; g += LL_GENES) {
        for (int rr = ly; rr < LL_CELLS; rr += 256 / LL_GENES) {
            const int64_t ii = ct * LL_CELLS + rr, j = g + lx;
            double v = 0.0;
            if (ii < reg.n_cells && j < reg.ng) v = a.x[(int64_t)a.cell_idx[reg.row0 + ii] * a.ld + reg.g0 + j];
            tile[rr][lx] = v;
        }
        __syncthreads();
        const int nj = (int)min((int64_t)LL_GENES, (int64_t)reg.ng - g);
        if (i < reg.n_cells) {
            for (int j = 0; j < nj; ++j) {
                const double v = tile[tx][j];
                const double d0 = v - mu0, d1 = v - mu1;
                acc0 = acc0 + d0 * d0;
                acc1 = acc1 + d1 * d1;
            }
        }
        __syncthreads();
    }
    const double hl = (double)reg.ng * 0.5;
    if (k0 < K) { const double t = a.mu_tau[K + k0]; s_ll[tx][k0] = hl * lib_log(t) - (t * 0.5) * acc0; }
    if (k1 < K) { const double t = a.mu_tau[K + k1]; s_ll[tx][k1] = hl * lib_log(t) - (t * 0.5) * acc1; }
    __syncthreads();
    if (ty == 0 && i < reg.n_cells) {
        double m = s_ll[tx][0];
        for (int k = 1; k < K; ++k) if (s_ll[tx][k] > m) m = s_ll[tx][k];
        double *ll = a.ll + (reg.row0 + i) * K, *L = a.L + (reg.row0 + i) * K;
        for (int k = 0; k < K; ++k) {
            const double v = s_ll[tx][k];
            ll[k] = v;
            L[k] = lib_exp(v - m);
        }
    }
}

__global__ void __launch_bounds__(64) bayes_prep_kernel(const double *L, const BayesRegion *regions, int K, int skip_decided, int n_keep,
                                                        int32_t *und, int32_t *n_und, int32_t *nfix, int32_t *freq) {
    __shared__ int s_fix[BAYES_MAX_K];
    const int r = blockIdx.x, lane = threadIdx.x;
    const BayesRegion reg = regions[r];
    if (lane < BAYES_MAX_K) s_fix[lane] = 0;
    __syncthreads();
    int base = 0;
    for (int c0 = 0; c0 < reg.n_cells; c0 += 64) {
        const int i = c0 + lane;
        bool u = false;
        if (i < reg.n_cells) {
            const double *row = L + (reg.row0 + i) * K;
            int nz = 0, kk = 0;
            for (int k = 0; k < K; ++k) if (row[k] > 0.0) { ++nz; kk = k; }
            if (skip_decided && nz == 1) {
                atomicAdd(&s_fix[kk], 1);
                freq[(reg.row0 + i) * K + kk] = K * n_keep;
            } else {
                u = true;
            }
        }
        const unsigned long long mask = __ballot(u);
        if (u) und[reg.row0 + base + __popcll(mask & ((1ull << lane) - 1ull))] = i;
        base += __popcll(mask);
    }
    __syncthreads();
    if (lane == 0) n_und[r] = base;
    if (lane < BAYES_MAX_K) nfix[r * BAYES_MAX_K + lane] = s_fix[lane];
}

// Gamma(shape, 1), shape >= 1, by Marsaglia and Tsang: attempt j of (chain, iteration, state) has its own stream
__device__ inline double bayes_gamma(double shape, uint64_t seed, uint64_t token, int k, int64_t t, int chain) {
    const double d = shape - 1.0 / 3.0;
    const double c = 1.0 / sqrt(9.0 * d);
    for (int att = 0; att < ICNV_BAYES_GAMMA_ATTEMPTS; ++att) {
        RtPhilox ph(seed, token, (uint64_t)k, (uint64_t)t, ((uint64_t)chain << 40) | (1ull << 32) | (uint64_t)att);
        const double u1 = ph.random();
        const double u2 = ph.random();
        if (u1 == 0.0) continue;
        const double x = lib_qnorm(u1);
        double v = 1.0 + c * x;
        if (!(v > 0.0)) continue;
        v = (v * v) * v;
        const double x2 = x * x;
        if (u2 < 1.0 - 0.0331 * (x2 * x2)) return d * v;
        if (lib_log(u2) < 0.5 * x2 + d * ((1.0 - v) + lib_log(v))) return d * v;
    }
    return d;
}

// eps of one cell: the first k with cum[k] > u cum[K-1], else the last k with w[k] > 0, else the last with L[k] > 0, else 0
__device__ inline int bayes_select(const double (&theta)[BAYES_MAX_K], const double *row, int K, double u) {
    double cums[BAYES_MAX_K];
    double cum = 0.0;
    int last_w = -1, last_l = -1;
#pragma unroll
    for (int k = 0; k < BAYES_MAX_K; ++k) {
        if (k < K) {
            const double l = row[k];
            const double w = theta[k] * l;
            cum = cum + w;
            if (w > 0.0) last_w = k;
            if (l > 0.0) last_l = k;
        }
        cums[k] = cum;
    }
    const double thr = u * cum;
    int sel = -1;
#pragma unroll
    for (int k = BAYES_MAX_K - 1; k >= 0; --k) if (k < K && cums[k] > thr) sel = k;
    if (sel < 0) sel = last_w >= 0 ? last_w : (last_l >= 0 ? last_l : 0);
    return sel;
}

template <bool LDS>
__global__ void __launch_bounds__(BAYES_THREADS) bayes_sample_kernel(BayesSample a, int lds_cells) {
    extern __shared__ double dyn[];
    __shared__ double s_g[BAYES_MAX_K];
    __shared__ int s_n[2][BAYES_MAX_K];
    const int K = a.K;
    const int r = a.list[blockIdx.x / K], ch = blockIdx.x % K;
    const BayesRegion reg = a.regions[r];
    const int tid = threadIdx.x;
    const int n = reg.n_cells;
    double *tsum_out = a.theta_sum + ((int64_t)r * K + ch) * K;
    double *samp = a.theta_samples ? a.theta_samples + ((int64_t)r * K + ch) * (int64_t)a.n_keep * K : nullptr;
    if (n == 0) {                                         // no cells: NaN theta, nothing sampled
        if (tid < K) tsum_out[tid] = __builtin_nan("");
        if (samp) for (int64_t q = tid; q < (int64_t)a.n_keep * K; q += BAYES_THREADS) samp[q] = __builtin_nan("");
        return;
    }
    const int nu = a.n_und[r];
    const int32_t *und = a.und + reg.row0;
    const double *Lg = a.L + reg.row0 * K;
    int32_t *freq = a.freq + reg.row0 * K;
    double *sL = dyn;                                     // [lds_cells x K]
    int *sF = (int *)(dyn + (size_t)lds_cells * K);       // [lds_cells x K]
    int *sI = sF + (size_t)lds_cells * K;                 // [lds_cells]
    if (LDS) {
        for (int q = tid; q < nu * K; q += BAYES_THREADS) {
            const int j = q / K, k = q - j * K;
            sL[q] = Lg[(int64_t)und[j] * K + k];
            sF[q] = 0;
        }
        for (int j = tid; j < nu; j += BAYES_THREADS) sI[j] = und[j];
    }
    if (tid < K) s_n[0][tid] = tid == ch ? n : 0;         // the chain starts from eps == ch
    __syncthreads();
    double tsum = 0.0;
    const int64_t T = (int64_t)a.n_discard + a.n_keep;
    for (int64_t t = 0; t < T; ++t) {
        const int cur = (int)(t & 1), nxt = cur ^ 1;
        if (tid < K) {
            s_g[tid] = bayes_gamma(1.0 + (double)s_n[cur][tid], a.seed, reg.token, tid, t, ch);
            s_n[nxt][tid] = a.nfix[r * BAYES_MAX_K + tid];
        }
        __syncthreads();
        double S = 0.0;
        for (int k = 0; k < K; ++k) S = S + s_g[k];
        double theta[BAYES_MAX_K];
#pragma unroll
        for (int k = 0; k < BAYES_MAX_K; ++k) theta[k] = k < K ? s_g[k] / S : 0.0;
        const bool keep = t >= a.n_discard;
        if (keep && tid < K) {
            const double th = s_g[tid] / S;
            tsum = tsum + th;
            if (samp) samp[(t - a.n_discard) * K + tid] = th;
        }
        int cnt[BAYES_MAX_K];
#pragma unroll
        for (int k = 0; k < BAYES_MAX_K; ++k) cnt[k] = 0;
        for (int j = tid; j < nu; j += BAYES_THREADS) {
            const int i = LDS ? sI[j] : und[j];
            const double *row = LDS ? sL + (size_t)j * K : Lg + (int64_t)i * K;
            RtPhilox ph(a.seed, reg.token, (uint64_t)i, (uint64_t)t, (uint64_t)ch << 40);
            const double u = ph.random();
            const int sel = bayes_select(theta, row, K, u);
#pragma unroll
            for (int k = 0; k < BAYES_MAX_K; ++k) cnt[k] += sel == k;
            if (keep) {
                if (LDS) sF[(size_t)j * K + sel] += 1;    // a cell belongs to one lane
                else atomicAdd(&freq[(int64_t)i * K + sel], 1);
            }
        }
#pragma unroll
        for (int k = 0; k < BAYES_MAX_K; ++k) if (cnt[k]) atomicAdd(&s_n[nxt][k], cnt[k]);
        __syncthreads();
    }
    if (tid < K) tsum_out[tid] = tsum;
    if (LDS) {
        for (int q = tid; q < nu * K; q += BAYES_THREADS) {
            const int j = q / K, k = q - j * K;
            if (sF[q]) atomicAdd(&freq[(int64_t)sI[j] * K + k], sF[q]);
        }
    }
}

// Regions with at most BAYES_PACKED_CELLS undecided cells (K25): an 8-lane group serves one (region, chain), a wavefront eight
// of them.  Lane k < K of the group draws gamma k and keeps n[k] and its kept-theta sum; lane j < n_und keeps undecided cell
// j's L row and kept-state counts in registers.  The gammas go round the group by shuffles, n[k] is nfix[k] plus the group's
// part of a ballot: no LDS, no barrier, no atomic in the loop.  Every value is the one bayes_sample_kernel computes.
__global__ void __launch_bounds__(BAYES_THREADS) bayes_sample_packed_kernel(BayesSample a) {
    const int K = a.K;
    const int64_t pair = (int64_t)blockIdx.x * (BAYES_THREADS / BAYES_PACKED_CELLS) + threadIdx.x / BAYES_PACKED_CELLS;
    if (pair >= (int64_t)a.n_list * K) return;            // whole groups leave; the groups of a wavefront never read each other
    const int r = a.list[pair / K], ch = (int)(pair % K);
    const BayesRegion reg = a.regions[r];
    const int lane = threadIdx.x & (BAYES_PACKED_CELLS - 1);
    const int shift = (threadIdx.x & 63) & ~(BAYES_PACKED_CELLS - 1);   // the group's first lane in its wavefront
    const int nu = min(a.n_und[r], BAYES_PACKED_CELLS);
    const bool has_cell = lane < nu;
    const int i = has_cell ? a.und[reg.row0 + lane] : 0;
    double row[BAYES_MAX_K];
#pragma unroll
    for (int k = 0; k < BAYES_MAX_K; ++k) row[k] = (has_cell && k < K) ? a.L[(reg.row0 + i) * K + k] : 0.0;
    const int nfix = lane < K ? a.nfix[r * BAYES_MAX_K + lane] : 0;
    int n = (lane < K && lane == ch) ? reg.n_cells : 0;   // the chain starts from eps == ch
    int fr[BAYES_MAX_K];
#pragma unroll
    for (int k = 0; k < BAYES_MAX_K; ++k) fr[k] = 0;
    double *samp = a.theta_samples ? a.theta_samples + ((int64_t)r * K + ch) * (int64_t)a.n_keep * K : nullptr;
    double tsum = 0.0;
    const int64_t T = (int64_t)a.n_discard + a.n_keep;
    for (int64_t t = 0; t < T; ++t) {
        double g = 0.0;
        if (lane < K) g = bayes_gamma(1.0 + (double)n, a.seed, reg.token, lane, t, ch);
        double gk[BAYES_MAX_K];
        double S = 0.0;
#pragma unroll
        for (int k = 0; k < BAYES_MAX_K; ++k) {
            gk[k] = __shfl(g, k, BAYES_PACKED_CELLS);
            if (k < K) S = S + gk[k];
        }
        double theta[BAYES_MAX_K];
#pragma unroll
        for (int k = 0; k < BAYES_MAX_K; ++k) theta[k] = k < K ? gk[k] / S : 0.0;
        const bool keep = t >= a.n_discard;
        if (keep && lane < K) {
            const double th = g / S;
            tsum = tsum + th;
            if (samp) samp[(t - a.n_discard) * K + lane] = th;
        }
        int sel = -1;
        if (has_cell) {
            RtPhilox ph(a.seed, reg.token, (uint64_t)i, (uint64_t)t, (uint64_t)ch << 40);
            const double u = ph.random();
            sel = bayes_select(theta, row, K, u);
        }
        n = nfix;
#pragma unroll
        for (int k = 0; k < BAYES_MAX_K; ++k) {
            const unsigned long long m = __ballot(sel == k);
            if (lane == k) n += __popcll((m >> shift) & ((1ull << BAYES_PACKED_CELLS) - 1ull));
            fr[k] += (keep && sel == k) ? 1 : 0;
        }
    }
    if (lane < K) a.theta_sum[((int64_t)r * K + ch) * K + lane] = tsum;
    if (has_cell) {
#pragma unroll
        for (int k = 0; k < BAYES_MAX_K; ++k)
            if (k < K && fr[k]) atomicAdd(&a.freq[(reg.row0 + i) * K + k], fr[k]);   // the region's K chains meet here
    }
}

}  // namespace

#define BAYES_LAUNCH_CHECK() ICNV_HIP(hipGetLastError())

int launch_bayes_loglik(const BayesLoglik &a, int64_t n_tiles, hipStream_t s) {
    if (n_tiles <= 0) return ICNV_OK;
    KernelTimer kt("bayes_loglik", s);
    hipLaunchKernelGGL(bayes_loglik_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, a);
    BAYES_LAUNCH_CHECK();
    return ICNV_OK;
}

int launch_bayes_prep(const double *L, const BayesRegion *regions, int32_t n_regions, int32_t K, int32_t skip_decided, int32_t n_keep,
                      int32_t *und, int32_t *n_und, int32_t *nfix, int32_t *freq, hipStream_t s) {
    if (n_regions <= 0) return ICNV_OK;
    KernelTimer kt("bayes_prep", s);
    hipLaunchKernelGGL(bayes_prep_kernel, dim3((unsigned)n_regions), dim3(64), 0, s, L, regions, K, skip_decided, n_keep, und, n_und,
                       nfix, freq);
    BAYES_LAUNCH_CHECK();
    return ICNV_OK;
}

int launch_bayes_sample(const BayesSample &a, int32_t lds_cells, hipStream_t s) {
    if (a.n_list <= 0) return ICNV_OK;
    KernelTimer kt("bayes_sample", s);
    const dim3 grid((unsigned)((int64_t)a.n_list * a.K));
    if (lds_cells > 0) {
        const size_t bytes = (size_t)lds_cells * ((size_t)a.K * (sizeof(double) + sizeof(int)) + sizeof(int));
        hipLaunchKernelGGL(bayes_sample_kernel<true>, grid, dim3(BAYES_THREADS), bytes, s, a, lds_cells);
    } else {
        hipLaunchKernelGGL(bayes_sample_kernel<false>, grid, dim3(BAYES_THREADS), 0, s, a, 0);
    }
    BAYES_LAUNCH_CHECK();
    return ICNV_OK;
}

int launch_bayes_sample_packed(const BayesSample &a, hipStream_t s) {
    static_assert(BAYES_PACKED_CELLS == BAYES_MAX_K && 64 % BAYES_PACKED_CELLS == 0, "a group's lanes hold the K gammas and the cells");
    if (a.n_list <= 0) return ICNV_OK;
    KernelTimer kt("bayes_sample_packed", s);
    const int64_t per_block = BAYES_THREADS / BAYES_PACKED_CELLS;
    const int64_t blocks = ((int64_t)a.n_list * a.K + per_block - 1) / per_block;
    hipLaunchKernelGGL(bayes_sample_packed_kernel, dim3((unsigned)blocks), dim3(BAYES_THREADS), 0, s, a);
    BAYES_LAUNCH_CHECK();
    return ICNV_OK;
}

}  // namespace icnv
