// The permutation statistic of the random-trees subclustering (R/inferCNV_tumor_subclusters.random_smoothed_trees.R:217-298):
// for every clade of a recursion level, the observed matrix and n_iter copies whose genes are each permuted across the
// clade's cells, smoothed along the genes with caTools::runmean and median-centred per cell, then clustered.  DESIGN.md
// section 4 K10.  This file holds the stages in front of K9's clustering:
//
//   rt_check_kernel      flags a non-finite value among the clades' cells (before anything is clustered)
//   rt_permute_kernel    one lane per (item, gene): gathers the gene's values over the clade's cells into the item's rows
//                        and shuffles them in place with NumPy's Generator(Philox).permutation (Durstenfeld, masked
//                        rejection); the observed matrix (iteration -1) is only gathered
//   rt_smooth_kernel     runmean(k = window, endrule = "mean") along the genes of every row: each output the sequential sum
//                        of its clipped window in gene order, then one division
//   rt_max_height_kernel max of a permuted tree's merge dissimilarities (sqrt for ward.D2) -- the only thing kept of it
//
// The median centring is step 11's own kernel (launch_chain_large_center), the distances and the chain are K9's.
// This file is compiled with -ffp-contract=off (Makefile): the window sums must not become FMAs.
#include "icnv_internal.h"
#include "random_trees_internal.h"

namespace icnv {

namespace {

constexpr int RT_NT = 256;
constexpr int RT_SMOOTH_PER_THREAD = 4;

__global__ void rt_check_kernel(const double *__restrict__ x, int32_t G, const int32_t *__restrict__ cells, int64_t n_cells,
                                uint32_t *__restrict__ bad) {
    uint32_t nonfinite = 0;
    const int64_t total = n_cells * G;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t c = e / G, g = e - c * G;
        if (!isfinite(x[(int64_t)cells[c] * G + g])) nonfinite = 1;
    }
    if (nonfinite) atomicOr(bad, 1u);
}

__global__ void __launch_bounds__(RT_NT) rt_permute_kernel(RtItems a) {
    const int g = blockIdx.x * RT_NT + threadIdx.x;
    const int item = blockIdx.y;
    if (g >= a.G) return;
    const int p = a.item_clade[item], r = a.item_iter[item];
    const int64_t c0 = a.cell_off[p];
    const int n = (int)(a.cell_off[p + 1] - c0);
    const int32_t *S = a.cell_idx + c0;
    double *col = a.m + a.item_row[item] * a.ld_m + g;   // this gene's value of cell c at col[c * ld_m]
    const int64_t ld = a.ld_m;
    for (int c = 0; c < n; ++c) col[c * ld] = a.x[(int64_t)S[c] * a.G + g];
    if (r < 0) return;
    RtPhilox rng(a.seed, a.token[p], (uint64_t)g, (uint64_t)r);
    for (int i = n - 1; i >= 1; --i) {
        const int j = (int)rng.interval((uint32_t)i);
        if (j != i) {
            const double vi = col[i * ld], vj = col[j * ld];
            col[i * ld] = vj;
            col[j * ld] = vi;
        }
    }
}

__global__ void __launch_bounds__(RT_NT) rt_smooth_kernel(RtItems a) {
    const int64_t row = blockIdx.x;
    const int G = a.G;
    const double *src = a.m + row * a.ld_m;
    double *dst = a.z + row * (int64_t)G;
    const int o0 = (blockIdx.y * RT_NT + threadIdx.x) * RT_SMOOTH_PER_THREAD;
    if (o0 >= G) return;
    const int k = a.window < G ? a.window : G;
    if (k <= 1) {
        for (int u = 0; u < RT_SMOOTH_PER_THREAD && o0 + u < G; ++u) dst[o0 + u] = src[o0 + u];
        return;
    }
    const int k2 = k / 2, left = k - 1 - k2;
    int lo[RT_SMOOTH_PER_THREAD], hi[RT_SMOOTH_PER_THREAD];
    double s[RT_SMOOTH_PER_THREAD];
    int qhi = 0;
#pragma unroll
    for (int u = 0; u < RT_SMOOTH_PER_THREAD; ++u) {
        const int o = o0 + u;
        lo[u] = o - left > 0 ? o - left : 0;
        hi[u] = o < G ? (o + k2 < G - 1 ? o + k2 : G - 1) : -1;   // an output past G sums nothing
        if (hi[u] > qhi) qhi = hi[u];
        s[u] = 0.0;
    }
    for (int q = lo[0]; q <= qhi; ++q) {
        const double v = src[q];
#pragma unroll
        for (int u = 0; u < RT_SMOOTH_PER_THREAD; ++u)
            if (q >= lo[u] && q <= hi[u]) s[u] = s[u] + v;
    }
#pragma unroll
    for (int u = 0; u < RT_SMOOTH_PER_THREAD; ++u)
        if (o0 + u < G) dst[o0 + u] = s[u] / (double)(hi[u] - lo[u] + 1);
}

__global__ void __launch_bounds__(RT_NT) rt_max_height_kernel(const double *__restrict__ mh, const int64_t *__restrict__ m_off,
                                                              const int32_t *__restrict__ n, const int64_t *__restrict__ out_idx,
                                                              int root, double *__restrict__ out) {
    __shared__ double red[RT_NT / 64];
    const int item = blockIdx.x;
    const int64_t m0 = m_off[item];
    const int nm = n[item] - 1;
    double v = -HUGE_VAL;
    for (int i = threadIdx.x; i < nm; i += RT_NT) v = fmax(v, mh[m0 + i]);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < RT_NT / 64; ++w) v = fmax(v, red[w]);
        v = fmax(v, red[0]);
        out[out_idx[item]] = root ? sqrt(v) : v;   // sqrt is monotone: the max of the sqrt heights
    }
}

}  // namespace

int launch_rt_check(const double *x, int32_t G, const int32_t *cells, int64_t n_cells, uint32_t *bad, hipStream_t s) {
    if (n_cells <= 0) return ICNV_OK;
    KernelTimer kt("rt_check", s);
    const int64_t blocks = std::min<int64_t>((n_cells * G + RT_NT - 1) / RT_NT, 16 * (int64_t)num_cus());
    hipLaunchKernelGGL(rt_check_kernel, dim3((unsigned)blocks), dim3(RT_NT), 0, s, x, G, cells, n_cells, bad);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_rt_permute(const RtItems &a, hipStream_t s) {
    if (a.n_items <= 0) return ICNV_OK;
    if (a.n_items > 65535) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: more than 65535 matrices in one wave");
    KernelTimer kt("rt_permute", s);
    hipLaunchKernelGGL(rt_permute_kernel, dim3((unsigned)((a.G + RT_NT - 1) / RT_NT), (unsigned)a.n_items), dim3(RT_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_rt_smooth(const RtItems &a, int64_t n_rows, hipStream_t s) {
    if (n_rows <= 0) return ICNV_OK;
    if (n_rows > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: too many rows in one wave");
    KernelTimer kt("rt_smooth", s);
    const int per_block = RT_NT * RT_SMOOTH_PER_THREAD;
    hipLaunchKernelGGL(rt_smooth_kernel, dim3((unsigned)n_rows, (unsigned)((a.G + per_block - 1) / per_block)), dim3(RT_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_rt_max_height(const double *mh, const int64_t *m_off, const int32_t *n, const int64_t *out_idx, int32_t n_items,
                         bool root, double *out, hipStream_t s) {
    if (n_items <= 0) return ICNV_OK;
    KernelTimer kt("rt_max_height", s);
    hipLaunchKernelGGL(rt_max_height_kernel, dim3((unsigned)n_items), dim3(RT_NT), 0, s, mh, m_off, n, out_idx, root ? 1 : 0, out);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
