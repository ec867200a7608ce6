// The PCA route of the Leiden subclustering (.leiden_seurat_preprocess_routine, R/inferCNV_tumor_subclusters.R:699-723:
// FindVariableFeatures -> ScaleData -> RunPCA -> FindNeighbors -> cluster_leiden on the SNN graph).  DESIGN.md section 4
// K18; the contract is in include/icnv.h and restated in tests/leiden_pca_restate.py.
//
//   lpca_vstd_kernel      one lane per (problem, gene): the standardised variance, a sequential fp64 sum down the cells
//   lpca_scale_kernel     32 x 32 tiles through LDS: z = min(10, (x - mean) / sd), written feature-major
//   lpca_gram_kernel      M = Z Z^T on the matrix cores (gram::tile_product): upper triangle of 64 x 64 tiles, mirrored
//   lpca_project_kernel   one lane per (cell, component): E = Z^T V, a sequential fp64 sum over the features
//   snn_t*_kernel         the transposed kNN lists: count (entries in range), scan, fill, sort per row (no row repeats an entry)
//   snn_rows_kernel       one wavefront per row: s_ij = |N(i) n N(j)| over the transposed lists of N(i); a count pass, then
//                         a fill pass into the exactly sized CSR (ascending columns, integer s, 24-bit fixed-point weight)
//   lg_check_kernel       a caller's CSR for icnv_leiden_graph_dev: ranges, order, weights; strengths
//
// vstd, scale and project are bit-equal to the restatement: this file is compiled with -ffp-contract=off (Makefile).
#include <algorithm>

#include "icnv_internal.h"
#include "gram_mfma.h"
#include "leiden_pca_internal.h"

namespace icnv {

namespace {

constexpr int LP_WAVE = 64;
constexpr int LP_NT = 256;

__device__ __forceinline__ int lp_lane() { return threadIdx.x & (LP_WAVE - 1); }

// ---------------------------------------------------------------------------------------------------- stage 1: v_std
__global__ void __launch_bounds__(LP_NT) lpca_vstd_kernel(LpArgs a) {
    const LpProb pr = a.prob[blockIdx.y];
    const int64_t j = (int64_t)blockIdx.x * LP_NT + threadIdx.x;
    if (j >= pr.n_gene) return;
    const int64_t g = a.gene_idx[pr.gene_off + j];
    const double mean = a.mean[pr.gene_off + j], sd = a.sd[pr.gene_off + j];
    double acc = 0.0;
    if (sd != 0.0) {   // a gene outside the fit (constant over the cells) keeps 0
        const double vmax = __dsqrt_rn((double)pr.n);
        const int32_t *cells = a.cell_idx + pr.cell_off;
        for (int32_t c = 0; c < pr.n; ++c) {
            double d = (a.x[(int64_t)cells[c] * a.ld + g] - mean) / sd;
            if (d > vmax) d = vmax;
            acc = acc + d * d;
        }
        acc = acc / (double)(pr.n - 1);
    }
    a.v_std[pr.gene_off + j] = acc;
}

// ---------------------------------------------------------------------------------------------------- stage 2: scale
__global__ void __launch_bounds__(LP_NT) lpca_scale_kernel(LpArgs a) {
    __shared__ double tile[32][33];
    const LpProb pr = a.prob[blockIdx.z];
    const int f0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    if (f0 >= pr.n_gene || c0 >= pr.ldz) return;   // uniform over the block
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int32_t *cells = a.cell_idx + pr.cell_off;
    {
        const int f = f0 + tx;
        int64_t g = 0;
        double mean = 0.0, sd = 0.0;
        if (f < pr.n_gene) { g = a.gene_idx[pr.gene_off + f]; mean = a.mean[pr.gene_off + f]; sd = a.sd[pr.gene_off + f]; }
        for (int r = ty; r < 32; r += 8) {
            const int c = c0 + r;
            double z = 0.0;
            if (f < pr.n_gene && c < pr.n && sd != 0.0) {
                z = (a.x[(int64_t)cells[c] * a.ld + g] - mean) / sd;
                if (z > 10.0) z = 10.0;
            }
            tile[r][tx] = z;
        }
    }
    __syncthreads();
    for (int r = ty; r < 32; r += 8) {
        const int f = f0 + r, c = c0 + tx;
        if (f < pr.n_gene && c < pr.ldz) a.Z[pr.z_off + (int64_t)f * pr.ldz + c] = tile[tx][r];
    }
}

// ---------------------------------------------------------------------------------------------------- stage 3: Gram
__global__ void __launch_bounds__(256) lpca_gram_kernel(LpArgs a, int nt_max) {
    constexpr int WM = 2, DT = 32 * WM;
    extern __shared__ __attribute__((aligned(16))) double smem_d[];
    const LpProb pr = a.prob[blockIdx.y];
    const int ti = blockIdx.x / nt_max, tj = blockIdx.x - ti * nt_max;
    const int F = pr.n_gene, nt = (F + DT - 1) / DT;
    if (ti > tj || tj >= nt) return;   // uniform over the block: the upper triangle of tiles
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wr = w >> 1, wc = w & 1, lrow = t >> 2;
    const double *Zp = a.Z + pr.z_off;
    const int ra = ti * DT + lrow, rb = tj * DT + lrow;
    const double *pa[1] = {ra < F ? Zp + (int64_t)ra * pr.ldz : nullptr};
    const double *pb[1] = {rb < F ? Zp + (int64_t)rb * pr.ldz : nullptr};
    gram::dbl4_t acc[WM][WM];
    gram::tile_product<WM>(pa, pb, pr.ldz, smem_d, acc);
    double *M = a.M + pr.m_off;
#pragma unroll
    for (int aa = 0; aa < WM; ++aa)
#pragma unroll
        for (int bb = 0; bb < WM; ++bb)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int row = ti * DT + wr * 16 * WM + aa * 16 + (lane >> 4) + 4 * reg;
                const int col = tj * DT + wc * 16 * WM + bb * 16 + (lane & 15);
                if (row < F && col < F && col >= row) {   // one value for (row, col) and (col, row): exactly symmetric
                    const double v = acc[aa][bb][reg];
                    M[(int64_t)row * F + col] = v;
                    M[(int64_t)col * F + row] = v;
                }
            }
}

// ---------------------------------------------------------------------------------------------------- stage 3: embedding
__global__ void __launch_bounds__(LP_NT) lpca_project_kernel(LpArgs a) {
    const LpProb pr = a.prob[blockIdx.z];
    const int64_t c = (int64_t)blockIdx.x * LP_NT + threadIdx.x;
    const int j = blockIdx.y;
    if (c >= pr.n || j >= pr.npcs) return;
    const double *z = a.Z + pr.z_off + c, *v = a.V + pr.m_off + j;
    double acc = 0.0;
    for (int32_t f = 0; f < pr.n_gene; ++f) acc = acc + z[(int64_t)f * pr.ldz] * v[(int64_t)f * pr.npcs];
    a.E[(pr.e_off + c) * a.e_ld + j] = acc;
}

// ---------------------------------------------------------------------------------------------------- stage 4: SNN
// exclusive scan of in[0, n) into out[0, n], out[n] = total, by one wavefront
template <typename TO>
__device__ void lp_wave_scan(const int32_t *in, TO *out, int64_t n) {
    int64_t carry = 0;
    for (int64_t b = 0; b < n; b += LP_WAVE) {
        const int64_t i = b + lp_lane();
        const int64_t x = i < n ? (int64_t)in[i] : 0;
        int64_t inc = x;
        for (int d = 1; d < LP_WAVE; d <<= 1) {
            const int64_t y = __shfl_up(inc, d, LP_WAVE);
            if (lp_lane() >= d) inc += y;
        }
        if (i < n) out[i] = (TO)(carry + inc - x);
        carry += __shfl(inc, LP_WAVE - 1, LP_WAVE);
    }
    if (lp_lane() == 0) out[n] = (TO)carry;
}

__global__ void __launch_bounds__(LP_NT) snn_tcount_kernel(SnnArgs a) {
    const int p = blockIdx.y;
    const int64_t n0 = a.node_off[p], n = a.node_off[p + 1] - n0;
    const int32_t *nn = a.nn + n0 * a.k;
    uint32_t bad = 0;
    for (int64_t e = (int64_t)blockIdx.x * LP_NT + threadIdx.x; e < n * a.k; e += (int64_t)gridDim.x * LP_NT) {
        const int32_t j = nn[e];
        if (j < 0 || j >= n) bad = 1;
        else atomicAdd(&a.t_cnt[n0 + j], 1);
    }
    if (bad) atomicOr(a.bad, SNN_BAD_RANGE);
}

__global__ void __launch_bounds__(LP_WAVE) snn_tscan_kernel(SnnArgs a) {
    const int p = blockIdx.x;
    const int64_t n0 = a.node_off[p], n = a.node_off[p + 1] - n0;
    lp_wave_scan(a.t_cnt + n0, a.t_off + n0 + p, n);
    __syncthreads();
    for (int64_t i = lp_lane(); i < n; i += LP_WAVE) a.t_cnt[n0 + i] = 0;   // the fill's cursors
}

__global__ void __launch_bounds__(LP_NT) snn_tfill_kernel(SnnArgs a) {
    const int p = blockIdx.y;
    const int64_t n0 = a.node_off[p], n = a.node_off[p + 1] - n0;
    const int32_t *nn = a.nn + n0 * a.k;
    const int64_t *toff = a.t_off + n0 + p;
    int32_t *list = a.t_list + n0 * a.k;
    for (int64_t e = (int64_t)blockIdx.x * LP_NT + threadIdx.x; e < n * a.k; e += (int64_t)gridDim.x * LP_NT) {
        const int32_t j = nn[e];   // in range: the count pass saw every entry
        list[toff[j] + atomicAdd(&a.t_cnt[n0 + j], 1)] = (int32_t)(e / a.k);
    }
}

// The order of the atomics is gone: sort each row.  An nn_idx row that repeats an entry m is then two equal neighbours in
// m's sorted list: bad |= SNN_BAD_REPEAT (the rows kernel relies on lists of distinct rows).
__global__ void __launch_bounds__(LP_NT) snn_tsort_kernel(SnnArgs a) {
    const int p = blockIdx.y;
    const int64_t n0 = a.node_off[p], n = a.node_off[p + 1] - n0;
    const int64_t *toff = a.t_off + n0 + p;
    int32_t *list = a.t_list + n0 * a.k;
    uint32_t bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * LP_NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * LP_NT) {
        int32_t *r = list + toff[i];
        const int64_t m = toff[i + 1] - toff[i];
        int64_t h = 1;
        while (h < m / 3) h = 3 * h + 1;
        for (; h >= 1; h /= 3)
            for (int64_t u = h; u < m; ++u) {
                const int32_t x = r[u];
                int64_t v = u;
                while (v >= h && r[v - h] > x) { r[v] = r[v - h]; v -= h; }
                r[v] = x;
            }
        for (int64_t u = 1; u < m; ++u)
            if (r[u] == r[u - 1]) bad = SNN_BAD_REPEAT;
    }
    if (bad) atomicOr(a.bad, bad);
}

__device__ __forceinline__ int32_t lp_load(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// One wavefront per row; block b of problem p owns the scratch rows mark / touched [(p * gridDim.x + b) * max_n, + n).
// mark[] is zero on entry and on exit.
template <bool FILL>
__global__ void __launch_bounds__(LP_WAVE) snn_rows_kernel(SnnArgs a) {
    const int p = blockIdx.y;
    const int64_t n0 = a.node_off[p], n = a.node_off[p + 1] - n0;
    const int k = a.k;
    const int32_t *nn = a.nn + n0 * k;
    const int64_t *toff = a.t_off + n0 + p;
    const int32_t *list = a.t_list + n0 * k;
    const int64_t scr = ((int64_t)p * gridDim.x + blockIdx.x) * a.max_n;
    int32_t *mark = a.mark + scr, *touched = a.touched + scr;
    const uint64_t below = (1ull << lp_lane()) - 1ull;
    for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
        int64_t nt = 0;
        for (int q = 0; q < k; ++q) {
            const int32_t m = nn[i * k + q];
            const int64_t beg = toff[m], len = toff[m + 1] - beg;
            for (int64_t b = 0; b < len; b += LP_WAVE) {   // a transposed list holds distinct rows: no lane meets another's j
                const int64_t t = b + lp_lane();
                bool first = false;
                int32_t j = 0;
                if (t < len) { j = list[beg + t]; first = atomicAdd(&mark[j], 1) == 0; }
                const uint64_t bm = __ballot(first);
                if (first) touched[nt + __popcll(bm & below)] = j;
                nt += __popcll(bm);
            }
            __syncthreads();
        }
        // keep j != i with 16 s >= 2 k, compacted to the front of touched[] (a chunk's writes stay behind its reads)
        int64_t nk = 0;
        for (int64_t b = 0; b < nt; b += LP_WAVE) {
            const int64_t t = b + lp_lane();
            bool keep = false;
            int32_t j = 0;
            if (t < nt) {
                j = touched[t];
                const int32_t s = lp_load(&mark[j]);
                keep = j != i && 16 * (int64_t)s >= 2 * (int64_t)k;
                if (!keep || !FILL) atomicExch(&mark[j], 0);
            }
            __syncthreads();
            const uint64_t bm = __ballot(keep);
            if (keep && FILL) touched[nk + __popcll(bm & below)] = j;
            nk += __popcll(bm);
            __syncthreads();
        }
        if (!FILL) {
            if (lp_lane() == 0) { a.row_cnt[n0 + i] = (int32_t)nk; a.loop[n0 + i] = 1; }   // s_ii = k: always kept
        } else {
            const int64_t out = a.row_off[n0 + i];
            for (int64_t t = lp_lane(); t < nk; t += LP_WAVE) {   // rank sort of the kept columns
                const int32_t j = touched[t];
                int64_t rank = 0;
                for (int64_t u = 0; u < nk; ++u) rank += touched[u] < j;
                const int64_t s = lp_load(&mark[j]), d = 2 * (int64_t)k - s;
                a.col[out + rank] = j;
                a.shared[out + rank] = (int32_t)s;
                a.weight[out + rank] = (2 * s * LPCA_WEIGHT_ONE + d) / (2 * d);
            }
            __syncthreads();
            for (int64_t t = lp_lane(); t < nk; t += LP_WAVE) atomicExch(&mark[touched[t]], 0);
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(LP_WAVE) snn_scan_kernel(SnnArgs a, int64_t total_n) {
    lp_wave_scan(a.row_cnt, a.row_off, total_n);
}

// ---------------------------------------------------------------------------------------------------- stage 5: a caller's CSR
constexpr int64_t LG_SAT = (int64_t)1 << 62;
__device__ __forceinline__ int64_t sat_add(int64_t x, int64_t y) { const int64_t s = x + y; return s > LG_SAT ? LG_SAT : s; }

__global__ void __launch_bounds__(LP_NT) lg_check_kernel(LgCheck c) {
    __shared__ int64_t part[LP_NT];
    const int p = blockIdx.x;
    const int64_t n0 = c.node_off[p], n = c.node_off[p + 1] - n0;
    const int64_t *off = c.off + n0 + p;
    const int64_t eb = c.edge_off[p];
    uint32_t bad = 0;
    int64_t sum = 0;
    for (int64_t i = threadIdx.x; i < n; i += LP_NT) {
        int64_t s = 0;
        for (int64_t t = off[i]; t < off[i + 1]; ++t) {
            const int32_t j = c.col[eb + t];
            const int64_t w = c.weight[eb + t];
            if (j < 0 || j >= n || j == i || (t > off[i] && j <= c.col[eb + t - 1]) || w < 1 || w > LG_SAT) bad = 1;
            else s = sat_add(s, w);
        }
        const int32_t lp = c.loop[n0 + i];
        if (lp != 0 && lp != 1) bad = 1;
        if (lp == 1) s = sat_add(sat_add(s, c.loop_weight), c.loop_weight);
        c.strength[n0 + i] = s;
        sum = sat_add(sum, s);
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = LP_NT / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) part[threadIdx.x] = sat_add(part[threadIdx.x], part[threadIdx.x + d]);
        __syncthreads();
    }
    if (threadIdx.x == 0) c.strength_sum[p] = part[0];
    if (bad) atomicOr(c.bad, 1u);
}

}  // namespace

int launch_lpca_vstd(const LpArgs &a, int32_t max_genes, hipStream_t s) {
    hipLaunchKernelGGL(lpca_vstd_kernel, dim3((unsigned)((max_genes + LP_NT - 1) / LP_NT), (unsigned)a.n_prob), dim3(LP_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_lpca_scale(const LpArgs &a, int32_t max_genes, int32_t max_ldz, hipStream_t s) {
    hipLaunchKernelGGL(lpca_scale_kernel, dim3((unsigned)((max_genes + 31) / 32), (unsigned)((max_ldz + 31) / 32), (unsigned)a.n_prob),
                       dim3(LP_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_lpca_gram(const LpArgs &a, int32_t max_genes, hipStream_t s) {
    const int nt = (max_genes + 63) / 64;
    hipLaunchKernelGGL(lpca_gram_kernel, dim3((unsigned)(nt * nt), (unsigned)a.n_prob), dim3(256), gram::lds_bytes(2), s, a, nt);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_lpca_project(const LpArgs &a, int32_t max_n, hipStream_t s) {
    int32_t max_npcs = a.e_ld;
    hipLaunchKernelGGL(lpca_project_kernel, dim3((unsigned)((max_n + LP_NT - 1) / LP_NT), (unsigned)max_npcs, (unsigned)a.n_prob),
                       dim3(LP_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int snn_blocks(int64_t max_n) { return (int)std::min<int64_t>(std::max<int64_t>((max_n + 63) / 64, 1), 256); }

int launch_snn_transpose(const SnnArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)std::min<int64_t>(std::max<int64_t>((a.max_n * a.k + LP_NT - 1) / LP_NT, 1), 1024), (unsigned)a.n_prob);
    hipLaunchKernelGGL(snn_tcount_kernel, grid, dim3(LP_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

// after the range check of launch_snn_transpose: the sorted transposed lists, and the check for a repeated entry
int launch_snn_lists(const SnnArgs &a, hipStream_t s) {
    const dim3 g2((unsigned)std::min<int64_t>(std::max<int64_t>((a.max_n * a.k + LP_NT - 1) / LP_NT, 1), 1024), (unsigned)a.n_prob);
    hipLaunchKernelGGL(snn_tscan_kernel, dim3((unsigned)a.n_prob), dim3(LP_WAVE), 0, s, a);
    hipLaunchKernelGGL(snn_tfill_kernel, g2, dim3(LP_NT), 0, s, a);
    hipLaunchKernelGGL(snn_tsort_kernel, g2, dim3(LP_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_snn_rows(const SnnArgs &a, bool fill, hipStream_t s) {
    const dim3 grid((unsigned)snn_blocks(a.max_n), (unsigned)a.n_prob);
    if (!fill) hipLaunchKernelGGL(snn_rows_kernel<false>, grid, dim3(LP_WAVE), 0, s, a);
    else hipLaunchKernelGGL(snn_rows_kernel<true>, grid, dim3(LP_WAVE), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_snn_scan(const SnnArgs &a, int64_t total_n, hipStream_t s) {
    hipLaunchKernelGGL(snn_scan_kernel, dim3(1), dim3(LP_WAVE), 0, s, a, total_n);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_lg_check(const LgCheck &c, hipStream_t s) {
    hipLaunchKernelGGL(lg_check_kernel, dim3((unsigned)c.n_prob), dim3(LP_NT), 0, s, c);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
