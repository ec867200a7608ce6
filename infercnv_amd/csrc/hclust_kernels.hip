// Hierarchical clustering of the cells of a group: fastcluster::hclust(parallelDist(t(x)), method) as the reference's
// subclustering calls it (R/inferCNV_tumor_subclusters.R:191, 582, 609, R/inferCNV_ops.R:1930, 3242, ...).  DESIGN.md
// section 4 K9.  The nearest-neighbour chain is sequential and each of its steps is O(n) parallel work, less than a grid
// barrier costs, so one problem runs in ONE persistent workgroup and a batch fills the CUs with problems:
//
//   the fused entry point's distances (R's sequential dist, bit for bit) come from distance_kernels.hip
//   hclust_prep_kernel  every problem's matrix: flags a non-finite distance, squares it for ward.D2 (d * d)
//   hclust_lds_kernel   n <= 200: one workgroup per problem, the condensed matrix in LDS
//   hclust_hbm_kernel   larger n: one workgroup per problem, the full square matrix in HBM (rows contiguous, the updated
//                       row mirrored into its column), the active bitmask in LDS
//
// Both chain kernels run the same nn_chain() with the same operation order and tie rule, so they agree bit for bit.
// The raw merges (chain order) go back to hclust_api.hip, which sorts and labels them as R does.
// This file is compiled with -ffp-contract=off (Makefile): the Lance-Williams updates must not become FMAs.
#include "icnv_internal.h"
#include "hclust_internal.h"

namespace icnv {

namespace {

__global__ void hclust_prep_kernel(double *__restrict__ D, int64_t total, int square, uint32_t *__restrict__ bad) {
    uint32_t nonfinite = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const double v = D[i];
        if (!isfinite(v)) nonfinite = 1;
        if (square) D[i] = v * v;
    }
    if (nonfinite) atomicOr(bad, 1u);
}

// ---------------------------------------------------------------- the nearest-neighbour chain
__device__ __forceinline__ double lance_williams(int method, double a, double b, double c, double s, double t, double v) {
    switch (method) {
    case ICNV_HCLUST_SINGLE: return a < b ? a : b;
    case ICNV_HCLUST_COMPLETE: return a > b ? a : b;
    case ICNV_HCLUST_AVERAGE: return (s * a + t * b) / (s + t);
    case ICNV_HCLUST_MCQUITTY: return (a + b) * 0.5;
    default: return ((v + s) * a - v * c + (v + t) * b) / (s + t + v);   // ward.D, ward.D2
    }
}

__device__ __forceinline__ bool key_less(double v, int r, double bv, int br) { return v < bv || (v == bv && r < br); }

__device__ __forceinline__ bool is_active(const uint32_t *act, int j) { return (act[j >> 5] >> (j & 31)) & 1u; }

struct Red {   // cross-wavefront argmin scratch (LDS)
    double v[16];
    int r[16], j[16];
};

// block-wide minimum of the key (v, r); every thread returns the same (v, j)
template <int NT>
__device__ __forceinline__ void block_argmin(double &v, int &r, int &j, Red &red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(v, off);
        const int orr = __shfl_xor(r, off), oj = __shfl_xor(j, off);
        if (key_less(ov, orr, v, r)) { v = ov; r = orr; j = oj; }
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red.v[w] = v; red.r[w] = r; red.j[w] = j; }
    __syncthreads();
    v = red.v[0]; r = red.r[0]; j = red.j[0];
#pragma unroll
    for (int q = 1; q < NT / 64; ++q)
        if (key_less(red.v[q], red.r[q], v, r)) { v = red.v[q]; r = red.r[q]; j = red.j[q]; }
    __syncthreads();
}

struct LdsStore {    // condensed upper triangle: (i < j) at i (2n - i - 1) / 2 + j - i - 1
    double *cd;
    int n;
    __device__ __forceinline__ int idx(int i, int j) const {
        if (i > j) { const int q = i; i = j; j = q; }
        return i * (2 * n - i - 1) / 2 + j - i - 1;
    }
    __device__ __forceinline__ double get(int i, int j) const { return cd[idx(i, j)]; }
    __device__ __forceinline__ void put(int y, int k, double v) const { cd[idx(y, k)] = v; }
};

struct HbmStore {    // full square matrix, row i at D + i n; kept symmetric on the active rows and columns
    double *D;
    int n;
    __device__ __forceinline__ double get(int i, int j) const { return D[(int64_t)i * n + j]; }
    __device__ __forceinline__ void put(int y, int k, double v) const {
        D[(int64_t)y * n + k] = v;
        D[(int64_t)k * n + y] = v;
    }
};

// Runs the whole chain of one problem.  chain [n], size [n], act [(n + 31) / 32] are initialised by the caller
// (act: bits 0 .. n-1 set; size: 1).  Every thread holds the same len / tip / prev / first.
template <int NT, class Store>
__device__ void nn_chain(const Store &st, int n, int method, int32_t *chain, int32_t *size, uint32_t *act, int32_t *mx,
                         int32_t *my, double *mh, int64_t *steps_out, Red &red) {
    const int tid = threadIdx.x;
    int len = 0, tip = -1, prev = -1, first = 0;
    int64_t steps = 0;
    for (int m = 0; m < n - 1;) {
        if (len == 0) {   // restart from the first active index
            tip = first;
            prev = -1;
            len = 1;
            if (tid == 0) chain[0] = tip;
        }
        ++steps;
        // nearest active neighbour of the tip: minimum of (D[tip, j], rank), rank(prev) = -1, else j
        double bv = HUGE_VAL;
        int br = 0x7fffffff, bj = -1;
        constexpr int U = 4;
        for (int j0 = tid; j0 < n; j0 += U * NT) {
            double v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = j0 + u * NT;
                v[u] = (j < n && j != tip) ? st.get(tip, j) : 0.0;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int j = j0 + u * NT;
                if (j < n && j != tip && is_active(act, j)) {
                    const int r = j == prev ? -1 : j;
                    if (key_less(v[u], r, bv, br)) { bv = v[u]; br = r; bj = j; }
                }
            }
        }
        block_argmin<NT>(bv, br, bj, red);
        if (bj < 0) {   // no finite candidate: a Lance-Williams update overflowed; reported by steps = -1
            steps = -1;
            break;
        }
        if (bj != prev) {   // extend the chain
            if (tid == 0) chain[len] = bj;
            ++len;
            prev = tip;
            tip = bj;
            continue;
        }
        // tip and prev are reciprocal nearest neighbours: merge them into the larger index
        const int x = tip < prev ? tip : prev, y = tip < prev ? prev : tip;
        const double c = bv;
        const double s = (double)size[x], t = (double)size[y];
        for (int k = tid; k < n; k += NT) {
            if (k == x || k == y || !is_active(act, k)) continue;
            const double nv = lance_williams(method, st.get(x, k), st.get(y, k), c, s, t, (double)size[k]);
            st.put(y, k, nv);
        }
        __syncthreads();
        if (tid == 0) {
            size[y] = size[x] + size[y];
            act[x >> 5] &= ~(1u << (x & 31));
            mx[m] = x;
            my[m] = y;
            mh[m] = c;
        }
        __syncthreads();
        ++m;
        if (x == first)   // the first active index only grows: a retired index is always the smaller of its pair
            while (first < n && !is_active(act, first)) ++first;
        len -= 2;
        if (len <= 1) {
            len = 0;
        } else {
            tip = chain[len - 1];
            prev = chain[len - 2];
        }
    }
    if (tid == 0) *steps_out = steps;
}

constexpr int LDS_NT = 256;
constexpr int HBM_NT = 1024;

__global__ void __launch_bounds__(LDS_NT) hclust_lds_kernel(HclustArgs a) {
    extern __shared__ __attribute__((aligned(16))) double hc_smem[];
    __shared__ Red red;
    const int p = a.run[blockIdx.x];
    const int n = a.n[p];
    const int ne = n * (n - 1) / 2;
    double *cd = hc_smem;
    int32_t *chain = reinterpret_cast<int32_t *>(cd + ne);
    int32_t *size = chain + n;
    uint32_t *act = reinterpret_cast<uint32_t *>(size + n);
    const int nw = (n + 31) / 32;
    const double *Dp = a.D + a.d_off[p];
    LdsStore st{cd, n};
    for (int e = threadIdx.x; e < n * n; e += LDS_NT) {
        const int i = e / n, j = e - i * n;
        if (j > i) cd[st.idx(i, j)] = Dp[e];
    }
    for (int k = threadIdx.x; k < n; k += LDS_NT) size[k] = 1;
    for (int q = threadIdx.x; q < nw; q += LDS_NT) act[q] = (q == nw - 1 && (n & 31)) ? ((1u << (n & 31)) - 1u) : 0xffffffffu;
    __syncthreads();
    const int64_t m0 = a.m_off[p];
    nn_chain<LDS_NT>(st, n, a.method, chain, size, act, a.mx + m0, a.my + m0, a.mh + m0, a.steps + p, red);
}

__global__ void __launch_bounds__(HBM_NT) hclust_hbm_kernel(HclustArgs a) {
    extern __shared__ uint32_t hc_act[];
    __shared__ Red red;
    const int p = a.run[blockIdx.x];
    const int n = a.n[p];
    const int nw = (n + 31) / 32;
    int32_t *chain = a.work + 2 * a.c_off[p];
    int32_t *size = chain + n;
    for (int k = threadIdx.x; k < n; k += HBM_NT) size[k] = 1;
    for (int q = threadIdx.x; q < nw; q += HBM_NT) hc_act[q] = (q == nw - 1 && (n & 31)) ? ((1u << (n & 31)) - 1u) : 0xffffffffu;
    __syncthreads();
    const int64_t m0 = a.m_off[p];
    HbmStore st{a.D + a.d_off[p], n};
    nn_chain<HBM_NT>(st, n, a.method, chain, size, hc_act, a.mx + m0, a.my + m0, a.mh + m0, a.steps + p, red);
}

}  // namespace

int launch_hclust_prep(double *D, int64_t total, bool square, uint32_t *bad, hipStream_t s) {
    if (total <= 0) return ICNV_OK;
    KernelTimer kt("hclust_prep", s);
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 16 * (int64_t)num_cus());
    hipLaunchKernelGGL(hclust_prep_kernel, dim3((unsigned)blocks), dim3(256), 0, s, D, total, square ? 1 : 0, bad);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_hclust_lds(const HclustArgs &a, int max_n, hipStream_t s) {
    if (a.n_run <= 0) return ICNV_OK;
    if (max_n < 2 || max_n > HC_LDS_MAX_N) ICNV_FAIL(ICNV_ERR_ARG, "hclust: problem too large for the LDS path");
    KernelTimer kt("hclust_lds", s);
    static DeviceOnce once;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(hclust_lds_kernel), (int)hc_lds_bytes(HC_LDS_MAX_N), once)) return rc;
    hipLaunchKernelGGL(hclust_lds_kernel, dim3((unsigned)a.n_run), dim3(LDS_NT), hc_lds_bytes(max_n), s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_hclust_hbm(const HclustArgs &a, int max_n, hipStream_t s) {
    if (a.n_run <= 0) return ICNV_OK;
    if (max_n < 2 || max_n > HC_HBM_MAX_N) ICNV_FAIL(ICNV_ERR_ARG, "hclust: problem too large for the HBM path");
    KernelTimer kt("hclust_hbm", s);
    const size_t lds = (size_t)(max_n + 31) / 32 * 4;
    static DeviceOnce once;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(hclust_hbm_kernel), HC_HBM_MAX_N / 8, once)) return rc;
    hipLaunchKernelGGL(hclust_hbm_kernel, dim3((unsigned)a.n_run), dim3(HBM_NT), lds, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
