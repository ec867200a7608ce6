// K33: the numbers under the Bayesian filter's probability plots: icnv_paint_regions_dev and icnv_theta_box_dev of
// include/icnv.h.  DESIGN.md section 4 K33.
//
//   paint_check_kernel    every index of the call against G, C and the offsets' own rules; the verdict comes back before a byte
//                         of the matrix is written
//   paint_owner_kernel    on the zeroed matrix.  One wavefront per (region, cell), its lanes along the cell's genes as in K25's
//                         fill: every element of the rectangle takes the INTEGER maximum of its eight bytes and r + 1 (one
//                         64-bit unsigned atomic max per element, a wavefront's 64 of them one contiguous run).  +0.0 is the
//                         integer 0, so afterwards an element holds 0 or 1 + the highest region that covers it, whatever the
//                         order the wavefronts ran in: a maximum of integers has no order.  No floating-point atomic exists here.
//   paint_value_kernel    every element g < G of every cell once: an owner o > 0 becomes value[o - 1], bits as they are (-0.0,
//                         NaN payloads); 0 stays +0.0 and is not written again.
//   theta_box_kernel      one workgroup per (region, state): the N pooled draws gathered from the strided samples into LDS, K31's
//                         sort (mcmc_lds_sort), and one lane forms the seven fields with box_stats of bayes_probs_internal.h.
// Every load and store is bounded: the paint's by the verdict of paint_check_kernel, the box's by N, which the host refuses
// above MCMC_MAX_POOLED before any launch.  -ffp-contract=off: lower - 1.5 * iqr is two rounded operations.
#include <algorithm>

#include "icnv_internal.h"
#include "bayes_probs_internal.h"

#pragma clang fp contract(off)

namespace icnv {

namespace {

constexpr int PAINT_THREADS = 256, PAINT_WAVES = PAINT_THREADS / 64;

__global__ void __launch_bounds__(PAINT_THREADS) paint_check_kernel(PaintRegions a, int64_t *verdict) {
    const int64_t stride = (int64_t)gridDim.x * PAINT_THREADS;
    const int64_t q0 = (int64_t)blockIdx.x * PAINT_THREADS + threadIdx.x;
    const int64_t total = a.cell_off[a.n_regions];
    int fault = 0;
    int64_t longest = 0, not_one = 0;
    if (q0 == 0) {
        if (a.cell_off[0] != 0 || total < 0 || total > a.n_idx) fault = 1;
        verdict[1] = total;
    }
    for (int64_t r = q0; r < a.n_regions; r += stride) {
        const int64_t g0 = a.gene_first[r], ng = a.gene_count[r];
        if (g0 < 0 || ng < 0 || g0 + ng > a.G) fault = 2;
        if (a.cell_off[r + 1] < a.cell_off[r]) fault = 1;
        if (a.cell_off[r] != r || a.cell_off[r + 1] != r + 1) not_one = 1;
        longest = max(longest, ng);
    }
    const int64_t n_cells = min(max(total, (int64_t)0), a.n_idx);
    for (int64_t i = q0; i < n_cells; i += stride) {
        const int64_t c = a.cell_idx[i];
        if (c < 0 || c >= a.C) fault = 3;
    }
    if (fault) atomicMax((unsigned long long *)&verdict[0], (unsigned long long)fault);
    if (longest > 0) atomicMax((unsigned long long *)&verdict[2], (unsigned long long)longest);
    if (not_one) atomicMax((unsigned long long *)&verdict[3], 1ull);
}

__device__ inline int paint_find_region(const int64_t *off, int n, int64_t b) {   // the last r with off[r] <= b
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (off[m] <= b) lo = m; else hi = m;
    }
    return lo;
}

template <bool ONE_CELL>
__global__ void __launch_bounds__(PAINT_THREADS) paint_owner_kernel(PaintRegions a, int64_t rows) {
    const int64_t row = (int64_t)blockIdx.x * PAINT_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    // (empty regions repeat an offset: the LAST region that starts at or before the row is the one that holds it)
    const int r = ONE_CELL ? (int)row : paint_find_region(a.cell_off, a.n_regions, row);
    const int64_t ng = a.gene_count[r];
    unsigned long long *dst = reinterpret_cast<unsigned long long *>(a.out + (int64_t)a.cell_idx[row] * a.ld + a.gene_first[r]);
    const unsigned long long owner = (unsigned long long)r + 1ull;
    for (int64_t g = (int64_t)blockIdx.y * 64 + lane; g < ng; g += (int64_t)gridDim.y * 64) atomicMax(dst + g, owner);
}

__global__ void __launch_bounds__(PAINT_THREADS) paint_value_kernel(PaintRegions a) {
    const int64_t g = (int64_t)blockIdx.x * PAINT_THREADS + threadIdx.x;
    if (g >= a.G) return;
    for (int64_t c = blockIdx.y; c < a.C; c += gridDim.y) {
        double *p = a.out + c * a.ld + g;
        const unsigned long long o = *reinterpret_cast<const unsigned long long *>(p);
        if (o) *p = a.value[o - 1];
    }
}

__global__ void __launch_bounds__(1024) theta_box_kernel(ThetaBoxArgs a) {
    extern __shared__ __attribute__((aligned(16))) double box_lds[];
    const int N = a.N, K = a.K;
    const int r = blockIdx.x / K, k = blockIdx.x - r * K;
    const int tid = threadIdx.x, nt = blockDim.x;
    const double *src = a.samples + (int64_t)r * N * K + k;
    int nan = 0;
    for (int q = tid; q < N; q += nt) {
        const double v = src[(int64_t)q * K];
        box_lds[q] = v;
        nan |= v != v;
    }
    const bool any_nan = __syncthreads_or(nan) != 0;
    if (!any_nan) mcmc_lds_sort(box_lds, N, a.n_pad, tid, nt);
    if (tid == 0) {
        double out[BOX_FIELDS];
        box_stats(box_lds, N, any_nan, out);
        double *dst = a.box + ((int64_t)r * K + k) * BOX_FIELDS;
        for (int i = 0; i < BOX_FIELDS; ++i) dst[i] = out[i];
    }
}

}  // namespace

int launch_paint_check(const PaintRegions &a, int64_t *verdict, hipStream_t s) {
    KernelTimer kt("paint_check", s);
    const int64_t work = std::max<int64_t>(a.n_regions, a.n_idx);
    const unsigned blocks = (unsigned)std::min<int64_t>((work + PAINT_THREADS - 1) / PAINT_THREADS, (int64_t)num_cus() * 8);
    hipLaunchKernelGGL(paint_check_kernel, dim3(std::max(blocks, 1u)), dim3(PAINT_THREADS), 0, s, a, verdict);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_paint(const PaintRegions &a, int64_t rows, int64_t longest, bool one_cell, hipStream_t s) {
    KernelTimer kt("paint_regions", s);
    ICNV_HIP(hipMemset2DAsync(a.out, (size_t)a.ld * sizeof(double), 0, (size_t)a.G * sizeof(double), (size_t)a.C, s));
    if (rows == 0 || longest == 0) return ICNV_OK;
    const int64_t blocks = (rows + PAINT_WAVES - 1) / PAINT_WAVES;
    if (blocks > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "paint_regions: too many (region, cell) rows");
    if (one_cell) {
        hipLaunchKernelGGL(paint_owner_kernel<true>, dim3((unsigned)blocks), dim3(PAINT_THREADS), 0, s, a, rows);
    } else {
        const unsigned pieces = (unsigned)std::min<int64_t>((longest + 63) / 64, 65535);
        hipLaunchKernelGGL(paint_owner_kernel<false>, dim3((unsigned)blocks, pieces), dim3(PAINT_THREADS), 0, s, a, rows);
    }
    ICNV_HIP(hipGetLastError());
    const unsigned gx = (unsigned)((a.G + PAINT_THREADS - 1) / PAINT_THREADS);
    const unsigned gy = (unsigned)std::min<int64_t>(a.C, 65535);
    hipLaunchKernelGGL(paint_value_kernel, dim3(gx, gy), dim3(PAINT_THREADS), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_theta_box(const ThetaBoxArgs &a, hipStream_t s) {
    KernelTimer kt("theta_box", s);
    static DeviceOnce once;
    if (int rc = ensure_dynamic_lds(reinterpret_cast<const void *>(theta_box_kernel), MCMC_MAX_POOLED * (int)sizeof(double), once))
        return rc;
    const unsigned threads = (unsigned)std::min(1024, std::max(64, a.n_pad / 2));
    hipLaunchKernelGGL(theta_box_kernel, dim3((unsigned)((int64_t)a.n_regions * a.K)), dim3(threads), (size_t)a.n_pad * sizeof(double), s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
