// Euclidean distances between the cells of a group: dist / parallelDist(t(expr[genes, cells])) as the reference calls it
// before hclust (R/inferCNV_tumor_subclusters.R:191, 582, 609, R/inferCNV_ops.R:1930, 3242).  Used by K7
// (icnv_cell_distances_dev), by K9's fused hclust (icnv_hclust_cells_dev) and by K10's random trees, which all hold the
// result bit for bit to R's sequential dist:
//
//   d2_ij = sum over the listed genes g, in list order, of fl(fl(x_gi - x_gj)^2)     raw values, no centring, no FMA
//   D_ij  = sqrt(d2_ij) (correctly rounded),  D_ii = 0
//
// A Gram formulation (|y_i|^2 + |y_j|^2 - 2 y_i.y_j) cancels: two identical cells come out a few ulps of |y|^2 apart and
// near-identical ones with relative errors of order 1, which reorders the hierarchical clustering's tied merges.  Here a
// pair-gene is three fp64 VALU operations (sub, mul, add), in the order above.  This file is compiled with
// -ffp-contract=off (Makefile): the mul and add must not become an FMA.
//
// One workgroup = one DT x DT upper-triangular tile of one problem (tile -> problem through tile_off, so a batch of problems
// is one launch).  Its 256 threads form a 16 x 16 grid, each owning an R x R register block of pairs; operand chunks of
// KC genes of the tile's DT row cells and DT column cells are staged gene-major through LDS.
#include "icnv_internal.h"

namespace icnv {

namespace {

constexpr int KC = 16;   // genes per LDS stage

__device__ __forceinline__ int find_tile_problem(const int64_t *__restrict__ off, int n, int64_t v) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <int R>
__global__ void __launch_bounds__(256, (R == 8 ? 2 : 4)) exact_dist_kernel(DistArgs a) {
    constexpr int DT = 16 * R;
    constexpr int LD = DT + 2;          // LDS stride of one gene's row (doubles): even, so the R-wide reads stay 16-byte aligned
    constexpr int PER = DT * KC / 256;  // values staged per thread and operand
    __shared__ __attribute__((aligned(16))) double As[KC * LD], Bs[KC * LD];
    __shared__ int64_t base_a[DT], base_b[DT];

    const int p = find_tile_problem(a.tile_off, a.n_prob, blockIdx.x);
    int64_t rem = blockIdx.x - a.tile_off[p];
    const int n = a.n[p];
    const int nt = (n + DT - 1) / DT;
    int bi = 0;
    while (rem >= nt - bi) { rem -= nt - bi; ++bi; }
    const int bj = bi + (int)rem;
    const int32_t *gidx = a.gene_idx ? a.gene_idx + a.gene_off[p] : nullptr;
    const int G = a.gene_idx ? (int)(a.gene_off[p + 1] - a.gene_off[p]) : a.G;
    const int32_t *cidx = a.cell_idx + a.cell_off[p];

    const int t = threadIdx.x;
    for (int r = t; r < DT; r += 256) {   // each row's first value; -1: a row past the problem's end
        const int ra = bi * DT + r, rb = bj * DT + r;
        base_a[r] = ra < n ? (int64_t)cidx[ra] * a.ldx : -1;
        base_b[r] = rb < n ? (int64_t)cidx[rb] * a.ldx : -1;
    }
    // staging: thread t moves gene k = t % KC of rows t / KC + 16 q -- consecutive lanes read consecutive genes of one cell
    const int sk = t % KC, sr = t / KC;
    const int ty = t >> 4, tx = t & 15;
    double s[R][R];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < R; ++j) s[i][j] = 0.0;

    for (int k0 = 0; k0 < G; k0 += KC) {
        __syncthreads();   // the previous stage is consumed (first pass: the row bases are written)
        const int g = k0 + sk;
        const int64_t gene = g < G ? (gidx ? gidx[g] : g) : -1;
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int r = sr + 16 * q;
            const int64_t ba = base_a[r], bb = base_b[r];
            // a gene past the end reads 0 in both operands: fl(0 - 0)^2 = +0 leaves every sum unchanged
            As[sk * LD + r] = (gene >= 0 && ba >= 0) ? a.x[ba + gene] : 0.0;
            Bs[sk * LD + r] = (gene >= 0 && bb >= 0) ? a.x[bb + gene] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < KC; ++k) {
            double av[R], bv[R];
#pragma unroll
            for (int i = 0; i < R; i += 2) {
                const double2 va = *reinterpret_cast<const double2 *>(&As[k * LD + ty * R + i]);
                const double2 vb = *reinterpret_cast<const double2 *>(&Bs[k * LD + tx * R + i]);
                av[i] = va.x; av[i + 1] = va.y;
                bv[i] = vb.x; bv[i + 1] = vb.y;
            }
#pragma unroll
            for (int i = 0; i < R; ++i)
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    const double d = __dsub_rn(av[i], bv[j]);
                    s[i][j] = __dadd_rn(s[i][j], __dmul_rn(d, d));
                }
        }
    }

    // one value per pair, mirrored: fl(a - b)^2 == fl(b - a)^2, so the matrix is exactly symmetric either way
    double *Dp = a.D + a.d_off[p];
#pragma unroll
    for (int i = 0; i < R; ++i)
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int row = bi * DT + ty * R + i, col = bj * DT + tx * R + j;
            if (row < n && col < n && row <= col) {
                const double v = row == col ? 0.0 : __dsqrt_rn(s[i][j]);
                Dp[(int64_t)row * n + col] = v;
                Dp[(int64_t)col * n + row] = v;
            }
        }
}

}  // namespace

int exact_dist_plan(const int32_t *n, int32_t n_prob, std::vector<int64_t> &tile_off) {
    // 128-cell tiles (8 x 8 pairs per thread) when they still fill the chip twice over, 64-cell tiles (4 x 4) otherwise
    int64_t t128 = 0;
    for (int32_t p = 0; p < n_prob; ++p) {
        const int64_t nt = (n[p] + 127) / 128;
        t128 += nt * (nt + 1) / 2;
    }
    const int DT = t128 >= 2 * (int64_t)num_cus() ? 128 : 64;
    tile_off.assign((size_t)n_prob + 1, 0);
    for (int32_t p = 0; p < n_prob; ++p) {
        const int64_t nt = (n[p] + DT - 1) / DT;
        tile_off[p + 1] = tile_off[p] + nt * (nt + 1) / 2;
    }
    return DT;
}

int launch_exact_dist(const DistArgs &a, int dt, int64_t n_tiles, hipStream_t stream) {
    if (n_tiles <= 0) return ICNV_OK;
    if (n_tiles > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "too many cells for one distance launch");
    KernelTimer kt("exact_dist", stream);
    if (dt == 128)
        hipLaunchKernelGGL(exact_dist_kernel<8>, dim3((unsigned)n_tiles), dim3(256), 0, stream, a);
    else
        hipLaunchKernelGGL(exact_dist_kernel<4>, dim3((unsigned)n_tiles), dim3(256), 0, stream, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
