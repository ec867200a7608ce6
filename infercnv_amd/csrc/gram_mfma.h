// The fp64 matrix-core tile product of the exact kNN's screen (knn_kernels.hip, K8): one workgroup of 4 wavefronts
// accumulates the DT x DT block  A B^T  of two row sets, DT = 32 WM, with v_mfma_f64_16x16x4_f64.  A row is given by a
// pointer to its first element (nullptr: a row past the end, read as zeros); the rows' elements 0 .. G-1 are contracted.
#pragma once
#include <hip/hip_runtime.h>

namespace icnv {
namespace gram {

typedef double dbl4_t __attribute__((ext_vector_type(4)));

constexpr int KC = 32;        // genes per LDS stage
constexpr int LDR = KC + 2;   // LDS row stride in doubles: (4 row + 2 k) dwords mod 64 are distinct within a 32-lane group

constexpr size_t lds_bytes(int WM) { return (size_t)2 * 32 * WM * LDR * sizeof(double); }

// One workgroup = 4 wavefronts = 2 x 2 sub-tiles; a wavefront holds WM x WM MFMA accumulators (16 x 16 each).
// Every row starts at an even element and G is even (16-byte loads).
// C/D layout of the result: acc[a][b][reg] is row wr * 16 WM + 16 a + (lane >> 4) + 4 reg, column wc * 16 WM + 16 b + (lane & 15)
// of the tile, with w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1.
template <int WM>
__device__ __forceinline__ void tile_product(const double *const (&pa)[WM / 2], const double *const (&pb)[WM / 2], int G,
                                             double *smem_d, dbl4_t (&acc)[WM][WM]) {
    constexpr int DT = 32 * WM;
    constexpr int RPT = DT / 64;          // rows staged per thread and tile
    double *As = smem_d;
    double *Bs = smem_d + DT * LDR;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int wr = w >> 1, wc = w & 1;
#pragma unroll
    for (int a = 0; a < WM; ++a)
#pragma unroll
        for (int b = 0; b < WM; ++b) acc[a][b] = (dbl4_t){0.0, 0.0, 0.0, 0.0};

    // staging: thread t loads 8 consecutive genes of rows t / 4 (+ 64) of each tile.  The next stage is requested into
    // registers before the current stage's MFMAs and parked in LDS after them: its HBM/L2 latency hides behind the
    // matrix instructions instead of standing between barriers.
    const int lrow = t >> 2, lseg = (t & 3) * 8;
    double ra_v[RPT][8], rb_v[RPT][8];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int r = 0; r < RPT; ++r) {
#pragma unroll
            for (int j = 0; j < 8; j += 2) {
                const int g = k0 + lseg + j;
                const bool in = g < G;
                const double2 va = (pa[r] && in) ? *reinterpret_cast<const double2 *>(pa[r] + g) : make_double2(0.0, 0.0);
                const double2 vb = (pb[r] && in) ? *reinterpret_cast<const double2 *>(pb[r] + g) : make_double2(0.0, 0.0);
                ra_v[r][j] = va.x; ra_v[r][j + 1] = va.y;
                rb_v[r][j] = vb.x; rb_v[r][j + 1] = vb.y;
            }
        }
    };
    auto park = [&]() {
#pragma unroll
        for (int r = 0; r < RPT; ++r)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                As[(lrow + 64 * r) * LDR + lseg + j] = ra_v[r][j];
                Bs[(lrow + 64 * r) * LDR + lseg + j] = rb_v[r][j];
            }
    };
    fetch(0);
    park();
    __syncthreads();
    for (int k0 = 0; k0 < G; k0 += KC) {
        const bool more = k0 + KC < G;
        if (more) fetch(k0 + KC);
#pragma unroll
        for (int kk = 0; kk < KC; kk += 4) {
            const int k = kk + (lane >> 4), r = lane & 15;
            double av[WM], bv[WM];
#pragma unroll
            for (int a = 0; a < WM; ++a) {
                av[a] = As[(wr * 16 * WM + 16 * a + r) * LDR + k];
                bv[a] = Bs[(wc * 16 * WM + 16 * a + r) * LDR + k];
            }
#pragma unroll
            for (int a = 0; a < WM; ++a)
#pragma unroll
                for (int b = 0; b < WM; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
        }
        __syncthreads();   // every wavefront is done with this stage's tiles
        if (more) park();
        __syncthreads();
    }
}

}  // namespace gram
}  // namespace icnv
