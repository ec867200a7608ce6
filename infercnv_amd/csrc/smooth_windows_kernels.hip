// K16: the banded window operator of step 10's "runmeans" and "coordinates" smoothers (R/inferCNV_ops.R:2534-2704):
//   out[g, c] = (sum over t = 0 .. len[g] - 1, in this order, of x[lo[g] + t, c] * w[w_off[g] + t]) / denom[g]
// one rounding per product, one per add, one division.  DESIGN.md section 4 K16.
//
//   sw_kernel<WEIGHTED, SPILL>   a workgroup owns a tile of up to 1024 output genes and SW_CB cells.  It stages the rows the
//                                tile's windows span into LDS once per cell; a lane owns SW_U adjacent genes for all the cells.
//                                The rows the lane's windows share ([max lo, min lo + len)) are read once and added to all
//                                SW_U x SW_CB sums; what a window has in front of and behind that range is summed by itself
//                                before and after it, so every sum still runs in t order.  SPILL: a tile whose span exceeds the
//                                LDS budget reads the rows from HBM with the same code.
//
// This file is compiled with -ffp-contract=off (Makefile): a product and its add must not become an FMA.
#include "icnv_internal.h"
#include "smooth_windows_internal.h"

namespace icnv {

namespace {

template <bool WEIGHTED, bool SPILL>
__global__ void __launch_bounds__(SW_NT) sw_kernel(SwArgs a) {
    __shared__ double sm[SPILL ? 1 : SW_CB][SPILL ? 1 : SW_LDS_ROWS];
    const SwTile tile = a.tiles[(SPILL ? a.n_lds : 0) + blockIdx.y];
    const int64_t c0 = (int64_t)blockIdx.x * SW_CB;
    const double *col[SW_CB];
#pragma unroll
    for (int c = 0; c < SW_CB; ++c) col[c] = a.x + (c0 + c < a.C ? c0 + c : a.C - 1) * a.ldx;   // a cell past C repeats the last one
    uint32_t bad = 0;

    if (!SPILL) {
#pragma unroll
        for (int c = 0; c < SW_CB; ++c) {
            const double *src = col[c] + tile.span_lo;
            for (int r = threadIdx.x; r < tile.span_len; r += SW_NT) {
                const double v = src[r];
                if (!isfinite(v)) bad = 1;
                sm[c][sw_skew(r)] = v;
            }
        }
        __syncthreads();
    }

    const int gb = tile.g0 + (int)threadIdx.x * SW_U;
    const int nvalid = tile.g1 - gb < SW_U ? tile.g1 - gb : SW_U;
    if (nvalid > 0) {
        int lo[SW_U], hi[SW_U];
        int64_t wo[SW_U];      // weight of row q of window u: w[wo[u] + q]
        double den[SW_U];
        int A = 0, B = 0x7fffffff;
#pragma unroll
        for (int u = 0; u < SW_U; ++u) {
            const int g = gb + (u < nvalid ? u : nvalid - 1);   // a gene past the tile repeats the last one and is not stored
            lo[u] = a.lo[g];
            hi[u] = lo[u] + a.len[g];
            wo[u] = WEIGHTED ? a.w_off[g] - lo[u] : 0;
            den[u] = a.denom[g];
            A = lo[u] > A ? lo[u] : A;
            B = hi[u] < B ? hi[u] : B;
        }
        const bool shared = A < B;
        double s[SW_U][SW_CB];
#pragma unroll
        for (int u = 0; u < SW_U; ++u)
#pragma unroll
            for (int c = 0; c < SW_CB; ++c) s[u][c] = 0.0;

        auto load = [&](int c, int q) -> double {
            if (SPILL) {
                const double v = col[c][q];
                if (!isfinite(v)) bad = 1;
                return v;
            }
            return sm[c][sw_skew(q - tile.span_lo)];
        };
        auto own = [&](int u, int q0, int q1) {   // rows [q0, q1) of window u alone
            for (int q = q0; q < q1; ++q) {
                if (WEIGHTED) {
                    const double wv = a.w[wo[u] + q];
#pragma unroll
                    for (int c = 0; c < SW_CB; ++c) s[u][c] = s[u][c] + load(c, q) * wv;
                } else {
#pragma unroll
                    for (int c = 0; c < SW_CB; ++c) s[u][c] = s[u][c] + load(c, q);
                }
            }
        };

#pragma unroll
        for (int u = 0; u < SW_U; ++u) own(u, lo[u], shared ? A : hi[u]);
        if (shared) {
            for (int q = A; q < B; ++q) {
                double v[SW_CB];
#pragma unroll
                for (int c = 0; c < SW_CB; ++c) v[c] = load(c, q);
#pragma unroll
                for (int u = 0; u < SW_U; ++u) {
                    if (WEIGHTED) {
                        const double wv = a.w[wo[u] + q];
#pragma unroll
                        for (int c = 0; c < SW_CB; ++c) s[u][c] = s[u][c] + v[c] * wv;
                    } else {
#pragma unroll
                        for (int c = 0; c < SW_CB; ++c) s[u][c] = s[u][c] + v[c];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < SW_U; ++u) own(u, B, hi[u]);
        }

#pragma unroll
        for (int c = 0; c < SW_CB; ++c) {
            if (c0 + c >= a.C) break;
            double *dst = a.out + (c0 + c) * a.ldo + gb;
#pragma unroll
            for (int u = 0; u < SW_U; ++u)
                if (u < nvalid) dst[u] = s[u][c] / den[u];
        }
    }
    if (bad) atomicOr(a.flag, 1u);
}

template <bool WEIGHTED>
int launch_both(const SwArgs &a, unsigned cell_blocks, hipStream_t s) {
    if (a.n_lds > 0) {
        hipLaunchKernelGGL((sw_kernel<WEIGHTED, false>), dim3(cell_blocks, (unsigned)a.n_lds), dim3(SW_NT), 0, s, a);
        ICNV_HIP(hipGetLastError());
    }
    if (a.n_spill > 0) {
        hipLaunchKernelGGL((sw_kernel<WEIGHTED, true>), dim3(cell_blocks, (unsigned)a.n_spill), dim3(SW_NT), 0, s, a);
        ICNV_HIP(hipGetLastError());
    }
    return ICNV_OK;
}

}  // namespace

int launch_smooth_windows(const SwArgs &a, hipStream_t s) {
    if (a.n_lds > 65535 || a.n_spill > 65535) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "smooth_windows: more than 65535 gene tiles");
    const int64_t cell_blocks = (a.C + SW_CB - 1) / SW_CB;
    KernelTimer kt("smooth_windows", s);
    return a.w ? launch_both<true>(a, (unsigned)cell_blocks, s) : launch_both<false>(a, (unsigned)cell_blocks, s);
}

}  // namespace icnv
