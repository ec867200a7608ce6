// K17: the data layer of plot_cnv (R/inferCNV_heatmap.R).  DESIGN.md section 4 K17.
//
//   hm_hist_kernel<FIRST>   one radix pass of the exact selection behind quantile(x[x != exclude], probs): reads the matrix once
//                           and counts one 8-bit digit of the order-preserving key under every tracked prefix.  A workgroup
//                           counts in LDS (uint32) and adds its non-zero bins to the int64 totals once: integer counts, so the
//                           result does not depend on arrival order.  FIRST also folds in the non-finite check and min / max.
//   hm_compact_kernel       appends the keys under the tracked prefixes to the candidate list (the host has made sure it fits)
//   hm_sort_kernel          one workgroup sorts the candidate list in LDS (bitonic network)
//   hm_bins_kernel          hist(x, breaks) over the listed rows (.bincode(right = TRUE, include.lowest = TRUE) after the clamp)
//   hm_raster_kernel        the H x W panel of bin indices, nearest-neighbour sampled
//
// The hot bin: the matrix sits in 0.8 .. 1.2 and is mostly ONE value after denoising, so nearly every lane of a wavefront
// wants the same counter in most passes, and an LDS atomic costs per wavefront instruction and per conflicting lane.
// hm_wave_add therefore peels the two most wanted counters of a wavefront with a ballot each (one LDS add of the lane
// count per counter) and leaves only what remains to per-lane LDS atomics.
#include "icnv_internal.h"
#include "heatmap_internal.h"

namespace icnv {

namespace {

__device__ inline uint64_t hm_bits(double v) {
    union { double d; uint64_t u; } c;
    c.d = v;
    return c.u;
}

// Every lane of the wavefront calls this together; slot < 0: nothing to add.
__device__ inline void hm_wave_add(uint32_t *h, int slot) {
    const int lane = (int)(threadIdx.x & 63);
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        const unsigned long long act = __ballot(slot >= 0);
        if (!act) return;                                  // wave-uniform
        const int leader = __ffsll(act) - 1;
        const int s = __shfl(slot, leader);
        const unsigned long long same = __ballot(slot == s);
        if (lane == leader) atomicAdd(&h[s], (uint32_t)__popcll(same));
        if (slot == s) slot = -1;
    }
    if (slot >= 0) atomicAdd(&h[slot], 1u);
}

// the slot of a kept key under the tracked prefixes, or -1
__device__ inline int hm_match(const HmScan &a, uint64_t key) {
    if (a.n_prefix == 0) return 0;
    const uint64_t pk = key >> a.match_shift;
    int j = -1;
    for (int q = 0; q < a.n_prefix; ++q)
        if (pk == a.prefix[q]) j = q;
    return j;
}

template <bool FIRST>
__global__ void __launch_bounds__(HM_NT) hm_hist_kernel(HmScan a) {
    __shared__ uint32_t h[HM_MAX_PREFIX * HM_BINS];
    __shared__ unsigned long long red[3][HM_NT / 64];
    const int nslots = (a.n_prefix > 0 ? a.n_prefix : 1) * HM_BINS;
    for (int i = threadIdx.x; i < nslots; i += HM_NT) h[i] = 0;
    __syncthreads();
    uint64_t kmin = ~0ull, kmax = 0;
    uint32_t bad = 0;
    for (int64_t q = blockIdx.x; q < a.n_chunks; q += gridDim.x) {
        const int64_t row = q / a.chunks_per_row;
        const int64_t base = (q - row * a.chunks_per_row) * HM_CHUNK + threadIdx.x;
        const double *p = a.x + row * a.ld;
        double v[HM_PER_LANE];
#pragma unroll
        for (int k = 0; k < HM_PER_LANE; ++k) {
            const int64_t col = base + (int64_t)k * HM_NT;
            v[k] = col < a.G ? p[col] : a.exclude;
        }
#pragma unroll
        for (int k = 0; k < HM_PER_LANE; ++k) {
            const bool valid = base + (int64_t)k * HM_NT < a.G;
            int slot = -1;
            if (valid) {
                const uint64_t key = hm_key(v[k]);
                if (FIRST) {
                    if (((hm_bits(v[k]) >> 52) & 0x7ff) == 0x7ff) bad = 1;
                    kmin = key < kmin ? key : kmin;
                    kmax = key > kmax ? key : kmax;
                }
                if (v[k] != a.exclude) {
                    const int j = hm_match(a, key);
                    if (j >= 0) slot = j * HM_BINS + (int)((key >> a.digit_shift) & (HM_BINS - 1));
                }
            }
            hm_wave_add(h, slot);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nslots; i += HM_NT)
        if (h[i]) atomicAdd(&a.hist[i], (unsigned long long)h[i]);
    if (FIRST) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t m0 = __shfl_xor((unsigned long long)kmin, o), m1 = __shfl_xor((unsigned long long)kmax, o);
            kmin = m0 < kmin ? m0 : kmin;
            kmax = m1 > kmax ? m1 : kmax;
            bad |= __shfl_xor(bad, o);
        }
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { red[0][w] = kmin; red[1][w] = kmax; red[2][w] = bad; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int i = 1; i < HM_NT / 64; ++i) {
                kmin = red[0][i] < kmin ? red[0][i] : kmin;
                kmax = red[1][i] > kmax ? red[1][i] : kmax;
                bad |= (uint32_t)red[2][i];
            }
            atomicMin(&a.summary[0], (unsigned long long)kmin);
            atomicMax(&a.summary[1], (unsigned long long)kmax);
            if (bad) atomicOr(&a.summary[2], 1ull);
        }
    }
}

__global__ void __launch_bounds__(HM_NT) hm_compact_kernel(HmScan a) {
    const int lane = (int)(threadIdx.x & 63);
    for (int64_t q = blockIdx.x; q < a.n_chunks; q += gridDim.x) {
        const int64_t row = q / a.chunks_per_row;
        const int64_t base = (q - row * a.chunks_per_row) * HM_CHUNK + threadIdx.x;
        const double *p = a.x + row * a.ld;
        double v[HM_PER_LANE];
#pragma unroll
        for (int k = 0; k < HM_PER_LANE; ++k) {
            const int64_t col = base + (int64_t)k * HM_NT;
            v[k] = col < a.G ? p[col] : a.exclude;
        }
#pragma unroll
        for (int k = 0; k < HM_PER_LANE; ++k) {
            const bool valid = base + (int64_t)k * HM_NT < a.G;
            const uint64_t key = hm_key(v[k]);
            const bool m = valid && v[k] != a.exclude && hm_match(a, key) >= 0;
            const unsigned long long mask = __ballot(m);
            if (!mask) continue;                           // wave-uniform
            const int leader = __ffsll(mask) - 1;
            uint32_t at = 0;
            if (lane == leader) at = atomicAdd(a.n_cand, (uint32_t)__popcll(mask));
            at = __shfl(at, leader);
            if (m) {
                const uint32_t idx = at + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
                if (idx < (uint32_t)HM_CAND) a.cand[idx] = key;   // the host's counts say it fits; never write past the list
            }
        }
    }
}

__global__ void __launch_bounds__(HM_NT) hm_sort_kernel(uint64_t *cand, const uint32_t *n_cand) {
    __shared__ uint64_t s[HM_CAND];
    const uint32_t n = *n_cand < (uint32_t)HM_CAND ? *n_cand : (uint32_t)HM_CAND;
    for (int i = threadIdx.x; i < HM_CAND; i += HM_NT) s[i] = (uint32_t)i < n ? cand[i] : ~0ull;
    __syncthreads();
    for (int k = 2; k <= HM_CAND; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < HM_CAND; i += HM_NT) {
                const int l = i ^ j;
                if (l > i) {
                    const uint64_t x = s[i], y = s[l];
                    if (((i & k) == 0) ? (x > y) : (x < y)) { s[i] = y; s[l] = x; }
                }
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; (uint32_t)i < n; i += HM_NT) cand[i] = s[i];
}

// .bincode(right = TRUE, include.lowest = TRUE) of the value forced into [br[0], br[nb - 1]]: bin b holds br[b] < v <= br[b + 1],
// and v == br[0] goes in bin 0.  v is not NaN.
__device__ inline int hm_bin(const double *br, int nb, double v) {
    v = v < br[0] ? br[0] : v;
    v = v > br[nb - 1] ? br[nb - 1] : v;
    int lo = 0, hi = nb - 1;                               // the first i with br[i] >= v; br[nb - 1] >= v
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (br[mid] >= v) hi = mid; else lo = mid + 1;
    }
    return lo > 0 ? lo - 1 : 0;
}

__global__ void __launch_bounds__(HM_NT) hm_bins_kernel(HmBins a) {
    __shared__ double br[HM_MAX_BREAKS];
    __shared__ uint32_t h[HM_MAX_BREAKS - 1];
    for (int i = threadIdx.x; i < a.nb; i += HM_NT) br[i] = a.breaks[i];
    for (int i = threadIdx.x; i < a.nb - 1; i += HM_NT) h[i] = 0;
    __syncthreads();
    uint32_t bad = 0;
    for (int64_t q = blockIdx.x; q < a.n_chunks; q += gridDim.x) {
        const int64_t li = q / a.chunks_per_row;
        const int64_t base = (q - li * a.chunks_per_row) * HM_CHUNK + threadIdx.x;
        const double *p = a.x + (int64_t)a.rows[li] * a.ld;
        double v[HM_PER_LANE];
#pragma unroll
        for (int k = 0; k < HM_PER_LANE; ++k) {
            const int64_t col = base + (int64_t)k * HM_NT;
            v[k] = col < a.G ? p[col] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < HM_PER_LANE; ++k) {
            int slot = -1;
            if (base + (int64_t)k * HM_NT < a.G) {
                if (v[k] != v[k]) bad = 1;
                else slot = hm_bin(br, a.nb, v[k]);
            }
            hm_wave_add(h, slot);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < a.nb - 1; i += HM_NT)
        if (h[i]) atomicAdd(&a.counts[i], (unsigned long long)h[i]);
    if (bad) atomicOr(a.flag, 1u);
}

__global__ void __launch_bounds__(HM_NT) hm_raster_kernel(HmBins a) {
    __shared__ double br[HM_MAX_BREAKS];
    for (int i = threadIdx.x; i < a.nb; i += HM_NT) br[i] = a.breaks[i];
    __syncthreads();
    uint32_t bad = 0;
    const int64_t n_pix = a.H * a.W;
    for (int64_t px = (int64_t)blockIdx.x * HM_NT + threadIdx.x; px < n_pix; px += (int64_t)gridDim.x * HM_NT) {
        const int64_t i = px / a.W, j = px - i * a.W;
        const int64_t li = ((2 * i + 1) * a.n_rows) / (2 * a.H);
        const int64_t g = ((2 * j + 1) * a.G) / (2 * a.W);
        const double v = a.x[(int64_t)a.rows[li] * a.ld + g];
        int b = 0;
        if (v != v) bad = 1;
        else b = hm_bin(br, a.nb, v);
        a.image[px] = (uint8_t)b;
    }
    if (bad) atomicOr(a.flag, 1u);
}

}  // namespace

// workgroups of a scan: enough to fill the device, and few enough chunks each that a uint32 LDS counter cannot wrap
int hm_grid(int64_t n_chunks) {
    int64_t g = (int64_t)num_cus() * 8;
    const int64_t least = (n_chunks + (1 << 19) - 1) >> 19;   // 2^19 chunks of 2^11 values = 2^30 per workgroup
    if (g < least) g = least;
    if (g > n_chunks) g = n_chunks;
    return (int)(g < 1 ? 1 : g);
}

int launch_hm_hist(const HmScan &a, bool first, hipStream_t s) {
    KernelTimer kt("heatmap_radix", s);
    const int grid = hm_grid(a.n_chunks);
    if (first) hipLaunchKernelGGL(hm_hist_kernel<true>, dim3(grid), dim3(HM_NT), 0, s, a);
    else hipLaunchKernelGGL(hm_hist_kernel<false>, dim3(grid), dim3(HM_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_hm_compact(const HmScan &a, hipStream_t s) {
    KernelTimer kt("heatmap_compact", s);
    hipLaunchKernelGGL(hm_compact_kernel, dim3(hm_grid(a.n_chunks)), dim3(HM_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_hm_sort(uint64_t *cand, const uint32_t *n_cand, hipStream_t s) {
    KernelTimer kt("heatmap_sort", s);
    hipLaunchKernelGGL(hm_sort_kernel, dim3(1), dim3(HM_NT), 0, s, cand, n_cand);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_hm_bins(const HmBins &a, hipStream_t s) {
    KernelTimer kt("heatmap_bins", s);
    hipLaunchKernelGGL(hm_bins_kernel, dim3(hm_grid(a.n_chunks)), dim3(HM_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_hm_raster(const HmBins &a, hipStream_t s) {
    KernelTimer kt("heatmap_raster", s);
    const int64_t blocks = (a.H * a.W + HM_NT - 1) / HM_NT;
    const int64_t cap = (int64_t)num_cus() * 16;
    hipLaunchKernelGGL(hm_raster_kernel, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(HM_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
