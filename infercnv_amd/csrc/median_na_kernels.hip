// NA-aware 2-D median denoise (K19): icnv_median_filter_na_dev.  R computes every output of apply_median_filtering as
// median(tile[a:b, c:d]) (R/noise_reduction.R:107) and median() returns NA as soon as its argument holds one NA or NaN.  The
// kernels of median_kernels.hip do not look for NaN (they are built with -fno-honor-nans), so this file keeps NaN away from them:
//
//   1. mna_scan_kernel          one read of the matrix: a wavefront takes 64 consecutive genes of a cell, ballots the NA test on the
//                               BITS (an x != x could be folded away) and one lane stores the 64-bit word of a bit mask
//                               (ceil(G / 64) words per cell: a cell starts on a word, a chromosome does not); one atomic per
//                               wavefront that saw an NA adds its count to a device counter
//   count == 0:                 the plain filter on the caller's input -- the extra cost is the scan
//   count  > 0:
//   2. mna_clean_kernel         a copy in pool scratch with 0.0 at the NA positions, bit-copied elsewhere; the plain filter runs
//                               from the copy into expr_out (a window without an NA holds no replaced element: its median is the
//                               plain entry's, whatever the NAs elsewhere were)
//   3. mna_dilate_genes_kernel  mask2 bit (cell, gene p) = any NA among the genes of p's window in that cell, the window clamped to
//                               p's chromosome (a bit range that may straddle the words of the mask)
//   4. mna_poison_kernel        per list position of a tile: the OR of mask2 over the cells of its window (clamped to the tile, in
//                               the order of the tile's index list), NA_real_ stored where a bit is set.  The two ORs together are
//                               the window of the output: [max(1, p - h), min(n, p + h)] in both directions.
//   5. mna_restore_kernel       cells in no tile: the input's own bits back at the NA positions (the plain filter copied the
//                               cleaned matrix through)
//
// No LDS, no barrier; every store is an ordinary vector store.
#include "icnv_internal.h"

#include <algorithm>
#include <vector>

namespace icnv {
namespace {

constexpr int MNA_UNROLL = 4;                              // mask words (64 genes each) per wavefront and step: four 8-byte loads in flight per lane
constexpr int MNA_WORDS_PER_WG = 4 * MNA_UNROLL;           // a workgroup of four wavefronts
constexpr uint64_t MNA_NA_REAL = 0x7FF00000000007A2ull;    // R's NA_real_: a NaN with the low word 1954

__device__ __forceinline__ bool mna_is_na(uint64_t bits) { return (bits & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull; }

// grid: x = blocks of MNA_WORDS_PER_WG words along a cell, y = cells (strided)
__global__ void __launch_bounds__(256) mna_scan_kernel(const uint64_t *__restrict__ in, int32_t G, int64_t C, int32_t Wc,
                                                       uint64_t *__restrict__ mask, unsigned long long *__restrict__ count) {
    const int lane = threadIdx.x & 63;
    const int32_t j0 = ((int32_t)blockIdx.x * 4 + (int32_t)(threadIdx.x >> 6)) * MNA_UNROLL;
    if (j0 >= Wc) return;                                  // (wave-uniform)
    unsigned long long seen = 0;
    for (int64_t c = blockIdx.y; c < C; c += gridDim.y) {
        const uint64_t *row = in + c * (int64_t)G;
        uint64_t v[MNA_UNROLL];
#pragma unroll
        for (int u = 0; u < MNA_UNROLL; ++u) {
            const int64_t g = (int64_t)(j0 + u) * 64 + lane;
            v[u] = g < G ? row[g] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < MNA_UNROLL; ++u) {
            const unsigned long long b = __ballot(mna_is_na(v[u]));
            if (j0 + u < Wc) {
                if (lane == 0) mask[c * (int64_t)Wc + j0 + u] = b;
                seen += (unsigned long long)__popcll(b);
            }
        }
    }
    if (lane == 0 && seen) atomicAdd(count, seen);
}

__global__ void __launch_bounds__(256) mna_clean_kernel(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, int64_t n) {
    const int64_t stride = (int64_t)gridDim.x * 256 * MNA_UNROLL;
    for (int64_t base = ((int64_t)blockIdx.x * 256 + threadIdx.x); base < n; base += stride) {
        uint64_t v[MNA_UNROLL];
#pragma unroll
        for (int u = 0; u < MNA_UNROLL; ++u) {
            const int64_t e = base + (int64_t)u * gridDim.x * 256;
            v[u] = e < n ? in[e] : 0ull;
        }
#pragma unroll
        for (int u = 0; u < MNA_UNROLL; ++u) {
            const int64_t e = base + (int64_t)u * gridDim.x * 256;
            if (e < n) out[e] = mna_is_na(v[u]) ? 0ull : v[u];
        }
    }
}

// the bits [a, b] (0 <= a <= b <= 191) of the 192-bit string w0 | w1 << 64 | w2 << 128: is one of them set?
__device__ __forceinline__ bool mna_range_any(uint64_t w0, uint64_t w1, uint64_t w2, int a, int b) {
    uint64_t any = 0;
    const uint64_t w[3] = {w0, w1, w2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int s = max(a, 64 * k) - 64 * k, e = min(b, 64 * k + 63) - 64 * k;
        if (s <= e) any |= w[k] & (~0ull >> (63 - e)) & (~0ull << s);
    }
    return any != 0;
}

// gene_lo_hi[g] = {first gene of g's chromosome, its last gene}
__global__ void __launch_bounds__(256) mna_dilate_genes_kernel(const uint64_t *__restrict__ mask, uint64_t *__restrict__ mask2, int32_t G,
                                                               int64_t C, int32_t Wc, const int2 *__restrict__ gene_lo_hi, int h) {
    const int lane = threadIdx.x & 63;
    const int32_t j = (int32_t)blockIdx.x * 4 + (int32_t)(threadIdx.x >> 6);
    if (j >= Wc) return;                                   // (wave-uniform)
    const int64_t g = (int64_t)j * 64 + lane;
    int2 lh = make_int2(0, -1);
    if (g < G) lh = gene_lo_hi[g];
    const int base = (j - 1) * 64;                         // gene of bit 0 of the three words
    const int a = max(lh.x, (int)g - h) - base, b = (int)min((int64_t)lh.y, g + h) - base;
    for (int64_t c = blockIdx.y; c < C; c += gridDim.y) {
        const uint64_t *row = mask + c * (int64_t)Wc;
        const uint64_t w0 = j > 0 ? row[j - 1] : 0ull, w1 = row[j], w2 = j + 1 < Wc ? row[j + 1] : 0ull;   // (the same word in every lane)
        unsigned long long r = 0;
        if (w0 | w1 | w2) r = __ballot(g < G && mna_range_any(w0, w1, w2, a, b));
        if (lane == 0) mask2[c * (int64_t)Wc + j] = r;
    }
}

// one wavefront per (list position i, 64 words of its cell's row); tile_lo_hi[i] = {first list position of i's tile, one past its last}
__global__ void __launch_bounds__(256) mna_poison_kernel(const uint64_t *__restrict__ mask2, uint64_t *__restrict__ out, int32_t G, int32_t Wc,
                                                         const int32_t *__restrict__ tile_idx, const int2 *__restrict__ tile_lo_hi,
                                                         int64_t n_list, int32_t chunks, int h) {
    const int lane = threadIdx.x & 63;
    const int64_t wv = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (wv >= n_list * chunks) return;                     // (wave-uniform)
    const int64_t i = wv / chunks;
    const int32_t j = (int32_t)(wv - i * chunks) * 64 + lane;
    const int2 t = tile_lo_hi[i];
    const int64_t qa = max((int64_t)t.x, i - h), qb = min((int64_t)t.y - 1, i + h);
    uint64_t m = 0;
    if (j < Wc)
        for (int64_t q = qa; q <= qb; ++q) m |= mask2[(int64_t)tile_idx[q] * Wc + j];
    unsigned long long nz = __ballot(m != 0);
    if (!nz) return;
    uint64_t *row = out + (int64_t)tile_idx[i] * G;
    const int32_t jw = (int32_t)(wv - i * chunks) * 64;
    while (nz) {                                           // (wave-uniform: the words of this chunk that poison an output)
        const int r = __ffsll((long long)nz) - 1;
        nz &= nz - 1;
        const uint64_t mr = __shfl(m, r);
        const int64_t g = (int64_t)(jw + r) * 64 + lane;
        if (((mr >> lane) & 1ull) && g < G) row[g] = MNA_NA_REAL;
    }
}

// grid: x = words along a cell (one per wavefront), y = the cells of `cells` (strided)
__global__ void __launch_bounds__(256) mna_restore_kernel(const uint64_t *__restrict__ in, uint64_t *__restrict__ out, int32_t G, int32_t Wc,
                                                          const uint64_t *__restrict__ mask, const int32_t *__restrict__ cells, int64_t n_cells) {
    const int lane = threadIdx.x & 63;
    const int32_t j = (int32_t)blockIdx.x * 4 + (int32_t)(threadIdx.x >> 6);
    if (j >= Wc) return;
    const int64_t g = (int64_t)j * 64 + lane;
    for (int64_t k = blockIdx.y; k < n_cells; k += gridDim.y) {
        const int64_t c = cells[k];
        const uint64_t m = mask[c * (int64_t)Wc + j];
        if (((m >> lane) & 1ull) && g < G) out[c * (int64_t)G + g] = in[c * (int64_t)G + g];
    }
}

template <typename T>
int mna_upload(DevBuf &b, const std::vector<T> &host, hipStream_t s) {
    int rc = b.alloc(std::max<size_t>(host.size(), 1) * sizeof(T));
    if (rc) return rc;
    if (!host.empty()) ICNV_HIP(hipMemcpyAsync(b.p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return ICNV_OK;
}

unsigned mna_grid_y(int64_t n, unsigned grid_x) {          // ~16 workgroups per CU over the whole grid, the rest of the cells strided
    const int64_t want = std::max<int64_t>(1, ((int64_t)num_cus() * 16 + grid_x - 1) / grid_x);
    return (unsigned)std::min<int64_t>(std::min<int64_t>(n, want), 65535);
}

// the refusals of icnv_median_filter_dev, before any launch
int mna_validate(const double *expr_in, double *expr_out, int64_t G, int64_t C, const int32_t *chr_start, int32_t n_chr,
                 const int32_t *tile_idx, const int32_t *tile_off, int32_t n_tiles, int32_t window_size) {
    if (!expr_in || !expr_out || G < 1 || C < 0 || G > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "bad argument");
    if (expr_in == expr_out) ICNV_FAIL(ICNV_ERR_ARG, "median filter cannot run in place");
    if (window_size < 1) ICNV_FAIL(ICNV_ERR_ARG, "window_size must be >= 1");
    if (!chr_start || n_chr < 1) ICNV_FAIL(ICNV_ERR_ARG, "chr_start/n_chr missing");
    if (chr_start[0] != 0 || chr_start[n_chr] != G) ICNV_FAIL(ICNV_ERR_ARG, "chr_start must run from 0 to G");
    for (int k = 0; k < n_chr; ++k)
        if (chr_start[k + 1] < chr_start[k]) ICNV_FAIL(ICNV_ERR_ARG, "chr_start must be non-decreasing");
    if (n_tiles < 0 || (n_tiles > 0 && (!tile_off || tile_off[0] != 0))) ICNV_FAIL(ICNV_ERR_ARG, "tiles: bad offsets");
    for (int t = 0; t < n_tiles; ++t)
        if (tile_off[t + 1] < tile_off[t]) ICNV_FAIL(ICNV_ERR_ARG, "tiles: offsets must be non-decreasing");
    const int64_t n = n_tiles > 0 ? tile_off[n_tiles] : 0;
    if (n > 0 && !tile_idx) ICNV_FAIL(ICNV_ERR_ARG, "tiles: index vector missing");
    for (int64_t i = 0; i < n; ++i)
        if (tile_idx[i] < 0 || tile_idx[i] >= C) ICNV_FAIL(ICNV_ERR_ARG, "tiles: cell index out of range");
    if (n_tiles > 0 && (window_size - 1) / 2 + 1 > 8) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "median filter supports window_size <= 15");
    return ICNV_OK;
}

}  // namespace
}  // namespace icnv

using namespace icnv;

extern "C" int icnv_median_filter_na_dev(const double *expr_in, double *expr_out, int64_t G, int64_t C, const int32_t *chr_start,
                                         int32_t n_chr, const int32_t *tile_idx, const int32_t *tile_off, int32_t n_tiles,
                                         int32_t window_size, int64_t *n_na_out, void *stream) {
    int rc = mna_validate(expr_in, expr_out, G, C, chr_start, n_chr, tile_idx, tile_off, n_tiles, window_size);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (n_na_out) *n_na_out = 0;
    if (C == 0) return icnv_median_filter_dev(expr_in, expr_out, G, C, chr_start, n_chr, tile_idx, tile_off, n_tiles, window_size, stream);
    const int32_t Wc = (int32_t)((G + 63) / 64);
    const size_t mask_bytes = (size_t)C * (size_t)Wc * sizeof(uint64_t);
    DevBuf d_mask, d_count;
    if ((rc = d_mask.alloc(mask_bytes)) || (rc = d_count.alloc(sizeof(unsigned long long)))) return rc;
    const uint64_t *in_bits = reinterpret_cast<const uint64_t *>(expr_in);
    uint64_t *out_bits = reinterpret_cast<uint64_t *>(expr_out);
    unsigned long long n_na = 0;
    {
        KernelTimer kt("median_na_scan", s);
        ICNV_HIP(hipMemsetAsync(d_count.p, 0, sizeof(unsigned long long), s));
        const unsigned gx = (unsigned)((Wc + MNA_WORDS_PER_WG - 1) / MNA_WORDS_PER_WG);
        hipLaunchKernelGGL(mna_scan_kernel, dim3(gx, mna_grid_y(C, gx)), dim3(256), 0, s, in_bits, (int32_t)G, C, Wc, d_mask.as<uint64_t>(),
                           d_count.as<unsigned long long>());
        ICNV_HIP(hipGetLastError());
    }
    // the count decides which launches follow: the one host wait of this entry
    ICNV_HIP(hipMemcpyAsync(&n_na, d_count.p, sizeof(n_na), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (n_na_out) *n_na_out = (int64_t)n_na;
    if (n_na == 0)
        return icnv_median_filter_dev(expr_in, expr_out, G, C, chr_start, n_chr, tile_idx, tile_off, n_tiles, window_size, stream);

    const int64_t n = G * C;
    DevBuf d_clean;
    if ((rc = d_clean.alloc((size_t)n * sizeof(double)))) return rc;
    {
        KernelTimer kt("median_na_clean", s);
        const unsigned grid = (unsigned)std::min<int64_t>((n + 256 * MNA_UNROLL - 1) / (256 * MNA_UNROLL), (int64_t)num_cus() * 16);
        hipLaunchKernelGGL(mna_clean_kernel, dim3(grid), dim3(256), 0, s, in_bits, d_clean.as<uint64_t>(), n);
        ICNV_HIP(hipGetLastError());
    }
    if ((rc = icnv_median_filter_dev(d_clean.as<double>(), expr_out, G, C, chr_start, n_chr, tile_idx, tile_off, n_tiles, window_size, stream)))
        return rc;

    const int h = (window_size - 1) / 2 + 1;
    const int64_t n_list = n_tiles > 0 ? tile_off[n_tiles] : 0;
    std::vector<int2> gene_lo_hi((size_t)G), tile_lo_hi((size_t)n_list);
    for (int k = 0; k < n_chr; ++k)
        for (int32_t g = chr_start[k]; g < chr_start[k + 1]; ++g) gene_lo_hi[(size_t)g] = make_int2(chr_start[k], chr_start[k + 1] - 1);
    std::vector<char> tiled((size_t)C, 0);
    for (int t = 0; t < n_tiles; ++t)
        for (int32_t i = tile_off[t]; i < tile_off[t + 1]; ++i) {
            tile_lo_hi[(size_t)i] = make_int2(tile_off[t], tile_off[t + 1]);
            tiled[(size_t)tile_idx[i]] = 1;
        }
    std::vector<int32_t> untiled;
    for (int64_t c = 0; c < C; ++c)
        if (!tiled[(size_t)c]) untiled.push_back((int32_t)c);
    KernelTimer kt("median_na_fixup", s);
    if (n_list > 0) {
        DevBuf d_mask2, d_gene, d_tile, d_idx;
        if ((rc = d_mask2.alloc(mask_bytes)) || (rc = mna_upload(d_gene, gene_lo_hi, s)) || (rc = mna_upload(d_tile, tile_lo_hi, s))) return rc;
        std::vector<int32_t> idx(tile_idx, tile_idx + n_list);
        if ((rc = mna_upload(d_idx, idx, s))) return rc;
        const unsigned gx = (unsigned)((Wc + 3) / 4);
        hipLaunchKernelGGL(mna_dilate_genes_kernel, dim3(gx, mna_grid_y(C, gx)), dim3(256), 0, s, (const uint64_t *)d_mask.as<uint64_t>(),
                           d_mask2.as<uint64_t>(), (int32_t)G, C, Wc, (const int2 *)d_gene.as<int2>(), h);
        const int32_t chunks = (Wc + 63) / 64;
        const int64_t blocks = (n_list * chunks + 3) / 4;
        if (blocks > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "median filter: more than 2^31 workgroups in one call");
        hipLaunchKernelGGL(mna_poison_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const uint64_t *)d_mask2.as<uint64_t>(), out_bits, (int32_t)G,
                           Wc, (const int32_t *)d_idx.as<int32_t>(), (const int2 *)d_tile.as<int2>(), n_list, chunks, h);
        ICNV_HIP(hipGetLastError());
    }
    if (!untiled.empty()) {
        DevBuf d_cells;
        if ((rc = mna_upload(d_cells, untiled, s))) return rc;
        const unsigned gx = (unsigned)((Wc + 3) / 4);
        hipLaunchKernelGGL(mna_restore_kernel, dim3(gx, mna_grid_y((int64_t)untiled.size(), gx)), dim3(256), 0, s, in_bits, out_bits, (int32_t)G, Wc,
                           (const uint64_t *)d_mask.as<uint64_t>(), (const int32_t *)d_cells.as<int32_t>(), (int64_t)untiled.size());
        ICNV_HIP(hipGetLastError());
    }
    return ICNV_OK;
}
