// K25: the rectangle rewrite of removeCNV / reassignCNV (R/inferCNV_BayesNet.R:562-630, 491-540) for every region of a run
// in one launch: icnv_state_fill_regions_dev of include/icnv.h.  DESIGN.md section 4 K25.
//
//   fill_check_kernel     every index of the call against G, C and the offsets' own rules; the verdict comes back before
//                         anything is written
//   fill_regions_kernel   one wavefront per (region, cell): its lanes go along the cell's genes, so a wavefront's byte stores
//                         are one contiguous run.  When every region is one cell the wavefront IS the region (no search);
//                         else a wavefront finds its region in the offsets and takes the 64-gene pieces blockIdx.y,
//                         blockIdx.y + gridDim.y, .. of its cell.
#include <algorithm>
#include <string>

#include "icnv_internal.h"
#include "../../include/icnv.h"

namespace icnv {

namespace {

constexpr int FILL_THREADS = 256, FILL_WAVES = FILL_THREADS / 64;

struct FillRegions {
    uint8_t *states;
    int64_t G, C, ld;
    int32_t n_regions;
    const int32_t *gene_first, *gene_count;
    const int64_t *cell_off;
    const int32_t *cell_idx;
    int64_t n_idx;
    const uint8_t *value;
};

// verdict[0]: 0 or the first kind of fault seen; [1]: cell_off[n_regions]; [2]: the longest gene run; [3]: regions that are
// not exactly the one cell at their own position (0: region r is row r)
__global__ void __launch_bounds__(FILL_THREADS) fill_check_kernel(FillRegions a, int64_t *verdict) {
    const int64_t stride = (int64_t)gridDim.x * FILL_THREADS;
    const int64_t q0 = (int64_t)blockIdx.x * FILL_THREADS + threadIdx.x;
    const int64_t total = a.cell_off[a.n_regions];
    int fault = 0;
    int64_t longest = 0, not_one = 0;
    if (q0 == 0) {
        if (a.cell_off[0] != 0 || total < 0 || total > a.n_idx) fault = 1;
        verdict[1] = total;
    }
    for (int64_t r = q0; r < a.n_regions; r += stride) {
        const int64_t g0 = a.gene_first[r], ng = a.gene_count[r];
        if (g0 < 0 || ng < 1 || g0 + ng > a.G) fault = 2;
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
    if (longest) atomicMax((unsigned long long *)&verdict[2], (unsigned long long)longest);
    if (not_one) atomicMax((unsigned long long *)&verdict[3], 1ull);
}

__device__ inline int fill_find_region(const int64_t *off, int n, int64_t b) {   // off[r] <= b < off[r + 1]
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (off[m] <= b) lo = m; else hi = m;
    }
    return lo;
}

template <bool ONE_CELL>
__global__ void __launch_bounds__(FILL_THREADS) fill_regions_kernel(FillRegions a, int64_t rows) {
    const int64_t row = (int64_t)blockIdx.x * FILL_WAVES + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const int r = ONE_CELL ? (int)row : fill_find_region(a.cell_off, a.n_regions, row);
    const uint8_t v = a.value[r];
    if (v == 0) return;                                   // 0: the rectangle stays as it is
    const int64_t ng = a.gene_count[r];
    uint8_t *dst = a.states + (int64_t)a.cell_idx[row] * a.ld + a.gene_first[r];
    for (int64_t g = (int64_t)blockIdx.y * 64 + lane; g < ng; g += (int64_t)gridDim.y * 64) dst[g] = v;
}

}  // namespace

}  // namespace icnv

using namespace icnv;

extern "C" int icnv_state_fill_regions_dev(uint8_t *states, int64_t G, int64_t C, int64_t ld, int32_t n_regions,
                                           const int32_t *gene_first, const int32_t *gene_count, const int64_t *cell_off,
                                           const int32_t *cell_idx, int64_t n_idx, const uint8_t *value, void *stream) {
    if (n_regions == 0) return ICNV_OK;
    if (!states || !gene_first || !gene_count || !cell_off || !value) ICNV_FAIL(ICNV_ERR_ARG, "state_fill_regions: null argument");
    if (n_regions < 0 || n_idx < 0 || (n_idx > 0 && !cell_idx)) ICNV_FAIL(ICNV_ERR_ARG, "state_fill_regions: bad region arrays");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff || ld < G) ICNV_FAIL(ICNV_ERR_ARG, "state_fill_regions: bad matrix dimensions");
    hipStream_t s = (hipStream_t)stream;
    FillRegions a{states, G, C, ld, n_regions, gene_first, gene_count, cell_off, cell_idx, n_idx, value};
    DevBuf d_verdict;
    int rc = d_verdict.alloc(4 * sizeof(int64_t));
    if (rc) return rc;
    ICNV_HIP(hipMemsetAsync(d_verdict.p, 0, 4 * sizeof(int64_t), s));
    {
        KernelTimer kt("state_fill_check", s);
        const int64_t work = std::max<int64_t>(n_regions, n_idx);
        const unsigned blocks = (unsigned)std::min<int64_t>((work + FILL_THREADS - 1) / FILL_THREADS, (int64_t)num_cus() * 8);
        hipLaunchKernelGGL(fill_check_kernel, dim3(std::max(blocks, 1u)), dim3(FILL_THREADS), 0, s, a, d_verdict.as<int64_t>());
        ICNV_HIP(hipGetLastError());
    }
    int64_t verdict[4];
    ICNV_HIP(hipMemcpyAsync(verdict, d_verdict.p, sizeof(verdict), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (verdict[0] == 1) ICNV_FAIL(ICNV_ERR_ARG, "state_fill_regions: cell_off must start at 0, be monotone and end within cell_idx");
    if (verdict[0] == 2) ICNV_FAIL(ICNV_ERR_ARG, "state_fill_regions: gene run out of range");
    if (verdict[0] == 3) ICNV_FAIL(ICNV_ERR_ARG, "state_fill_regions: cell index out of range");
    const int64_t rows = verdict[1];
    if (rows == 0) return ICNV_OK;
    const int64_t blocks = (rows + FILL_WAVES - 1) / FILL_WAVES;
    if (blocks > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "state_fill_regions: too many (region, cell) rows");
    KernelTimer kt("state_fill_regions", s);
    if (verdict[3] == 0) {
        hipLaunchKernelGGL(fill_regions_kernel<true>, dim3((unsigned)blocks), dim3(FILL_THREADS), 0, s, a, rows);
    } else {
        const unsigned pieces = (unsigned)std::min<int64_t>((verdict[2] + 63) / 64, 65535);
        hipLaunchKernelGGL(fill_regions_kernel<false>, dim3((unsigned)blocks, pieces), dim3(FILL_THREADS), 0, s, a, rows);
    }
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}
