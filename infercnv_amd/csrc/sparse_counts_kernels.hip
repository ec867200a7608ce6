// K22: sparse count matrices (include/icnv.h "sparse count matrices").  Three groups of kernels, all integer arithmetic:
//   triplets  a chunk of the body of a MatrixMarket coordinate file to (row, col, val): structure (the non-blank lines counted
//             per segment, scanned), index (the list of their first bytes), parse (one lane per entry);
//   build     the column pointers of row / col / val that are sorted by (col, row): a check pass that finds the first pair of
//             neighbours out of order, and a pass that stores k where the column changes;
//   select    .order_reduce and the cell filter on a CSC matrix: the kept entries of every output column counted, the counts
//             scanned in two levels, the entries compacted in source order by ballot and lane prefix.
// The host side -- validation, the order of the passes, the error text -- is sparse_counts_api.hip.  DESIGN.md section 4 K22.
#include "icnv_internal.h"
#include "sparse_counts_internal.h"

namespace icnv {

namespace {

// ---- triplets: structure --------------------------------------------------------------------------------------------------
// Position p (0 .. n - 1) starts an entry when it begins a line (p == 0 or text[p - 1] == '\n') that is not blank.  A lane
// looks at SC_BYTES positions from `base`: b[k] is the byte at base - 1 + k, '\n' before the text and beyond it.  A line that
// begins with a blank or a '\r' is walked to its first other byte (sc_blank_line); every other line is decided from b alone.
__device__ inline uint32_t sc_entry_mask(const ScParseArgs &a, int64_t base) {
    uint8_t b[SC_BYTES + 1];
    b[0] = (base > 0 && base - 1 < a.n) ? a.text[base - 1] : (uint8_t)'\n';
    if (base + SC_BYTES <= a.n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(a.text + base);
        const uint32_t word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < SC_BYTES; ++j) b[1 + j] = (uint8_t)(word[j >> 2] >> (8 * (j & 3)));
    } else {
#pragma unroll
        for (int j = 0; j < SC_BYTES; ++j) b[1 + j] = base + j < a.n ? a.text[base + j] : (uint8_t)'\n';
    }
    uint32_t entries = 0;
#pragma unroll
    for (int j = 0; j < SC_BYTES; ++j) {
        if (b[j] != '\n' || base + j >= a.n) continue;
        const uint8_t c = b[j + 1];
        const bool maybe_blank = c == ' ' || c == '\t' || c == '\r' || c == '\n';
        if (!maybe_blank || !sc_blank_line(a.text, a.n, base + j)) entries |= 1u << j;
    }
    return entries;
}

// Inclusive scan of one word per lane over the workgroup (s_scan: SC_NT words).
template <typename T>
__device__ inline T sc_block_scan(T v, T *s_scan) {
    const int tid = threadIdx.x;
    s_scan[tid] = v;
    __syncthreads();
    for (int d = 1; d < SC_NT; d <<= 1) {
        const T add = tid >= d ? s_scan[tid - d] : (T)0;
        __syncthreads();
        s_scan[tid] += add;
        __syncthreads();
    }
    return s_scan[tid];
}

__global__ __launch_bounds__(SC_NT) void sc_count_kernel(ScParseArgs a) {
    __shared__ uint32_t s_part[SC_NT / 64];
    uint32_t v = (uint32_t)__popc(sc_entry_mask(a, ((int64_t)blockIdx.x * SC_NT + threadIdx.x) * SC_BYTES));
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) a.seg_count[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// One workgroup: the exclusive scan of the segments' counts, and the total (a chunk has fewer than 2^31 / 4 entries).
__global__ __launch_bounds__(SC_NT) void sc_seg_scan_kernel(ScParseArgs a) {
    __shared__ uint32_t s_scan[SC_NT];
    uint32_t carry = 0;
    for (int64_t i0 = 0; i0 < a.n_seg; i0 += SC_NT) {
        const int64_t i = i0 + threadIdx.x;
        const uint32_t c = i < a.n_seg ? a.seg_count[i] : 0u;
        const uint32_t inc = sc_block_scan(c, s_scan), tot = s_scan[SC_NT - 1];
        __syncthreads();
        if (i < a.n_seg) a.seg_off[i] = carry + inc - c;
        carry += tot;
    }
    if (threadIdx.x == 0) a.total[0] = carry;
}

// ---- triplets: index ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_NT) void sc_index_kernel(ScParseArgs a) {
    __shared__ uint32_t s_scan[SC_NT];
    const int64_t base = ((int64_t)blockIdx.x * SC_NT + threadIdx.x) * SC_BYTES;
    uint32_t entries = sc_entry_mask(a, base);
    const uint32_t mine = (uint32_t)__popc(entries), excl = sc_block_scan(mine, s_scan) - mine;
    int64_t k = (int64_t)a.seg_off[blockIdx.x] + excl;
    while (entries) {
        const int j = __ffs((int)entries) - 1;
        entries &= entries - 1;
        if (k < a.n_entries) a.line_pos[k] = (uint32_t)(base + j);
        ++k;
    }
}

// ---- triplets: parse ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_NT) void sc_parse_kernel(ScParseArgs a) {
    const int64_t k = (int64_t)blockIdx.x * SC_NT + threadIdx.x;
    if (k >= a.n_entries) return;
    const int64_t p = a.line_pos[k];
    if (p >= a.n) return;                                      // cannot happen: the index pass wrote every entry from the same masks
    int32_t row = 0, col = 0, val = 0;
    int64_t at = p;
    const int code = sc_parse_line(a.text, a.n, p, a.field, a.G, a.C, row, col, val, at);
    if (code) {
        atomicMin(a.error, ((unsigned long long)at << 8) | (unsigned long long)code);
        return;
    }
    a.row[k] = row;
    a.col[k] = col;
    a.val[k] = val;
}

// ---- build ----------------------------------------------------------------------------------------------------------------
// The word of entry k whose key col * G + row is not above its predecessor's: k << 2 | (1 equal, 2 below).
__device__ inline unsigned long long sc_violation(const int32_t *row, const int32_t *col, int64_t k, int64_t G) {
    const int64_t key = (int64_t)col[k] * G + row[k], prev = (int64_t)col[k - 1] * G + row[k - 1];
    if (key > prev) return SC_NO_VIOLATION;
    return ((unsigned long long)k << 2) | (key == prev ? 1ull : 2ull);
}

__device__ inline unsigned long long sc_block_min(unsigned long long v, unsigned long long *s_part) {
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = __shfl_down(v, d, 64);
        v = o < v ? o : v;
    }
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long m = s_part[0];
    for (int w = 1; w < SC_NT / 64; ++w) m = s_part[w] < m ? s_part[w] : m;
    return m;
}

// The smallest violation word of the entries a workgroup strides over, one word per workgroup: no atomics.
__global__ __launch_bounds__(SC_NT) void sc_build_check_kernel(const int32_t *row, const int32_t *col, int64_t nnz, int64_t G,
                                                               unsigned long long *block_min) {
    __shared__ unsigned long long s_part[SC_NT / 64];
    unsigned long long v = SC_NO_VIOLATION;
    for (int64_t k = 1 + (int64_t)blockIdx.x * SC_NT + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * SC_NT) {
        const unsigned long long w = sc_violation(row, col, k, G);
        v = w < v ? w : v;
    }
    const unsigned long long m = sc_block_min(v, s_part);
    if (threadIdx.x == 0) block_min[blockIdx.x] = m;
}

__global__ __launch_bounds__(SC_NT) void sc_build_reduce_kernel(const unsigned long long *block_min, int n, unsigned long long *out) {
    __shared__ unsigned long long s_part[SC_NT / 64];
    unsigned long long v = SC_NO_VIOLATION;
    for (int i = threadIdx.x; i < n; i += SC_NT) v = block_min[i] < v ? block_min[i] : v;
    const unsigned long long m = sc_block_min(v, s_part);
    if (threadIdx.x == 0) out[0] = m;
}

// Entry k stores k into colptr[col[k - 1] + 1 .. col[k]] (col[-1] = -1), the last entry also nnz into colptr[col + 1 .. C]:
// every element of colptr is written by exactly one lane.  Runs only on checked input (col ascending, 0 .. C - 1).
__global__ __launch_bounds__(SC_NT) void sc_build_colptr_kernel(const int32_t *col, int64_t nnz, int64_t C, int64_t *colptr) {
    for (int64_t k = (int64_t)blockIdx.x * SC_NT + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * SC_NT) {
        const int64_t cur = col[k], prev = k > 0 ? (int64_t)col[k - 1] : -1;
        if (cur < 0 || cur >= C) continue;                     // cannot happen on checked input
        for (int64_t c = (prev < -1 ? -1 : prev) + 1; c <= cur; ++c) colptr[c] = k;
        if (k == nnz - 1)
            for (int64_t c = cur + 1; c <= C; ++c) colptr[c] = nnz;
    }
}

// Are the indices of the triplets inside the matrix?  (The parser's are; a caller's own arrays are checked here.)
__global__ __launch_bounds__(SC_NT) void sc_build_range_kernel(const int32_t *row, const int32_t *col, int64_t nnz, int64_t G, int64_t C,
                                                               unsigned long long *block_min) {
    __shared__ unsigned long long s_part[SC_NT / 64];
    unsigned long long v = SC_NO_VIOLATION;
    for (int64_t k = (int64_t)blockIdx.x * SC_NT + threadIdx.x; k < nnz; k += (int64_t)gridDim.x * SC_NT) {
        const bool bad = row[k] < 0 || row[k] >= G || col[k] < 0 || col[k] >= C;
        if (bad && (unsigned long long)k < v) v = (unsigned long long)k;
    }
    const unsigned long long m = sc_block_min(v, s_part);
    if (threadIdx.x == 0) block_min[blockIdx.x] = m;
}

// ---- select ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_NT) void sc_check_maps_kernel(ScSelectArgs a) {
    const int64_t i = (int64_t)blockIdx.x * SC_NT + threadIdx.x;
    if (i < a.n_cells && (a.cells[i] < 0 || a.cells[i] >= a.C)) atomicMin(a.error, ((unsigned long long)i << 8) | SC_E_CELL);
    if (i < a.G && (a.gene_map[i] < -1 || a.gene_map[i] >= a.n_genes_out)) atomicMin(a.error, ((unsigned long long)i << 8) | SC_E_GENE);
}

// The stored range of a source column, held inside 0 .. nnz whatever colptr says.
__device__ inline void sc_column(const ScSelectArgs &a, int64_t src, int64_t &b, int64_t &e) {
    b = a.colptr[src];
    e = a.colptr[src + 1];
    b = b < 0 ? 0 : (b > a.nnz ? a.nnz : b);
    e = e < b ? b : (e > a.nnz ? a.nnz : e);
}

__device__ inline bool sc_kept(const ScSelectArgs &a, int64_t i, int32_t &new_row) {
    const int32_t r = a.rowidx[i];
    new_row = (r >= 0 && r < a.G) ? a.gene_map[r] : -1;
    return new_row >= 0;
}

// One wavefront per output column: how many entries of its source column keep their gene.
__global__ __launch_bounds__(SC_NT) void sc_select_count_kernel(ScSelectArgs a) {
    const int lane = threadIdx.x & 63;
    for (int64_t j = (int64_t)blockIdx.x * (SC_NT / 64) + (threadIdx.x >> 6); j < a.n_cells; j += (int64_t)gridDim.x * (SC_NT / 64)) {
        int64_t b, e, count = 0;
        sc_column(a, a.cells[j], b, e);
        for (int64_t i0 = b; i0 < e; i0 += 64) {               // wave-uniform bounds: every lane reaches the ballot
            int32_t nr;
            const bool keep = i0 + lane < e && sc_kept(a, i0 + lane, nr);
            count += __popcll(__ballot(keep));
        }
        if (lane == 0) a.counts[j] = count;
    }
}

// The two-level exclusive int64 scan of counts[n_cells] into colptr_out[n_cells + 1]: the sum of every tile of SC_SCAN_TILE
// counts, the scan of the tile sums by one workgroup, the scan inside every tile from its offset.  Integer sums in a fixed
// order: exact and the same on every run.
__global__ __launch_bounds__(SC_NT) void sc_tile_sum_kernel(ScSelectArgs a) {
    __shared__ int64_t s_scan[SC_NT];
    const int64_t j0 = ((int64_t)blockIdx.x * SC_NT + threadIdx.x) * SC_SCAN_ITEMS;
    int64_t v = 0;
    for (int t = 0; t < SC_SCAN_ITEMS; ++t)
        if (j0 + t < a.n_cells) v += a.counts[j0 + t];
    sc_block_scan(v, s_scan);
    if (threadIdx.x == 0) a.tile_sum[blockIdx.x] = s_scan[SC_NT - 1];
}

__global__ __launch_bounds__(SC_NT) void sc_tile_scan_kernel(ScSelectArgs a, int64_t n_tiles) {
    __shared__ int64_t s_scan[SC_NT];
    int64_t carry = 0;
    for (int64_t i0 = 0; i0 < n_tiles; i0 += SC_NT) {
        const int64_t i = i0 + threadIdx.x;
        const int64_t c = i < n_tiles ? a.tile_sum[i] : 0;
        const int64_t inc = sc_block_scan(c, s_scan), tot = s_scan[SC_NT - 1];
        __syncthreads();
        if (i < n_tiles) a.tile_sum[i] = carry + inc - c;
        carry += tot;
    }
    if (threadIdx.x == 0) a.colptr_out[a.n_cells] = carry;
}

__global__ __launch_bounds__(SC_NT) void sc_tile_apply_kernel(ScSelectArgs a) {
    __shared__ int64_t s_scan[SC_NT];
    const int64_t j0 = ((int64_t)blockIdx.x * SC_NT + threadIdx.x) * SC_SCAN_ITEMS;
    int64_t c[SC_SCAN_ITEMS], v = 0;
    for (int t = 0; t < SC_SCAN_ITEMS; ++t) {
        c[t] = j0 + t < a.n_cells ? a.counts[j0 + t] : 0;
        v += c[t];
    }
    int64_t run = a.tile_sum[blockIdx.x] + sc_block_scan(v, s_scan) - v;
    for (int t = 0; t < SC_SCAN_ITEMS; ++t) {
        if (j0 + t < a.n_cells) a.colptr_out[j0 + t] = run;
        run += c[t];
    }
}

// One wavefront per output column: the kept entries of the source column in source order.  Of the 64 entries a step looks
// at, lane l's goes to the slot after those of the kept lanes below it.
__global__ __launch_bounds__(SC_NT) void sc_select_fill_kernel(ScSelectArgs a) {
    const int lane = threadIdx.x & 63;
    const unsigned long long below = (1ull << lane) - 1;
    for (int64_t j = (int64_t)blockIdx.x * (SC_NT / 64) + (threadIdx.x >> 6); j < a.n_cells; j += (int64_t)gridDim.x * (SC_NT / 64)) {
        int64_t b, e;
        sc_column(a, a.cells[j], b, e);
        int64_t out = a.colptr_out[j];
        const int64_t out_end = a.colptr_out[j + 1];
        for (int64_t i0 = b; i0 < e; i0 += 64) {
            int32_t nr = -1;
            const bool keep = i0 + lane < e && sc_kept(a, i0 + lane, nr);
            const unsigned long long mask = __ballot(keep);
            const int64_t slot = out + __popcll(mask & below);
            if (keep && slot < out_end) {                      // slot < out_end always: the count pass used the same predicate
                a.rowidx_out[slot] = nr;
                a.vals_out[slot] = a.vals[i0 + lane];
            }
            out += __popcll(mask);
        }
    }
}

int sc_grid(int64_t blocks, const char *who, unsigned &grid) {
    if (blocks < 1 || blocks > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, std::string(who) + ": the call needs more than 2^31 - 1 workgroups");
    grid = (unsigned)blocks;
    return ICNV_OK;
}

// The workgroups of a kernel whose lanes stride over their items: `blocks` of them, at most eight per CU.
unsigned sc_capped_grid(int64_t blocks) {
    const int64_t cap = (int64_t)num_cus() * 8;
    return (unsigned)(blocks < 1 ? 1 : (blocks < cap ? blocks : cap));
}

}  // namespace

int launch_sc_structure(const ScParseArgs &a, hipStream_t s) {
    KernelTimer kt("triplets_structure", s);
    unsigned grid;
    int rc;
    if ((rc = sc_grid(a.n_seg, "parse_triplets", grid))) return rc;
    hipLaunchKernelGGL(sc_count_kernel, dim3(grid), dim3(SC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    hipLaunchKernelGGL(sc_seg_scan_kernel, dim3(1), dim3(SC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_sc_index(const ScParseArgs &a, hipStream_t s) {
    KernelTimer kt("triplets_index", s);
    unsigned grid;
    int rc;
    if ((rc = sc_grid(a.n_seg, "parse_triplets", grid))) return rc;
    hipLaunchKernelGGL(sc_index_kernel, dim3(grid), dim3(SC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_sc_parse(const ScParseArgs &a, hipStream_t s) {
    KernelTimer kt("triplets_parse", s);
    unsigned grid;
    int rc;
    if ((rc = sc_grid((a.n_entries + SC_NT - 1) / SC_NT, "parse_triplets", grid))) return rc;
    hipLaunchKernelGGL(sc_parse_kernel, dim3(grid), dim3(SC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

// write = false: violation[0] = the smallest violation word of the order (SC_NO_VIOLATION: none), violation[1] = the first
// entry outside the matrix.  write = true: colptr.  nnz >= 1.
int launch_sc_build(const int32_t *row, const int32_t *col, int64_t nnz, int64_t G, int64_t C, unsigned long long *violation,
                    int64_t *colptr, bool write, hipStream_t s) {
    const unsigned grid = sc_capped_grid((nnz + SC_NT - 1) / SC_NT);
    if (write) {
        KernelTimer kt("csc_build_colptr", s);
        hipLaunchKernelGGL(sc_build_colptr_kernel, dim3(grid), dim3(SC_NT), 0, s, col, nnz, C, colptr);
        ICNV_HIP(hipGetLastError());
        return ICNV_OK;
    }
    KernelTimer kt("csc_build_check", s);
    DevBuf d_min;
    int rc;
    if ((rc = d_min.alloc((size_t)grid * sizeof(unsigned long long)))) return rc;
    hipLaunchKernelGGL(sc_build_range_kernel, dim3(grid), dim3(SC_NT), 0, s, row, col, nnz, G, C, d_min.as<unsigned long long>());
    ICNV_HIP(hipGetLastError());
    hipLaunchKernelGGL(sc_build_reduce_kernel, dim3(1), dim3(SC_NT), 0, s, d_min.as<unsigned long long>(), (int)grid, violation + 1);
    ICNV_HIP(hipGetLastError());
    hipLaunchKernelGGL(sc_build_check_kernel, dim3(grid), dim3(SC_NT), 0, s, row, col, nnz, G, d_min.as<unsigned long long>());
    ICNV_HIP(hipGetLastError());
    hipLaunchKernelGGL(sc_build_reduce_kernel, dim3(1), dim3(SC_NT), 0, s, d_min.as<unsigned long long>(), (int)grid, violation);
    ICNV_HIP(hipGetLastError());
    ICNV_HIP(hipStreamSynchronize(s));                              // the partial minima go back to the pool
    return ICNV_OK;
}

int launch_sc_check_maps(const ScSelectArgs &a, hipStream_t s) {
    const int64_t n = a.n_cells > a.G ? a.n_cells : a.G;
    unsigned grid;
    int rc;
    if ((rc = sc_grid((n + SC_NT - 1) / SC_NT, "csc_select", grid))) return rc;
    hipLaunchKernelGGL(sc_check_maps_kernel, dim3(grid), dim3(SC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_sc_select_count(const ScSelectArgs &a, hipStream_t s) {
    KernelTimer kt("csc_select_count", s);
    hipLaunchKernelGGL(sc_select_count_kernel, dim3(sc_capped_grid((a.n_cells + SC_NT / 64 - 1) / (SC_NT / 64))), dim3(SC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    const int64_t n_tiles = (a.n_cells + SC_SCAN_TILE - 1) / SC_SCAN_TILE;
    hipLaunchKernelGGL(sc_tile_sum_kernel, dim3((unsigned)n_tiles), dim3(SC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    hipLaunchKernelGGL(sc_tile_scan_kernel, dim3(1), dim3(SC_NT), 0, s, a, n_tiles);
    ICNV_HIP(hipGetLastError());
    hipLaunchKernelGGL(sc_tile_apply_kernel, dim3((unsigned)n_tiles), dim3(SC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_sc_select_fill(const ScSelectArgs &a, hipStream_t s) {
    KernelTimer kt("csc_select_fill", s);
    hipLaunchKernelGGL(sc_select_fill_kernel, dim3(sc_capped_grid((a.n_cells + SC_NT / 64 - 1) / (SC_NT / 64))), dim3(SC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
