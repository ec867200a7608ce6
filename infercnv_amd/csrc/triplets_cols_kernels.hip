// K26: the entries of a rank's columns out of a parsed chunk of triplets (include/icnv.h "reading a selection of columns").
// K22's passes parse and validate every entry into staged arrays; here the entries whose column the map keeps are compacted
// in file order: the kept entries of every tile of SC_KEEP_TILE entries counted by ballot, the counts scanned by one workgroup, the
// entries stored behind the kept ones before them.  No atomics; the order is the file's whatever the launch shape.
// The host side is icnv_parse_triplets_cols_dev in sparse_counts_api.hip.  DESIGN.md section 4 K26.
#include "icnv_internal.h"
#include "sparse_counts_internal.h"

namespace icnv {

namespace {

__device__ inline bool sc_keep(const ScKeepArgs &a, int64_t k, int32_t &new_col) {
    new_col = -1;
    if (k < a.n_entries) {
        const int32_t c = a.col[k];                            // 0 .. C - 1: the parse pass refused every other entry
        if (c >= 0 && c < a.C) new_col = a.col_map[c];
    }
    return new_col >= 0;
}

// A workgroup looks at SC_KEEP_TILE entries in SC_KEEP_STEPS steps of SC_NT: step t, lane l has entry tile * SC_KEEP_TILE +
// t * SC_NT + l, so file order is step, then wavefront, then lane.
__global__ __launch_bounds__(SC_NT) void sc_keep_count_kernel(ScKeepArgs a) {
    __shared__ uint32_t s_part[SC_NT / 64];
    uint32_t n = 0;
    for (int t = 0; t < SC_KEEP_STEPS; ++t) {                  // every lane of the workgroup reaches every ballot
        int32_t nc;
        n += (uint32_t)__popcll(__ballot(sc_keep(a, (int64_t)blockIdx.x * SC_KEEP_TILE + t * SC_NT + threadIdx.x, nc)));
    }
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) a.block_count[blockIdx.x] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// One workgroup: the exclusive scan of the blocks' counts, and the total (a chunk has fewer than 2^31 / 4 entries).
__global__ __launch_bounds__(SC_NT) void sc_keep_scan_kernel(ScKeepArgs a, int64_t n_blocks) {
    __shared__ uint32_t s_scan[SC_NT];
    const int tid = threadIdx.x;
    uint32_t carry = 0;
    for (int64_t i0 = 0; i0 < n_blocks; i0 += SC_NT) {
        const int64_t i = i0 + tid;
        const uint32_t c = i < n_blocks ? a.block_count[i] : 0u;
        s_scan[tid] = c;
        __syncthreads();
        for (int d = 1; d < SC_NT; d <<= 1) {
            const uint32_t add = tid >= d ? s_scan[tid - d] : 0u;
            __syncthreads();
            s_scan[tid] += add;
            __syncthreads();
        }
        if (i < n_blocks) a.block_off[i] = carry + s_scan[tid] - c;
        carry += s_scan[SC_NT - 1];
        __syncthreads();
    }
    if (tid == 0) a.total[0] = carry;
}

// An entry goes behind the kept entries of the tiles before its tile and, inside the tile, of the steps before its step, of
// the wavefronts before its wavefront and of the lanes below it.  Runs only when total <= the caller's capacity.
__global__ __launch_bounds__(SC_NT) void sc_keep_fill_kernel(ScKeepArgs a) {
    __shared__ uint32_t s_part[SC_KEEP_STEPS][SC_NT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool keep[SC_KEEP_STEPS];
    int32_t nc[SC_KEEP_STEPS];
    uint32_t below[SC_KEEP_STEPS];
    for (int t = 0; t < SC_KEEP_STEPS; ++t) {
        keep[t] = sc_keep(a, (int64_t)blockIdx.x * SC_KEEP_TILE + t * SC_NT + threadIdx.x, nc[t]);
        const unsigned long long mask = __ballot(keep[t]);
        below[t] = (uint32_t)__popcll(mask & ((1ull << lane) - 1));
        if (lane == 0) s_part[t][wave] = (uint32_t)__popcll(mask);
    }
    __syncthreads();
    uint32_t before = a.block_off[blockIdx.x];
    const int64_t total = a.total[0];
    for (int t = 0; t < SC_KEEP_STEPS; ++t) {
        for (int w = 0; w < SC_NT / 64; ++w) {
            if (w == wave) {
                const int64_t k = (int64_t)blockIdx.x * SC_KEEP_TILE + t * SC_NT + threadIdx.x, slot = (int64_t)before + below[t];
                if (keep[t] && slot < total) {                 // slot < total always: the count pass used the same predicate
                    a.row_out[slot] = a.row[k];
                    a.col_out[slot] = nc[t];
                    a.val_out[slot] = a.val[k];
                }
            }
            before += s_part[t][w];
        }
    }
}

}  // namespace

int launch_sc_keep_count(const ScKeepArgs &a, hipStream_t s) {
    KernelTimer kt("triplets_keep_count", s);
    const int64_t n_blocks = (a.n_entries + SC_KEEP_TILE - 1) / SC_KEEP_TILE;    // n_entries < 2^29: the grid fits
    hipLaunchKernelGGL(sc_keep_count_kernel, dim3((unsigned)n_blocks), dim3(SC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    hipLaunchKernelGGL(sc_keep_scan_kernel, dim3(1), dim3(SC_NT), 0, s, a, n_blocks);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_sc_keep_fill(const ScKeepArgs &a, hipStream_t s) {
    KernelTimer kt("triplets_keep_fill", s);
    const int64_t n_blocks = (a.n_entries + SC_KEEP_TILE - 1) / SC_KEEP_TILE;
    hipLaunchKernelGGL(sc_keep_fill_kernel, dim3((unsigned)n_blocks), dim3(SC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
