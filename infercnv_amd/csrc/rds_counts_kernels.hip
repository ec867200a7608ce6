// K34 kernels: count matrices out of R's serialisation stream.  The per-element arithmetic -- the unaligned big-endian fetch from
// aligned words, the int -> double rule, the count test on a double's bits -- is rds_counts_internal.h's __host__ __device__ code;
// the kernels below only hand out the work.  Integer loads and stores throughout: no floating-point operation sees a REALSXP
// element.  Every index is 64-bit.
//   columns     a workgroup step converts RC_ROWS_PER_BLOCK rows of one output column: neighbouring lanes read neighbouring
//               elements (the words two lanes share come from the cache), and write neighbouring doubles
//   csc check   p: one lane per element of p; entries: one wavefront per selected column, striding its entries.  A lane keeps
//               the smallest key it met and does one atomic minimum at the end, and only when it met one
//   csc colptr  one workgroup scans the selected columns' lengths, RC_NT at a time, with a carry
//   csc fill    one wavefront per output column
// The column ranges read from p are clamped to [0, nnz] before they are used, so an unchecked or refused p still leads to no
// access outside the payloads.  DESIGN.md section 4 K34.
#include "icnv_internal.h"
#include "rds_counts_internal.h"

namespace icnv {

namespace {

__device__ inline int32_t rc_p(const RdsCscArgs &a, int64_t j) {
    return (int32_t)rc_fetch_be32(a.stream, a.stream_bytes, a.p_off + 4 * j);
}

// the entries [lo, hi) of file column c, inside [0, nnz] whatever p holds
__device__ inline void rc_column_range(const RdsCscArgs &a, int64_t c, int64_t &lo, int64_t &hi) {
    lo = rc_p(a, c);
    hi = rc_p(a, c + 1);
    lo = lo < 0 ? 0 : (lo > a.nnz ? a.nnz : lo);
    hi = hi < lo ? lo : (hi > a.nnz ? a.nnz : hi);
}

__global__ __launch_bounds__(RC_NT) void rds_columns_kernel(RdsColumnsArgs a, int64_t blocks_per_col, int64_t n_blocks) {
    for (int64_t b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        const int64_t j = b / blocks_per_col, r0 = (b % blocks_per_col) * RC_ROWS_PER_BLOCK;
        const int64_t off = a.col_off[j];
        const bool real = a.col_kind[j] == ICNV_RDS_REAL;
        uint64_t *dst = a.out + j * a.ld;
        for (int k = 0; k < RC_ROWS_PER_BLOCK / RC_NT; ++k) {
            const int64_t r = r0 + (int64_t)k * RC_NT + threadIdx.x;
            if (r >= a.rows) break;
            dst[r] = real ? rc_fetch_be64(a.stream, a.stream_bytes, off + 8 * r)
                          : rc_int_to_real_bits(rc_fetch_be32(a.stream, a.stream_bytes, off + 4 * r));
        }
    }
}

__global__ __launch_bounds__(RC_NT) void rds_csc_p_kernel(RdsCscArgs a) {
    unsigned long long best = RC_NO_VIOLATION;
    const int64_t step = (int64_t)gridDim.x * RC_NT;
    for (int64_t j = (int64_t)blockIdx.x * RC_NT + threadIdx.x; j <= a.C; j += step) {
        const int32_t v = rc_p(a, j);
        unsigned long long k = RC_NO_VIOLATION;
        if (j == 0 && v != 0) k = rc_key(0, ICNV_RDS_P_FIRST, false);
        else if (j > 0 && v < rc_p(a, j - 1)) k = rc_key(j, ICNV_RDS_P_DESCENT, false);
        else if (j == a.C && (int64_t)v != a.nnz) k = rc_key(j, ICNV_RDS_P_LAST, false);
        best = k < best ? k : best;
    }
    if (best != RC_NO_VIOLATION) atomicMin(a.key, best);
}

__global__ __launch_bounds__(RC_NT) void rds_csc_entries_kernel(RdsCscArgs a) {
    unsigned long long best = RC_NO_VIOLATION;
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * (RC_NT / 64);
    for (int64_t k = (int64_t)blockIdx.x * (RC_NT / 64) + threadIdx.x / 64; k < a.n_out; k += n_waves) {
        const int64_t c = a.cells ? a.cells[k] : k;
        int64_t lo, hi;
        rc_column_range(a, c, lo, hi);
        for (int64_t e = lo + lane; e < hi; e += 64) {
            const int32_t row = (int32_t)rc_fetch_be32(a.stream, a.stream_bytes, a.i_off + 4 * e);
            const int32_t prev = e > lo ? (int32_t)rc_fetch_be32(a.stream, a.stream_bytes, a.i_off + 4 * (e - 1)) : 0;
            const int code = rc_entry_code(e, lo, row, prev, a.G, rc_fetch_be64(a.stream, a.stream_bytes, a.x_off + 8 * e));
            if (code) {
                const unsigned long long key = rc_key(e, code, true);
                best = key < best ? key : best;
            }
        }
    }
    if (best != RC_NO_VIOLATION) atomicMin(a.key, best);
}

__global__ __launch_bounds__(RC_NT) void rds_csc_colptr_kernel(RdsCscArgs a) {
    __shared__ int64_t s_scan[RC_NT];
    __shared__ int64_t s_carry;
    const int t = threadIdx.x;
    if (t == 0) {
        s_carry = 0;
        a.colptr[0] = 0;
    }
    __syncthreads();
    for (int64_t base = 0; base < a.n_out; base += RC_NT) {
        const int64_t k = base + t;
        int64_t len = 0;
        if (k < a.n_out) {
            int64_t lo, hi;
            rc_column_range(a, a.cells ? a.cells[k] : k, lo, hi);
            len = hi - lo;
        }
        s_scan[t] = len;
        __syncthreads();
        for (int d = 1; d < RC_NT; d <<= 1) {                            // inclusive scan, Hillis-Steele
            const int64_t add = t >= d ? s_scan[t - d] : 0;
            __syncthreads();
            s_scan[t] += add;
            __syncthreads();
        }
        if (k < a.n_out) a.colptr[k + 1] = s_carry + s_scan[t];
        __syncthreads();
        if (t == RC_NT - 1) s_carry += s_scan[t];
        __syncthreads();
    }
}

// the file column that holds `entry` under a valid p: the first c with p[c + 1] > entry
__global__ void rds_csc_find_column_kernel(RdsCscArgs a, int64_t entry, int64_t *col) {
    int64_t lo = 0, hi = a.C - 1;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if ((int64_t)rc_p(a, mid + 1) > entry) hi = mid;
        else lo = mid + 1;
    }
    *col = lo;
}

__global__ __launch_bounds__(RC_NT) void rds_csc_fill_kernel(RdsCscArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t n_waves = (int64_t)gridDim.x * (RC_NT / 64);
    for (int64_t k = (int64_t)blockIdx.x * (RC_NT / 64) + threadIdx.x / 64; k < a.n_out; k += n_waves) {
        int64_t lo, hi;
        rc_column_range(a, a.cells ? a.cells[k] : k, lo, hi);
        const int64_t d0 = a.colptr[k];
        for (int64_t e = lo + lane; e < hi; e += 64) {
            const int64_t d = d0 + (e - lo);
            if (d < 0 || d >= a.out_cap) continue;                       // (a colptr that is not this check's)
            a.rowidx[d] = (int32_t)rc_fetch_be32(a.stream, a.stream_bytes, a.i_off + 4 * e);
            a.vals[d] = (int32_t)rc_count_of_bits(rc_fetch_be64(a.stream, a.stream_bytes, a.x_off + 8 * e));
        }
    }
}

unsigned rc_grid(int64_t blocks) {
    const int64_t cap = (int64_t)num_cus() * 16;
    return (unsigned)std::max<int64_t>(1, std::min(blocks, cap));
}

}  // namespace

int launch_rds_columns(const RdsColumnsArgs &a, hipStream_t s) {
    KernelTimer kt("rds_columns", s);
    const int64_t bpc = (a.rows + RC_ROWS_PER_BLOCK - 1) / RC_ROWS_PER_BLOCK, n_blocks = bpc * a.n_out;
    hipLaunchKernelGGL(rds_columns_kernel, dim3(rc_grid(n_blocks)), dim3(RC_NT), 0, s, a, bpc, n_blocks);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_rds_csc_check(const RdsCscArgs &a, hipStream_t s) {
    KernelTimer kt("rds_csc_check", s);
    hipLaunchKernelGGL(rds_csc_p_kernel, dim3(rc_grid((a.C + RC_NT) / RC_NT)), dim3(RC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    hipLaunchKernelGGL(rds_csc_entries_kernel, dim3(rc_grid((a.n_out + RC_NT / 64 - 1) / (RC_NT / 64))), dim3(RC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_rds_csc_colptr(const RdsCscArgs &a, hipStream_t s) {
    KernelTimer kt("rds_csc_check", s);
    hipLaunchKernelGGL(rds_csc_colptr_kernel, dim3(1), dim3(RC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_rds_csc_find_column(const RdsCscArgs &a, int64_t entry, int64_t *col_dev, hipStream_t s) {
    hipLaunchKernelGGL(rds_csc_find_column_kernel, dim3(1), dim3(1), 0, s, a, entry, col_dev);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_rds_csc_fill(const RdsCscArgs &a, hipStream_t s) {
    KernelTimer kt("rds_csc_fill", s);
    hipLaunchKernelGGL(rds_csc_fill_kernel, dim3(rc_grid((a.n_out + RC_NT / 64 - 1) / (RC_NT / 64))), dim3(RC_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
