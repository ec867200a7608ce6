// K27 kernels: a segment [e0, e1) of R's XDR stream of a rows x cols matrix (column-major, every element big-endian) from or
// into a device matrix.  The kernels move bytes: integer loads, a byte swap, integer stores -- no floating-point operation sees
// the data, so a NaN keeps its payload (NA_real_ is one).  Every index is 64-bit.
//   linear   ICNV_XDR_COLS: the matrix is (cols, rows) with contiguous rows, which is the stream's own order.  Where the segment
//            is contiguous in the matrix (ld == rows, or the segment lies in one column) and both sides share their position
//            in a 16-byte word, the body goes through 16-byte loads and stores; the few elements before and after it, and
//            every other case, through the element kernel.
//   tile     ICNV_XDR_ROWS: the matrix is (rows, cols) with contiguous rows.  A 64 x 64 tile through LDS: the matrix side
//            runs along a matrix row (stream columns), the stream side along a stream column, both contiguous.  The LDS row
//            is padded by one element as in the table reader's transposer (K21): the row-wise writes and the column-wise
//            reads are free of bank conflicts.  The segment's ends cut tiles and columns: every lane tests its own element.
// DESIGN.md section 4 K27.
#include "icnv_internal.h"
#include "xdr_internal.h"

namespace icnv {

namespace {

__device__ inline uint64_t xdr_swap(uint64_t v) { return __builtin_bswap64(v); }
__device__ inline uint32_t xdr_swap(uint32_t v) { return __builtin_bswap32(v); }

// ---- linear, one element per lane and step ----------------------------------------------------------------------------------
template <typename T, bool DEC>
__global__ __launch_bounds__(XDR_NT) void xdr_linear_kernel(XdrArgs a) {
    T *mat = reinterpret_cast<T *>(a.mat), *st = reinterpret_cast<T *>(a.stream);
    const int64_t n = a.e1 - a.e0, step = (int64_t)gridDim.x * XDR_NT;
    for (int64_t i = (int64_t)blockIdx.x * XDR_NT + threadIdx.x; i < n; i += step) {
        const int64_t e = a.e0 + i;
        const int64_t m = a.ld == a.rows ? e : (e / a.rows) * a.ld + e % a.rows;
        if (DEC) mat[m] = xdr_swap(st[i]);
        else st[i] = xdr_swap(mat[m]);
    }
}

// ---- linear, 16 bytes per lane and step: two 8-byte or four 4-byte elements ---------------------------------------------------
template <int ES>
__global__ __launch_bounds__(XDR_NT) void xdr_vec_kernel(const uint4 *src, uint4 *dst, int64_t n16) {
    const int64_t step = (int64_t)gridDim.x * XDR_NT;
    for (int64_t i = (int64_t)blockIdx.x * XDR_NT + threadIdx.x; i < n16; i += step) {
        const uint4 v = src[i];
        uint4 o;
        if (ES == 8) {
            o.x = __builtin_bswap32(v.y); o.y = __builtin_bswap32(v.x);
            o.z = __builtin_bswap32(v.w); o.w = __builtin_bswap32(v.z);
        } else {
            o.x = __builtin_bswap32(v.x); o.y = __builtin_bswap32(v.y);
            o.z = __builtin_bswap32(v.z); o.w = __builtin_bswap32(v.w);
        }
        dst[i] = o;
    }
}

// ---- tile: the stream columns c_first + 64 j .. of the stream rows 64 i .. ------------------------------------------------------
template <typename T, bool DEC>
__global__ __launch_bounds__(XDR_NT) void xdr_tile_kernel(XdrArgs a, int64_t c_first, int64_t c_last, int64_t tiles_r) {
    __shared__ T s_tile[XDR_TILE][XDR_TILE + 1];
    T *mat = reinterpret_cast<T *>(a.mat), *st = reinterpret_cast<T *>(a.stream);
    const int64_t r_base = ((int64_t)blockIdx.x % tiles_r) * XDR_TILE, c_base = c_first + ((int64_t)blockIdx.x / tiles_r) * XDR_TILE;
    const int tx = threadIdx.x & (XDR_TILE - 1), ty = threadIdx.x / XDR_TILE;
    if (!DEC) {
        for (int k = ty; k < XDR_TILE; k += XDR_NT / XDR_TILE) {          // lanes along a matrix row
            const int64_t r = r_base + k, c = c_base + tx;
            if (r < a.rows && c <= c_last) s_tile[k][tx] = mat[r * a.ld + c];
        }
        __syncthreads();
        for (int k = ty; k < XDR_TILE; k += XDR_NT / XDR_TILE) {          // lanes along a stream column
            const int64_t r = r_base + tx, c = c_base + k;
            if (r < a.rows && c <= c_last) {
                const int64_t e = c * a.rows + r;
                if (e >= a.e0 && e < a.e1) st[e - a.e0] = xdr_swap(s_tile[tx][k]);
            }
        }
    } else {
        for (int k = ty; k < XDR_TILE; k += XDR_NT / XDR_TILE) {          // lanes along a stream column
            const int64_t r = r_base + tx, c = c_base + k;
            if (r < a.rows && c <= c_last) {
                const int64_t e = c * a.rows + r;
                if (e >= a.e0 && e < a.e1) s_tile[k][tx] = xdr_swap(st[e - a.e0]);
            }
        }
        __syncthreads();
        for (int k = ty; k < XDR_TILE; k += XDR_NT / XDR_TILE) {          // lanes along a matrix row
            const int64_t r = r_base + k, c = c_base + tx;
            if (r < a.rows && c <= c_last) {
                const int64_t e = c * a.rows + r;
                if (e >= a.e0 && e < a.e1) mat[r * a.ld + c] = s_tile[tx][k];
            }
        }
    }
}

unsigned xdr_grid(int64_t items) {      // workgroups of a grid-stride kernel over `items` lanes' worth of work
    const int64_t blocks = (items + XDR_NT - 1) / XDR_NT, cap = (int64_t)num_cus() * 32;
    return (unsigned)(blocks < cap ? blocks : cap);
}

template <typename T>
int xdr_launch_linear(const XdrArgs &a, hipStream_t s) {
    if (a.e1 <= a.e0) return ICNV_OK;
    if (a.decode) hipLaunchKernelGGL((xdr_linear_kernel<T, true>), dim3(xdr_grid(a.e1 - a.e0)), dim3(XDR_NT), 0, s, a);
    else hipLaunchKernelGGL((xdr_linear_kernel<T, false>), dim3(xdr_grid(a.e1 - a.e0)), dim3(XDR_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

template <typename T>
int xdr_launch_cols(const XdrArgs &a, hipStream_t s) {
    constexpr int64_t ES = (int64_t)sizeof(T);
    const int64_t n = a.e1 - a.e0, c0 = a.e0 / a.rows;
    const bool contiguous = a.ld == a.rows || c0 == (a.e1 - 1) / a.rows;
    uint8_t *pm = reinterpret_cast<uint8_t *>(a.mat) + (c0 * a.ld + a.e0 % a.rows) * ES, *ps = reinterpret_cast<uint8_t *>(a.stream);
    const uintptr_t um = reinterpret_cast<uintptr_t>(pm) & 15, us = reinterpret_cast<uintptr_t>(ps) & 15;
    if (!contiguous || um != us) return xdr_launch_linear<T>(a, s);
    const int64_t head = std::min<int64_t>(n, (int64_t)((16 - um) & 15) / ES), n16 = (n - head) * ES / 16;
    const int64_t body = n16 * (16 / ES);
    int rc;
    XdrArgs part = a;                                                    // the elements before the first whole 16-byte word
    part.e1 = a.e0 + head;
    if ((rc = xdr_launch_linear<T>(part, s))) return rc;
    if (n16 > 0) {
        const uint4 *src = reinterpret_cast<const uint4 *>((a.decode ? ps : pm) + head * ES);
        uint4 *dst = reinterpret_cast<uint4 *>((a.decode ? pm : ps) + head * ES);
        hipLaunchKernelGGL((xdr_vec_kernel<(int)ES>), dim3(xdr_grid(n16)), dim3(XDR_NT), 0, s, src, dst, n16);
        ICNV_HIP(hipGetLastError());
    }
    part = a;                                                            // and those after the last one
    part.e0 = a.e0 + head + body;
    part.stream = ps + (head + body) * ES;
    return xdr_launch_linear<T>(part, s);
}

template <typename T>
int xdr_launch_rows(const XdrArgs &a, hipStream_t s) {
    const int64_t c_first = a.e0 / a.rows, c_last = (a.e1 - 1) / a.rows;
    const int64_t tiles_r = (a.rows + XDR_TILE - 1) / XDR_TILE, tiles_c = (c_last - c_first) / XDR_TILE + 1;
    if (tiles_c > 0x7fffffff / tiles_r) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "xdr: the segment needs more than 2^31 - 1 workgroups");
    const dim3 grid((unsigned)(tiles_r * tiles_c));
    if (a.decode) hipLaunchKernelGGL((xdr_tile_kernel<T, true>), grid, dim3(XDR_NT), 0, s, a, c_first, c_last, tiles_r);
    else hipLaunchKernelGGL((xdr_tile_kernel<T, false>), grid, dim3(XDR_NT), 0, s, a, c_first, c_last, tiles_r);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace

int launch_xdr(const XdrArgs &a, hipStream_t s) {
    if (a.e1 <= a.e0) return ICNV_OK;
    KernelTimer kt(a.decode ? "xdr_decode" : "xdr_encode", s);
    if (a.layout == ICNV_XDR_COLS) return a.elem_size == 8 ? xdr_launch_cols<uint64_t>(a, s) : xdr_launch_cols<uint32_t>(a, s);
    return a.elem_size == 8 ? xdr_launch_rows<uint64_t>(a, s) : xdr_launch_rows<uint32_t>(a, s);
}

}  // namespace icnv
