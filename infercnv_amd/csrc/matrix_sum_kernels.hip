// K23: the exact sum of a (C, G) matrix of doubles (include/icnv.h "exact sum of a matrix").  DESIGN.md section 4 K23.
//
// Every finite double is an integer multiple of 2^-1074 below 2^2098: a 53-bit significand m shifted to bit p of a long
// fixed-point number.  The number is kept as 32-bit digits in signed 64-bit limbs, so that adding a value is three integer
// adds (m << (p & 31) spans at most 85 bits) and no carry moves until the host's one pass at the end.  Integer adds commute:
// the record of a workgroup, and so the sum, is the same for every launch shape and every order of arrival.
//
// A lane keeps a window of four limbs in registers, starting at digit `wb`.  A value whose first digit is wb or wb + 1 is
// added there: a matrix whose magnitudes stay within 2^32 of each other (counts, the chain's output around 1) never leaves the
// registers.  Any other value moves the window: the four limbs go to the wave's 68 limbs in LDS with 64-bit LDS atomic adds
// and the window restarts at the value's digit.  At the end the windows are flushed, the waves' limbs are added and the
// workgroup stores its record with plain vector stores.  Non-finite values set a flag and add nothing.
#include "icnv_internal.h"
#include "matrix_sum_internal.h"

namespace icnv {
namespace {

struct MsWindow {
    long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    unsigned wb = 0;
    int flags = 0;
};

__device__ __forceinline__ void ms_flush(const MsWindow &w, unsigned long long *limbs) {
    // (wb <= 63 and the window has four limbs: the last index is 66 < MS_LIMBS)
    if (w.a0) atomicAdd(limbs + w.wb, (unsigned long long)w.a0);
    if (w.a1) atomicAdd(limbs + w.wb + 1, (unsigned long long)w.a1);
    if (w.a2) atomicAdd(limbs + w.wb + 2, (unsigned long long)w.a2);
    if (w.a3) atomicAdd(limbs + w.wb + 3, (unsigned long long)w.a3);
}

__device__ __forceinline__ void ms_add(MsWindow &w, double v, unsigned long long *limbs) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    const unsigned e = (unsigned)(u >> 52) & 0x7ffu;
    const unsigned long long frac = u & 0xfffffffffffffull;
    if (e == 0x7ffu) {
        w.flags |= frac ? MS_NAN : ((u >> 63) ? MS_NEG_INF : MS_POS_INF);
        return;
    }
    const unsigned long long m = e ? (frac | (1ull << 52)) : frac;
    if (!m) return;
    const unsigned p = e ? e - 1 : 0;            // the value is m * 2^(p - 1074)
    const unsigned d = p >> 5, sh = p & 31;
    const unsigned long long lo = m << sh, hi = sh ? (m >> (64 - sh)) : 0ull;
    long long p0 = (long long)(lo & 0xffffffffull), p1 = (long long)(lo >> 32), p2 = (long long)hi;
    if (u >> 63) { p0 = -p0; p1 = -p1; p2 = -p2; }
    unsigned k = d - w.wb;
    if (k > 1u) {
        ms_flush(w, limbs);
        w.a0 = w.a1 = w.a2 = w.a3 = 0;
        w.wb = d;
        k = 0;
    }
    w.a0 += k ? 0 : p0;
    w.a1 += k ? p0 : p1;
    w.a2 += k ? p1 : p2;
    w.a3 += k ? p2 : 0;
}

// Tiles are runs of at most MS_TILE values of one row; tile t of row r starts at x[r * ld + t * MS_TILE].  A workgroup takes
// the tiles blockIdx.x, blockIdx.x + gridDim.x, ...: at most MS_MAX_TILES_PER_WG of them (the launch sizes the grid), so a
// lane adds at most 2^22 values and no limb of a record leaves 64 bits.
__global__ __launch_bounds__(MS_NT) void matrix_sum_kernel(const double *x, int64_t ld, int64_t G, int64_t tiles_per_row, int64_t n_tiles,
                                                           long long *records) {
    __shared__ unsigned long long s_limbs[MS_WAVES][MS_LIMBS];
    __shared__ int s_flags;
    const int lane = threadIdx.x;
    for (int i = lane; i < MS_WAVES * MS_LIMBS; i += MS_NT) (&s_limbs[0][0])[i] = 0;
    if (lane == 0) s_flags = 0;
    __syncthreads();
    unsigned long long *limbs = s_limbs[lane >> 6];
    MsWindow w;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t row = tile / tiles_per_row, t = tile - row * tiles_per_row;
        const double *p = x + row * ld + t * MS_TILE;
        const int64_t left = G - t * MS_TILE;
        const int n = left < MS_TILE ? (int)left : MS_TILE;
        if (n == MS_TILE && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const double2 *p2 = reinterpret_cast<const double2 *>(p);
            double2 v[MS_UNROLL];
#pragma unroll
            for (int j = 0; j < MS_UNROLL; ++j) v[j] = p2[j * MS_NT + lane];
#pragma unroll
            for (int j = 0; j < MS_UNROLL; ++j) {
                ms_add(w, v[j].x, limbs);
                ms_add(w, v[j].y, limbs);
            }
        } else {
            for (int i = lane; i < n; i += MS_NT) ms_add(w, p[i], limbs);
        }
    }
    ms_flush(w, limbs);
    if (w.flags) atomicOr(&s_flags, w.flags);
    __syncthreads();
    long long *rec = records + (int64_t)blockIdx.x * MS_SLOTS;
    if (lane < MS_LIMBS) {
        unsigned long long sum = 0;
#pragma unroll
        for (int wv = 0; wv < MS_WAVES; ++wv) sum += s_limbs[wv][lane];
        rec[lane] = (long long)sum;
    } else if (lane == MS_LIMBS) {
        rec[MS_LIMBS] = s_flags;
    }
}

int64_t ms_tiles(int64_t ld, int64_t G, int64_t C, int64_t &tiles_per_row, int64_t &row_len) {
    // rows that touch are one long row: the common case, and then only the last tile is partial
    row_len = ld == G ? G * C : G;
    tiles_per_row = (row_len + MS_TILE - 1) / MS_TILE;
    return tiles_per_row * (ld == G ? 1 : C);
}

}  // namespace

int64_t matrix_sum_workgroups(int64_t ld, int64_t G, int64_t C) {
    int64_t tiles_per_row, row_len;
    const int64_t n_tiles = ms_tiles(ld, G, C, tiles_per_row, row_len);
    int64_t grid = (int64_t)num_cus() * 8;
    if (grid > n_tiles) grid = n_tiles;
    const int64_t need = (n_tiles + MS_MAX_TILES_PER_WG - 1) / MS_MAX_TILES_PER_WG;
    if (grid < need) grid = need;
    return grid > 0x7fffffff ? 0 : grid;
}

int launch_matrix_sum(const double *x, int64_t ld, int64_t G, int64_t C, int64_t *records, int64_t *n_wg, hipStream_t s) {
    KernelTimer kt("matrix_sum", s);
    int64_t tiles_per_row, row_len;
    const int64_t n_tiles = ms_tiles(ld, G, C, tiles_per_row, row_len);
    const int64_t grid = matrix_sum_workgroups(ld, G, C);
    if (grid < 1) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "matrix_sum: the matrix needs more than 2^31 - 1 workgroups");
    hipLaunchKernelGGL(matrix_sum_kernel, dim3((unsigned)grid), dim3(MS_NT), 0, s, x, ld == G ? row_len : ld, row_len, tiles_per_row, n_tiles,
                       reinterpret_cast<long long *>(records));
    ICNV_HIP(hipGetLastError());
    *n_wg = grid;
    return ICNV_OK;
}

}  // namespace icnv
