// K30 kernels: a gzip stream WITHOUT flush points inflated on the device.  DESIGN.md section 4 K30; the contract is in
// include/icnv.h "INFLATE with unknown history"; the parser and the bodies of find, measure and symbols are inflate_internal.h's,
// shared with K29, under the policy GzSymbols of gunzip_internal.h.
//
//   find      a lane per bit offset runs gz_header_ok (cheap tests first).  Count, K29's one-workgroup prefix sum, emit
//             (sc_count_tile, sc_emit_tile): the flags are ranked by ballot and popcount, so the list is ascending and no
//             atomic is involved.  Every offset reads its own bits through a bounds-tested reader: a header that straddles
//             two workgroups' ranges is nothing special, and one cut by the end of the stream runs dry and is no candidate.
//   measure   lane 0 of a wavefront walks its unit's bits (code tables in LDS), stores nothing, and reports the bit offset
//             where the unit ends, the symbols it produces, and its status (if_measure_lane).
//   symbols   the same walk with stores of 16-bit symbols (if_decode_wave).  Lane 0 stores literals and short matches; a match
//             of at least IF_WIDE_MIN symbols and every stored block is copied by the 64 lanes together.  A source position in
//             front of the unit becomes a marker; an overlapping match is a periodic fill, over markers as over bytes.
//   tails     ONE workgroup goes through the units in order and resolves the last min(W, out_len) symbols of each into
//             `out`; a marker reads out[off - W + w], which an earlier unit's tail has written (a barrier stands between
//             two units).  The only sequential step: at most W symbols per unit.
//   resolve   a lane per output byte in front of the tails: the unit by binary search over out_off, then the same rule.
#include "icnv_internal.h"
#include "gunzip_internal.h"

namespace icnv {

namespace {

// ---- find -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SC_NT) void gunzip_find_count_kernel(const uint8_t *src, int64_t n, int64_t n_blocks, int64_t *block_off) {
    sc_count_tile<gz_header_ok>(src, n, n_blocks, block_off);
}

__global__ __launch_bounds__(SC_NT) void gunzip_find_emit_kernel(const uint8_t *src, int64_t n, int64_t n_blocks, const int64_t *block_off,
                                                                 int64_t *cand, int64_t cand_cap) {
    sc_emit_tile<gz_header_ok>(src, n, n_blocks, block_off, cand, cand_cap);
}

// ---- argument check -------------------------------------------------------------------------------------------------------------------
__device__ inline bool gz_place_ok(const GunzipArgs &a, int64_t i) {   // unit i's range of sym / out: inside [0, cap], behind unit i - 1's
    const int64_t off = a.out_off[i], len = a.out_len[i];
    if (off < 0 || len < 0 || off > a.cap || len > a.cap - off) return false;
    return i == 0 ? off == 0 : off == a.out_off[i - 1] + a.out_len[i - 1];
}

__global__ __launch_bounds__(256) void gunzip_check_kernel(GunzipArgs a, int mode, int32_t *bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_units) return;
    bool ok = true;
    if (mode != GZ_CHECK_PLACES) {
        const int64_t st = a.start[i];
        ok = st >= 0 && (st >> 3) < a.n;
        if (mode == GZ_CHECK_SYMBOLS) ok = ok && a.end[i] >= st && a.end[i] <= a.n * 8;
    }
    if (mode != GZ_CHECK_MEASURE) ok = ok && gz_place_ok(a, i);
    if (!ok) *bad = 1;                                              // every writer stores the same value
}

// ---- measure ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IF_NT) void gunzip_measure_kernel(GunzipArgs a) { if_measure_lane(a, GzSymbols{a.cand, a.n_cand, 0}); }

// ---- symbols ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IF_NT) void gunzip_symbols_kernel(GunzipArgs a) { if_decode_wave(a, GzSymbols{a.cand, a.n_cand, 0}, a.sym, a.cap); }

// ---- tails ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GZ_TAILS_NT) void gunzip_tails_kernel(GunzipArgs a, int32_t *bad, int64_t *markers) {
    __shared__ int64_t s_count[GZ_TAILS_NT / 64];
    int64_t mine = 0;
    for (int64_t u = 0; u < a.n_units; ++u) {
        const int64_t off = a.out_off[u], len = a.out_len[u];
        if (off < 0 || len < 0 || off > a.cap || len > a.cap - off) {   // (the check kernel has refused it; uniform across the workgroup)
            if (threadIdx.x == 0) *bad = 1;
            break;
        }
        const int64_t tail = len < GZ_W ? len : GZ_W, t0 = off + len - tail;
        for (int64_t j = threadIdx.x; j < tail; j += GZ_TAILS_NT) {
            const uint16_t v = a.sym[t0 + j];
            uint8_t byte;
            mine += v >= 256;
            if (gz_resolve_one(v, a.out, a.cap, off, byte)) a.out[t0 + j] = byte;
            else *bad = 1;
        }
        __syncthreads();                                            // this tail is visible to the workgroup before the next unit reads it
    }
    for (int dlt = 32; dlt >= 1; dlt >>= 1) mine += __shfl_xor(mine, dlt, 64);
    if ((threadIdx.x & 63) == 0) s_count[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t total = 0;
        for (int w = 0; w < GZ_TAILS_NT / 64; ++w) total += s_count[w];
        *markers = total;
    }
}

// ---- resolve ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GZ_RESOLVE_NT) void gunzip_resolve_kernel(GunzipArgs a, int64_t total, int32_t *bad) {
    const int64_t stride = (int64_t)gridDim.x * GZ_RESOLVE_NT;
    for (int64_t g = (int64_t)blockIdx.x * GZ_RESOLVE_NT + threadIdx.x; g < total; g += stride) {
        int64_t lo = 0, hi = a.n_units;                             // the last unit with out_off <= g: the one that holds byte g
        while (hi - lo > 1) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (a.out_off[mid] <= g) lo = mid; else hi = mid;
        }
        const int64_t off = a.out_off[lo], len = a.out_len[lo];
        if (off < 0 || off > g || len < 0 || g - off >= len) continue;     // (the check kernel has refused such places)
        if (g - off >= len - GZ_W) continue;                        // the tails pass has written it
        uint8_t byte;
        if (gz_resolve_one(a.sym[g], a.out, a.cap, off, byte)) a.out[g] = byte;
        else *bad = 1;
    }
}

}  // namespace

int launch_gunzip_find_count(const uint8_t *src, int64_t n, int64_t n_blocks, int64_t *block_off, hipStream_t s) {
    hipLaunchKernelGGL(gunzip_find_count_kernel, dim3((unsigned)n_blocks), dim3(SC_NT), 0, s, src, n, n_blocks, block_off);
    ICNV_HIP(hipGetLastError());
    return launch_scan_offsets(n_blocks, block_off, s);
}

int launch_gunzip_find_emit(const uint8_t *src, int64_t n, int64_t n_blocks, const int64_t *block_off, int64_t *cand, int64_t cand_cap,
                            hipStream_t s) {
    hipLaunchKernelGGL(gunzip_find_emit_kernel, dim3((unsigned)n_blocks), dim3(SC_NT), 0, s, src, n, n_blocks, block_off, cand, cand_cap);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_gunzip_check(const GunzipArgs &a, int mode, int32_t *bad, hipStream_t s) {
    hipLaunchKernelGGL(gunzip_check_kernel, dim3((unsigned)((a.n_units + 255) / 256)), dim3(256), 0, s, a, mode, bad);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_gunzip_measure(const GunzipArgs &a, hipStream_t s) {
    KernelTimer kt("gunzip_measure", s);
    hipLaunchKernelGGL(gunzip_measure_kernel, dim3((unsigned)((a.n_units + IF_WAVES - 1) / IF_WAVES)), dim3(IF_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_gunzip_symbols(const GunzipArgs &a, hipStream_t s) {
    KernelTimer kt("gunzip_symbols", s);
    hipLaunchKernelGGL(gunzip_symbols_kernel, dim3((unsigned)((a.n_units + IF_WAVES - 1) / IF_WAVES)), dim3(IF_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_gunzip_tails(const GunzipArgs &a, int32_t *bad, int64_t *markers, hipStream_t s) {
    KernelTimer kt("gunzip_tails", s);
    hipLaunchKernelGGL(gunzip_tails_kernel, dim3(1), dim3(GZ_TAILS_NT), 0, s, a, bad, markers);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_gunzip_resolve(const GunzipArgs &a, int32_t *bad, hipStream_t s) {
    KernelTimer kt("gunzip_resolve", s);
    const int64_t want = (a.cap + GZ_RESOLVE_NT - 1) / GZ_RESOLVE_NT, most = (int64_t)num_cus() * 32;
    hipLaunchKernelGGL(gunzip_resolve_kernel, dim3((unsigned)(want < most ? want : most)), dim3(GZ_RESOLVE_NT), 0, s, a, a.cap, bad);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
