// K29 kernels: a gzip stream with flush points inflated in independent units, one wavefront per unit; the scan for the units'
// possible starts; the CRC-32 of equal pieces of a buffer.  DESIGN.md section 4 K29; the contract is in include/icnv.h.
//
//   scan      a candidate is an offset p in [4, n] with src[p - 4, p) = 00 00 FF FF.  Two passes over workgroup tiles of
//             SC_NT * SC_ROUNDS positions: count, a one-workgroup prefix sum of the counts, then emit -- per round the lanes'
//             flags are ranked by ballot and popcount inside a wavefront and by the wavefronts' sums across the workgroup, so
//             the list is ascending and no atomic is involved.  Every position reads its own four bytes: a marker that
//             straddles a tile, a round or a wavefront is nothing special.  The tile bodies are sc_count_tile / sc_emit_tile.
//   measure   lane 0 of a wavefront walks its unit's bit stream with the parser of inflate_internal.h (the code tables, 1 KiB,
//             in LDS), stores nothing, and reports where the unit ends, what it inflates to, and its status: if_measure_lane.
//   units     the same walk with stores, wide matches and stored blocks copied by all 64 lanes: if_decode_wave, with K29's
//             policy IfBytes.  K30's kernels (gunzip_kernels.hip) are the same bodies with another policy.
//   crc       one wavefront per piece; a lane folds CRC_SUB bytes at a time, moves its running CRC across the 63 other
//             lanes' bytes with one fixed operator (crc32_combine's identity), and the 64 lanes' values are XOR-ed.
#include "icnv_internal.h"
#include "inflate_internal.h"

namespace icnv {

namespace {

// ---- scan -------------------------------------------------------------------------------------------------------------------------------
__device__ inline bool sc_is_candidate(const uint8_t *src, int64_t n, int64_t p) {     // p - 4 >= 0 and p - 1 < n are tested here
    if (p < 4 || p > n) return false;
    return src[p - 4] == 0x00 && src[p - 3] == 0x00 && src[p - 2] == 0xFF && src[p - 1] == 0xFF;
}

__global__ __launch_bounds__(SC_NT) void inflate_scan_count_kernel(const uint8_t *src, int64_t n, int64_t n_blocks, int64_t *block_off) {
    sc_count_tile<sc_is_candidate>(src, n, n_blocks, block_off);
}

// one workgroup: block_off[i] becomes the sum of the counts before tile i, block_off[n_blocks] the total
__global__ __launch_bounds__(1024) void inflate_scan_offsets_kernel(int64_t n_blocks, int64_t *block_off) {
    __shared__ int64_t s_w[1024 / 64];
    __shared__ int64_t s_carry;
    const int t = threadIdx.x;
    if (t == 0) s_carry = 0;
    __syncthreads();
    for (int64_t i0 = 0; i0 < n_blocks; i0 += 1024) {
        const int64_t i = i0 + t;
        const int64_t v = i < n_blocks ? block_off[i] : 0;
        int64_t incl = v;
        for (int dlt = 1; dlt < 64; dlt <<= 1) {
            const int64_t u = __shfl_up(incl, dlt, 64);
            if ((t & 63) >= dlt) incl += u;
        }
        if ((t & 63) == 63) s_w[t >> 6] = incl;
        __syncthreads();
        int64_t base = s_carry, total = 0;
        for (int w = 0; w < 1024 / 64; ++w) {
            if (w < (t >> 6)) base += s_w[w];
            total += s_w[w];
        }
        if (i < n_blocks) block_off[i] = base + incl - v;
        __syncthreads();
        if (t == 0) s_carry += total;
        __syncthreads();
    }
    if (t == 0) block_off[n_blocks] = s_carry;
}

__global__ __launch_bounds__(SC_NT) void inflate_scan_emit_kernel(const uint8_t *src, int64_t n, int64_t n_blocks, const int64_t *block_off,
                                                                  int64_t *cand, int64_t cand_cap) {
    sc_emit_tile<sc_is_candidate>(src, n, n_blocks, block_off, cand, cand_cap);
}

// ---- argument check -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void inflate_check_kernel(InflateArgs a, int units, int32_t *bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_units) return;
    const int64_t st = a.start[i];
    bool ok = st >= 0 && st < a.n;
    if (units) {
        const int64_t e = a.end[i], off = a.out_off[i], len = a.out_len[i];
        ok = ok && e >= st && e <= a.n && off >= 0 && len >= 0 && off <= a.out_cap && len <= a.out_cap - off;
    }
    if (!ok) *bad = 1;                                              // every writer stores the same value
}

// ---- measure ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IF_NT) void inflate_measure_kernel(InflateArgs a) { if_measure_lane(a, IfBytes()); }

// ---- decode -----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IF_NT) void inflate_units_kernel(InflateArgs a) { if_decode_wave(a, IfBytes(), a.out, a.out_cap); }

// ---- CRC-32 of pieces -------------------------------------------------------------------------------------------------------------------
constexpr uint32_t CRC_POLY = 0xEDB88320u;

__device__ inline uint32_t crc_mul(uint32_t a, uint32_t b) {       // a(x) * b(x) mod P, reflected: bit 31 is x^0
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : b >> 1;
    }
    return p;
}

__device__ inline uint32_t crc_xpow8(uint64_t nbytes) {            // x^(8 * nbytes) mod P: at most 64 squarings
    uint32_t r = 0x80000000u, b = 0x00800000u;                     // x^0, x^8
    while (nbytes) {
        if (nbytes & 1u) r = crc_mul(r, b);
        b = crc_mul(b, b);
        nbytes >>= 1;
    }
    return r;
}

__global__ __launch_bounds__(IF_NT) void crc32_pieces_kernel(const uint8_t *src, int64_t n, int64_t piece_bytes, int64_t n_pieces, uint32_t *crc) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * IF_WAVES + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * IF_WAVES;
    const uint32_t across = crc_xpow8((uint64_t)64 * CRC_SUB);     // moves a CRC across one round of the wavefront
    for (int64_t piece = wave; piece < n_pieces; piece += n_waves) {
        const int64_t p0 = piece * piece_bytes;
        const int64_t len = n - p0 < piece_bytes ? n - p0 : piece_bytes;       // 1 .. piece_bytes
        uint32_t acc = 0;
        int64_t prev_end = 0;
        for (int64_t b0 = (int64_t)lane * CRC_SUB; b0 < len; b0 += (int64_t)64 * CRC_SUB) {
            const int64_t b1 = b0 + CRC_SUB < len ? b0 + CRC_SUB : len;
            uint32_t c = 0xFFFFFFFFu;
            for (int64_t i = b0; i < b1; ++i) {                     // p0 + i < p0 + len <= n
                c ^= src[p0 + i];
                for (int j = 0; j < 8; ++j) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1u)));
            }
            c ^= 0xFFFFFFFFu;
            if (prev_end) acc = crc_mul(b1 - prev_end == (int64_t)64 * CRC_SUB ? across : crc_xpow8((uint64_t)(b1 - prev_end)), acc);
            acc ^= c;
            prev_end = b1;
        }
        if (prev_end) acc = crc_mul(crc_xpow8((uint64_t)(len - prev_end)), acc);
        for (int dlt = 32; dlt >= 1; dlt >>= 1) acc ^= __shfl_xor(acc, dlt, 64);
        if (lane == 0) crc[piece] = acc;
    }
}

}  // namespace

int launch_inflate_scan_count(const uint8_t *src, int64_t n, int64_t n_blocks, int64_t *block_off, hipStream_t s) {
    hipLaunchKernelGGL(inflate_scan_count_kernel, dim3((unsigned)n_blocks), dim3(SC_NT), 0, s, src, n, n_blocks, block_off);
    ICNV_HIP(hipGetLastError());
    return launch_scan_offsets(n_blocks, block_off, s);
}

int launch_scan_offsets(int64_t n_blocks, int64_t *block_off, hipStream_t s) {
    hipLaunchKernelGGL(inflate_scan_offsets_kernel, dim3(1), dim3(1024), 0, s, n_blocks, block_off);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_inflate_scan_emit(const uint8_t *src, int64_t n, int64_t n_blocks, const int64_t *block_off, int64_t *cand, int64_t cand_cap,
                             hipStream_t s) {
    hipLaunchKernelGGL(inflate_scan_emit_kernel, dim3((unsigned)n_blocks), dim3(SC_NT), 0, s, src, n, n_blocks, block_off, cand, cand_cap);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_inflate_check(const InflateArgs &a, bool units, int32_t *bad, hipStream_t s) {
    hipLaunchKernelGGL(inflate_check_kernel, dim3((unsigned)((a.n_units + 255) / 256)), dim3(256), 0, s, a, units ? 1 : 0, bad);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_inflate_measure(const InflateArgs &a, hipStream_t s) {
    KernelTimer kt("inflate_measure", s);
    hipLaunchKernelGGL(inflate_measure_kernel, dim3((unsigned)((a.n_units + IF_WAVES - 1) / IF_WAVES)), dim3(IF_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_inflate_units(const InflateArgs &a, hipStream_t s) {
    KernelTimer kt("inflate_units", s);
    hipLaunchKernelGGL(inflate_units_kernel, dim3((unsigned)((a.n_units + IF_WAVES - 1) / IF_WAVES)), dim3(IF_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_crc32_pieces(const uint8_t *src, int64_t n, int64_t piece_bytes, int64_t n_pieces, uint32_t *crc, hipStream_t s) {
    KernelTimer kt("crc32_pieces", s);
    const int64_t want = (n_pieces + IF_WAVES - 1) / IF_WAVES, cap = (int64_t)num_cus() * 16;
    hipLaunchKernelGGL(crc32_pieces_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(IF_NT), 0, s, src, n, piece_bytes, n_pieces, crc);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
