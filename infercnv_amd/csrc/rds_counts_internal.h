// K34: count matrices out of R's serialisation stream (include/icnv.h "K34").  Shared between rds_counts_api.hip (validation,
// the status record), rds_counts_kernels.hip and rds_counts_host_check.cpp: the per-element arithmetic below is __host__
// __device__ code, so the host program runs the very routines the kernels run, under the sanitizers, without a GPU.
//   * the unaligned big-endian fetch: a payload lies at an arbitrary BYTE offset of the stream, and the stream's first byte at an
//     arbitrary address.  The fetch loads the 4-byte-aligned words that cover the element and shifts; a word that is not wholly
//     inside [stream, stream + stream_bytes) is put together from the single bytes of it that are.  No byte outside the stream
//     is ever loaded.
//   * the int -> double rule: exact, NA_integer_ (INT_MIN) becomes NA_real_ (0x7FF00000000007A2).
//   * the count test on a double's bits: integer arithmetic only, so no NaN is ever an operand.
// DESIGN.md section 4 K34.
#pragma once
#include <stdint.h>

#include "../../include/icnv.h"

#if defined(__HIPCC__)
#define ICNV_RC_HD __host__ __device__ inline
#else
#define ICNV_RC_HD inline
#endif

namespace icnv {

constexpr int RC_NT = 256;                          // lanes of a workgroup
constexpr int RC_ROWS_PER_BLOCK = RC_NT * 4;        // rows of one column that one workgroup step converts
constexpr uint64_t RC_NA_REAL = 0x7FF00000000007A2ull;
constexpr uint64_t RC_NO_VIOLATION = ~0ull;         // the key word's value while nothing was found
constexpr uint64_t RC_ENTRY_PHASE = 1ull << 62;     // keys of entry violations lie above every key of a p violation

// The aligned 32-bit word at address `w` (w % 4 == 0) as a little-endian load sees it; the bytes of it outside [lo, hi) count as 0
// and are not loaded.
ICNV_RC_HD uint32_t rc_word(uintptr_t w, uintptr_t lo, uintptr_t hi) {
    if (w >= lo && w + 4 <= hi) return *reinterpret_cast<const uint32_t *>(w);
    uint32_t v = 0;
    for (uintptr_t b = 0; b < 4; ++b)
        if (w + b >= lo && w + b < hi) v |= (uint32_t) * reinterpret_cast<const uint8_t *>(w + b) << (8 * b);
    return v;
}

ICNV_RC_HD uint32_t rc_bswap32(uint32_t v) { return __builtin_bswap32(v); }

// The big-endian 32-bit element at byte `off` of the stream; [off, off + 4) lies inside [0, n).
ICNV_RC_HD uint32_t rc_fetch_be32(const uint8_t *stream, int64_t n, int64_t off) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(stream), hi = lo + (uintptr_t)n, a = lo + (uintptr_t)off;
    const unsigned sh = (unsigned)(a & 3) * 8;
    const uintptr_t w = a & ~(uintptr_t)3;
    const uint32_t w0 = rc_word(w, lo, hi);
    if (sh == 0) return rc_bswap32(w0);
    const uint32_t w1 = rc_word(w + 4, lo, hi);
    return rc_bswap32((w0 >> sh) | (w1 << (32 - sh)));
}

// The big-endian 64-bit element at byte `off` of the stream; [off, off + 8) lies inside [0, n).
ICNV_RC_HD uint64_t rc_fetch_be64(const uint8_t *stream, int64_t n, int64_t off) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(stream), hi = lo + (uintptr_t)n, a = lo + (uintptr_t)off;
    const unsigned sh = (unsigned)(a & 3) * 8;
    const uintptr_t w = a & ~(uintptr_t)3;
    const uint32_t w0 = rc_word(w, lo, hi), w1 = rc_word(w + 4, lo, hi);
    if (sh == 0) return ((uint64_t)rc_bswap32(w0) << 32) | rc_bswap32(w1);
    const uint32_t w2 = rc_word(w + 8, lo, hi);
    const uint32_t m0 = (w0 >> sh) | (w1 << (32 - sh)), m1 = (w1 >> sh) | (w2 << (32 - sh));
    return ((uint64_t)rc_bswap32(m0) << 32) | rc_bswap32(m1);
}

// The bits of the double an R integer stands for.
ICNV_RC_HD uint64_t rc_int_to_real_bits(uint32_t be_value) {
    const int32_t v = (int32_t)be_value;
    if (v == INT32_MIN) return RC_NA_REAL;
    const double d = (double)v;                    // exact: every int32 is a double
    uint64_t bits;
    __builtin_memcpy(&bits, &d, sizeof bits);
    return bits;
}

// The count a double's bits stand for: an integer value in 0 .. 2^31 - 1 (-0 counts as 0), or -1 for anything else -- a
// fraction, a negative value, 2^31 and beyond, an infinity, a NaN (NA_real_ is one).
ICNV_RC_HD int64_t rc_count_of_bits(uint64_t bits) {
    if ((bits << 1) == 0) return 0;                                   // +0, -0
    if (bits >> 63) return -1;
    const int e = (int)((bits >> 52) & 0x7FF) - 1023;
    if (e < 0 || e > 30) return -1;                                   // below 1 (denormals too); 2^31 and beyond, Inf, NaN
    const uint64_t mant = bits & ((1ull << 52) - 1);
    if (mant & ((1ull << (52 - e)) - 1)) return -1;                   // a fraction
    return (int64_t)(((1ull << 52) | mant) >> (52 - e));
}

// the key of a violation: smaller keys win (an integer atomic minimum).  p violations: the index into p; entry violations: the
// entry's index in the stream, above RC_ENTRY_PHASE.  The code breaks ties.
ICNV_RC_HD uint64_t rc_key(int64_t index, int code, bool entry) {
    return (entry ? RC_ENTRY_PHASE : 0) | ((uint64_t)index << 3) | (uint64_t)code;
}

// The violation of entry e of file column c whose entries are [e_lo, e_hi): 0 or an ICNV_RDS_* code (the smallest that applies).
// `row` and `prev_row` are the decoded row indices of e and e - 1 (prev_row is read only when e > e_lo).
ICNV_RC_HD int rc_entry_code(int64_t e, int64_t e_lo, int32_t row, int32_t prev_row, int64_t G, uint64_t x_bits) {
    if (row < 0 || (int64_t)row >= G) return ICNV_RDS_ROW_RANGE;
    if (e > e_lo && prev_row >= row) return ICNV_RDS_ROW_ORDER;
    if (rc_count_of_bits(x_bits) < 0) return ICNV_RDS_VALUE;
    return 0;
}

struct RdsColumnsArgs {
    const uint8_t *stream;
    int64_t stream_bytes;
    const int64_t *col_off;      // device [n_out]
    const int32_t *col_kind;     // device [n_out]
    int64_t n_out, rows, ld;
    uint64_t *out;               // (n_out, rows) doubles as their bits, rows ld apart
};

struct RdsCscArgs {
    const uint8_t *stream;
    int64_t stream_bytes;
    int64_t i_off, p_off, x_off; // byte offsets of the payloads of i (nnz int32), p (C + 1 int32) and x (nnz doubles)
    int64_t G, C, nnz;
    const int32_t *cells;        // device [n_out] file columns, or null: all of them in order
    int64_t n_out;
    unsigned long long *key;     // device: the smallest violation key
    int64_t *colptr;             // device [n_out + 1]
    int32_t *rowidx, *vals;      // device [out_cap] (fill)
    int64_t out_cap;
};

#ifdef __HIPCC__
int launch_rds_columns(const RdsColumnsArgs &a, hipStream_t s);
int launch_rds_csc_check(const RdsCscArgs &a, hipStream_t s);            // p, then the entries of the selected columns -> a.key
int launch_rds_csc_colptr(const RdsCscArgs &a, hipStream_t s);           // the scan of the selected columns' lengths -> a.colptr
int launch_rds_csc_find_column(const RdsCscArgs &a, int64_t entry, int64_t *col_dev, hipStream_t s);
int launch_rds_csc_fill(const RdsCscArgs &a, hipStream_t s);
#endif

}  // namespace icnv
