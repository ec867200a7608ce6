// Shared between gunzip_api.hip (validation), gunzip_kernels.hip (K30: a gzip stream without flush points inflated on the
// device) and gunzip_host_check.cpp (the same finder test, measure and marker decoder on the host, under the sanitizers).
// DESIGN.md section 4 K30; the contract is in include/icnv.h "INFLATE with unknown history".
//
// Everything up to the launch declarations is __host__ __device__ and free of HIP.  The parser, its safety contract and the
// kernel bodies are inflate_internal.h's; what K30 adds to them is
//   * gz_header_ok   the per-bit-offset candidate test: if_dynamic_tables' acceptance rules without its tables (a lane keeps the
//                    code-length code and two sets of counts, about 140 bytes; they are indexed by value, so they live in
//                    scratch, but not the 1.3 KiB per lane an IfTables would take);
//   * GzSymbols      the policy of if_run for a unit that starts at a bit offset, ends on a listed candidate or behind BFINAL,
//                    and writes 16-bit symbols: a byte, or a marker for a byte of the 32 KiB in front of the unit.
#pragma once
#include "inflate_internal.h"

namespace icnv {

// if_run reports K29's codes: the codes the two contracts share must be the same numbers
static_assert(ICNV_GUNZIP_OK_BOUNDARY == ICNV_INFLATE_OK_MARKER && ICNV_GUNZIP_OK_FINAL == ICNV_INFLATE_OK_FINAL &&
              ICNV_GUNZIP_TRUNCATED == ICNV_INFLATE_TRUNCATED && ICNV_GUNZIP_TOO_LONG == ICNV_INFLATE_TOO_LONG &&
              ICNV_GUNZIP_BAD_STREAM == ICNV_INFLATE_BAD_STREAM, "K29's and K30's status codes");

constexpr int GZ_W = 32768;             // the window: the furthest a match reaches back
constexpr int GZ_TAILS_NT = 1024;       // tails: the one workgroup
constexpr int GZ_RESOLVE_NT = 256;

// Is bit offset `bit` of src[0, n) a candidate: BFINAL = 0, BTYPE = 10 and a dynamic header that if_dynamic_tables accepts,
// entirely inside the stream.  The cheap tests come first: 3 header bits and HLIT / HDIST (about 11 % of offsets pass), the
// code-length code's completeness, then the lengths.
IF_HD inline bool gz_header_ok(const uint8_t *src, int64_t n, int64_t bit) {
    if (bit < 0 || (bit >> 3) >= n) return false;
    IfReader r;
    if_reader_at(r, src, n, bit);
    if (!r.need(17)) return false;
    if (r.take(3) != 4u) return false;                              // BFINAL 0, BTYPE 10
    const int nlen = (int)r.take(5) + 257, ndist = (int)r.take(5) + 1, ncode = (int)r.take(4) + 4;
    if (nlen > IF_MAX_LIT || ndist > IF_MAX_DIST) return false;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint8_t cl[19];
    for (int i = 0; i < 19; ++i) cl[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        if (!r.need(3)) return false;
        cl[order[i]] = (uint8_t)r.take(3);
    }
    uint16_t ccount[16], csym[19];
    if (if_construct(ccount, csym, 19, cl, 19) != 0) return false; // the code-length code: complete
    uint16_t lcount[16], dcount[16];
    for (int l = 0; l < 16; ++l) lcount[l] = dcount[l] = 0;
    const int total = nlen + ndist;
    int at = 0, prev = 0;
    bool end_of_block = false;
    while (at < total) {                                            // every round takes at least one bit
        const int sym = if_symbol(r, ccount, csym, 19);
        if (sym < 0 || sym > 18) return false;                      // dry, or bits that are no code
        int value = 0, rep = 1;
        if (sym < 16) value = sym;
        else if (sym == 16) {
            if (at == 0 || !r.need(2)) return false;
            value = prev;
            rep = 3 + (int)r.take(2);
        } else if (sym == 17) {
            if (!r.need(3)) return false;
            rep = 3 + (int)r.take(3);
        } else {
            if (!r.need(7)) return false;
            rep = 11 + (int)r.take(7);
        }
        if (at + rep > total) return false;
        for (int k = 0; k < rep; ++k, ++at) {
            if (at < nlen) lcount[value]++; else dcount[value]++;
            if (at == 256 && value != 0) end_of_block = true;
        }
        prev = value;
    }
    if (!end_of_block) return false;
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - lcount[l];
        if (left < 0) return false;
    }
    if (!if_code_ok(left, lcount, nlen)) return false;
    left = 1;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - dcount[l];
        if (left < 0) return false;
    }
    return if_code_ok(left, dcount, ndist);
}

// Is b in the ascending list cand[0, n_cand)?
IF_HD inline bool gz_is_stop(const int64_t *cand, int64_t n_cand, int64_t b) {
    int64_t lo = 0, hi = n_cand;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cand[mid] < b) lo = mid + 1; else hi = mid;
    }
    return lo < n_cand && cand[lo] == b;
}

// if_run's policy for K30 (the five points are listed there).  A match may reach GZ_W symbols in front of the unit (the 30
// distance codes end at GZ_W: the test is kept as the store's own); the unit ends on a listed candidate once it is past its
// first block header; an empty stored block is a block like any other; positions are bit offsets.
struct GzSymbols {
    typedef uint16_t Elem;
    static constexpr int POS_SHIFT = 3;
    static constexpr int64_t REACH = GZ_W;
    static constexpr int TOO_FAR = ICNV_GUNZIP_BAD_STREAM;
    static constexpr bool MARKER_ENDS = false;
    const int64_t *cand;                // ascending bit offsets
    int64_t n_cand;
    int32_t past_first;                 // the unit has read its first block header
    IF_HD static uint16_t back(const uint16_t *sym, int64_t pos) {  // the symbol at unit position pos, pos >= -GZ_W
        return pos >= 0 ? sym[pos] : (uint16_t)(0x8000 | (int)(GZ_W + pos));
    }
    IF_HD bool stop(int64_t bit) {
        const bool hit = past_first && gz_is_stop(cand, n_cand, bit);
        past_first = 1;
        return hit;
    }
};

// One symbol into its byte: a marker reads the finished output in front of the unit (at `off`).  False: it points in front of
// byte 0 (or beyond the buffer) and nothing is to be written.
IF_HD inline bool gz_resolve_one(uint16_t v, const uint8_t *out, int64_t out_cap, int64_t off, uint8_t &byte) {
    if (v < 256) { byte = (uint8_t)v; return true; }
    const int64_t at = off - GZ_W + (v & 0x7FFF);
    if (!(v & 0x8000) || at < 0 || at >= off || at >= out_cap) return false;
    byte = out[at];
    return true;
}

struct GunzipArgs {
    const uint8_t *src;
    int64_t n;
    const int64_t *cand;
    int64_t n_cand;
    const int64_t *start;       // bits
    int64_t n_units;
    int64_t max_in;             // measure
    int64_t *end;               // bits.  measure: written; symbols: read
    int64_t *out_len;           // measure: written; symbols / tails / resolve: read
    const int64_t *out_off;     // symbols / tails / resolve
    uint16_t *sym;              // symbols: written; tails / resolve: read
    uint8_t *out;               // tails / resolve
    int64_t cap;                // symbols of sym, bytes of out
    int32_t *status;
};

#ifdef __HIPCC__
enum { GZ_CHECK_MEASURE = 0, GZ_CHECK_SYMBOLS = 1, GZ_CHECK_PLACES = 2 };
int launch_gunzip_find_count(const uint8_t *src, int64_t n, int64_t n_blocks, int64_t *block_off, hipStream_t s);   // block_off[n_blocks]: the total
int launch_gunzip_find_emit(const uint8_t *src, int64_t n, int64_t n_blocks, const int64_t *block_off, int64_t *cand, int64_t cand_cap, hipStream_t s);
int launch_gunzip_check(const GunzipArgs &a, int mode, int32_t *bad, hipStream_t s);
int launch_gunzip_measure(const GunzipArgs &a, hipStream_t s);
int launch_gunzip_symbols(const GunzipArgs &a, hipStream_t s);
int launch_gunzip_tails(const GunzipArgs &a, int32_t *bad, int64_t *markers, hipStream_t s);
int launch_gunzip_resolve(const GunzipArgs &a, int32_t *bad, hipStream_t s);
#endif

}  // namespace icnv
