// Shared between gunzip_api.hip (validation), gunzip_kernels.hip (K30: a gzip stream without flush points inflated on the
// device) and gunzip_host_check.cpp (the same finder test, measure and marker decoder on the host, under the sanitizers).
// DESIGN.md section 4 K30; the contract is in include/icnv.h "INFLATE with unknown history".
//
// Everything up to the launch declarations is __host__ __device__ and free of HIP.  The block parser is K29's
// (inflate_internal.h: IfReader, if_symbol, if_dynamic_tables); what is new is
//   * gz_header_ok   the per-bit-offset candidate test: if_dynamic_tables' acceptance rules without its tables (a lane keeps the
//                    code-length code and two sets of counts, about 140 bytes; they are indexed by value, so they live in
//                    scratch, but not the 1.3 KiB per lane an IfTables would take);
//   * gz_run         a sibling of if_run whose unit starts at a bit offset, ends on a listed candidate or behind BFINAL, and
//                    writes 16-bit symbols: a byte, or a marker for a byte of the 32 KiB in front of the unit.
// The safety rules are K29's: every load goes through IfReader (never at or beyond `limit` <= n), every store is tested against
// the unit's own range, every loop consumes at least one bit (a stored block: four bytes).
#pragma once
#include "inflate_internal.h"

namespace icnv {

// gz_run hands on what if_dry and if_dynamic_tables return: the codes the two contracts share must be the same numbers
static_assert(ICNV_GUNZIP_OK_FINAL == ICNV_INFLATE_OK_FINAL && ICNV_GUNZIP_TRUNCATED == ICNV_INFLATE_TRUNCATED &&
              ICNV_GUNZIP_TOO_LONG == ICNV_INFLATE_TOO_LONG && ICNV_GUNZIP_BAD_STREAM == ICNV_INFLATE_BAD_STREAM, "K29's and K30's status codes");

constexpr int GZ_W = 32768;             // the window: the furthest a match reaches back
constexpr int GZ_FIND_NT = 256;         // finder: lanes of a workgroup, one bit offset per lane and round
constexpr int GZ_FIND_ROUNDS = 16;      // finder: a workgroup covers GZ_FIND_NT * GZ_FIND_ROUNDS bit offsets
constexpr int GZ_TAILS_NT = 1024;       // tails: the one workgroup
constexpr int GZ_RESOLVE_NT = 256;

// A reader that stands on bit `bit` of src (bit b of the stream is bit b & 7 of byte b >> 3); bytes [0, limit) may be read.
IF_HD inline void gz_reader_at(IfReader &r, const uint8_t *src, int64_t limit, int64_t bit) {
    r.src = src;
    r.limit = limit;
    r.budget_cut = 0;
    r.p = bit >> 3;
    r.bb = 0;
    r.bc = 0;
    const int k = (int)(bit & 7);
    if (k && r.need(k)) r.take(k);      // (need fails only where every later need fails too: p >= limit)
}

// Is bit offset `bit` of src[0, n) a candidate: BFINAL = 0, BTYPE = 10 and a dynamic header that if_dynamic_tables accepts,
// entirely inside the stream.  The cheap tests come first: 3 header bits and HLIT / HDIST (about 11 % of offsets pass), the
// code-length code's completeness, then the lengths.
IF_HD inline bool gz_header_ok(const uint8_t *src, int64_t n, int64_t bit) {
    if (bit < 0 || (bit >> 3) >= n) return false;
    IfReader r;
    gz_reader_at(r, src, n, bit);
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

struct GzState {
    IfState s;                          // s.end and s.r count as in K29, but s.end is a BIT offset here
    int32_t past_first;                 // the unit has read its first block header
};

IF_HD inline void gz_init(GzState &g, const uint8_t *src, int64_t n, int64_t start_bit, int64_t max_in) {
    if_init(g.s, src, n, start_bit >> 3, max_in);
    const int k = (int)(start_bit & 7);
    if (k && g.s.r.need(k)) g.s.r.take(k);
    g.s.end = start_bit;
    g.past_first = 0;
}

IF_HD inline uint16_t gz_back(const uint16_t *sym, int64_t pos) {   // the symbol at unit position pos, pos >= -GZ_W
    return pos >= 0 ? sym[pos] : (uint16_t)(0x8000 | (int)(GZ_W + pos));
}

// Runs the unit from where it stands.  sym == nullptr: measure.  Otherwise the symbols go to sym[0, cap); a match of at least
// wide_min symbols and every stored block is handed back as an IfOp for the caller to copy (the caller then adds op.len to
// s.out_pos and calls again).  Ends with IF_OP_DONE and the status in op.len; s.end (bits) is set with the OK statuses.
IF_HD inline void gz_run(GzState &g, IfTables &t, const int64_t *cand, int64_t n_cand, uint16_t *sym, int64_t cap, int wide_min, IfOp &op) {
    IfState &s = g.s;
    IfReader &r = s.r;
    op.kind = IF_OP_DONE;
    op.a = 0;
    for (;;) {
        if (!s.in_block) {
            if (s.last) { op.len = if_finish(s, ICNV_GUNZIP_OK_FINAL, ((r.bit_pos() + 7) >> 3) << 3); return; }
            if (g.past_first && gz_is_stop(cand, n_cand, r.bit_pos())) { op.len = if_finish(s, ICNV_GUNZIP_OK_BOUNDARY, r.bit_pos()); return; }
            g.past_first = 1;
            if (!r.need(3)) { op.len = if_dry(s); return; }
            s.last = (int32_t)r.take(1);
            const int type = (int)r.take(2);
            if (type == 3) { op.len = ICNV_GUNZIP_BAD_STREAM; return; }
            if (type == 0) {
                const int64_t q = r.align_to_byte();
                if (q + 4 > r.limit) { op.len = if_dry(s); return; }
                const int len = r.src[q] | (r.src[q + 1] << 8), nlen = r.src[q + 2] | (r.src[q + 3] << 8);
                if ((len ^ 0xFFFF) != nlen) { op.len = ICNV_GUNZIP_BAD_STREAM; return; }
                r.p = q + 4;
                if (len == 0) continue;                             // (four bytes were taken)
                if (r.p + len > r.limit) { op.len = if_dry(s); return; }
                r.p += len;
                if (!sym) { s.out_pos += len; continue; }
                if (len > cap - s.out_pos) { op.len = ICNV_GUNZIP_BAD_STREAM; return; }
                op.kind = IF_OP_STORED;
                op.len = len;
                op.a = q + 4;
                return;
            }
            if (type == 1) {
                if_fixed_tables(t);
                s.have_dist = 1;
            } else {
                const int rc = if_dynamic_tables(s, t);
                if (rc) { op.len = rc; return; }
            }
            s.in_block = 1;
        }
        // ---- symbols of a Huffman-coded block: every round takes at least one bit
        const int c = if_symbol(r, t.lcount, t.lsym, 288);
        if (c == -2) { op.len = if_dry(s); return; }
        if (c < 0 || c >= IF_MAX_LIT) { op.len = ICNV_GUNZIP_BAD_STREAM; return; }
        if (c < 256) {
            if (sym) {
                if (s.out_pos >= cap) { op.len = ICNV_GUNZIP_BAD_STREAM; return; }
                sym[s.out_pos] = (uint16_t)c;
            }
            ++s.out_pos;
            continue;
        }
        if (c == 256) { s.in_block = 0; continue; }
        const int lc = c - 257;                                     // 0 .. 28
        int len;
        if (lc < 8) len = 3 + lc;
        else if (lc == 28) len = 258;
        else {
            const int eb = (lc >> 2) - 1;
            if (!r.need(eb)) { op.len = if_dry(s); return; }
            len = 3 + ((4 + (lc & 3)) << eb) + (int)r.take(eb);
        }
        if (!s.have_dist) { op.len = ICNV_GUNZIP_BAD_STREAM; return; }
        const int dc = if_symbol(r, t.dcount, t.dsym, 32);
        if (dc == -2) { op.len = if_dry(s); return; }
        if (dc < 0 || dc >= IF_MAX_DIST) { op.len = ICNV_GUNZIP_BAD_STREAM; return; }
        int64_t dist;
        if (dc < 4) dist = dc + 1;
        else {
            const int eb = (dc >> 1) - 1;
            if (!r.need(eb)) { op.len = if_dry(s); return; }
            dist = 1 + ((2 + (dc & 1)) << eb) + (int)r.take(eb);
        }
        if (dist > s.out_pos + GZ_W) { op.len = ICNV_GUNZIP_BAD_STREAM; return; }   // (the 30 distance codes end at GZ_W: kept as the store's own test)
        if (!sym) { s.out_pos += len; continue; }
        if (len > cap - s.out_pos) { op.len = ICNV_GUNZIP_BAD_STREAM; return; }
        if (len >= wide_min) {
            op.kind = IF_OP_MATCH;
            op.len = len;
            op.a = dist;
            return;
        }
        for (int k = 0; k < len; ++k, ++s.out_pos) sym[s.out_pos] = gz_back(sym, s.out_pos - dist);
    }
}

// A unit's ops on one thread: the host's way through gz_run, and the measure pass of either side.
IF_HD inline int gz_unit_serial(const uint8_t *src, int64_t n, int64_t start_bit, int64_t max_in, const int64_t *cand, int64_t n_cand,
                                IfTables &t, uint16_t *sym, int64_t cap, int64_t *end, int64_t *out_len) {
    GzState g;
    IfOp op;
    gz_init(g, src, n, start_bit, max_in);
    for (;;) {
        gz_run(g, t, cand, n_cand, sym, cap, 1 << 30, op);
        if (op.kind == IF_OP_DONE) break;
        for (int k = 0; k < op.len; ++k) sym[g.s.out_pos + k] = src[op.a + k];   // IF_OP_STORED: tested against cap and the limit
        g.s.out_pos += op.len;
    }
    *end = g.s.end;
    *out_len = g.s.out_pos;
    return op.len;
}

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
