// The one DEFLATE parser of the library, shared by K29 (inflate_*.hip: gzip streams with flush points, a unit starts on a byte
// and gives bytes) and K30 (gunzip_*.hip, gunzip_internal.h: any gzip stream, a unit starts on a bit, ends on a listed candidate
// and gives 16-bit symbols), and by inflate_host_check.cpp / gunzip_host_check.cpp, which run it on the host under the
// sanitizers.  DESIGN.md section 4 K29 and K30; the contracts are in include/icnv.h "INFLATE in independent units" and "INFLATE
// with unknown history".
//
// Everything up to `#ifdef __HIPCC__` is __host__ __device__ and free of HIP: a plain C++ compiler builds it.  There is one
// block walker (if_run) and, for the device, one measure body, one wavefront decode loop (if_decode_wave) and one pair of finder
// tiles; what differs between K29 and K30 is a policy type (IfBytes here, GzSymbols in gunzip_internal.h) that answers five
// questions and nothing else.  The safety contract, stated next to if_run, is kept in this one place.
#pragma once
#include <stdint.h>

#include "../../include/icnv.h"

#if defined(__HIPCC__)
#define IF_HD __host__ __device__
#else
#define IF_HD
#endif

namespace icnv {

constexpr int IF_WAVES = 4;             // wavefronts of a workgroup: one unit per wavefront
constexpr int IF_NT = IF_WAVES * 64;
constexpr int IF_WIDE_MIN = 8;          // matches of at least this many bytes are copied by the whole wavefront
constexpr int SC_NT = 256;              // scan / find: lanes of a workgroup
constexpr int SC_ROUNDS = 16;           // scan / find: positions per lane; a workgroup covers SC_NT * SC_ROUNDS positions
constexpr int CRC_SUB = 64;             // crc32_pieces: bytes a lane folds at a time; a wavefront covers 64 * CRC_SUB per round

constexpr int IF_MAX_LIT = 286, IF_MAX_DIST = 30;    // the symbols a dynamic header may define (zlib's limits)

struct IfTables {                       // canonical Huffman codes: counts per length, symbols in code order (1 KiB per wavefront)
    uint16_t lcount[16], dcount[16];
    uint16_t lsym[288], dsym[32];
    uint8_t lens[320];                  // the code lengths while a header is parsed
};

struct IfReader {
    const uint8_t *src;
    int64_t limit;                      // bytes [0, limit) of src may be read: min(n, start + max_in)
    int64_t p;                          // the next byte to load
    uint64_t bb;                        // loaded bits, the stream's next bit at bit 0
    int32_t bc;                         // how many
    int32_t budget_cut;                 // limit < n: running dry is TOO_LONG, not TRUNCATED

    IF_HD void refill() {               // at least 32 bits, or everything up to the limit
        while (bc <= 56 && p < limit) {
            bb |= (uint64_t)src[p++] << bc;
            bc += 8;
        }
    }
    IF_HD bool need(int k) {            // k <= 32
        if (bc < k) refill();
        return bc >= k;
    }
    IF_HD uint32_t take(int k) {        // after need(k)
        const uint32_t v = (uint32_t)(bb & ((1ull << k) - 1));
        bb >>= k;
        bc -= k;
        return v;
    }
    IF_HD int64_t bit_pos() const { return p * 8 - bc; }
    IF_HD int64_t align_to_byte() {     // drops the rest of the current byte and the loaded bytes: returns the byte position
        const int64_t q = (bit_pos() + 7) >> 3;
        bb = 0;
        bc = 0;
        p = q;
        return q;
    }
};

// A reader that stands on bit `bit` of src (bit b of the stream is bit b & 7 of byte b >> 3); bytes [0, limit) may be read.
IF_HD inline void if_reader_at(IfReader &r, const uint8_t *src, int64_t limit, int64_t bit) {
    r.src = src;
    r.limit = limit;
    r.budget_cut = 0;
    r.p = bit >> 3;
    r.bb = 0;
    r.bc = 0;
    const int k = (int)(bit & 7);
    if (k && r.need(k)) r.take(k);      // (need fails only where every later need fails too: p >= limit)
}

struct IfState {
    IfReader r;
    int64_t out_pos;                    // elements (K29: bytes, K30: symbols) the unit has produced
    int64_t end;                        // with a final status: the position just behind the unit (K29: a byte, K30: a bit offset)
    int32_t in_block;                   // 1: inside a Huffman-coded block
    int32_t last;                       // BFINAL of the current (or the latest) block
    int32_t have_dist;                  // the block defines at least one distance code
};

enum { IF_OP_DONE = 0, IF_OP_MATCH = 1, IF_OP_STORED = 2 };
struct IfOp {
    int32_t kind;
    int32_t len;                        // DONE: the status; MATCH / STORED: elements to produce
    int64_t a;                          // MATCH: the distance; STORED: the offset in src
};

// The unit that starts at position `start`, counted as policy P counts (1 << P::POS_SHIFT positions in a byte), and may take
// max_in bytes from the start's byte on.
template <class P>
IF_HD inline void if_init(IfState &s, const uint8_t *src, int64_t n, int64_t start, int64_t max_in) {
    const int64_t byte = start >> P::POS_SHIFT;
    const int64_t limit = max_in < n - byte ? byte + max_in : n;
    if_reader_at(s.r, src, limit, start << (3 - P::POS_SHIFT));
    s.r.budget_cut = limit < n ? 1 : 0;
    s.out_pos = 0;
    s.end = start;
    s.in_block = 0;
    s.last = 0;
    s.have_dist = 0;
}

IF_HD inline int if_dry(const IfState &s) { return s.r.budget_cut ? ICNV_INFLATE_TOO_LONG : ICNV_INFLATE_TRUNCATED; }

// count[1..15], sym[] from the n code lengths; returns the code space left over (> 0: incomplete, < 0: over-subscribed)
IF_HD inline int if_construct(uint16_t *count, uint16_t *sym, int sym_cap, const uint8_t *lens, int n) {
    for (int l = 0; l < 16; ++l) count[l] = 0;
    for (int i = 0; i < n; ++i) count[lens[i] & 15]++;
    int left = 1;
    for (int l = 1; l < 16; ++l) {
        left = (left << 1) - count[l];
        if (left < 0) return left;
    }
    uint16_t offs[16];
    offs[1] = 0;
    for (int l = 1; l < 15; ++l) offs[l + 1] = (uint16_t)(offs[l] + count[l]);
    for (int i = 0; i < n; ++i) {
        const int l = lens[i] & 15;
        if (l && offs[l] < sym_cap) sym[offs[l]++] = (uint16_t)i;
    }
    return left;
}

// The next symbol of a canonical code: >= 0, -1 when the bits are no code, -2 when the stream runs dry inside the code.
IF_HD inline int if_symbol(IfReader &r, const uint16_t *count, const uint16_t *sym, int sym_cap) {
    if (r.bc < 15) r.refill();
    uint32_t bits = (uint32_t)r.bb;
    const int avail = r.bc;
    int code = 0, first = 0, index = 0;
    for (int len = 1; len <= 15; ++len) {
        if (len > avail) return -2;
        code |= (int)(bits & 1u);
        bits >>= 1;
        const int c = count[len];
        if (code - c < first) {
            const int at = index + (code - first);
            r.bb >>= len;
            r.bc -= len;
            return at < sym_cap ? sym[at] : -1;
        }
        index += c;
        first += c;
        first <<= 1;
        code <<= 1;
    }
    return -1;
}

// zlib's rule for the literal/length and the distance code: complete, or no code at all, or one single code of length one
IF_HD inline bool if_code_ok(int left, const uint16_t *count, int n) {
    if (left < 0) return false;
    if (left == 0) return true;
    const int used = n - count[0];
    return used == 0 || (used == 1 && count[1] == 1);
}

IF_HD inline int if_fixed_tables(IfTables &t) {
    for (int i = 0; i < 288; ++i) t.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
    if_construct(t.lcount, t.lsym, 288, t.lens, 288);
    for (int i = 0; i < 32; ++i) t.lens[i] = 5;
    if_construct(t.dcount, t.dsym, 32, t.lens, 32);
    return 0;
}

// The header of a dynamic block into the tables: 0, or a final status.  (K30's finder, gz_header_ok of gunzip_internal.h, applies
// the same acceptance rules without the tables; the two are kept apart because a shared walk cost the finder registers and
// time, and gunzip_host_check.cpp holds them against each other at every bit offset of its corpus.)
IF_HD inline int if_dynamic_tables(IfState &s, IfTables &t) {
    IfReader &r = s.r;
    if (!r.need(14)) return if_dry(s);
    const int nlen = (int)r.take(5) + 257, ndist = (int)r.take(5) + 1, ncode = (int)r.take(4) + 4;
    if (nlen > IF_MAX_LIT || ndist > IF_MAX_DIST) return ICNV_INFLATE_BAD_STREAM;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    for (int i = 0; i < 19; ++i) t.lens[i] = 0;
    for (int i = 0; i < ncode; ++i) {
        if (!r.need(3)) return if_dry(s);
        t.lens[order[i]] = (uint8_t)r.take(3);
    }
    if (if_construct(t.lcount, t.lsym, 288, t.lens, 19) != 0) return ICNV_INFLATE_BAD_STREAM;   // the code-length code: complete
    const int total = nlen + ndist;                                 // <= 316
    int at = 0;
    while (at < total) {                                            // every round takes at least one bit
        const int sym = if_symbol(r, t.lcount, t.lsym, 288);
        if (sym == -2) return if_dry(s);
        if (sym < 0 || sym > 18) return ICNV_INFLATE_BAD_STREAM;
        if (sym < 16) {
            t.lens[at++] = (uint8_t)sym;
            continue;
        }
        int value = 0, rep;
        if (sym == 16) {
            if (at == 0) return ICNV_INFLATE_BAD_STREAM;            // nothing to repeat
            if (!r.need(2)) return if_dry(s);
            value = t.lens[at - 1];
            rep = 3 + (int)r.take(2);
        } else if (sym == 17) {
            if (!r.need(3)) return if_dry(s);
            rep = 3 + (int)r.take(3);
        } else {
            if (!r.need(7)) return if_dry(s);
            rep = 11 + (int)r.take(7);
        }
        if (at + rep > total) return ICNV_INFLATE_BAD_STREAM;      // lengths running past HLIT + HDIST
        while (rep-- > 0) t.lens[at++] = (uint8_t)value;
    }
    if (t.lens[256] == 0) return ICNV_INFLATE_BAD_STREAM;           // a block that could never end
    uint8_t dl[32];                                                 // the distance lengths: lcount / lsym are rebuilt over lens first
    for (int i = 0; i < 32; ++i) dl[i] = i < ndist ? t.lens[nlen + i] : 0;
    int left = if_construct(t.lcount, t.lsym, 288, t.lens, nlen);
    if (!if_code_ok(left, t.lcount, nlen)) return ICNV_INFLATE_BAD_STREAM;
    left = if_construct(t.dcount, t.dsym, 32, dl, ndist);
    if (!if_code_ok(left, t.dcount, ndist)) return ICNV_INFLATE_BAD_STREAM;
    s.have_dist = ndist - t.dcount[0] > 0 ? 1 : 0;
    return 0;
}

IF_HD inline int if_finish(IfState &s, int status, int64_t end) {
    s.end = end;
    return status;
}

// ---- the block walker -----------------------------------------------------------------------------------------------------------------
// This is the one parser of the library that faces untrusted bytes.  Its contract, for every policy:
//   * every load of the compressed stream goes through IfReader, which never reads at or beyond `limit` <= n (the stored block's
//     four length bytes and its payload are tested against r.limit here);
//   * every store is tested against the unit's own out_cap: the literal and the short match here, and the caller's copy of an
//     IfOp, which this function has tested and which the caller tests again;
//   * a match never reads in front of out[0]: a distance beyond out_pos + P::REACH is refused, and P::back answers for the
//     REACH positions in front of the unit without a load;
//   * every loop consumes at least one bit of the stream per round (a stored block: four bytes), so it ends with the budget.
//
// A policy P answers the five points at which K29's and K30's units differ, and nothing else:
//   Elem, back(out, pos)   the sink's element, and the element at unit position pos >= -REACH (pos < 0: in front of the unit);
//   REACH, TOO_FAR         how far in front of the unit a match may reach, and the status of one that reaches further;
//   MARKER_ENDS            does an empty stored block (a flush marker) end the unit;
//   stop(bit)              called ahead of every block header: does the unit end here, on bit offset `bit`, with status 0;
//   POS_SHIFT              log2 of the positions per byte (0: start and s.end count bytes; 3: they count bits).
struct IfBytes {                        // K29: bytes out, nothing in front of the unit, ends on a flush marker
    typedef uint8_t Elem;
    static constexpr int POS_SHIFT = 0;
    static constexpr int64_t REACH = 0;
    static constexpr int TOO_FAR = ICNV_INFLATE_NEEDS_HISTORY;
    static constexpr bool MARKER_ENDS = true;
    IF_HD static uint8_t back(const uint8_t *out, int64_t pos) { return out[pos]; }
    IF_HD bool stop(int64_t) { return false; }
};

// Runs the unit from where it stands.  out == nullptr: measure -- nothing is stored, every match and stored block is only
// counted.  Otherwise the elements go to out[0, out_cap); a match of at least wide_min elements and every stored block is handed
// back as an IfOp for the caller to copy (the caller then adds op.len to s.out_pos and calls again).  Ends with IF_OP_DONE and
// the status in op.len; s.end is set with the OK statuses.
template <class P>
IF_HD inline void if_run(P &p, IfState &s, IfTables &t, typename P::Elem *out, int64_t out_cap, int wide_min, IfOp &op) {
    typedef typename P::Elem Elem;
    IfReader &r = s.r;
    op.kind = IF_OP_DONE;
    op.a = 0;
    for (;;) {
        if (!s.in_block) {
            if (s.last) { op.len = if_finish(s, ICNV_INFLATE_OK_FINAL, ((r.bit_pos() + 7) >> 3) << P::POS_SHIFT); return; }
            if (p.stop(r.bit_pos())) { op.len = if_finish(s, ICNV_INFLATE_OK_MARKER, r.bit_pos() >> (3 - P::POS_SHIFT)); return; }
            if (!r.need(3)) { op.len = if_dry(s); return; }
            s.last = (int32_t)r.take(1);
            const int type = (int)r.take(2);
            if (type == 3) { op.len = ICNV_INFLATE_BAD_STREAM; return; }
            if (type == 0) {
                const int64_t q = r.align_to_byte();
                if (q + 4 > r.limit) { op.len = if_dry(s); return; }
                const int len = r.src[q] | (r.src[q + 1] << 8), nlen = r.src[q + 2] | (r.src[q + 3] << 8);
                if ((len ^ 0xFFFF) != nlen) { op.len = ICNV_INFLATE_BAD_STREAM; return; }
                r.p = q + 4;
                if (len == 0) {                                     // the flush marker (four bytes were taken)
                    if (!P::MARKER_ENDS) continue;
                    op.len = if_finish(s, s.last ? ICNV_INFLATE_OK_FINAL : ICNV_INFLATE_OK_MARKER, r.p << P::POS_SHIFT);
                    return;
                }
                if (r.p + len > r.limit) { op.len = if_dry(s); return; }
                r.p += len;
                if (!out) { s.out_pos += len; continue; }
                if (len > out_cap - s.out_pos) { op.len = ICNV_INFLATE_BAD_STREAM; return; }
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
        const int sym = if_symbol(r, t.lcount, t.lsym, 288);
        if (sym == -2) { op.len = if_dry(s); return; }
        if (sym < 0 || sym >= IF_MAX_LIT) { op.len = ICNV_INFLATE_BAD_STREAM; return; }
        if (sym < 256) {
            if (out) {
                if (s.out_pos >= out_cap) { op.len = ICNV_INFLATE_BAD_STREAM; return; }
                out[s.out_pos] = (Elem)sym;
            }
            ++s.out_pos;
            continue;
        }
        if (sym == 256) { s.in_block = 0; continue; }
        const int lc = sym - 257;                                   // 0 .. 28
        int len;
        if (lc < 8) len = 3 + lc;
        else if (lc == 28) len = 258;
        else {
            const int eb = (lc >> 2) - 1;
            if (!r.need(eb)) { op.len = if_dry(s); return; }
            len = 3 + ((4 + (lc & 3)) << eb) + (int)r.take(eb);
        }
        if (!s.have_dist) { op.len = ICNV_INFLATE_BAD_STREAM; return; }
        const int dc = if_symbol(r, t.dcount, t.dsym, 32);
        if (dc == -2) { op.len = if_dry(s); return; }
        if (dc < 0 || dc >= IF_MAX_DIST) { op.len = ICNV_INFLATE_BAD_STREAM; return; }
        int64_t dist;
        if (dc < 4) dist = dc + 1;
        else {
            const int eb = (dc >> 1) - 1;
            if (!r.need(eb)) { op.len = if_dry(s); return; }
            dist = 1 + ((2 + (dc & 1)) << eb) + (int)r.take(eb);
        }
        if (dist > s.out_pos + P::REACH) { op.len = P::TOO_FAR; return; }
        if (!out) { s.out_pos += len; continue; }
        if (len > out_cap - s.out_pos) { op.len = ICNV_INFLATE_BAD_STREAM; return; }
        if (len >= wide_min) {
            op.kind = IF_OP_MATCH;
            op.len = len;
            op.a = dist;
            return;
        }
        for (int k = 0; k < len; ++k, ++s.out_pos) out[s.out_pos] = P::back(out, s.out_pos - dist);
    }
}

// A unit's ops on one thread: the host's way through if_run, and the measure pass of either side.
template <class P>
IF_HD inline int if_unit_serial(P p, const uint8_t *src, int64_t n, int64_t start, int64_t max_in, IfTables &t, typename P::Elem *out,
                                int64_t out_cap, int64_t *end, int64_t *out_len) {
    IfState s;
    IfOp op;
    if_init<P>(s, src, n, start, max_in);
    for (;;) {
        if_run(p, s, t, out, out_cap, 1 << 30, op);
        if (op.kind == IF_OP_DONE) break;
        for (int k = 0; k < op.len; ++k) out[s.out_pos + k] = src[op.a + k];   // IF_OP_STORED: tested against out_cap and the limit
        s.out_pos += op.len;
    }
    *end = s.end;
    *out_len = s.out_pos;
    return op.len;
}

struct InflateArgs {
    const uint8_t *src;
    int64_t n;
    const int64_t *start;
    int64_t n_units;
    int64_t max_in;             // measure
    int64_t *end;               // measure: written; units: read (const there)
    int64_t *out_len;           // measure: written; units: read
    const int64_t *out_off;     // units
    uint8_t *out;               // units
    int64_t out_cap;
    int32_t *status;
};

#ifdef __HIPCC__
// The workgroup's exclusive rank of this lane's flag in lane order, and the workgroup's total.  s_w: SC_NT / 64 ints.
__device__ inline int sc_rank(bool flag, int *s_w, int &total) {
    const int t = threadIdx.x, lane = t & 63;
    const unsigned long long b = __ballot(flag);
    const int below = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();                                                // the sums of the round before have been read
    if (lane == 0) s_w[t >> 6] = __popcll(b);
    __syncthreads();
    int base = 0;
    total = 0;
    for (int w = 0; w < SC_NT / 64; ++w) {
        if (w < (t >> 6)) base += s_w[w];
        total += s_w[w];
    }
    return base + below;
}

// The bodies of a finder's two kernels (K29's scan for flush markers, K30's find of block headers), launched with SC_NT lanes
// over n_blocks tiles of SC_NT * SC_ROUNDS positions.  hit(src, n, p) tests position p and every load it makes against n itself.
// count: block_off[tile] = the tile's hits.  emit, after the prefix sum of the counts: the hits of a tile in ascending order to
// cand[block_off[tile] ...], each store tested against cand_cap.  The predicate is a template argument, a function named at
// compile time: the call is direct, and the predicate is compiled as the one function it is, not once more inside a wrapper.
typedef bool ScHit(const uint8_t *src, int64_t n, int64_t p);
template <ScHit hit>
__device__ inline void sc_count_tile(const uint8_t *src, int64_t n, int64_t n_blocks, int64_t *block_off) {
    __shared__ int s_w[SC_NT / 64];
    const int64_t tile0 = (int64_t)blockIdx.x * (SC_NT * SC_ROUNDS);
    int count = 0;
    for (int r = 0; r < SC_ROUNDS; ++r) {
        int total;
        sc_rank(hit(src, n, tile0 + r * SC_NT + threadIdx.x), s_w, total);
        count += total;
    }
    if (threadIdx.x == 0 && blockIdx.x < n_blocks) block_off[blockIdx.x] = count;
}

template <ScHit hit>
__device__ inline void sc_emit_tile(const uint8_t *src, int64_t n, int64_t n_blocks, const int64_t *block_off, int64_t *cand,
                                    int64_t cand_cap) {
    __shared__ int s_w[SC_NT / 64];
    if (blockIdx.x >= n_blocks) return;
    const int64_t tile0 = (int64_t)blockIdx.x * (SC_NT * SC_ROUNDS);
    int64_t at = block_off[blockIdx.x];
    for (int r = 0; r < SC_ROUNDS; ++r) {
        const int64_t p = tile0 + r * SC_NT + threadIdx.x;
        const bool flag = hit(src, n, p);
        int total;
        const int rank = sc_rank(flag, s_w, total);
        if (flag && at + rank >= 0 && at + rank < cand_cap) cand[at + rank] = p;
        at += total;
    }
}

// The body of a measure kernel (IF_NT lanes, a unit per wavefront; A: InflateArgs or GunzipArgs): lane 0 walks the unit, stores
// nothing, and reports where it ends, how many elements it gives, and its status.
template <class P, class A>
__device__ inline void if_measure_lane(const A &a, P p) {
    __shared__ IfTables s_tab[IF_WAVES];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * IF_WAVES + w;
    if (u >= a.n_units || lane != 0) return;
    const int64_t start = a.start[u];
    int64_t end = start, out_len = 0;
    int status = ICNV_INFLATE_BAD_STREAM;
    if (start >= 0 && (start >> P::POS_SHIFT) < a.n)                    // (the check kernel has refused anything else)
        status = if_unit_serial(p, a.src, a.n, start, a.max_in, s_tab[w], (typename P::Elem *)nullptr, 0, &end, &out_len);
    a.end[u] = end;
    a.out_len[u] = out_len;
    a.status[u] = status;
}

// The body of a decode kernel (IF_NT lanes, a unit per wavefront): the walk of if_measure_lane with stores into
// out_all[out_off[u], + out_len[u]) of out_all[0, out_cap).  Lane 0 stores the literals and copies matches shorter than
// IF_WIDE_MIN itself; a longer match and every stored block is handed through LDS to all 64 lanes, which copy it together (a
// match whose distance is below its length is a periodic fill: element k comes from offset k mod distance).  A workgroup-scope
// fence stands on either side of such a copy: the lanes of a wavefront share one L1.
template <class P, class A>
__device__ inline void if_decode_wave(const A &a, P p, typename P::Elem *out_all, int64_t out_cap) {
    __shared__ IfTables s_tab[IF_WAVES];
    __shared__ IfOp s_op[IF_WAVES];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * IF_WAVES + w;
    if (u >= a.n_units) return;                                     // whole wavefronts leave: no workgroup barrier follows
    const int64_t start = a.start[u], end = a.end[u], off = a.out_off[u], cap = a.out_len[u];
    const bool sane = start >= 0 && (start >> P::POS_SHIFT) < a.n && end >= start && end <= (a.n << P::POS_SHIFT) && off >= 0 && cap >= 0 &&
                      off <= out_cap && cap <= out_cap - off;
    if (!sane) {                                                    // (the check kernel has refused it)
        if (lane == 0) a.status[u] = ICNV_INFLATE_BAD_STREAM;
        return;
    }
    typename P::Elem *out = out_all + off;
    IfState s;
    if_init<P>(s, a.src, a.n, start, ((end + (1 << P::POS_SHIFT) - 1) >> P::POS_SHIFT) - (start >> P::POS_SHIFT));     // the budget is the caller's end
    int status;
    for (;;) {                                                      // every round but the last consumes bits of the unit
        if (lane == 0) {
            IfOp op;
            if_run(p, s, s_tab[w], out, cap, IF_WIDE_MIN, op);
            s_op[w] = op;
        }
        __threadfence_block();                                      // lane 0's op and its stores are visible to the wavefront
        const IfOp op = s_op[w];
        if (op.kind == IF_OP_DONE) { status = op.len; break; }
        const int64_t o0 = __shfl(s.out_pos, 0, 64);                // lane 0's value
        const int len = op.len;
        if (len > 0 && len <= cap - o0) {                           // if_run has tested this; the store's own test all the same
            if (op.kind == IF_OP_MATCH) {
                const int64_t dist = op.a;
                if (dist >= 1 && dist <= o0 + P::REACH)
                    for (int k = lane; k < len; k += 64) out[o0 + k] = P::back(out, o0 - dist + (dist >= len ? k : k % dist));
            } else if (op.a >= 0 && op.a + len <= a.n) {
                for (int k = lane; k < len; k += 64) out[o0 + k] = a.src[op.a + k];
            }
        }
        __threadfence_block();                                      // the copy is visible before lane 0 reads behind it
        s.out_pos = o0 + len;
    }
    if (lane == 0) {
        const bool ok = status == ICNV_INFLATE_OK_MARKER || status == ICNV_INFLATE_OK_FINAL;
        if (ok && (s.end != end || s.out_pos != cap)) status = ICNV_INFLATE_BAD_STREAM;
        if (status == ICNV_INFLATE_TOO_LONG) status = ICNV_INFLATE_BAD_STREAM;     // the budget was the caller's end: it is too early
        a.status[u] = status;
    }
}

int launch_scan_offsets(int64_t n_blocks, int64_t *block_off, hipStream_t s);   // block_off[i]: the sum before i; block_off[n_blocks]: the total (K30's finder shares it)
int launch_inflate_scan_count(const uint8_t *src, int64_t n, int64_t n_blocks, int64_t *block_off, hipStream_t s);   // block_off[n_blocks]: the total
int launch_inflate_scan_emit(const uint8_t *src, int64_t n, int64_t n_blocks, const int64_t *block_off, int64_t *cand, int64_t cand_cap, hipStream_t s);
int launch_inflate_check(const InflateArgs &a, bool units, int32_t *bad, hipStream_t s);
int launch_inflate_measure(const InflateArgs &a, hipStream_t s);
int launch_inflate_units(const InflateArgs &a, hipStream_t s);
int launch_crc32_pieces(const uint8_t *src, int64_t n, int64_t piece_bytes, int64_t n_pieces, uint32_t *crc, hipStream_t s);
#endif

}  // namespace icnv
