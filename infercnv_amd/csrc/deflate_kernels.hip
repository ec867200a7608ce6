// K28 kernels: DEFLATE (RFC 1951) of a byte stream in independent pieces, one workgroup of 256 lanes per piece, and the packing
// of the pieces into one buffer.  DESIGN.md section 4 K28.
//
// A piece (at most DF_MAX_PIECE = 16 KiB) lives in LDS from its load to its last output byte:
//   load     the piece into s_in (dword loads where src + offset is 4-byte aligned, byte loads otherwise), zero padded; every
//            lane folds its 64 bytes into a CRC-32 and multiplies it by x^(8 * bytes behind it) mod P; the piece's CRC is the
//            XOR of the 256 products (crc32_combine's identity, so the order of the lanes does not matter).
//   match    chunks of 256 positions, one per lane, in order.  A lane reads the hash table's candidate for the 4 bytes at its
//            position (the latest such position of an EARLIER chunk: the table is updated with atomicMax after the reads, so
//            its content is a function of the input alone), and measures three candidates 8 bytes at a time: distance 8 (a
//            repeated double), distance 1 (a repeated byte) and the table's.  The longest wins, the earlier in that order on a
//            tie; the table's needs 4 bytes, the others 3.  Lengths are capped by 258 and by the piece's end.
//   parse    greedy, inside the same chunk loop: the chunk's entry position is carried from the chunk before; the positions
//            reachable from it by "next = position + (match ? length : 1)" are marked by pointer doubling over the chunk's
//            256 successors: at most eight rounds, fewer once every pointer has left the chunk (__syncthreads_or).  Unmarked
//            positions are flagged as skipped; marked ones count into the histograms (integer LDS atomics: sums).
//   codes    lane-parallel rank sort of the used symbols by (frequency, symbol), then lane 0 runs the in-place
//            minimum-redundancy algorithm of Moffat and Katajainen; when the longest code exceeds the limit (15, or 7 for the
//            code-length alphabet) every frequency is halved (rounded up) and the lengths are rebuilt, at most 16 times --
//            equal frequencies give depth <= 9.  Failing that the piece is stored.  The run-length coding of the length
//            sequence is lane 0's; the canonical codes are one symbol per lane, bit-reversed once.
//   cost     the exact size of the dynamic block (integer sums over the lanes); the piece is stored when that is not smaller.
//   emit     header by lane 0; tokens chunk by chunk: every lane's bits (<= 48) are placed by an exclusive prefix sum of the bit
//            counts and OR-ed into a 2 KiB staging area (LDS atomicOr: order free); whole bytes are copied out and the partial
//            byte carried whenever the next chunk might not fit.  Then the end-of-block code and the empty stored block of a
//            sync flush (000, pad, 00 00 FF FF).
// Every store to dst passes through df_store, which tests the offset against the bound; every LDS index is masked or tested.
#include "icnv_internal.h"
#include "deflate_internal.h"

namespace icnv {

namespace {

constexpr int DF_HASH_BITS = 11, DF_HASH_SIZE = 1 << DF_HASH_BITS;
constexpr int DF_STAGE_WORDS = 512;                 // 2 KiB: 256 tokens of <= 48 bits and a carried byte; the header (<= 563 bytes)
constexpr int DF_NLIT = 286, DF_NDIST = 30, DF_NCL = 19, DF_NSEQ = DF_NLIT + DF_NDIST;
constexpr int DF_ASZ = 288;                         // room of the sort arrays (>= DF_NLIT)
constexpr uint32_t DF_POLY = 0xEDB88320u;
constexpr uint16_t DF_SKIP = 0xFFFF;                // s_dist: the position lies inside a match

__constant__ uint8_t c_cl_order[DF_NCL] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

// ---- CRC-32 (zlib's: reflected 0xEDB88320) ----------------------------------------------------------------------------------------
__device__ inline uint32_t crc_mul(uint32_t a, uint32_t b) {        // a(x) * b(x) mod P, reflected: bit 31 is x^0
    uint32_t p = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ DF_POLY : b >> 1;
    }
    return p;
}

__device__ inline uint32_t crc_xpow8(uint32_t nbytes) {             // x^(8 * nbytes) mod P, nbytes < 2^15
    uint32_t r = 0x80000000u, b = 0x00800000u;                      // x^0, x^8
    for (int i = 0; i < 15; ++i) {
        if (nbytes & 1u) r = crc_mul(r, b);
        b = crc_mul(b, b);
        nbytes >>= 1;
    }
    return r;
}

// ---- symbols ----------------------------------------------------------------------------------------------------------------------
__device__ inline void len_symbol(int len, int &code, int &ebits, int &eval) {   // len 3..258 -> code 0..28 (symbol 257 + code)
    const int l = len - 3;
    if (len == 258) { code = 28; ebits = 0; eval = 0; return; }
    if (l < 8) { code = l; ebits = 0; eval = 0; return; }
    const int k = 31 - __builtin_clz((unsigned)l);                  // 3..7
    code = ((k - 1) << 2) + ((l >> (k - 2)) & 3);
    ebits = k - 2;
    eval = l & ((1 << ebits) - 1);
}

__device__ inline void dist_symbol(int dist, int &code, int &ebits, int &eval) {  // dist 1..32768 -> code 0..29
    const int d = dist - 1;
    if (d < 4) { code = d; ebits = 0; eval = 0; return; }
    const int k = 31 - __builtin_clz((unsigned)d);                  // 2..14
    code = 2 * k + ((d >> (k - 1)) & 1);
    ebits = k - 1;
    eval = d & ((1 << ebits) - 1);
}

__device__ inline int len_extra_bits(int code) { return (code < 8 || code == 28) ? 0 : (code >> 2) - 1; }
__device__ inline int dist_extra_bits(int code) { return code < 4 ? 0 : (code >> 1) - 1; }

__device__ inline uint32_t bit_reverse(uint32_t code, int len) { return len ? __builtin_bitreverse32(code) >> (32 - len) : 0; }

// ---- LDS byte stream ----------------------------------------------------------------------------------------------------------------
__device__ inline uint64_t load64(const uint64_t *in64, int p) {    // the 8 bytes at byte p; p <= DF_MAX_PIECE - 1
    const int w = p >> 3, s = (p & 7) * 8;
    const uint64_t a = in64[w], b = in64[w + 1];
    return s ? (a >> s) | (b << (64 - s)) : a;
}

// The 8 bytes at byte p of the LDS stream, then the next 8, and so on: one new aligned word per step.
struct ByteStream {
    const uint64_t *in;
    int w, s;
    uint64_t lo, hi;
    __device__ ByteStream(const uint64_t *in64, int p) : in(in64), w(p >> 3), s((p & 7) * 8) { lo = in[w]; hi = in[w + 1]; }
    __device__ uint64_t get() const { return s ? (lo >> s) | (hi << (64 - s)) : lo; }
    __device__ void next() {
        lo = hi;
        ++w;
        hi = in[w + 1 < DF_MAX_PIECE / 8 + 2 ? w + 1 : DF_MAX_PIECE / 8 + 1];
    }
};

// Equal bytes of [p..) and [q..), q < p, at most maxlen <= 258: <= 33 rounds each.
__device__ inline int match_len(const uint64_t *in64, int p, int q, int maxlen) {
    ByteStream a(in64, p), b(in64, q);
    int l = 0;
    while (l < maxlen) {
        const uint64_t x = a.get() ^ b.get();
        if (x) { l += __builtin_ctzll(x) >> 3; break; }
        a.next();
        b.next();
        l += 8;
    }
    return l < maxlen ? l : maxlen;
}

__device__ inline int match_len_8(const uint64_t *in64, int p, int maxlen) {   // q = p - 8: the word before is the one just read
    ByteStream a(in64, p);
    uint64_t prev = load64(in64, p - 8);
    int l = 0;
    while (l < maxlen) {
        const uint64_t cur = a.get(), x = cur ^ prev;
        if (x) { l += __builtin_ctzll(x) >> 3; break; }
        prev = cur;
        a.next();
        l += 8;
    }
    return l < maxlen ? l : maxlen;
}

__device__ inline int match_len_1(const uint64_t *in64, int p, int maxlen) {   // q = p - 1: the word shifted by one byte
    ByteStream a(in64, p);
    uint64_t before = load64(in64, p - 1) & 0xFF;
    int l = 0;
    while (l < maxlen) {
        const uint64_t cur = a.get(), x = cur ^ ((cur << 8) | before);
        if (x) { l += __builtin_ctzll(x) >> 3; break; }
        before = cur >> 56;
        a.next();
        l += 8;
    }
    return l < maxlen ? l : maxlen;
}

__device__ inline void put_bits(uint32_t *stage, uint32_t bitpos, uint64_t value, int nbits) {   // value < 2^nbits, nbits <= 48
    if (nbits <= 0) return;
    const uint32_t w = bitpos >> 5, sh = bitpos & 31;
    const uint64_t lo = value << sh;
    const uint32_t v0 = (uint32_t)lo, v1 = (uint32_t)(lo >> 32), v2 = sh ? (uint32_t)(value >> (64 - sh)) : 0u;
    if (v0 && w < DF_STAGE_WORDS) atomicOr(&stage[w], v0);
    if (v1 && w + 1 < DF_STAGE_WORDS) atomicOr(&stage[w + 1], v1);
    if (v2 && w + 2 < DF_STAGE_WORDS) atomicOr(&stage[w + 2], v2);
}

__device__ inline void df_store(uint8_t *slot, int bound, int at, uint8_t v) {
    if (at >= 0 && at < bound) slot[at] = v;
}

// ---- code lengths -------------------------------------------------------------------------------------------------------------------
// Lane 0: the Moffat-Katajainen lengths of the n ascending frequencies B[0..n), into A[0..n).  Returns the longest.
__device__ int mk_lengths(int *A, const int *B, int n) {
    for (int i = 0; i < n; ++i) A[i] = B[i];
    if (n == 1) { A[0] = 1; return 1; }
    A[0] += A[1];
    int root = 0, leaf = 2;
    for (int next = 1; next < n - 1; ++next) {
        if (leaf >= n || A[root] < A[leaf]) { A[next] = A[root]; A[root++] = next; }
        else A[next] = A[leaf++];
        if (leaf >= n || (root < next && A[root] < A[leaf])) { A[next] += A[root]; A[root++] = next; }
        else A[next] += A[leaf++];
    }
    A[n - 2] = 0;
    for (int next = n - 3; next >= 0; --next) A[next] = A[A[next] & 511 /* an internal node's index < n */] + 1;
    int avbl = 1, used = 0, dpth = 0, next = n - 1;
    root = n - 2;
    for (int guard = 0; avbl > 0 && guard <= n; ++guard) {          // one round per depth: at most n - 1 depths
        while (root >= 0 && A[root] == dpth) { ++used; --root; }
        while (avbl > used && next >= 0) { A[next--] = dpth; --avbl; }
        avbl = 2 * used;
        ++dpth;
        used = 0;
    }
    return A[0];
}

// All lanes: the code lengths (<= limit) of the alphabet freq[0..nsym) into lens; *ok = 0 when the limit could not be met.
// A, B, ord: DF_ASZ ints each; cnt: one int.
__device__ void build_lengths(const uint32_t *freq, int nsym, int limit, uint8_t *lens, int *A, int *B, int *ord, int *cnt, int *ok, int t) {
    if (t == 0) *cnt = 0;
    __syncthreads();
    for (int s = t; s < nsym; s += DF_NT) {
        const uint32_t f = freq[s];
        lens[s] = 0;
        if (f) {
            int rank = 0;
            for (int u = 0; u < nsym; ++u) {
                const uint32_t g = freq[u];
                rank += (g && (g < f || (g == f && u < s))) ? 1 : 0;
            }
            if (rank < DF_ASZ) { B[rank] = (int)f; ord[rank] = s; }
            atomicAdd(cnt, 1);
        }
    }
    __syncthreads();
    if (t == 0) {
        const int n = *cnt < DF_ASZ ? *cnt : DF_ASZ;
        bool good = n == 0;
        for (int round = 0; round < 16 && n > 0; ++round) {
            if (mk_lengths(A, B, n) <= limit) { good = true; break; }
            for (int i = 0; i < n; ++i) B[i] = (B[i] + 1) >> 1;     // monotone: the order stays ascending
        }
        if (good) for (int i = 0; i < n; ++i) lens[ord[i] % nsym] = (uint8_t)A[i];
        else *ok = 0;
    }
    __syncthreads();
}

// All lanes: canonical codes by (length, symbol), bit-reversed for the LSB-first stream.  count: 16 ints.
__device__ void canonical_codes(const uint8_t *lens, int nsym, uint16_t *codes, int *count, int t) {
    if (t < 16) count[t] = 0;
    __syncthreads();
    for (int s = t; s < nsym; s += DF_NT)
        if (lens[s]) atomicAdd(&count[lens[s] & 15], 1);
    __syncthreads();
    for (int s = t; s < nsym; s += DF_NT) {
        const int l = lens[s] & 15;
        int code = 0, rank = 0;
        for (int b = 1; b <= l; ++b) code = (code + (b > 1 ? count[b - 1] : 0)) << 1;   // the first code of length l
        for (int u = 0; u < s; ++u) rank += lens[u] == l ? 1 : 0;
        codes[s] = l ? (uint16_t)bit_reverse((uint32_t)(code + rank), l) : 0;
    }
    __syncthreads();
}

// ---- the piece kernel -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DF_NT) void deflate_piece_kernel(DeflateArgs a) {
    __shared__ uint64_t s_in64[DF_MAX_PIECE / 8 + 2];
    __shared__ uint16_t s_dist[DF_MAX_PIECE];       // 0: literal; DF_SKIP: inside a match; else the match's distance
    __shared__ uint8_t s_len[DF_MAX_PIECE];         // the match's length - 3
    __shared__ uint32_t s_scratch[DF_HASH_SIZE];    // the hash table; afterwards the staging area and the sort arrays
    __shared__ uint32_t s_freqL[DF_ASZ], s_freqD[32], s_freqC[32];
    __shared__ uint8_t s_lenL[DF_ASZ], s_lenD[32], s_lenC[32], s_seq[DF_NSEQ + 4];
    __shared__ uint16_t s_codeL[DF_ASZ], s_codeD[32], s_codeC[32];
    __shared__ uint16_t s_cls[DF_NSEQ + 4];         // the run-length coded sequence: symbol | extra value << 8
    __shared__ uint16_t s_nxt[2][DF_NT];
    __shared__ uint8_t s_mark[DF_NT];
    __shared__ int s_wsum[DF_NT / 64], s_count[16];
    __shared__ int s_entry, s_cnt, s_ok, s_ncls, s_nlit, s_ndist, s_ncl, s_use_dyn;
    __shared__ uint32_t s_bits, s_crc, s_cost;

    const int t = threadIdx.x;
    const int64_t piece = blockIdx.x;
    const int64_t off = piece * a.piece_bytes;
    if (piece >= a.n_pieces || off >= a.n) return;
    const int n = (int)((a.n - off) < (int64_t)a.piece_bytes ? (a.n - off) : (int64_t)a.piece_bytes);   // 1 .. DF_MAX_PIECE
    const uint8_t *src = a.src + off;
    uint8_t *slot = a.dst + piece * a.dst_stride;
    const int bound = a.bound;
    uint8_t *s_in = reinterpret_cast<uint8_t *>(s_in64);
    int *s_hash = reinterpret_cast<int *>(s_scratch);

    // ---- load
    for (int i = t; i < DF_MAX_PIECE / 8 + 2; i += DF_NT) s_in64[i] = 0;
    for (int i = t; i < DF_HASH_SIZE; i += DF_NT) s_hash[i] = -1;
    for (int i = t; i < DF_ASZ; i += DF_NT) s_freqL[i] = 0;
    if (t < 32) { s_freqD[t] = 0; s_freqC[t] = 0; s_lenD[t] = 0; s_lenC[t] = 0; }
    if (t == 0) { s_entry = 0; s_ok = 1; s_crc = 0; s_bits = 0; }
    __syncthreads();
    if ((reinterpret_cast<uintptr_t>(src) & 3) == 0) {
        const uint32_t *src32 = reinterpret_cast<const uint32_t *>(src);
        uint32_t *in32 = reinterpret_cast<uint32_t *>(s_in64);
        const int n4 = n >> 2;
        for (int i = t; i < n4; i += DF_NT) in32[i] = src32[i];
        for (int i = (n4 << 2) + t; i < n; i += DF_NT) s_in[i] = src[i];
    } else {
        for (int i = t; i < n; i += DF_NT) s_in[i] = src[i];
    }
    __syncthreads();
    {   // CRC-32 of the piece
        const int b0 = t * DF_SUB, b1 = b0 + DF_SUB < n ? b0 + DF_SUB : n;
        if (b0 < n) {
            uint32_t c = 0xFFFFFFFFu;
            for (int w = 0; w < DF_SUB / 8; ++w) {
                const uint64_t v = s_in64[(b0 >> 3) + w];
                for (int k = 0; k < 8; ++k) {
                    if (b0 + w * 8 + k < b1) {
                        c ^= (uint32_t)(v >> (8 * k)) & 0xFFu;
                        for (int j = 0; j < 8; ++j) c = (c >> 1) ^ (DF_POLY & (0u - (c & 1u)));
                    }
                }
            }
            c ^= 0xFFFFFFFFu;
            atomicXor(&s_crc, crc_mul(crc_xpow8((uint32_t)(n - b1)), c));
        }
    }

    // ---- match and parse
    const int n_chunks = (n + DF_NT - 1) / DF_NT;                   // <= 64
    for (int c = 0; c < n_chunks; ++c) {
        const int p = c * DF_NT + t;
        const bool valid = p < n;
        const int maxlen = valid ? (n - p < 258 ? n - p : 258) : 0;
        const bool hashed = valid && p + 4 <= n;
        int cand = -1;
        uint32_t h = 0;
        if (hashed) {
            h = (((uint32_t)load64(s_in64, p)) * 2654435761u) >> (32 - DF_HASH_BITS);   // < DF_HASH_SIZE
            cand = s_hash[h];
        }
        __syncthreads();                                            // every read of the table precedes this chunk's updates
        if (hashed) atomicMax(&s_hash[h], p);
        int best_len = 0, best_dist = 0;
        if (maxlen >= 3) {
            if (p >= 8) {
                const int l = match_len_8(s_in64, p, maxlen);
                if (l >= 3) { best_len = l; best_dist = 8; }
            }
            if (best_len < maxlen && p >= 1) {
                const int l = match_len_1(s_in64, p, maxlen);
                if (l >= 3 && l > best_len) { best_len = l; best_dist = 1; }
            }
            if (best_len < maxlen && cand >= 0 && cand < p) {
                const int l = match_len(s_in64, p, cand, maxlen);
                if (l >= 4 && l > best_len) { best_len = l; best_dist = p - cand; }
            }
        }
        const int adv = best_dist ? best_len : 1;
        if (valid) {
            s_dist[p] = (uint16_t)best_dist;
            s_len[p] = (uint8_t)(best_dist ? best_len - 3 : 0);
        }
        const int entry = s_entry;                                  // written by the chunk before, ahead of its last barrier
        s_nxt[0][t] = (uint16_t)((valid && t + adv < DF_NT) ? t + adv : DF_NT);
        s_mark[t] = (valid && p == entry) ? 1 : 0;
        __syncthreads();
        int b = 0;
        for (int r = 0; r < 8; ++r) {                               // marks reach 2^(r + 1) - 1 tokens behind the entry
            const int m = s_mark[t], j = s_nxt[b][t];
            __syncthreads();
            if (m && j < DF_NT) s_mark[j] = 1;
            const uint16_t jj = j < DF_NT ? s_nxt[b][j] : (uint16_t)DF_NT;
            s_nxt[b ^ 1][t] = jj;
            b ^= 1;
            if (!__syncthreads_or(jj < DF_NT)) break;               // every pointer has left the chunk: nothing more to mark
        }
        if (valid) {
            if (s_mark[t]) {
                if (best_dist) {
                    int code, eb, ev;
                    len_symbol(best_len, code, eb, ev);
                    atomicAdd(&s_freqL[257 + code], 1u);
                    dist_symbol(best_dist, code, eb, ev);
                    atomicAdd(&s_freqD[code & 31], 1u);
                } else {
                    atomicAdd(&s_freqL[s_in[p]], 1u);
                }
                if (t + adv >= DF_NT || p + adv >= n) s_entry = p + adv;   // the chunk's last token: one lane
            } else {
                s_dist[p] = DF_SKIP;
            }
        }
        __syncthreads();
    }
    if (t == 0) s_freqL[256] = 1;                                   // end of block
    __syncthreads();

    // ---- codes (the hash table is dead: its memory holds the staging area and the sort arrays)
    uint32_t *s_stage = s_scratch;                                  // [0, 512)
    int *s_A = reinterpret_cast<int *>(s_scratch + DF_STAGE_WORDS);
    int *s_B = s_A + DF_ASZ, *s_ord = s_B + DF_ASZ;                 // 512 + 3 * 288 = 1376 <= DF_HASH_SIZE words
    static_assert(DF_STAGE_WORDS + 3 * DF_ASZ <= DF_HASH_SIZE, "the sort arrays must fit the hash table's memory");
    build_lengths(s_freqL, DF_NLIT, 15, s_lenL, s_A, s_B, s_ord, &s_cnt, &s_ok, t);
    build_lengths(s_freqD, DF_NDIST, 15, s_lenD, s_A, s_B, s_ord, &s_cnt, &s_ok, t);
    if (t == 0) {
        int nlit = DF_NLIT, ndist = DF_NDIST;
        while (nlit > 257 && s_lenL[nlit - 1] == 0) --nlit;
        while (ndist > 1 && s_lenD[ndist - 1] == 0) --ndist;
        if (ndist == 1 && s_lenD[0] == 0) s_lenD[0] = 1;            // a block with no match still needs one distance code length
        s_nlit = nlit;
        s_ndist = ndist;
        s_cost = 0;
    }
    __syncthreads();
    for (int i = t; i < s_nlit + s_ndist; i += DF_NT) s_seq[i] = i < s_nlit ? s_lenL[i] : s_lenD[(i - s_nlit) & 31];
    __syncthreads();
    if (t == 0) {
        const int total = s_nlit + s_ndist;
        int m = 0;
        auto emit = [&](int sym, int extra) {
            if (m < DF_NSEQ) { s_cls[m++] = (uint16_t)(sym | (extra << 8)); s_freqC[sym & 31]++; }
        };
        for (int i = 0; i < total;) {                               // runs: symbols 16, 17, 18
            const int v = s_seq[i];
            int run = 1;
            while (i + run < total && s_seq[i + run] == v) ++run;
            int r = run;
            if (v == 0) {
                while (r >= 11) { const int k = r < 138 ? r : 138; emit(18, k - 11); r -= k; }
                if (r >= 3) { emit(17, r - 3); r = 0; }
                while (r > 0) { emit(0, 0); --r; }
            } else {
                emit(v, 0);
                --r;
                while (r >= 3) { const int k = r < 6 ? r : 6; emit(16, k - 3); r -= k; }
                while (r > 0) { emit(v, 0); --r; }
            }
            i += run;
        }
        s_ncls = m;
        int used = 0, only = 0;
        for (int s = 0; s < DF_NCL; ++s) if (s_freqC[s]) { ++used; only = s; }
        if (used < 2) s_freqC[only == 0 ? 1 : 0] = 1;               // the code-length code must be complete: two symbols at least
    }
    __syncthreads();
    build_lengths(s_freqC, DF_NCL, 7, s_lenC, s_A, s_B, s_ord, &s_cnt, &s_ok, t);
    canonical_codes(s_lenL, DF_NLIT, s_codeL, s_count, t);
    canonical_codes(s_lenD, DF_NDIST, s_codeD, s_count, t);
    canonical_codes(s_lenC, DF_NCL, s_codeC, s_count, t);
    {   // ---- cost: the exact bits of the dynamic block (integer sums)
        uint32_t bits = 0;
        for (int i = t; i < s_ncls; i += DF_NT) {
            const int sym = s_cls[i] & 31;
            bits += s_lenC[sym] + (sym == 16 ? 2 : sym == 17 ? 3 : sym == 18 ? 7 : 0);
        }
        for (int s = t; s < DF_NLIT; s += DF_NT) bits += s_freqL[s] * (s_lenL[s] + (s > 256 ? len_extra_bits(s - 257) : 0));
        if (t < DF_NDIST) bits += s_freqD[t] * (s_lenD[t] + dist_extra_bits(t));
        if (bits) atomicAdd(&s_cost, bits);
    }
    __syncthreads();
    if (t == 0) {
        int ncl = DF_NCL;
        while (ncl > 4 && s_lenC[c_cl_order[ncl - 1]] == 0) --ncl;
        s_ncl = ncl;
        const uint32_t bits = s_cost + 3 + 5 + 5 + 4 + 3 * (uint32_t)ncl;
        const uint32_t dyn_bytes = ((bits + 3 + 7) >> 3) + 4;       // + the empty stored block of the sync flush
        s_use_dyn = (s_ok && dyn_bytes < (uint32_t)n + 5u) ? 1 : 0;
    }
    for (int i = t; i < DF_STAGE_WORDS; i += DF_NT) s_stage[i] = 0;
    __syncthreads();

    if (!s_use_dyn) {                                               // ---- stored: n <= 16 384, one block
        if (t == 0) {
            df_store(slot, bound, 0, 0);
            df_store(slot, bound, 1, (uint8_t)(n & 0xFF));
            df_store(slot, bound, 2, (uint8_t)(n >> 8));
            df_store(slot, bound, 3, (uint8_t)(~n & 0xFF));
            df_store(slot, bound, 4, (uint8_t)((~n >> 8) & 0xFF));
            a.piece_len[piece] = n + 5;
            a.piece_crc[piece] = s_crc;
        }
        for (int i = t; i < n; i += DF_NT) df_store(slot, bound, 5 + i, s_in[i]);
        return;
    }

    // ---- emit
    int out_pos = 0;                                                // the same in every lane
    const uint8_t *stage_bytes = reinterpret_cast<const uint8_t *>(s_stage);
    auto flush = [&](bool final) {                                  // all lanes; the staged bits are complete and visible
        const uint32_t nbits = s_bits;
        const int nbytes = (int)(final ? (nbits + 7) >> 3 : nbits >> 3);
        const uint32_t carry = (!final && (nbits & 7)) ? stage_bytes[nbytes & (DF_STAGE_WORDS * 4 - 1)] : 0u;
        for (int i = t; i < nbytes && i < DF_STAGE_WORDS * 4; i += DF_NT) df_store(slot, bound, out_pos + i, stage_bytes[i]);
        __syncthreads();
        for (int i = t; i < DF_STAGE_WORDS; i += DF_NT) s_stage[i] = 0;
        __syncthreads();
        if (t == 0) { s_stage[0] = carry; s_bits = final ? 0 : (nbits & 7); }
        out_pos += nbytes;
        __syncthreads();
    };

    if (t == 0) {                                                   // the block header
        uint32_t bp = 0;
        auto put = [&](uint32_t v, int nb) { put_bits(s_stage, bp, v, nb); bp += nb; };
        put(0, 1);                                                  // BFINAL
        put(2, 2);                                                  // BTYPE 10
        put((uint32_t)(s_nlit - 257), 5);
        put((uint32_t)(s_ndist - 1), 5);
        put((uint32_t)(s_ncl - 4), 4);
        for (int i = 0; i < s_ncl; ++i) put(s_lenC[c_cl_order[i]], 3);
        for (int i = 0; i < s_ncls; ++i) {
            const int sym = s_cls[i] & 31, extra = s_cls[i] >> 8;
            put(s_codeC[sym], s_lenC[sym]);
            if (sym == 16) put((uint32_t)extra, 2);
            else if (sym == 17) put((uint32_t)extra, 3);
            else if (sym == 18) put((uint32_t)extra, 7);
        }
        s_bits = bp;
    }
    __syncthreads();
    flush(false);

    for (int c = 0; c < n_chunks; ++c) {
        const int p = c * DF_NT + t;
        uint64_t val = 0;
        int nb = 0;
        if (p < n) {
            const uint16_t d = s_dist[p];
            if (d == 0) {
                const int s = s_in[p];
                val = s_codeL[s];
                nb = s_lenL[s];
            } else if (d != DF_SKIP) {
                int code, eb, ev;
                len_symbol((int)s_len[p] + 3, code, eb, ev);
                val = s_codeL[257 + code];
                nb = s_lenL[257 + code];
                val |= (uint64_t)ev << nb;
                nb += eb;
                dist_symbol((int)d, code, eb, ev);
                val |= (uint64_t)s_codeD[code & 31] << nb;
                nb += s_lenD[code & 31];
                val |= (uint64_t)ev << nb;
                nb += eb;
            }
        }
        int incl = nb;                                              // exclusive prefix sum of nb over the workgroup
        for (int dlt = 1; dlt < 64; dlt <<= 1) {
            const int v = __shfl_up(incl, dlt, 64);
            if ((t & 63) >= dlt) incl += v;
        }
        if ((t & 63) == 63) s_wsum[t >> 6] = incl;
        __syncthreads();
        int base = 0, total = 0;
        for (int w = 0; w < DF_NT / 64; ++w) {
            if (w < (t >> 6)) base += s_wsum[w];
            total += s_wsum[w];
        }
        put_bits(s_stage, s_bits + (uint32_t)(base + incl - nb), val, nb);
        __syncthreads();
        if (t == 0) s_bits += (uint32_t)total;
        __syncthreads();
        if (s_bits >= DF_STAGE_WORDS * 32 - DF_NT * 48 - 64) flush(false);   // the next chunk's <= 256 * 48 bits must fit behind these
    }

    if (t == 0) {
        uint32_t bp = s_bits;
        put_bits(s_stage, bp, s_codeL[256], s_lenL[256]);           // end of block
        bp += s_lenL[256];
        bp = (bp + 3 + 7) & ~7u;                                    // 000: an empty stored block; pad to the byte
        put_bits(s_stage, bp, 0xFFFF0000u, 32);                     // LEN 0000, NLEN FFFF
        s_bits = bp + 32;
    }
    __syncthreads();
    flush(true);
    if (t == 0) {
        a.piece_len[piece] = out_pos;
        a.piece_crc[piece] = s_crc;
    }
}

// ---- pack ---------------------------------------------------------------------------------------------------------------------------------
constexpr int PK_NT = 1024;

// one workgroup: offsets[i] = sum of the lengths before piece i (a length outside [0, dst_stride] counts as clamped)
__global__ __launch_bounds__(PK_NT) void deflate_offsets_kernel(const int32_t *piece_len, int64_t n_pieces, int64_t dst_stride, int64_t *offsets) {
    __shared__ int64_t s_w[PK_NT / 64];
    __shared__ int64_t s_carry;
    const int t = threadIdx.x;
    if (t == 0) s_carry = 0;
    __syncthreads();
    for (int64_t i0 = 0; i0 < n_pieces; i0 += PK_NT) {
        const int64_t i = i0 + t;
        int64_t len = 0;
        if (i < n_pieces) {
            len = piece_len[i];
            len = len < 0 ? 0 : (len > dst_stride ? dst_stride : len);
        }
        int64_t incl = len;
        for (int dlt = 1; dlt < 64; dlt <<= 1) {
            const int64_t v = __shfl_up(incl, dlt, 64);
            if ((t & 63) >= dlt) incl += v;
        }
        if ((t & 63) == 63) s_w[t >> 6] = incl;
        __syncthreads();
        int64_t base = s_carry, total = 0;
        for (int w = 0; w < PK_NT / 64; ++w) {
            if (w < (t >> 6)) base += s_w[w];
            total += s_w[w];
        }
        if (i < n_pieces) offsets[i] = base + incl - len;
        __syncthreads();
        if (t == 0) s_carry += total;
        __syncthreads();
    }
    if (t == 0) offsets[n_pieces] = s_carry;
}

__global__ __launch_bounds__(DF_NT) void deflate_copy_kernel(const uint8_t *dst, int64_t dst_stride, const int64_t *offsets, int64_t n_pieces,
                                                             uint8_t *out, int64_t out_cap) {
    for (int64_t i = blockIdx.x; i < n_pieces; i += gridDim.x) {
        const int64_t o0 = offsets[i], len = offsets[i + 1] - o0;   // 0 <= len <= dst_stride
        const uint8_t *from = dst + i * dst_stride;
        for (int64_t j = threadIdx.x; j < len; j += DF_NT)
            if (o0 + j < out_cap) out[o0 + j] = from[j];
    }
}

}  // namespace

int launch_deflate_pieces(const DeflateArgs &a, hipStream_t s) {
    if (a.n_pieces <= 0) return ICNV_OK;
    KernelTimer kt("deflate_pieces", s);
    hipLaunchKernelGGL(deflate_piece_kernel, dim3((unsigned)a.n_pieces), dim3(DF_NT), 0, s, a);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_deflate_offsets(const int32_t *piece_len, int64_t n_pieces, int64_t dst_stride, int64_t *offsets, hipStream_t s) {
    hipLaunchKernelGGL(deflate_offsets_kernel, dim3(1), dim3(PK_NT), 0, s, piece_len, n_pieces, dst_stride, offsets);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_deflate_copy(const uint8_t *dst, int64_t dst_stride, const int64_t *offsets, int64_t n_pieces, uint8_t *out, int64_t out_cap,
                        hipStream_t s) {
    if (n_pieces <= 0) return ICNV_OK;
    KernelTimer kt("deflate_pack", s);
    const int64_t cap = (int64_t)num_cus() * 8;
    hipLaunchKernelGGL(deflate_copy_kernel, dim3((unsigned)(n_pieces < cap ? n_pieces : cap)), dim3(DF_NT), 0, s, dst, dst_stride, offsets,
                       n_pieces, out, out_cap);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
