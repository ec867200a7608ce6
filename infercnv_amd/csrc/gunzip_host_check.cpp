// The finder's per-offset test, the measure and the marker decoder of K30 (gunzip_internal.h) on the host, built with
// -fsanitize=address,undefined by `make gunzip_host_check` and run over a corpus of raw DEFLATE streams
// (scripts/make_gunzip_corpus.py writes the valid and the malformed streams of the K30 tests).  Every stream lives in a heap block
// of exactly its size and every unit's symbols in one of exactly its out_len, so a load or store outside them stops the program.
// Per stream:
//   * gz_header_ok at EVERY bit offset, against if_dynamic_tables behind the three header bits (the rule it restates);
//   * a valid stream that is one unit for K29 from byte 0: the same unit for K30 from bit 0 under an empty candidate list;
//   * the measure from bit 0 and from every candidate, the chain walk, the symbols of the chain's units, tails and resolve by
//     gz_resolve_one: a valid stream must give exactly its inflated bytes;
//   * the symbols call with out_len and end wrong by one, short budgets, starts at the bits around every candidate;
//   * seeded copies with one to three bits flipped: the finder, every measure, and where a measure says OK the symbols.
// Not part of libicnv_hip.so and never loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "gunzip_internal.h"

using namespace icnv;

namespace {

struct Record {
    uint32_t valid;
    std::string name;
    std::vector<uint8_t> comp, raw;
};

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}

template <class T>
struct Heap {                           // exactly n elements (one when n == 0: never dereferenced then)
    T *p;
    explicit Heap(size_t n) : p((T *)malloc((n ? n : 1) * sizeof(T))) {}
    Heap(const T *from, size_t n) : Heap(n) { if (n) memcpy(p, from, n * sizeof(T)); }
    ~Heap() { free(p); }
};

long g_offsets = 0, g_measures = 0, g_decodes = 0, g_failures = 0;
const int64_t MAX_IN = 16 << 20;

void fail(const Record &r, const char *what, long a = 0, long b = 0) {
    ++g_failures;
    fprintf(stderr, "FAIL %s: %s (%ld, %ld)\n", r.name.c_str(), what, a, b);
}

bool header_by_k29(const uint8_t *src, int64_t n, int64_t bit) {    // the rule gz_header_ok restates
    IfState s;
    if_init<GzSymbols>(s, src, n, bit, n);
    if (!s.r.need(3) || s.r.take(3) != 4u) return false;
    IfTables t;
    return if_dynamic_tables(s, t) == 0;
}

// Both policies go through one walker: a stream that is ONE unit for K29 from byte 0 (no flush marker in front of BFINAL) is the
// same unit for K30 from bit 0 with no candidate listed -- as many symbols as bytes, the end counted in bits, and every symbol
// K29's byte (so none a marker).  Not counted among the measures and decodes of the summary line.
void one_unit_under_both_policies(const Record &r, const uint8_t *src, int64_t n) {
    IfTables t;
    int64_t end29 = 0, len29 = 0, end30 = 0, len30 = 0, e = 0, l = 0;
    if (if_unit_serial(IfBytes(), src, n, 0, n, t, nullptr, 0, &end29, &len29) != ICNV_INFLATE_OK_FINAL) return;
    Heap<uint8_t> bytes((size_t)len29);
    Heap<uint16_t> sym((size_t)len29);
    if (if_unit_serial(IfBytes(), src, n, 0, end29, t, bytes.p, len29, &e, &l) != ICNV_INFLATE_OK_FINAL || e != end29 || l != len29)
        return fail(r, "K29's decode of its own measure");
    if (if_unit_serial(GzSymbols{nullptr, 0, 0}, src, n, 0, n, t, sym.p, len29, &end30, &len30) != ICNV_GUNZIP_OK_FINAL)
        return fail(r, "one unit for K29 is not one for K30");
    if (len30 != len29) return fail(r, "the two policies' out_len", (long)len29, (long)len30);
    if (end30 != 8 * end29) fail(r, "K30's end is not 8 x K29's", (long)end29, (long)end30);
    for (int64_t j = 0; j < len29; ++j)
        if (sym.p[j] >= 256 || sym.p[j] != bytes.p[j]) return fail(r, "a symbol is not K29's byte", (long)j, sym.p[j]);
}

std::vector<int64_t> find(const Record &r, const uint8_t *src, int64_t n, bool compare) {
    std::vector<int64_t> cand;
    for (int64_t b = 0; b < n * 8; ++b) {
        ++g_offsets;
        const bool ok = gz_header_ok(src, n, b);
        if (compare && ok != header_by_k29(src, n, b)) fail(r, "gz_header_ok disagrees with if_dynamic_tables", (long)b);
        if (ok) cand.push_back(b);
    }
    return cand;
}

int measure(const uint8_t *src, int64_t n, int64_t start, int64_t max_in, const std::vector<int64_t> &cand, int64_t *end, int64_t *out_len) {
    IfTables t;
    ++g_measures;
    return if_unit_serial(GzSymbols{cand.data(), (int64_t)cand.size(), 0}, src, n, start, max_in, t, nullptr, 0, end, out_len);
}

// the symbols as the device calls them: budget up to the end's byte, symbols of exactly out_len
int symbols(const uint8_t *src, int64_t n, int64_t start, int64_t end, int64_t out_len, const std::vector<int64_t> &cand, std::vector<uint16_t> *got) {
    if (end < start || end > n * 8 || out_len < 0) return ICNV_GUNZIP_BAD_STREAM;
    IfTables t;
    Heap<uint16_t> sym((size_t)out_len);
    int64_t got_end = 0, got_len = 0;
    ++g_decodes;
    int st = if_unit_serial(GzSymbols{cand.data(), (int64_t)cand.size(), 0}, src, n, start, ((end + 7) >> 3) - (start >> 3), t, sym.p, out_len, &got_end, &got_len);
    if (st <= ICNV_GUNZIP_OK_FINAL && (got_end != end || got_len != out_len)) st = ICNV_GUNZIP_BAD_STREAM;
    if (st == ICNV_GUNZIP_TOO_LONG) st = ICNV_GUNZIP_BAD_STREAM;
    if (got) got->assign(sym.p, sym.p + (st <= ICNV_GUNZIP_OK_FINAL ? out_len : 0));
    return st;
}

void measure_then_symbols(const uint8_t *src, int64_t n, int64_t start, int64_t max_in, const std::vector<int64_t> &cand) {
    int64_t end, out_len;
    const int st = measure(src, n, start, max_in, cand, &end, &out_len);
    if (st <= ICNV_GUNZIP_OK_FINAL && out_len <= (16 << 20)) symbols(src, n, start, end, out_len, cand, nullptr);
}

void run(const Record &r, int flips) {
    const int64_t n = (int64_t)r.comp.size();
    Heap<uint8_t> src(r.comp.data(), r.comp.size());
    const std::vector<int64_t> cand = find(r, src.p, n, true);
    std::vector<int64_t> start(1, 0);
    for (int64_t c : cand) if (c > 0) start.push_back(c);
    std::vector<int64_t> end(start.size()), len(start.size());
    std::vector<int> status(start.size());
    for (size_t i = 0; i < start.size(); ++i) status[i] = measure(src.p, n, start[i], MAX_IN, cand, &end[i], &len[i]);
    if (r.valid) {
        // the chain, the symbols, tails then the rest: the output must be the stream's own bytes
        std::vector<uint8_t> out;
        std::vector<size_t> chain;
        size_t i = 0;
        bool ok = true;
        for (;;) {
            chain.push_back(i);
            if (status[i] == ICNV_GUNZIP_OK_FINAL) break;
            if (status[i] != ICNV_GUNZIP_OK_BOUNDARY) { fail(r, "a chain unit's status", (long)start[i], status[i]); ok = false; break; }
            size_t j = i + 1;
            while (j < start.size() && start[j] != end[i]) ++j;
            if (j == start.size()) { fail(r, "a chain unit does not end on a candidate", (long)start[i]); ok = false; break; }
            i = j;
        }
        for (size_t c = 0; ok && c < chain.size(); ++c) {
            const size_t u = chain[c];
            std::vector<uint16_t> sym;
            if (symbols(src.p, n, start[u], end[u], len[u], cand, &sym) != status[u]) { fail(r, "symbols status", (long)start[u]); ok = false; break; }
            const int64_t off = (int64_t)out.size(), tail = len[u] < GZ_W ? len[u] : GZ_W;
            out.resize((size_t)(off + len[u]));
            for (int pass = 0; pass < 2; ++pass)                    // the tail first, then what lies in front of it
                for (int64_t j = pass ? 0 : len[u] - tail; j < (pass ? len[u] - tail : len[u]); ++j)
                    if (!gz_resolve_one(sym[(size_t)j], out.data(), (int64_t)out.size(), off, out[(size_t)(off + j)])) { fail(r, "a marker in front of byte 0", (long)j); ok = false; }
            for (int d = -1; d <= 1; d += 2) {
                if (symbols(src.p, n, start[u], end[u] + d * 8, len[u], cand, nullptr) <= ICNV_GUNZIP_OK_FINAL) fail(r, "a wrong end was accepted", d);
                if (symbols(src.p, n, start[u], end[u], len[u] + d, cand, nullptr) <= ICNV_GUNZIP_OK_FINAL) fail(r, "a wrong out_len was accepted", d);
            }
        }
        if (ok && out != r.raw) fail(r, "the inflated bytes", (long)out.size(), (long)r.raw.size());
        if (ok && end[chain.back()] != n * 8) fail(r, "the chain does not end with the stream", (long)end[chain.back()]);
        one_unit_under_both_policies(r, src.p, n);
    }
    for (size_t i = 0; i < start.size(); ++i) {
        if (status[i] <= ICNV_GUNZIP_OK_FINAL && len[i] <= (16 << 20)) symbols(src.p, n, start[i], end[i], len[i], cand, nullptr);
        for (int64_t d = -8; d <= 8; ++d)
            if (start[i] + d >= 0 && ((start[i] + d) >> 3) < n) measure_then_symbols(src.p, n, start[i] + d, n, cand);
    }
    for (int64_t m = 0; m <= n && m <= 48; ++m) measure_then_symbols(src.p, n, 0, m, cand);
    const int64_t step = n > 400 ? n / 100 : 1;
    for (int64_t cut = 0; cut < n; cut += step) {
        Heap<uint8_t> part(r.comp.data(), (size_t)cut);
        const std::vector<int64_t> none;
        int64_t e, l;
        const int s2 = measure(part.p, cut, 0, MAX_IN, none, &e, &l);
        if (r.valid && s2 != ICNV_GUNZIP_TRUNCATED) fail(r, "a cut stream is not TRUNCATED", (long)cut, s2);
        if (cut > n - 64 || cut < 64)
            for (int64_t b = cut * 8 - 400 > 0 ? cut * 8 - 400 : 0; b < cut * 8; ++b) gz_header_ok(part.p, cut, b);
    }
    for (int f = 0; f < flips && n > 0; ++f) {
        Heap<uint8_t> bad(r.comp.data(), r.comp.size());
        for (int k = 1 + (int)(rnd() % 3); k > 0; --k) bad.p[rnd() % n] ^= (uint8_t)(1u << (rnd() % 8));
        std::vector<int64_t> c2 = n <= 8192 ? find(r, bad.p, n, true) : cand;      // (a long stream: the flipped copy under the true list)
        measure_then_symbols(bad.p, n, 0, n, c2);
        for (int64_t c : c2) measure_then_symbols(bad.p, n, c, n, c2);
        measure_then_symbols(bad.p, n, rnd() % (n * 8), 1 + rnd() % n, c2);
    }
}

bool read_exact(FILE *f, void *p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) {
        fprintf(stderr, "usage: %s corpus [flips per stream]\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<Record> recs;
    for (;;) {
        uint32_t head[2];
        uint64_t clen, rlen;
        if (fread(head, sizeof head, 1, f) != 1) break;
        Record r;
        r.valid = head[0];
        r.name.resize(head[1]);
        if (!read_exact(f, &r.name[0], head[1]) || fread(&clen, 8, 1, f) != 1) return 2;
        r.comp.resize(clen);
        if (!read_exact(f, r.comp.data(), clen) || fread(&rlen, 8, 1, f) != 1) return 2;
        r.raw.resize(rlen);
        if (!read_exact(f, r.raw.data(), rlen)) return 2;
        recs.push_back(std::move(r));
    }
    fclose(f);
    if (recs.empty()) { fprintf(stderr, "the corpus is empty\n"); return 2; }
    const int flips = argc > 2 ? atoi(argv[2]) : 24;
    for (const Record &r : recs) run(r, flips);
    printf("%zu streams, %d flipped copies of each: %ld offsets tested, %ld measures, %ld symbol decodes, %ld failures\n", recs.size(), flips, g_offsets,
           g_measures, g_decodes, g_failures);
    return g_failures ? 1 : 0;
}
