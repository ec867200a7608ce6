// The block parser and symbol decoder of K29 (inflate_internal.h) on the host, built with -fsanitize=address,undefined by
// `make inflate_host_check` and run over a corpus of streams (scripts/make_inflate_corpus.py writes the valid and the malformed
// streams of tests/inflate_restate.py).  Every stream lives in a heap block of exactly its size and every output in one of exactly
// the unit's out_len, so a load or store outside them stops the program.  Per stream:
//   * the measure from byte 0: the expected status, and for a valid unit the expected length;
//   * the decode against the expected bytes, and with end / out_len wrong by one in either direction;
//   * the measure from other starting bytes, with short budgets, and of every (or 200) truncated copies;
//   * seeded copies with one to three bits flipped: the measure, and where it says OK the decode.
// Not part of libicnv_hip.so and never loaded into Python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "inflate_internal.h"

using namespace icnv;

namespace {

struct Record {
    uint32_t valid, status;
    std::string name;
    std::vector<uint8_t> comp, raw;
};

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
    g_rng = g_rng * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_rng >> 33);
}

struct Heap {                           // exactly n bytes (one when n == 0: never dereferenced then)
    uint8_t *p;
    explicit Heap(size_t n) : p((uint8_t *)malloc(n ? n : 1)) {}
    Heap(const uint8_t *from, size_t n) : Heap(n) { if (n) memcpy(p, from, n); }
    ~Heap() { free(p); }
};

long g_measures = 0, g_decodes = 0, g_failures = 0;

int measure(const uint8_t *src, int64_t n, int64_t start, int64_t max_in, int64_t *end, int64_t *out_len) {
    IfTables t;
    ++g_measures;
    return if_unit_serial(IfBytes(), src, n, start, max_in, t, nullptr, INT64_MAX, end, out_len);
}

// the decode as the device calls it: budget end - start, output of exactly out_len bytes
int decode(const uint8_t *src, int64_t n, int64_t start, int64_t end, int64_t out_len, std::vector<uint8_t> *bytes) {
    if (end < start || end > n || out_len < 0) return ICNV_INFLATE_BAD_STREAM;
    IfTables t;
    Heap out((size_t)out_len);
    int64_t got_end = 0, got_len = 0;
    ++g_decodes;
    int st = if_unit_serial(IfBytes(), src, n, start, end - start, t, out.p, out_len, &got_end, &got_len);
    if ((st == ICNV_INFLATE_OK_MARKER || st == ICNV_INFLATE_OK_FINAL) && (got_end != end || got_len != out_len)) st = ICNV_INFLATE_BAD_STREAM;
    if (st == ICNV_INFLATE_TOO_LONG) st = ICNV_INFLATE_BAD_STREAM;
    if (bytes) bytes->assign(out.p, out.p + (st <= ICNV_INFLATE_OK_FINAL ? out_len : 0));
    return st;
}

void fail(const Record &r, const char *what, long a = 0, long b = 0) {
    ++g_failures;
    fprintf(stderr, "FAIL %s: %s (%ld, %ld)\n", r.name.c_str(), what, a, b);
}

void measure_then_decode(const uint8_t *src, int64_t n, int64_t start, int64_t max_in) {
    int64_t end, out_len;
    const int st = measure(src, n, start, max_in, &end, &out_len);
    if (st <= ICNV_INFLATE_OK_FINAL && out_len <= (16 << 20)) decode(src, n, start, end, out_len, nullptr);
}

void run(const Record &r, int flips) {
    const int64_t n = (int64_t)r.comp.size();
    Heap src(r.comp.data(), r.comp.size());
    int64_t end = 0, out_len = 0;
    const int st = measure(src.p, n, 0, n, &end, &out_len);
    if (st != (int)r.status) fail(r, "status", st, r.status);
    if (r.valid) {
        if (out_len != (int64_t)r.raw.size()) fail(r, "out_len", out_len, (long)r.raw.size());
        std::vector<uint8_t> got;
        if (decode(src.p, n, 0, end, out_len, &got) != st) fail(r, "decode status");
        else if (got != r.raw) fail(r, "decoded bytes");
        for (int d = -1; d <= 1; d += 2) {
            if (decode(src.p, n, 0, end + d, out_len, nullptr) <= ICNV_INFLATE_OK_FINAL) fail(r, "a wrong end was accepted", d);
            if (decode(src.p, n, 0, end, out_len + d, nullptr) <= ICNV_INFLATE_OK_FINAL) fail(r, "a wrong out_len was accepted", d);
        }
        int64_t e2, l2;
        if (measure(src.p, n, 0, end - 1, &e2, &l2) != ICNV_INFLATE_TOO_LONG) fail(r, "max_in one byte short is not TOO_LONG");
        if (measure(src.p, n, 0, end, &e2, &l2) != st || e2 != end) fail(r, "max_in of exactly the unit");
    }
    for (int64_t s = 0; s < n; s += (n > 4096 ? 1 + rnd() % 97 : 1)) measure_then_decode(src.p, n, s, n);
    for (int64_t m = 0; m <= n && m <= 48; ++m) measure_then_decode(src.p, n, 0, m);
    const int64_t step = n > 600 ? n / 200 : 1;
    for (int64_t cut = 0; cut < n; cut += step) {
        Heap part(r.comp.data(), (size_t)cut);
        int64_t e, l;
        const int s2 = measure(part.p, cut, 0, cut, &e, &l);
        if (r.valid && cut < end && s2 != ICNV_INFLATE_TRUNCATED) fail(r, "a cut unit is not TRUNCATED", (long)cut, s2);
    }
    for (int f = 0; f < flips && n > 0; ++f) {
        Heap bad(r.comp.data(), r.comp.size());
        for (int k = 1 + (int)(rnd() % 3); k > 0; --k) bad.p[rnd() % n] ^= (uint8_t)(1u << (rnd() % 8));
        measure_then_decode(bad.p, n, 0, n);
        measure_then_decode(bad.p, n, rnd() % n, 1 + rnd() % n);
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
        uint32_t head[3];
        uint64_t clen, rlen;
        if (fread(head, sizeof head, 1, f) != 1) break;
        Record r;
        r.valid = head[0];
        r.status = head[1];
        r.name.resize(head[2]);
        if (!read_exact(f, &r.name[0], head[2]) || fread(&clen, 8, 1, f) != 1) return 2;
        r.comp.resize(clen);
        if (!read_exact(f, r.comp.data(), clen) || fread(&rlen, 8, 1, f) != 1) return 2;
        r.raw.resize(rlen);
        if (!read_exact(f, r.raw.data(), rlen)) return 2;
        recs.push_back(std::move(r));
    }
    fclose(f);
    if (recs.empty()) { fprintf(stderr, "the corpus is empty\n"); return 2; }
    const int flips = argc > 2 ? atoi(argv[2]) : (int)(6000 / recs.size()) + 8;
    for (const Record &r : recs) run(r, flips);
    printf("%zu streams, %d flipped copies of each: %ld measures, %ld decodes, %ld failures\n", recs.size(), flips, g_measures, g_decodes, g_failures);
    return g_failures ? 1 : 0;
}
