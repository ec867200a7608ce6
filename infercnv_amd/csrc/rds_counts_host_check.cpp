// The per-element routines of K34 (rds_counts_internal.h: the unaligned big-endian fetch from aligned words, the int -> double
// rule, the count test on a double's bits) as a host program under AddressSanitizer and UBSan: never part of the library, never
// loaded into Python.  `make rds_counts_check CORPUS=file` runs it over the corpus scripts/make_rds_counts_corpus.py writes:
// records of {kind, residue of the payload's address mod 16, length, the big-endian payload, the expected 64-bit results}.
// Every record is decoded four times: the stream begins (a) at the payload itself, at an address with the record's residue, or
// (b) at a 16-byte-aligned address, the payload at that byte offset in it; and the bytes in front of the stream are (1) 0x00 or
// (2) 0xFF.  The allocation ends with the payload's last byte, so a load behind the stream is an AddressSanitizer report; the
// whole 8-byte granules in front of the stream are poisoned, so a load there is one too; the bytes of a granule the stream
// shares are covered by (1) against (2): the results must not differ.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <sanitizer/asan_interface.h>

#include "rds_counts_internal.h"

using namespace icnv;

namespace {

int g_failures = 0;

void fail(const char *what, long record, long element) {
    if (++g_failures <= 20) std::fprintf(stderr, "rds_counts_host_check: %s (record %ld, element %ld)\n", what, record, element);
}

uint64_t decode(int kind, const uint8_t *stream, int64_t n, int64_t off) {
    if (kind == ICNV_RDS_INT) return rc_int_to_real_bits(rc_fetch_be32(stream, n, off));
    const uint64_t bits = rc_fetch_be64(stream, n, off);
    return kind == ICNV_RDS_REAL ? bits : (uint64_t)rc_count_of_bits(bits);
}

void run_record(long rec, int kind, int residue, int n, const uint8_t *payload, const uint64_t *expect) {
    const int64_t es = kind == ICNV_RDS_INT ? 4 : 8, bytes = n * es;
    for (int mode = 0; mode < 2; ++mode)
        for (int fill = 0; fill < 2; ++fill) {
            uint8_t *base = static_cast<uint8_t *>(std::malloc((size_t)(residue + bytes) + (residue + bytes == 0)));
            if (!base || (reinterpret_cast<uintptr_t>(base) & 15)) { fail("malloc is not 16-byte aligned", rec, -1); std::free(base); return; }
            std::memset(base, fill ? 0xFF : 0x00, (size_t)residue);
            if (bytes) std::memcpy(base + residue, payload, (size_t)bytes);
            const uint8_t *stream = mode == 0 ? base + residue : base;
            const int64_t stream_bytes = mode == 0 ? bytes : residue + bytes, off0 = mode == 0 ? 0 : residue;
            if (mode == 0) __asan_poison_memory_region(base, (size_t)(residue & ~7));
            for (int k = 0; k < n; ++k)
                if (decode(kind, stream, stream_bytes, off0 + k * es) != expect[k]) fail("a decoded element differs from the corpus", rec, k);
            __asan_unpoison_memory_region(base, (size_t)(residue & ~7));
            std::free(base);
        }
}

void entry_rules() {
    const uint64_t one = 0x3FF0000000000000ull, half = 0x3FE0000000000000ull;
    struct { int64_t e, lo; int32_t row, prev; int64_t G; uint64_t x; int want; } t[] = {
        {5, 5, 0, 9, 3, one, 0},                         // the first entry of a column: the previous row is another column's
        {6, 5, 2, 1, 3, one, 0},
        {6, 5, 3, 1, 3, one, ICNV_RDS_ROW_RANGE},
        {6, 5, -1, 1, 3, one, ICNV_RDS_ROW_RANGE},
        {6, 5, 1, 1, 3, one, ICNV_RDS_ROW_ORDER},
        {6, 5, 0, 1, 3, one, ICNV_RDS_ROW_ORDER},
        {6, 5, 2, 1, 3, half, ICNV_RDS_VALUE},
        {6, 5, 3, 1, 3, half, ICNV_RDS_ROW_RANGE},     // the smallest code that applies
    };
    for (size_t k = 0; k < sizeof t / sizeof t[0]; ++k)
        if (rc_entry_code(t[k].e, t[k].lo, t[k].row, t[k].prev, t[k].G, t[k].x) != t[k].want) fail("rc_entry_code", -1, (long)k);
    if (rc_key(7, ICNV_RDS_P_LAST, false) >= rc_key(0, ICNV_RDS_ROW_RANGE, true)) fail("a p violation must come before every entry violation", -1, 0);
    if (rc_key(3, ICNV_RDS_VALUE, true) >= rc_key(4, ICNV_RDS_ROW_RANGE, true)) fail("the smaller entry index must win", -1, 1);
}

}  // namespace

int main(int argc, char **argv) {
    entry_rules();
    if (argc < 2) {
        std::fprintf(stderr, "usage: rds_counts_host_check CORPUS (scripts/make_rds_counts_corpus.py writes it)\n");
        return 2;
    }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    char magic[4];
    if (std::fread(magic, 1, 4, f) != 4 || std::memcmp(magic, "RCC1", 4)) { std::fprintf(stderr, "not a corpus\n"); return 2; }
    long records = 0, elements = 0;
    for (;;) {
        uint8_t head[4];
        if (std::fread(head, 1, 4, f) != 4) break;
        const int kind = head[0], residue = head[1], n = head[2] | (head[3] << 8);
        if ((kind != ICNV_RDS_INT && kind != ICNV_RDS_REAL && kind != 1) || residue > 15) { std::fprintf(stderr, "bad record %ld\n", records); return 2; }
        const size_t es = kind == ICNV_RDS_INT ? 4 : 8;
        std::vector<uint8_t> payload(n * es + 1);
        std::vector<uint64_t> expect((size_t)n + 1);
        if (std::fread(payload.data(), 1, n * es, f) != n * es || std::fread(expect.data(), 8, (size_t)n, f) != (size_t)n) {
            std::fprintf(stderr, "truncated corpus\n");
            return 2;
        }
        run_record(records, kind, residue, n, payload.data(), expect.data());
        ++records;
        elements += n;
    }
    std::fclose(f);
    std::printf("rds_counts_host_check: %ld records, %ld elements, %d failures\n", records, elements, g_failures);
    return g_failures || records == 0 ? 1 : 0;
}
