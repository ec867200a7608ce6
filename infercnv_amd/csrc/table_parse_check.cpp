// Stand-alone CPU check of K21's host side and field arithmetic (table_parse_num.h, table_parse_host.h): the certified
// conversion against strtod on random and adversarial fields, and -- for every file named on the command line -- the
// chunking at whole lines through a small growing buffer, the fields' extents, the label slices and the strtod path;
// and the text of a refusal (tp_describe).  The chunking here re-enacts in C++ what device.read_table does in Python: the
// shipped host routines it runs are tp_scan_number, tp_convert, tp_field_end, tp_host_field, tp_label_slice and tp_describe.
//   g++ -O2 -std=c++17 -o table_parse_check table_parse_check.cpp && ./table_parse_check [n_random] [chunk_bytes] [files...]
// A file is read twice: whole, and in chunks of chunk_bytes; both readings must give the same labels and the same bits.
// Prints what it checked; exits 1 on the first difference.  It uses no GPU, so it may be built with
// -fsanitize=address,undefined.
#include <cinttypes>
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "table_parse_host.h"

using namespace icnv;

static long n_certified = 0, n_declined = 0;

static uint64_t strtod_bits(const std::string &s) {
    const double v = std::strtod(s.c_str(), nullptr);
    uint64_t b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

// A field of the decimal grammar: whatever the device certifies must be strtod's bits, and the host path always is.
static int check_field(const std::string &s) {
    const uint8_t *t = reinterpret_cast<const uint8_t *>(s.data());
    uint64_t bits, w, host_bits;
    int q;
    bool neg;
    const int kind = tp_scan_number(t, (int64_t)s.size(), bits, w, q, neg);
    const uint64_t want = strtod_bits(s);
    if (kind == TP_BAD) { std::printf("REFUSED '%s'\n", s.c_str()); return 1; }
    if (kind == TP_DECIMAL) {
        if (tp_convert(w, q, neg, bits)) {
            ++n_certified;
            if (bits != want) { std::printf("MISMATCH '%s': certified %016" PRIx64 ", strtod %016" PRIx64 "\n", s.c_str(), bits, want); return 1; }
        } else ++n_declined;
    } else if (kind == TP_HOST) ++n_declined;
    else if (bits != want) { std::printf("MISMATCH '%s': value %016" PRIx64 ", strtod %016" PRIx64 "\n", s.c_str(), bits, want); return 1; }
    if (tp_host_field(t, (int64_t)s.size(), 0, '\t', host_bits) != TP_VALUE || host_bits != want) {
        std::printf("MISMATCH '%s': host path %016" PRIx64 ", strtod %016" PRIx64 "\n", s.c_str(), host_bits, want);
        return 1;
    }
    return 0;
}

static int check_refused(const std::string &s) {
    uint64_t bits;
    if (tp_host_field(reinterpret_cast<const uint8_t *>(s.data()), (int64_t)s.size(), 0, '\t', bits) == TP_BAD) return 0;
    std::printf("ACCEPTED '%s'\n", s.c_str());
    return 1;
}

struct Parsed {
    std::vector<std::string> labels;
    std::vector<uint64_t> bits;
    long bad = 0;
};

// The rows of text[0 .. n): whole lines (the last may lack its '\n').
static void parse_lines(const uint8_t *text, int64_t n, uint8_t sep, Parsed &out) {
    int64_t p = 0;
    while (p < n) {
        if (tp_at_line_end(text, n, p)) {                               // a blank line
            while (p < n && text[p] != '\n') ++p;
            ++p;
            continue;
        }
        int64_t b = p, e = tp_field_end(text, n, p, sep);
        tp_label_slice(text, b, e);
        out.labels.emplace_back(reinterpret_cast<const char *>(text + b), (size_t)(e - b));
        p = tp_field_end(text, n, p, sep);
        while (p < n && text[p] == sep) {
            ++p;
            uint64_t bits = 0;
            if (tp_host_field(text, n, p, sep, bits) != TP_VALUE) ++out.bad;
            out.bits.push_back(bits);
            p = tp_field_end(text, n, p, sep);
        }
        while (p < n && text[p] != '\n') ++p;
        ++p;
    }
}

static int check_file(const char *path, int64_t chunk) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); return 1; }
    std::vector<uint8_t> all;
    uint8_t block[4096];
    for (size_t got; (got = std::fread(block, 1, sizeof block, f)) > 0;) all.insert(all.end(), block, block + got);
    std::fclose(f);
    Parsed whole, pieces;
    parse_lines(all.data(), (int64_t)all.size(), '\t', whole);
    // the same bytes through a buffer of `chunk` bytes that is cut at whole lines and grows when a line does not fit
    std::vector<uint8_t> buf((size_t)chunk);
    int64_t fill = 0, at = 0, grown = 0, chunks = 0;
    const int64_t n = (int64_t)all.size();
    while (at < n || fill > 0) {
        const int64_t take = std::min<int64_t>((int64_t)buf.size() - fill, n - at);
        std::memcpy(buf.data() + fill, all.data() + at, (size_t)take);
        fill += take;
        at += take;
        const bool eof = at >= n;
        const int64_t cut = eof ? fill : tp_cut_whole_lines(buf.data(), fill);
        if (cut == 0 && !eof) { buf.resize(buf.size() * 2); ++grown; continue; }
        std::vector<uint8_t> exact(buf.begin(), buf.begin() + cut);   // an allocation of exactly the chunk: any read past it is seen
        parse_lines(exact.data(), cut, '\t', pieces);
        ++chunks;
        std::memmove(buf.data(), buf.data() + cut, (size_t)(fill - cut));
        fill -= cut;
    }
    if (whole.labels != pieces.labels || whole.bits != pieces.bits || whole.bad != pieces.bad) {
        std::printf("MISMATCH %s: whole and chunked readings differ\n", path);
        return 1;
    }
    std::printf("%s: %zu rows, %zu fields, %ld refused, %" PRId64 " chunks, buffer grown %" PRId64 " times\n", path, whole.labels.size(),
                whole.bits.size(), whole.bad, chunks, grown);
    return 0;
}

// tp_describe on refused offsets of a text that is allocated to its exact size: line, field and bytes, up to the offset n.
static int check_describe() {
    const std::string src = "g1\t1\t2\n\ng\"2\t3\n\"g3\"\t1.2.3\t4\r\ng4\t5\t";
    const std::vector<uint8_t> t(src.begin(), src.end());
    const int64_t n = (int64_t)t.size();
    const struct { int64_t offset; int code; int64_t n_cols; const char *want; } cases[] = {
        {8, TP_E_RAGGED, 2, "line 3, field 2: the row has 2 fields, 3 are expected (a label and 2 numbers)"},
        {9, TP_E_LABEL, 2, "line 3, field 1: a label may hold a quote only as its first and its last byte: 'g\"2'"},
        {19, TP_E_NUMBER, 2, "line 4, field 2: not a number of the table grammar: '1.2.3'"},
        {n, TP_E_NUMBER, 2, "line 5, field 3: not a number of the table grammar: ''"},
        {n - 5, TP_E_RAGGED, 3, "line 5, field 3: the row has 3 fields, 4 are expected (a label and 3 numbers)"}};
    for (const auto &c : cases) {
        const std::string got = tp_describe(t.data(), n, c.offset, c.code, '\t', 1, c.n_cols);
        if (got != c.want) { std::printf("DESCRIBE offset %ld: '%s', expected '%s'\n", (long)c.offset, got.c_str(), c.want); return 1; }
    }
    return 0;
}

int main(int argc, char **argv) {
    const long n = argc > 1 ? std::atol(argv[1]) : 1000000;
    const int64_t chunk = argc > 2 ? std::atoll(argv[2]) : 4096;
    const char *hard[] = {"9007199254740993", "2.2250738585072011e-308", "1.7976931348623158e308", "4.9e-324", "1e-400", "1e400", "-0", "0", "+3",
                          ".5", "5.", "1E5", "1e22", "1e23", "8.5e22", "123456789012345678", "1234567890123456789", "12345678901234567890",
                          "0.000001", "0.1", "0.30000000000000004", "5e-324", "2.4703282292062327e-324", "2.4703282292062328e-324",
                          "9007199254740992.5", "9007199254740991.5", "4503599627370497.5", "1.00000000000000011102230246251565404236316680908203125",
                          "1.00000000000000011102230246251565404236316680908203124", "1.00000000000000011102230246251565404236316680908203126",
                          "179769313486231580793728971405303415079934132710037826936173778980444968292764750946649017977587207096330286416692887910946"
                          "555547851940402630657488671505820681908902000708383676273854845817711531764475730270069855571366959622842914819860834936475"
                          "29222636984749999999999999999", "00000000000000000000000000012", "0.00000000000000000000000000000000012", "1e+5", "1e-5"};
    for (const char *h : hard)
        if (check_field(h) || (h[0] != '-' && h[0] != '+' && check_field(std::string("-") + h))) return 1;
    const char *refused[] = {"1.2.3", "abc", "\"1\"", "0x10", " 1", "1 ", "1e", "1e+", ".", "+", "-", "e5", "nan", "inf", "Infinity", "NaNa", "1,5", "--1",
                             "1d5", "-NaN", "-NA"};
    for (const char *r : refused)
        if (check_refused(r)) return 1;
    const uint8_t na[] = "NA";
    uint64_t bits;
    if (tp_host_field(na, 2, 0, '\t', bits) != TP_VALUE || bits != TP_NA_BITS || tp_host_field(na, 0, 0, '\t', bits) != TP_VALUE || bits != TP_NA_BITS) {
        std::printf("NA is not NA_real_\n");
        return 1;
    }
    if (check_describe()) return 1;
    std::mt19937_64 rng(21);
    long done = 0;
    char buf[64];
    for (long i = 0; i < n; ++i) {                                      // 1 .. 19 digits, every exponent the doubles reach and some beyond
        const int nd = 1 + (int)(rng() % 19);
        uint64_t w = rng();
        uint64_t lim = 1;
        for (int d = 0; d < nd; ++d) lim *= 10;
        w %= lim;
        std::snprintf(buf, sizeof buf, "%" PRIu64 "e%d", w, (int)(rng() % 700) - 360);
        if (check_field(buf)) return 1;
        ++done;
    }
    for (long i = 0; i < n; ++i) {                                      // the shape of the data: integers and short decimals
        std::snprintf(buf, sizeof buf, "%.6g", std::ldexp((double)(rng() % 1000000), -(int)(rng() % 20)));
        if (check_field(buf)) return 1;
        ++done;
    }
    for (long i = 0; i < n / 4; ++i) {                                  // halfway decimals (2 m + 1) 2^(e - 1), printed exactly, cut to 19 digits
        const uint64_t m = (1ull << 52) | (rng() >> 12);
        const int e = (int)(rng() % 60);                                // value (2 m + 1) * 2^e: an integer, exact in %.0f up to 2^113
        const long double v = std::ldexp((long double)(2 * m + 1), e);
        char big[80];
        std::snprintf(big, sizeof big, "%.0Lf", v);
        std::string s(big);
        if (check_field(s)) return 1;
        if (s.size() > 19) {
            const std::string cut = s.substr(0, 19) + "e" + std::to_string(s.size() - 19);
            if (check_field(cut)) return 1;
        }
        ++done;
    }
    std::printf("ok: %ld fields, %ld certified on the device path, %ld declined\n", done, n_certified, n_declined);
    for (int i = 3; i < argc; ++i)
        if (check_file(argv[i], chunk)) return 1;
    return 0;
}
