// The box statistics of K33 (bayes_probs_internal.h) as a host program with its own main, built with
// -fsanitize=address,undefined -ffp-contract=off (make bayes_probs_check CORPUS=file).  Never part of the library, never loaded
// into Python.  The corpus (scripts/make_bayes_probs_corpus.py) holds pooled draws and the outputs of
// tests/bayes_probs_restate.py; the program sorts each series as the kernel does (-0.0 as +0.0), runs box_stats -- the routine
// the kernel's first lane runs on the LDS-sorted draws -- and compares bits.
//
// Corpus: "BAYESBOX", int32 n_cases; per case int32 N, doubles y[N], box[7].
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "bayes_probs_internal.h"

using namespace icnv;

namespace {

bool same_bits(double a, double b) {
    if (a != a && b != b) return true;
    return std::memcmp(&a, &b, 8) == 0;
}

template <typename T>
bool take(FILE *f, T *out, size_t n) { return std::fread(out, sizeof(T), n, f) == n; }

}  // namespace

int main(int argc, char **argv) {
    if (argc != 2) { std::fprintf(stderr, "usage: %s corpus\n", argv[0]); return 2; }
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    char magic[8];
    int32_t n_cases = 0;
    if (!take(f, magic, 8) || std::memcmp(magic, "BAYESBOX", 8) != 0 || !take(f, &n_cases, 1) || n_cases < 1) {
        std::fprintf(stderr, "not a corpus of make_bayes_probs_corpus.py\n");
        return 2;
    }
    static const char *BF[BOX_FIELDS] = {"ymin", "lower", "middle", "upper", "ymax", "n_low", "n_high"};
    long bad = 0, values = 0;
    for (int32_t cs = 0; cs < n_cases; ++cs) {
        int32_t N = 0;
        if (!take(f, &N, 1)) { std::fprintf(stderr, "case %d: truncated\n", cs); return 2; }
        if (N < MCMC_MIN_CHAINS || N > MCMC_MAX_POOLED) {
            std::fprintf(stderr, "case %d: %d pooled draws are outside what the entry point accepts\n", cs, N);
            return 2;
        }
        // exactly sized: an index past the series is the sanitizer's to find
        std::vector<double> y((size_t)N), want(BOX_FIELDS), got(BOX_FIELDS);
        if (!take(f, y.data(), y.size()) || !take(f, want.data(), want.size())) { std::fprintf(stderr, "case %d: truncated\n", cs); return 2; }
        bool any_nan = false;
        for (double &v : y) {
            any_nan |= v != v;
            if (v == 0.0) v = 0.0;
        }
        if (!any_nan) std::sort(y.begin(), y.end());
        box_stats(y.data(), N, any_nan, got.data());
        for (int i = 0; i < BOX_FIELDS; ++i, ++values)
            if (!same_bits(got[i], want[i])) {
                std::fprintf(stderr, "case %d (%d draws) %s: %.17g, the corpus has %.17g\n", cs, N, BF[i], got[i], want[i]);
                ++bad;
            }
    }
    std::fclose(f);
    if (bad) { std::fprintf(stderr, "%ld differences\n", bad); return 1; }
    std::printf("bayes_probs_host_check: %d cases, %ld values bit-equal\n", n_cases, values);
    return 0;
}
