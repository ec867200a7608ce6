// The per-series routines of the MCMC diagnostics (K31, mcmc_diag_internal.h) as a host program with its own main, built with
// -fsanitize=address,undefined -ffp-contract=off (make mcmc_diag_check CORPUS=file).  Never part of the library, never loaded
// into Python.  The corpus (scripts/make_mcmc_diag_corpus.py) holds series and the outputs of tests/mcmc_diag_restate.py; the
// program runs the routines the kernel deals to its lanes one after the other and compares bits.
//
// Corpus: "MCMCDIAG", int32 n_cases; per case int32 n_chains, n_keep, int32 windows[3][3] (lo, m, P of the whole series, Geweke's A
// and B), doubles x[n_chains][n_keep], chain_stats[n_chains][9], pooled[7].
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "icnv_log_table.h"
#include "mcmc_diag_internal.h"

using namespace icnv;

namespace {

const double LOG_TAB[ICNV_LOG_N][3] = ICNV_LOG_TABLE_INIT;

// lib_log of lib_math.h, operation by operation, with the host's correctly rounded fma
struct HostLog {
    double operator()(double x) const {
        uint64_t ix;
        std::memcpy(&ix, &x, 8);
        if (ix - 0x0010000000000000ull >= 0x7fe0000000000000ull) {
            if ((ix << 1) == 0) return -INFINITY;
            if (ix == 0x7ff0000000000000ull) return x;
            if ((ix >> 63) || (ix & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) return NAN;
            const double xs = x * 0x1p52;
            std::memcpy(&ix, &xs, 8);
            ix -= 52ull << 52;
        }
        const uint64_t tmp = ix - ICNV_LOG_OFF;
        const int i = (int)((tmp >> 45) & 127);
        const int k = (int)((int64_t)tmp >> 52);
        const uint64_t iz = ix - (tmp & 0xfff0000000000000ull);
        double z;
        std::memcpy(&z, &iz, 8);
        const double r = std::fma(z, LOG_TAB[i][0], -1.0);
        const double kd = (double)k;
        const double w = std::fma(kd, ICNV_LOG_LN2HI, LOG_TAB[i][1]);
        const double hi = w + r;
        const double lo = ((w - hi) + r) + (kd * ICNV_LOG_LN2LO + LOG_TAB[i][2]);
        const double r2 = r * r;
        double q = std::fma(r, ICNV_LOG_B6, ICNV_LOG_B5);
        q = std::fma(r, q, ICNV_LOG_B4);
        q = std::fma(r, q, ICNV_LOG_B3);
        q = std::fma(r, q, ICNV_LOG_B2);
        q = std::fma(r, q, ICNV_LOG_B1);
        q = std::fma(r, q, ICNV_LOG_B0);
        return hi + std::fma(r2, q, lo);
    }
};

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
    if (!take(f, magic, 8) || std::memcmp(magic, "MCMCDIAG", 8) != 0 || !take(f, &n_cases, 1) || n_cases < 1) {
        std::fprintf(stderr, "not a corpus of make_mcmc_diag_corpus.py\n");
        return 2;
    }
    static const char *CF[MCMC_CHAIN_FIELDS] = {"mean", "var", "spec0", "order", "geweke", "acf1", "acf5", "acf10", "acf50"};
    static const char *PF[MCMC_POOLED_FIELDS] = {"mean", "sd", "q2.5", "q50", "q97.5", "psrf", "ess"};
    long bad = 0, values = 0;
    for (int32_t cs = 0; cs < n_cases; ++cs) {
        int32_t dims[2], win[9];
        if (!take(f, dims, 2) || !take(f, win, 9)) { std::fprintf(stderr, "case %d: truncated\n", cs); return 2; }
        const int m = dims[0], n = dims[1];
        if (m < MCMC_MIN_CHAINS || m > MCMC_MAX_CHAINS || n < MCMC_MIN_KEEP || (int64_t)m * n > MCMC_MAX_POOLED) {
            std::fprintf(stderr, "case %d: %d chains of %d draws are outside what the entry points accept\n", cs, m, n);
            return 2;
        }
        const size_t N = (size_t)m * n;
        std::vector<double> x(N), want_cs((size_t)m * MCMC_CHAIN_FIELDS), want_po(MCMC_POOLED_FIELDS);
        if (!take(f, x.data(), N) || !take(f, want_cs.data(), want_cs.size()) || !take(f, want_po.data(), want_po.size())) {
            std::fprintf(stderr, "case %d: truncated\n", cs);
            return 2;
        }
        McmcWindow w[3];
        mcmc_windows(n, w);
        for (int q = 0; q < 3; ++q)
            if (w[q].lo != win[3 * q] || w[q].m != win[3 * q + 1] || w[q].P != win[3 * q + 2]) {
                std::fprintf(stderr, "case %d window %d: (%d, %d, %d), the corpus has (%d, %d, %d)\n", cs, q, w[q].lo, w[q].m, w[q].P,
                             win[3 * q], win[3 * q + 1], win[3 * q + 2]);
                ++bad;
            }
        // exactly sized work space: an index past the contract's bounds is the sanitizer's to find
        std::vector<double> c((size_t)w[MCMC_FULL].P + 1), phi((size_t)w[MCMC_FULL].P + 1), got_cs(want_cs.size()), got_po(MCMC_POOLED_FIELDS);
        for (int ch = 0; ch < m; ++ch) {
            const std::vector<double> series(x.begin() + (size_t)ch * n, x.begin() + (size_t)(ch + 1) * n);
            mcmc_chain_stats(series.data(), n, w, HostLog{}, c.data(), phi.data(), got_cs.data() + (size_t)ch * MCMC_CHAIN_FIELDS);
        }
        bool any_nan = false;
        std::vector<double> sorted(x);
        for (double &v : sorted) {
            any_nan |= v != v;
            if (v == 0.0) v = 0.0;
        }
        if (!any_nan) std::sort(sorted.begin(), sorted.end());
        mcmc_pooled_stats(x.data(), sorted.data(), any_nan, got_cs.data(), m, n, got_po.data());
        for (int ch = 0; ch < m; ++ch)
            for (int i = 0; i < MCMC_CHAIN_FIELDS; ++i, ++values) {
                const double g = got_cs[(size_t)ch * MCMC_CHAIN_FIELDS + i], e = want_cs[(size_t)ch * MCMC_CHAIN_FIELDS + i];
                if (!same_bits(g, e)) { std::fprintf(stderr, "case %d chain %d %s: %.17g, the corpus has %.17g\n", cs, ch, CF[i], g, e); ++bad; }
            }
        for (int i = 0; i < MCMC_POOLED_FIELDS; ++i, ++values)
            if (!same_bits(got_po[i], want_po[i])) {
                std::fprintf(stderr, "case %d pooled %s: %.17g, the corpus has %.17g\n", cs, PF[i], got_po[i], want_po[i]);
                ++bad;
            }
    }
    std::fclose(f);
    if (bad) { std::fprintf(stderr, "%ld differences\n", bad); return 1; }
    std::printf("mcmc_diag_host_check: %d cases, %ld values bit-equal\n", n_cases, values);
    return 0;
}
