// Stand-alone CPU check of K20's field arithmetic (table_text_digits.h): the certified digits, the host's exact path for
// flagged elements, the width rule and the characters, against a formatter written here from snprintf("%.14e") alone.
//   g++ -O2 -std=c++17 -o table_text_check table_text_check.cpp && ./table_text_check [n_random]
// Prints the number of values checked and how many were flagged; exits 1 on the first difference.  It uses no GPU, so it
// may be built with -fsanitize=address,undefined.
#include <cinttypes>
#include <random>
#include <string>

#include "table_text_digits.h"

using namespace icnv;

static std::string reference(double v) {
    if (v != v) return "NaN";
    if (std::isinf(v)) return v > 0 ? "Inf" : "-Inf";
    if (v == 0.0) return "0";
    char buf[48];
    std::snprintf(buf, sizeof buf, "%.14e", std::fabs(v));
    std::string s(buf), digits;
    const size_t epos = s.find('e');
    for (size_t i = 0; i < epos; ++i)
        if (s[i] != '.') digits += s[i];
    const int e = std::atoi(s.c_str() + epos + 1);
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    const int nsig = (int)digits.size(), neg = v < 0;
    const int w_sci = neg + (nsig > 1 ? nsig + 1 : 1) + (std::abs(e) < 100 ? 4 : 5);
    const int rgt = std::max(0, nsig - e - 1);
    const int w_fix = neg + (e >= 0 ? e + 1 : 1) + (rgt ? rgt + 1 : 0);
    std::string out = neg ? "-" : "";
    if (w_fix <= w_sci) {
        if (e >= 0) {
            std::string whole = digits + std::string((size_t)std::max(0, e + 1 - nsig), '0');
            out += whole.substr(0, (size_t)e + 1);
            if (nsig > e + 1) out += "." + digits.substr((size_t)e + 1);
        } else {
            out += "0." + std::string((size_t)(-e - 1), '0') + digits;
        }
        return out;
    }
    out += digits.substr(0, 1);
    if (nsig > 1) out += "." + digits.substr(1);
    char ex[16];
    std::snprintf(ex, sizeof ex, "e%c%02d", e >= 0 ? '+' : '-', std::abs(e));
    return out + ex;
}

static long n_flagged = 0;

static std::string ours(double v) {
    uint64_t bits, rec;
    uint16_t meta;
    std::memcpy(&bits, &v, sizeof bits);
    tt_digits(bits, rec, meta);
    if (rec & TT_FLAG_BIT) {
        ++n_flagged;
        tt_host_record(bits, rec, meta);
    }
    const int len = meta >> 10, E = (int)(meta & 1023) - TT_E_BIAS;
    std::string s;
    for (int p = 0; p < len; ++p) s += (char)tt_char(p, rec, E, len);
    return s;
}

static int check(double v) {
    const std::string a = ours(v), b = reference(v);
    if (a == b && (int)a.size() <= TT_MAX_FIELD) return 0;
    std::printf("MISMATCH %a: ours '%s' reference '%s'\n", v, a.c_str(), b.c_str());
    return 1;
}

int main(int argc, char **argv) {
    const long n = argc > 1 ? std::atol(argv[1]) : 2000000;
    long done = 0;
    const double special[] = {0.0, -0.0, 1.0, 0.1, 0.3, 2.0 / 3.0, 0.30000000000000004, 1e5, 1e-4, 0.0001234, 1234567.125, 9.5367431640625e-07,
                              1e15, 1e22, 999999999999999.5, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, NAN, INFINITY,
                              100000000000000.5, 123456789012345.5, 123456789012346.5, 123456789012345678.0, 1e-300, 1e100, 1e-100,
                              99999999999999.99, 9999999999999995.0, 0.99999999999999994};
    for (double v : special) {
        if (check(v) || check(-v)) return 1;
        done += 2;
    }
    const long planted = n_flagged;
    for (int b = -1074; b <= 1023; ++b)                        // every binary exponent: its powers of two and their neighbours
        for (double v : {std::ldexp(1.0, b), std::nextafter(std::ldexp(1.0, b), INFINITY), std::nextafter(std::ldexp(1.0, b), 0.0)}) {
            if (check(v)) return 1;
            ++done;
        }
    for (int e = -323; e <= 308; ++e) {                        // every power of ten as strtod reads it, and its neighbours
        char buf[16];
        std::snprintf(buf, sizeof buf, "1e%d", e);
        const double p = std::strtod(buf, nullptr);
        for (double v : {p, std::nextafter(p, INFINITY), std::nextafter(p, 0.0)}) {
            if (check(v)) return 1;
            ++done;
        }
    }
    std::mt19937_64 rng(20);
    for (long i = 0; i < n; ++i) {                             // uniform over bit patterns
        const uint64_t u = rng();
        double v;
        std::memcpy(&v, &u, sizeof v);
        if (check(v)) return 1;
        ++done;
    }
    const long before = n_flagged;
    std::normal_distribution<double> norm(1.0, 0.1);
    std::uniform_real_distribution<double> unif(-0.3, 0.3);
    for (long i = 0; i < n; ++i) {                             // what a clamped heatmap holds
        if (check(norm(rng)) || check(std::exp2(unif(rng)))) return 1;
        done += 2;
    }
    const long heat = n_flagged - before;
    for (long i = 0; i < n / 4; ++i) {                         // integers and halves at 15 - 16 digits: ties are common here
        const double v = (double)(rng() % 2000000000000000ull) * 0.5;
        if (check(v)) return 1;
        ++done;
    }
    std::printf("ok: %ld values, %ld flagged in all, %ld among the specials, %ld among the heatmap-like values\n", done, n_flagged, planted,
                heat);
    return 0;
}
