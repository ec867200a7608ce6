// The arithmetic of K20's fields (include/icnv.h "matrix files of plot_cnv"): the record of one element, the certified 15-digit
// rounding, the width rule and the characters.  Plain C++ that compiles for the device and for the host, so that the same
// functions can be checked on a CPU against snprintf.  DESIGN.md section 4 K20.
#pragma once
#include <stdint.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#if defined(__HIPCC__)
#define TT_HD __host__ __device__
#else
#define TT_HD
#endif

#include "tt_pow10_table.h"

namespace icnv {

constexpr int TT_MAX_FIELD = 22;           // "-d.dddddddddddddde-XXX"

// One element's record.  rec: bits 0..59 the 15 decimal digits, one per nibble, the most significant in bits 56..59; bit 60
// needs-exact (the host replaces the record); bit 61 the sign; bits 62..63 the class.  meta: bits 0..9 the decimal
// exponent + 324, bits 10..14 the field length in bytes.
constexpr int TT_FINITE = 0, TT_ZERO = 1, TT_NAN = 2, TT_INF = 3;
constexpr uint64_t TT_BCD_MASK = (1ull << 60) - 1;
constexpr uint64_t TT_FLAG_BIT = 1ull << 60;
constexpr int TT_E_BIAS = 324;

TT_HD inline int tt_nsig(uint64_t bcd) {          // significant digits after dropping trailing zeros (bcd != 0)
    return 15 - (__builtin_ctzll(bcd) >> 2);
}
// The width rule of formatReal: fixed notation unless scientific is strictly narrower.
TT_HD inline int tt_field_len(int nsig, int e, int neg, bool &sci) {
    const int w_sci = neg + (nsig > 1 ? nsig + 1 : 1) + ((e > -100 && e < 100) ? 4 : 5);
    const int rgt = nsig - e - 1 > 0 ? nsig - e - 1 : 0;
    const int w_fix = neg + (e >= 0 ? e + 1 : 1) + (rgt ? rgt + 1 : 0);
    sci = w_fix > w_sci;
    return sci ? w_sci : w_fix;
}
TT_HD inline uint16_t tt_meta(int e, int len) { return (uint16_t)((e + TT_E_BIAS) | (len << 10)); }


// ---- digits ---------------------------------------------------------------------------------------------------------------
// |x| = m * 2^ee with 2^63 <= m < 2^64 (the significand shifted up; exact).  With b = ee + 63 = floor(log2 |x|),
// E_est = floor(b log10 2) (gen_pow10_table.py checks the integer formula for every b) has 10^E_est <= 2^b <= |x| < 2^(b+1)
// < 20 * 10^E_est, so the decimal exponent E is E_est or E_est + 1, and with k = 14 - E_est
//     10^14 <= |x| 10^k < 2 * 10^15.
// The table holds P = floor(10^k / 2^q) with 2^127 <= P < 2^128, so 10^k = (P + d) 2^q with 0 <= d < 1, and
//     |x| 10^k = (m P + m d) 2^(ee + q).
// m P is a 192-bit integer w2 : w1 : w0 (64-bit words).  The kernel forms w2 and w1 exactly except that it leaves out the low
// word b_lo of m * P_lo, whose high word b_hi is added into w1 -- b_lo is all of w0 and carries nothing upwards.  With
// t = -(ee + q) - 128 (1 <= t <= 63, checked by the generator for every b and both k) the integer part and the first 64
// fraction bits of |x| 10^k are
//     I = w2 >> t,     f = (w2 << (64 - t)) | (w1 >> t),
// and what is discarded is  (w1 mod 2^t) 2^64 + w0 + m d  <  (2^t - 1) 2^64 + 2^64 + 2^64 = (2^t + 1) 2^64  in units of
// 2^(ee + q), that is less than 1 + 2^-t units of f.  All discarded terms are >= 0.  So the true fraction F satisfies
//     f <= F 2^64 < f + 1 + 2^-t.
// F > 1/2 is certain when f >= 2^63 + 1 and F < 1/2 is certain when f + 2 <= 2^63.  The two values f = 2^63 - 1 and
// f = 2^63 are not decided: the element is flagged and formatted on the host.  An exact tie (F = 1/2) has f = 2^63 when the
// table entry is exact and f = 2^63 - 1 otherwise, so it is always flagged.
// The exponent: I >= 10^15 proves |x| 10^k >= 10^15 (the product is a lower bound), so E = E_est + 1 and the product is
// taken again with k - 1.  I = 10^15 - 1 with f >= 2^64 - 2 leaves open whether |x| 10^k reaches 10^15; both readings round
// to the same text (D = 10^15 carries to 10^14 with E + 1), and the element is flagged all the same.
// The certified domain, then, in terms of s = |x| 10^(14 - E) in [10^14, 10^15): every finite non-zero double except those whose
// fraction of s lies within 2^-62 of 1/2 (f is one of the two undecided values only if |F - 1/2| < 2^-63 + 2^-64 (1 + 2^-t)) and
// those with s within 2^-62 of 10^15 or of 10^14 (|x| within that of a power of ten, seen from the estimate's side).
constexpr uint64_t TT_1E15 = 1000000000000000ull, TT_1E14 = 100000000000000ull;
constexpr uint64_t TT_HALF = 1ull << 63;

TT_HD inline uint64_t tt_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

TT_HD inline void tt_product(uint64_t m, int ee, int k, uint64_t &I, uint64_t &f) {
    const int i = k - TT_K_MIN;
    const uint64_t hi = tt_pow10_hi[i], lo = tt_pow10_lo[i];
    const int q = tt_pow10_q[i];
    const uint64_t a_hi = tt_mulhi(m, hi), a_lo = m * hi, b_hi = tt_mulhi(m, lo);
    const uint64_t w1 = a_lo + b_hi;
    const uint64_t w2 = a_hi + (w1 < a_lo ? 1ull : 0ull);
    const int t = -(ee + q) - 128;
    I = w2 >> t;
    f = (w2 << (64 - t)) | (w1 >> t);
}

TT_HD inline uint64_t tt_bcd(uint64_t D) {     // D < 10^15: one decimal digit per nibble
    uint32_t h = (uint32_t)(D / 100000000ull), l = (uint32_t)(D - (uint64_t)h * 100000000ull);
    uint64_t bcd = 0;
    for (int i = 0; i < 8; ++i) { bcd |= (uint64_t)(l % 10u) << (4 * i); l /= 10u; }
    for (int i = 8; i < 15; ++i) { bcd |= (uint64_t)(h % 10u) << (4 * i); h /= 10u; }
    return bcd;
}

TT_HD inline void tt_digits(uint64_t u, uint64_t &rec, uint16_t &meta) {
    const uint64_t neg = u >> 63, a = u & 0x7fffffffffffffffull;
    if (a > 0x7ff0000000000000ull) { rec = (uint64_t)TT_NAN << 62; meta = tt_meta(0, 3); return; }
    if (a == 0x7ff0000000000000ull) { rec = ((uint64_t)TT_INF << 62) | (neg << 61); meta = tt_meta(0, 3 + (int)neg); return; }
    if (a == 0) { rec = (uint64_t)TT_ZERO << 62; meta = tt_meta(0, 1); return; }
    const int ex = (int)(a >> 52);
    uint64_t m = a & ((1ull << 52) - 1);
    int ee = -1074;
    if (ex) { m |= 1ull << 52; ee = ex - 1075; }
    const int lz = __builtin_clzll(m);
    m <<= lz;
    ee -= lz;
    int E = ((ee + 63) * 78913) >> 18;
    uint64_t I, f;
    tt_product(m, ee, 14 - E, I, f);
    if (I >= TT_1E15) {
        E += 1;
        tt_product(m, ee, 14 - E, I, f);
    }
    const bool flag = f == TT_HALF - 1 || f == TT_HALF || (I == TT_1E15 - 1 && f >= ~1ull);
    uint64_t D = I + (f > TT_HALF ? 1ull : 0ull);
    if (D >= TT_1E15) { D = TT_1E14; E += 1; }
    const uint64_t bcd = tt_bcd(D);
    bool sci;
    const int len = tt_field_len(tt_nsig(bcd), E, (int)neg, sci);
    rec = bcd | (flag ? TT_FLAG_BIT : 0ull) | (neg << 61);
    meta = tt_meta(E, len);
}


// ---- characters ----------------------------------------------------------------------------------------------------------
TT_HD inline uint8_t tt_char(int p, uint64_t rec, int E, int len) {
    const int cls = (int)(rec >> 62), neg = (int)((rec >> 61) & 1);
    if (cls != TT_FINITE) {
        const uint32_t w = cls == TT_ZERO ? 0x30u : cls == TT_NAN ? 0x4e614eu /* NaN */ : neg ? 0x666e492du /* -Inf */ : 0x666e49u /* Inf */;
        return (uint8_t)(w >> (8 * p));
    }
    if (p < neg) return '-';
    const uint64_t bcd = rec & TT_BCD_MASK;
    const int nsig = tt_nsig(bcd), p0 = p - neg;
    bool sci;
    tt_field_len(nsig, E, neg, sci);
    auto digit = [bcd](int i) -> uint8_t { return (uint8_t)('0' + (i < 15 ? (int)((bcd >> (4 * (14 - i))) & 15) : 0)); };
    if (!sci) {
        if (E >= 0) return p0 <= E ? digit(p0) : p0 == E + 1 ? '.' : digit(p0 - 1);
        const int z = -E - 1;                                  // zeros between the point and the first digit
        return p0 == 1 ? '.' : p0 < 2 + z ? '0' : digit(p0 - 2 - z);
    }
    const int ml = nsig > 1 ? nsig + 1 : 1;                    // mantissa bytes
    if (p0 < ml) return p0 == 0 ? digit(0) : p0 == 1 ? '.' : digit(p0 - 1);
    const int q = p0 - ml, ae = E < 0 ? -E : E;
    if (q == 0) return 'e';
    if (q == 1) return E < 0 ? '-' : '+';
    const int d = ae >= 100 ? (q == 2 ? ae / 100 : q == 3 ? (ae / 10) % 10 : ae % 10) : (q == 2 ? ae / 10 : ae % 10);
    return (uint8_t)('0' + d);
}

// ---- the host's exact path ------------------------------------------------------------------------------------------------
// What snprintf("%.14e") gives for |x| (correctly rounded in glibc), as a record without the needs-exact bit.
inline void tt_host_record(uint64_t bits, uint64_t &rec, uint16_t &meta) {
    double v;
    std::memcpy(&v, &bits, sizeof v);
    char buf[48];
    std::snprintf(buf, sizeof buf, "%.14e", std::fabs(v));
    uint64_t bcd = 0;
    const char *c = buf;
    for (; *c && *c != 'e'; ++c)
        if (*c >= '0' && *c <= '9') bcd = (bcd << 4) | (uint64_t)(*c - '0');
    const int E = *c ? std::atoi(c + 1) : 0;
    const int neg = (int)(bits >> 63);
    bool sci;
    const int len = tt_field_len(tt_nsig(bcd), E, neg, sci);
    rec = bcd | ((uint64_t)neg << 61);
    meta = tt_meta(E, len);
}

}  // namespace icnv
