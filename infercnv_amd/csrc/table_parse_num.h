// The arithmetic of K21's fields (include/icnv.h "count matrices from text"): the grammar of one numeric field and its
// conversion to the correctly rounded double.  Plain C++ that compiles for the device and for the host, so that the same
// functions can be checked on a CPU against strtod (table_parse_check.cpp); gen_parse_pow10_table.py restates them in exact
// Python integers.  DESIGN.md section 4 K21.
#pragma once
#include <stdint.h>
#include <cstring>

#if defined(__HIPCC__)
#define TP_HD __host__ __device__
#else
#define TP_HD
#endif

#include "tp_pow10_table.h"

namespace icnv {

constexpr uint64_t TP_NA_BITS = 0x7FF00000000007A2ull;    // R's NA_real_, the bits K19 stores
constexpr uint64_t TP_NAN_BITS = 0x7FF8000000000000ull;
constexpr uint64_t TP_INF_BITS = 0x7FF0000000000000ull;
constexpr uint64_t TP_SIGN = 1ull << 63;
constexpr int TP_MAX_DIGITS = 19;          // significant digits the device converts: 10^19 < 2^64
constexpr int TP_MAX_SCAN = 40;            // bytes of a field the device reads; a longer field goes to the host unread

constexpr int TP_VALUE = 0, TP_DECIMAL = 1, TP_HOST = 2, TP_BAD = 3;

// The grammar of a numeric field s[0 .. len):
//   empty | NA | NaN | [+-]Inf | [+-] (digits [. [digits]] | . digits) [(e|E) [+-] digits]
// TP_VALUE: `bits` is the result (NA, NaN, an infinity, a zero).  TP_DECIMAL: the value is (neg ? -1 : 1) * w * 10^q with
// 1 <= w < 10^19.  TP_HOST: the grammar holds but there are more than 19 significant digits.  TP_BAD: anything else.
TP_HD inline int tp_scan_number(const uint8_t *s, int64_t len, uint64_t &bits, uint64_t &w, int &q, bool &neg) {
    bits = 0; w = 0; q = 0; neg = false;
    if (len == 0 || (len == 2 && s[0] == 'N' && s[1] == 'A')) { bits = TP_NA_BITS; return TP_VALUE; }
    if (len == 3 && s[0] == 'N' && s[1] == 'a' && s[2] == 'N') { bits = TP_NAN_BITS; return TP_VALUE; }
    int64_t i = 0;
    if (s[0] == '+' || s[0] == '-') { neg = s[0] == '-'; i = 1; }
    if (len - i == 3 && s[i] == 'I' && s[i + 1] == 'n' && s[i + 2] == 'f') { bits = TP_INF_BITS | (neg ? TP_SIGN : 0); return TP_VALUE; }
    int nd = 0;
    int64_t frac = 0;
    bool any = false, point = false;
    for (; i < len; ++i) {
        const uint8_t c = s[i];
        if (c >= '0' && c <= '9') {
            any = true;
            if (point) ++frac;
            if (w == 0 && c == '0') {}                       // a leading zero is not significant
            else if (nd < TP_MAX_DIGITS) { w = w * 10 + (uint64_t)(c - '0'); ++nd; }
            else nd = TP_MAX_DIGITS + 1;
        } else if (c == '.' && !point) point = true;
        else break;
    }
    if (!any) return TP_BAD;
    int64_t e10 = 0;
    if (i < len && (s[i] == 'e' || s[i] == 'E')) {
        ++i;
        bool eneg = false;
        if (i < len && (s[i] == '+' || s[i] == '-')) { eneg = s[i] == '-'; ++i; }
        if (i >= len || s[i] < '0' || s[i] > '9') return TP_BAD;
        for (; i < len && s[i] >= '0' && s[i] <= '9'; ++i)
            if (e10 < 100000) e10 = e10 * 10 + (s[i] - '0');
        if (eneg) e10 = -e10;
    }
    if (i != len) return TP_BAD;
    if (nd > TP_MAX_DIGITS) return TP_HOST;
    if (w == 0) { bits = neg ? TP_SIGN : 0; return TP_VALUE; }
    int64_t qq = e10 - frac;
    q = qq < -1000000 ? -1000000 : qq > 1000000 ? 1000000 : (int)qq;
    return TP_DECIMAL;
}

// Is position p the end of a line: a '\n', the end of the text, or the '\r' of a "\r\n" (or of a last line that ends in '\r')?
TP_HD inline bool tp_at_line_end(const uint8_t *text, int64_t n, int64_t p) {
    if (p >= n || text[p] == '\n') return true;
    return text[p] == '\r' && (p + 1 >= n || text[p + 1] == '\n');
}

// One past the last byte of the field that starts at p.
TP_HD inline int64_t tp_field_end(const uint8_t *text, int64_t n, int64_t p, uint8_t sep) {
    while (!tp_at_line_end(text, n, p) && text[p] != sep) ++p;
    return p;
}

TP_HD inline uint64_t tp_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

TP_HD inline double tp_exact_pow10(int k) {                  // 10^k, 0 <= k <= 22: exactly representable
    const double t[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21,
                          1e22};
    return t[k];
}

// The bits of the double nearest to w * 10^q (ties to even), or false when this code cannot certify the rounding.
//
// Exact path (Clinger): w < 2^53 and |q| <= 22.  w and 10^|q| are doubles, so one IEEE multiply or divide rounds once.
//
// Product path: 10^q = (P + d) 2^e with P = floor(10^q / 2^e), 2^127 <= P < 2^128, 0 <= d < 1 (tp_pow10_table.h).  With
// m = w << lz, 2^63 <= m < 2^64, the value is V 2^(e - lz) for V = m (P + d).  X = m P is a 192-bit integer x2 : x1 : x0 and
// X <= V < X + m < X + 2^64, so with H = x2 : x1 = floor(X / 2^64)
//     H <= V / 2^64 < H + 2.
// H has 127 or 128 bits.  Its top 53 bits are the candidate significand M = H >> s (s = 74 or 75), r = H mod 2^s the bits
// that are discarded, so the fraction that decides the rounding, (V / 2^64 - M 2^s) / 2^s, lies in [r, r + 2) / 2^s.
//   r + 2 <= 2^(s-1)                       the fraction is below 1/2: M stands;
//   2^(s-1) + 1 <= r <= 2^s - 3            the fraction is above 1/2 and the value below the next boundary (M + 1) 2^s: M + 1;
//   otherwise                              not certified: r is one of the 3 values at the halfway point or of the 2 at the boundary.
// An exact tie has d = 0, x0 = 0 and r = 2^(s-1), so it is never certified.  The result M' 2^(s + 64 + e - lz) is stored when
// its biased exponent is 1 .. 2046; subnormal results, underflow and overflow are not certified.
TP_HD inline bool tp_convert(uint64_t w, int q, bool neg, uint64_t &bits) {
    const uint64_t sign = neg ? TP_SIGN : 0;
    if (w < (1ull << 53) && q >= -22 && q <= 22) {
        double d = (double)w;
        d = q < 0 ? d / tp_exact_pow10(-q) : d * tp_exact_pow10(q);
        uint64_t b;
        memcpy(&b, &d, sizeof b);
        bits = b | sign;
        return true;
    }
    if (q < TP_K_MIN || q > TP_K_MAX) return false;
    const int lz = __builtin_clzll(w);
    const uint64_t m = w << lz;
    const uint64_t p_hi = tp_pow10_hi[q - TP_K_MIN], p_lo = tp_pow10_lo[q - TP_K_MIN];
    const int e2 = tp_pow10_e[q - TP_K_MIN];
    const uint64_t a_hi = tp_mulhi(m, p_lo), b_lo = m * p_hi, b_hi = tp_mulhi(m, p_hi);
    const uint64_t x1 = a_hi + b_lo, x2 = b_hi + (x1 < a_hi ? 1u : 0u);
    const int sh = 10 + (int)(x2 >> 63);
    uint64_t mant = x2 >> sh;
    const uint64_t mask = (1ull << sh) - 1, r_hi = x2 & mask, r_lo = x1, half_hi = 1ull << (sh - 1);
    if (r_hi < half_hi - 1 || (r_hi == half_hi - 1 && r_lo <= ~0ull - 1)) {}
    else if ((r_hi > half_hi || (r_hi == half_hi && r_lo >= 1)) && !(r_hi == mask && r_lo >= ~0ull - 1)) ++mant;
    else return false;
    int s = 64 + sh;
    if (mant == (1ull << 53)) { mant >>= 1; ++s; }
    const int biased = s + 64 + e2 - lz + 52 + 1023;
    if (biased < 1 || biased > 2046) return false;
    bits = sign | ((uint64_t)biased << 52) | (mant & ((1ull << 52) - 1));
    return true;
}

}  // namespace icnv
