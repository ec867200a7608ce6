#!/usr/bin/env python3
"""Generate tp_pow10_table.h: the 128-bit normalised powers of ten of the table reader (K21, table_parse_num.h), and hold the
Python-integer model of the reader's number arithmetic.

  python infercnv_amd/csrc/gen_parse_pow10_table.py            # writes infercnv_amd/csrc/tp_pow10_table.h (the Makefile does)
  python infercnv_amd/csrc/gen_parse_pow10_table.py --check    # verifies the built header
  (--out PATH: another file than infercnv_amd/csrc/tp_pow10_table.h; the tests write and check their own copy)

For every k in K_MIN .. K_MAX the header holds  P_k = floor(10^k / 2^e_k)  with  2^127 <= P_k < 2^128  (two 64-bit words) and
e_k.  All arithmetic here is exact Python integers.

The model (scan_field, convert, model_field) restates table_parse_num.h operation for operation: the grammar of a field, the
exact path (one correctly rounded multiply or divide of two exactly representable doubles, which Python's float does as the
device does) and the certified product with P_k.  tests/test_table_parse_host.py compares every result the model certifies with
float(): the model may decline, it may never certify another value.
"""
import os
import struct
import sys

K_MIN, K_MAX = -342, 308
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "tp_pow10_table.h")

NA_BITS = 0x7FF00000000007A2        # R's NA_real_
NAN_BITS = 0x7FF8000000000000
INF_BITS = 0x7FF0000000000000
SIGN = 1 << 63
MAX_DIGITS = 19
MAX_SCAN = 40                       # TP_MAX_SCAN: longer fields go to the host unread
M64 = (1 << 64) - 1


def entry(k):
    """(P, e): P = floor(10^k * 2^-e), 2^127 <= P < 2^128."""
    if k >= 0:
        v = 10 ** k
        e = v.bit_length() - 128
        p = v >> e if e >= 0 else v << -e
    else:
        d = 10 ** -k
        e = -(d.bit_length() + 127)
        p = (1 << -e) // d
        if p >= 1 << 128:
            e += 1
            p = (1 << -e) // d
    assert (1 << 127) <= p < (1 << 128), k
    return p, e


TABLE = [entry(k) for k in range(K_MIN, K_MAX + 1)]


def bits_of(x):
    return struct.unpack("<q", struct.pack("<d", x))[0] & M64


# ---- the model ---------------------------------------------------------------------------------------------------------------
def scan_field(s):
    """tp_scan_number: ("value", bits) | ("decimal", w, q, neg) | ("host",) | ("bad",) for the bytes of one numeric field."""
    n = len(s)
    if n == 0 or s == b"NA":
        return ("value", NA_BITS)
    if s == b"NaN":
        return ("value", NAN_BITS)
    i, neg = 0, False
    if s[0] in b"+-":
        neg = s[0] == ord("-")
        i = 1
    if s[i:] == b"Inf":
        return ("value", INF_BITS | (SIGN if neg else 0))
    w = nd = frac = 0
    any_digit = point = False
    while i < n:
        c = s[i]
        if 48 <= c <= 57:
            any_digit = True
            if point:
                frac += 1
            if w == 0 and c == 48:
                pass                                   # a leading zero is not significant
            elif nd < MAX_DIGITS:
                w = w * 10 + (c - 48)
                nd += 1
            else:
                nd += 1
        elif c == 46 and not point:
            point = True
        else:
            break
        i += 1
    if not any_digit:
        return ("bad",)
    e10 = 0
    if i < n and s[i] in b"eE":
        i += 1
        eneg = False
        if i < n and s[i] in b"+-":
            eneg = s[i] == ord("-")
            i += 1
        if i >= n or not 48 <= s[i] <= 57:
            return ("bad",)
        while i < n and 48 <= s[i] <= 57:
            if e10 < 100000:
                e10 = e10 * 10 + (s[i] - 48)
            i += 1
        if eneg:
            e10 = -e10
    if i != n:
        return ("bad",)
    if nd > MAX_DIGITS:
        return ("host",)
    if w == 0:
        return ("value", SIGN if neg else 0)
    return ("decimal", w, e10 - frac, neg)


def convert(w, q, neg):
    """tp_convert: the bits of the double nearest to w * 10^q, or None when the rounding is not certified."""
    sign = SIGN if neg else 0
    if w < (1 << 53) and -22 <= q <= 22:
        d = float(w)
        d = d / float(10 ** -q) if q < 0 else d * float(10 ** q)      # 10^|q| <= 10^22 is a double; one rounding
        return bits_of(d) | sign
    if q < K_MIN or q > K_MAX:
        return None
    lz = 64 - w.bit_length()
    m = (w << lz) & M64
    p, e2 = TABLE[q - K_MIN]
    p_hi, p_lo = p >> 64, p & M64
    a_hi = (m * p_lo) >> 64
    b = m * p_hi
    b_lo, b_hi = b & M64, b >> 64
    x1 = (a_hi + b_lo) & M64
    x2 = (b_hi + (1 if x1 < a_hi else 0)) & M64
    top = x2 >> 63
    sh = 10 + top
    mant = x2 >> sh
    r_hi = x2 & ((1 << sh) - 1)
    r_lo = x1
    half_hi = 1 << (sh - 1)
    if r_hi < half_hi - 1 or (r_hi == half_hi - 1 and r_lo <= M64 - 1):
        up = 0
    elif (r_hi > half_hi or (r_hi == half_hi and r_lo >= 1)) and not (r_hi == (1 << sh) - 1 and r_lo >= M64 - 1):
        up = 1
    else:
        return None
    mant += up
    s = 64 + sh
    if mant == 1 << 53:
        mant >>= 1
        s += 1
    biased = s + 64 + e2 - lz + 52 + 1023
    if biased < 1 or biased > 2046:
        return None
    return sign | (biased << 52) | (mant & ((1 << 52) - 1))


def model_field(s):
    """What the device does with the bytes of one numeric field: ("value", bits), ("host",) or ("bad",)."""
    if len(s) > MAX_SCAN:
        return ("host",)
    r = scan_field(s)
    if r[0] != "decimal":
        return r
    bits = convert(*r[1:])
    return ("host",) if bits is None else ("value", bits)


def expected_bits(s):
    """float() of a field of the grammar, with R's NA for `NA` and the empty field."""
    if s in (b"", b"NA"):
        return NA_BITS
    if s == b"NaN":
        return NAN_BITS
    return bits_of(float(s.decode("ascii")))


def render():
    lines = ["// Generated by gen_parse_pow10_table.py -- do not edit.  P_k = floor(10^k / 2^e_k), 2^127 <= P_k < 2^128, for",
             "// k = TP_K_MIN .. TP_K_MAX: tp_pow10_hi / tp_pow10_lo are its two 64-bit words, tp_pow10_e is e_k.  DESIGN.md section 4 K21.",
             "#pragma once",
             "#include <stdint.h>",
             "",
             f"#define TP_K_MIN ({K_MIN})",
             f"#define TP_K_MAX ({K_MAX})",
             "",
             "#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__",
             "#define TP_TABLE_QUAL __device__",
             "#else",
             "#define TP_TABLE_QUAL",
             "#endif",
             ""]
    for name, ctype, fmt in (("tp_pow10_hi", "uint64_t", lambda e: "0x%016xull" % (e[0] >> 64)),
                             ("tp_pow10_lo", "uint64_t", lambda e: "0x%016xull" % (e[0] & M64)),
                             ("tp_pow10_e", "int16_t", lambda e: "%d" % e[1])):
        per = 4 if ctype == "uint64_t" else 16
        lines.append(f"TP_TABLE_QUAL static const {ctype} {name}[{len(TABLE)}] = {{")
        for i in range(0, len(TABLE), per):
            lines.append("    " + ", ".join(fmt(e) for e in TABLE[i:i + per]) + ",")
        lines.append("};")
        lines.append("")
    return "\n".join(lines)


def main():
    text = render()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else OUT
    if "--check" in sys.argv:
        if not os.path.exists(out) or open(out).read() != text:
            print(f"{out} is stale: run gen_parse_pow10_table.py")
            return 1
        print(f"{out} is up to date")
        return 0
    with open(out, "w") as f:
        f.write(text)
    print("wrote", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
