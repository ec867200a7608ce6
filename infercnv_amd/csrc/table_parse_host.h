// Host side of K21 (include/icnv.h "count matrices from text"): cutting a buffer at whole lines, the extent of a field, the
// strtod path for the fields the device does not certify, the slice of a label, the description of a refused byte offset.
// Plain C++ without HIP, shared by table_parse_api.hip and the stand-alone table_parse_check.cpp.  DESIGN.md section 4 K21.
#pragma once
#include <stdint.h>
#include <cstdlib>
#include <cstring>
#include <string>

#include "table_parse_num.h"

namespace icnv {

// error codes of a refused chunk (the low byte of the device's error word)
constexpr int TP_E_RAGGED = 1, TP_E_NUMBER = 2, TP_E_LABEL = 3;

// Bytes of text[0 .. n) up to and including its last '\n' (0: no whole line).
inline int64_t tp_cut_whole_lines(const uint8_t *text, int64_t n) {
    for (int64_t i = n; i > 0; --i)
        if (text[i - 1] == '\n') return i;
    return 0;
}

// The numeric field at p, read by the host: the grammar of tp_scan_number, then the device's certified conversion where it
// applies and strtod otherwise (strtod alone would take hex floats, blanks and "infinity").  TP_VALUE or TP_BAD.
inline int tp_host_field(const uint8_t *text, int64_t n, int64_t p, uint8_t sep, uint64_t &bits) {
    const int64_t end = tp_field_end(text, n, p, sep);
    uint64_t w;
    int q;
    bool neg;
    const int kind = tp_scan_number(text + p, end - p, bits, w, q, neg);
    if (kind == TP_VALUE || kind == TP_BAD) return kind;
    if (kind == TP_DECIMAL && tp_convert(w, q, neg, bits)) return TP_VALUE;
    const std::string copy(reinterpret_cast<const char *>(text + p), (size_t)(end - p));   // NUL-terminated for strtod
    const double v = std::strtod(copy.c_str(), nullptr);
    std::memcpy(&bits, &v, sizeof bits);
    return TP_VALUE;
}

// The label text[b .. e) without its enclosing quotes.
inline void tp_label_slice(const uint8_t *text, int64_t &b, int64_t &e) {
    if (e - b >= 2 && text[b] == '"' && text[e - 1] == '"') { ++b; --e; }
}

// "line L, field K: <what>: '<bytes>'" for the byte offset a chunk was refused at.  line0: the 1-based file line of the
// chunk's first line.  A ragged row is reported at its first byte, with the number of fields it has.
inline std::string tp_describe(const uint8_t *text, int64_t n, int64_t offset, int code, uint8_t sep, int64_t line0, int64_t n_cols) {
    int64_t line = line0, start = 0;
    for (int64_t i = 0; i < offset && i < n; ++i)
        if (text[i] == '\n') { ++line; start = i + 1; }
    int64_t field = 1, fstart = start;
    for (int64_t i = start; i < offset && i < n; ++i)
        if (text[i] == sep) { ++field; fstart = i + 1; }
    std::string what;
    if (code == TP_E_RAGGED) {
        int64_t count = 1, i = start;
        for (; !tp_at_line_end(text, n, i); ++i)
            if (text[i] == sep) ++count;
        return "line " + std::to_string(line) + ", field " + std::to_string(count) + ": the row has " + std::to_string(count) +
               " fields, " + std::to_string(n_cols + 1) + " are expected (a label and " + std::to_string(n_cols) + " numbers)";
    }
    const int64_t end = tp_field_end(text, n, fstart, sep);
    std::string bytes(reinterpret_cast<const char *>(text + fstart), (size_t)((end - fstart) < 60 ? (end - fstart) : 60));
    what = code == TP_E_LABEL ? "a label may hold a quote only as its first and its last byte" : "not a number of the table grammar";
    return "line " + std::to_string(line) + ", field " + std::to_string(field) + ": " + what + ": '" + bytes + "'";
}

}  // namespace icnv
