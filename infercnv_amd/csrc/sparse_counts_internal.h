// Shared between sparse_counts_api.hip (validation, the order of the passes, the text of a refusal; K22's entries and K26's) and
// sparse_counts_kernels.hip (K22, sparse count matrices: the triplet parser, the CSC builder, the CSC selector).
// The grammar of one triplet line lives here as plain C++ that compiles for the device and for the host, so that the
// kernel and the refusal text of the entry read a line with the same code.  DESIGN.md section 4 K22.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>

#include "table_parse_num.h"

namespace icnv {

constexpr int SC_NT = 256;                 // lanes of a workgroup
constexpr int SC_BYTES = 16;               // text positions of one lane of the structure passes
constexpr int SC_SEG = SC_NT * SC_BYTES;   // text positions of one workgroup: a segment
constexpr int SC_SCAN_ITEMS = 8;           // counts of one lane of the selector's column scan
constexpr int SC_SCAN_TILE = SC_NT * SC_SCAN_ITEMS;
constexpr int SC_KEEP_STEPS = 8;           // steps of SC_NT staged entries one workgroup of the K26 compaction looks at
constexpr int SC_KEEP_TILE = SC_NT * SC_KEEP_STEPS;
constexpr uint64_t SC_NO_ERROR = ~0ull;
constexpr unsigned long long SC_NO_VIOLATION = ~0ull;

// the `field` of a MatrixMarket banner (ICNV_MM_* of include/icnv.h)
constexpr int SC_MM_INTEGER = 0, SC_MM_REAL = 1, SC_MM_PATTERN = 2;
// error codes of a refused chunk (the low byte of the error word; the offset above it is the field's first byte, for
// SC_E_FIELDS and SC_E_COMMENT the line's first byte)
constexpr int SC_E_FIELDS = 1, SC_E_INDEX = 2, SC_E_VALUE = 3, SC_E_COMMENT = 4;
// error codes of the selector (the low byte; the position in the list above it)
constexpr int SC_E_CELL = 1, SC_E_GENE = 2;

TP_HD inline bool sc_blank(uint8_t c) { return c == ' ' || c == '\t'; }

// The first position at or after p that is not a blank.
TP_HD inline int64_t sc_skip_blanks(const uint8_t *text, int64_t n, int64_t p) {
    while (p < n && sc_blank(text[p])) ++p;
    return p;
}

// Is the line that starts at p empty, a lone '\r' or only blanks (followed by its line end)?
TP_HD inline bool sc_blank_line(const uint8_t *text, int64_t n, int64_t p) { return tp_at_line_end(text, n, sc_skip_blanks(text, n, p)); }

// One past the last byte of the token that starts at p (p is not a blank and not a line end).
TP_HD inline int64_t sc_token_end(const uint8_t *text, int64_t n, int64_t p) {
    while (!tp_at_line_end(text, n, p) && !sc_blank(text[p])) ++p;
    return p;
}

// An index field text[p .. e): a plain unsigned decimal of at most 10 digits in 1 .. limit.  Stored 0-based.
TP_HD inline bool sc_index(const uint8_t *text, int64_t p, int64_t e, int64_t limit, int32_t &out) {
    if (e - p < 1 || e - p > 10) return false;
    int64_t v = 0;
    for (int64_t i = p; i < e; ++i) {
        if (text[i] < '0' || text[i] > '9') return false;
        v = v * 10 + (text[i] - '0');
    }
    if (v < 1 || v > limit) return false;
    out = (int32_t)(v - 1);
    return true;
}

// Is w * 10^q (w >= 1) an integer in 0 .. 2^31 - 1?  Exact integer arithmetic.
TP_HD inline bool sc_exact_count(uint64_t w, int q, int32_t &out) {
    uint64_t v = w;
    if (q >= 0) {
        for (int i = 0; i < q; ++i) {
            v *= 10;
            if (v > 0x7fffffffull) return false;               // v <= 2^31 * 10 here: no overflow
        }
    } else {
        if (q < -19) return false;                             // w < 10^19 is not a multiple of 10^20
        uint64_t d = 1;
        for (int i = 0; i < -q; ++i) d *= 10;                  // 10^19 < 2^64
        if (w % d) return false;
        v = w / d;
    }
    if (v > 0x7fffffffull) return false;
    out = (int32_t)v;
    return true;
}

// A value field text[p .. e): K21's grammar (tp_scan_number), accepted when the double nearest to the field is an integer
// in 0 .. 2^31 - 1.  A field whose exact value w * 10^q is such an integer is its own double and is taken by integer
// arithmetic, whatever its spelling (9.600000000000000e+01 has a 16-digit significand above 2^53, which K21 hands to the
// host).  Any other field goes through K21's certified conversion (2147483646.999999999 rounds to 2147483647); what that
// cannot certify is refused -- within 19 digits no such field rounds to an integer.  More than 19 digits: refused.
TP_HD inline bool sc_value(const uint8_t *text, int64_t p, int64_t e, int32_t &out) {
    if (e - p < 1 || e - p > TP_MAX_SCAN) return false;
    uint64_t bits, w;
    int q;
    bool neg;
    int kind = tp_scan_number(text + p, e - p, bits, w, q, neg);
    if (kind == TP_DECIMAL) {
        if (sc_exact_count(w, q, out)) return !neg;            // a negative count is refused
        kind = tp_convert(w, q, neg, bits) ? TP_VALUE : TP_BAD;
    }
    if (kind != TP_VALUE) return false;
    if (bits == 0) { out = 0; return true; }                  // +0; -0 carries a sign and is refused with the negatives
    if (bits >> 63) return false;
    const int ex = (int)(bits >> 52) - 1023;                  // NA, NaN and Inf have ex = 1024
    if (ex < 0 || ex > 30) return false;
    const uint64_t m = (bits & ((1ull << 52) - 1)) | (1ull << 52);
    if (m & ((1ull << (52 - ex)) - 1)) return false;          // a fraction
    out = (int32_t)(m >> (52 - ex));
    return true;
}

// One line of the body, starting at its first byte p (not a blank line).  Returns 0 and the entry, or the error code with
// `at` the offset the refusal is reported at: the line's first byte for a field count or a comment, else the field's.
TP_HD inline int sc_parse_line(const uint8_t *text, int64_t n, int64_t p, int field, int64_t G, int64_t C, int32_t &row, int32_t &col,
                               int32_t &val, int64_t &at) {
    const int want = field == SC_MM_PATTERN ? 2 : 3;
    int64_t tok[3], end[3];
    int count = 0;
    int64_t q = sc_skip_blanks(text, n, p);
    at = p;
    if (q < n && text[q] == '%') return SC_E_COMMENT;
    while (!tp_at_line_end(text, n, q)) {
        const int64_t e = sc_token_end(text, n, q);
        if (count < 3) { tok[count] = q; end[count] = e; }
        ++count;
        if (count > want) return SC_E_FIELDS;
        q = sc_skip_blanks(text, n, e);
    }
    if (count != want) return SC_E_FIELDS;
    if (!sc_index(text, tok[0], end[0], G, row)) { at = tok[0]; return SC_E_INDEX; }
    if (!sc_index(text, tok[1], end[1], C, col)) { at = tok[1]; return SC_E_INDEX; }
    val = 1;
    if (want == 3 && !sc_value(text, tok[2], end[2], val)) { at = tok[2]; return SC_E_VALUE; }
    return 0;
}

// (host) the text of a refusal of the triplet parsers
// "line L, field K: <what>: '<bytes>'" for the error word of a refused chunk, read from the host copy of the text with the
// grammar the kernel read it with.  SC_E_FIELDS and SC_E_COMMENT are reported at the line's first byte, K the line's number
// of fields (1 for a comment) and the bytes the line's; the others at the field's first byte.
inline std::string sc_describe(const uint8_t *text, int64_t n, uint64_t word, int field, int64_t G, int64_t C, int64_t line0) {
    const int64_t offset = (int64_t)(word >> 8);
    const int code = (int)(word & 0xff);
    int64_t line = line0, start = 0;
    for (int64_t i = 0; i < offset && i < n; ++i)
        if (text[i] == '\n') { ++line; start = i + 1; }
    int64_t k = 0, tokens = 0, b = offset, e = offset;
    for (int64_t q = sc_skip_blanks(text, n, start); !tp_at_line_end(text, n, q);) {
        const int64_t te = sc_token_end(text, n, q);
        ++tokens;
        if (q == offset) { k = tokens; e = te; }
        q = sc_skip_blanks(text, n, te);
    }
    std::string what;
    if (code == SC_E_FIELDS || code == SC_E_COMMENT) {
        k = code == SC_E_COMMENT ? 1 : tokens;
        b = start;
        for (e = start; !tp_at_line_end(text, n, e);) ++e;
        what = code == SC_E_COMMENT ? "a comment line inside the body"
                                    : std::to_string(tokens) + " fields where " + std::to_string(field == SC_MM_PATTERN ? 2 : 3) + " are expected";
    } else if (code == SC_E_INDEX) {
        what = "not an index in 1 .. " + std::to_string(k == 1 ? G : C);
    } else {
        what = "not an integer count in 0 .. 2147483647";
    }
    const std::string bytes(reinterpret_cast<const char *>(text + b), (size_t)((e - b) < 60 ? (e - b) : 60));
    return "line " + std::to_string(line) + ", field " + std::to_string(k) + ": " + what + ": '" + bytes + "'";
}

struct ScParseArgs {
    const uint8_t *text;                   // device, 16-byte aligned, n bytes
    int64_t n;                             // 1 .. 2^31 - 2
    int field;                             // SC_MM_*
    int64_t G, C;
    int64_t n_seg;                         // segments covering the positions 0 .. n - 1
    uint32_t *seg_count;                   // [n_seg] entries (non-blank lines) that start in the segment
    uint32_t *seg_off;                     // [n_seg] exclusive scan
    uint32_t *total;                       // [1]
    int64_t n_entries;                     // known on the host after the structure pass
    uint32_t *line_pos;                    // [n_entries] first byte of the line of entry k
    unsigned long long *error;             // offset << 8 | code, the smallest wins; SC_NO_ERROR
    int32_t *row, *col, *val;              // [n_entries] staged; copied to the caller's arrays when nothing was refused
};

struct ScSelectArgs {
    const int64_t *colptr;                 // [C + 1] source
    const int32_t *rowidx, *vals;
    int64_t G, C, nnz;
    const int32_t *gene_map;               // [G] new row or -1
    int64_t n_genes_out;
    const int32_t *cells;                  // [n_cells] source columns
    int64_t n_cells;
    int64_t *counts;                       // [n_cells] kept entries per output column
    int64_t *tile_sum;                     // [tiles] then its exclusive scan
    int64_t *colptr_out;                   // [n_cells + 1]
    int32_t *rowidx_out, *vals_out;
    unsigned long long *error;             // position << 8 | code, the smallest wins
};

int launch_sc_structure(const ScParseArgs &a, hipStream_t s);   // seg_count, seg_off, total
int launch_sc_index(const ScParseArgs &a, hipStream_t s);       // line_pos
int launch_sc_parse(const ScParseArgs &a, hipStream_t s);       // row, col, val (staged), error
int launch_sc_build(const int32_t *row, const int32_t *col, int64_t nnz, int64_t G, int64_t C, unsigned long long *violation,
                    int64_t *colptr, bool write, hipStream_t s);
int launch_sc_check_maps(const ScSelectArgs &a, hipStream_t s);
int launch_sc_select_count(const ScSelectArgs &a, hipStream_t s);   // counts, colptr_out
int launch_sc_select_fill(const ScSelectArgs &a, hipStream_t s);

// K26, the column-selected triplet parser (triplets_cols_kernels.hip): the stable compaction of the staged entries
struct ScKeepArgs {
    const int32_t *row, *col, *val;        // [n_entries] staged by launch_sc_parse
    int64_t n_entries;
    const int32_t *col_map;                // [C] output column or -1
    int64_t C;
    uint32_t *block_count, *block_off;     // [tiles of SC_KEEP_TILE entries] kept entries, their exclusive scan
    uint32_t *total;                       // [1]
    int32_t *row_out, *col_out, *val_out;  // the caller's arrays
};
int launch_sc_keep_count(const ScKeepArgs &a, hipStream_t s);   // block_count, block_off, total
int launch_sc_keep_fill(const ScKeepArgs &a, hipStream_t s);

}  // namespace icnv
