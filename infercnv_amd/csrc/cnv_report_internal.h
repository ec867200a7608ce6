// Shared between cnv_report_api.hip (validation, the plan of a file, chunk planning) and cnv_report_kernels.hip (K24, the CNV
// region reports as text: per-gene prefix sum, record lengths, scan, emit pass).  DESIGN.md section 4 K24.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace icnv {

constexpr int CR_NT = 256;                 // lanes of a workgroup
constexpr int CR_TILE = 16384;             // bytes of the output one workgroup of the emit pass owns (a multiple of 16)
constexpr int CR_SCAN_NT = 1024;           // lanes of the single workgroup of the two scans

constexpr int CR_GENES = 0, CR_REGIONS = 1;   // ICNV_REPORT_GENES / ICNV_REPORT_REGIONS

// bytes of the decimal text of v: plain digits, `-` in front of a negative number
__host__ __device__ inline int cr_int_len(int64_t v) {
    uint64_t m = v < 0 ? 0 - (uint64_t)v : (uint64_t)v, p = 10;
    int d = 1;
    while (d < 19 && m >= p) { ++d; p *= 10; }
    return d + (v < 0 ? 1 : 0);
}
// state 255 is the library's invalid state, written as -1
__host__ __device__ inline int64_t cr_state_value(int32_t state) { return state == 255 ? -1 : state; }

struct CrArgs {                            // device pointers
    int32_t kind;
    const int32_t *col, *chr, *first, *last, *state, *ordinal;   // [n_rec] the record arrays of icnv_cnv_runs_dev
    int64_t n_rec;
    const uint8_t *grp_b, *chr_b, *gene_b;                       // string tables: entry i is bytes[off[i] .. off[i + 1])
    const int64_t *grp_off, *chr_off, *gene_off;
    const int64_t *gstart, *gend;                                // [G]
    int64_t G;
    int64_t *P;                            // [G + 1] prefix sum of len(gene name) + digits(start) + digits(end)
    int64_t *rec_off;                      // [n_rec + 1] first byte of a record, counted from the first byte of the file's body
    int64_t *line_base;                    // [n_rec + 1] GENES: lines before a record (REGIONS: a record is a line, not used)
    int64_t *rmin, *rmax;                  // [n_rec] REGIONS: min start / max end over the record's genes
};

int launch_cr_gene_prefix(const CrArgs &a, hipStream_t s);
int launch_cr_lengths(const CrArgs &a, hipStream_t s);      // record bytes and lines into rec_off[r + 1] / line_base[r + 1], then the scans
// the bytes [base, base + n_bytes) of the body, which are whole records rec0 .. rec1 - 1, into out[0 .. n_bytes)
int launch_cr_emit(const CrArgs &a, int64_t rec0, int64_t rec1, int64_t base, int64_t n_bytes, uint8_t *out, hipStream_t s);

}  // namespace icnv
