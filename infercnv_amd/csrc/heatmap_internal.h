// Shared between heatmap_api.hip (validation, the radix driver, uploads) and heatmap_kernels.hip (K17, the data layer of
// plot_cnv: exact quantiles without a sort, the colour key's bin counts, the raster panel).  DESIGN.md section 4 K17.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace icnv {

constexpr int HM_NT = 256;                 // lanes of a workgroup
constexpr int HM_PER_LANE = 8;             // values of one lane per chunk
constexpr int HM_CHUNK = HM_NT * HM_PER_LANE;   // values of one chunk: a run of one row
constexpr int HM_DIGIT_BITS = 8;           // radix digit
constexpr int HM_BINS = 1 << HM_DIGIT_BITS;
constexpr int HM_MAX_PROBS = 8;
constexpr int HM_MAX_PREFIX = 2 * HM_MAX_PROBS;   // a probability's lo and hi ranks may part into two bins
constexpr int HM_CAND = 4096;              // candidates the finishing workgroup sorts in LDS (32 KiB)
constexpr int HM_MAX_BREAKS = 257;

// Order-preserving key of a finite double: -0.0 counts as +0.0; a < b  <=>  key(a) < key(b) as unsigned integers.
__host__ __device__ inline uint64_t hm_key(double v) {
    v = v + 0.0;                           // -0.0 + 0.0 = +0.0 (round to nearest); every other value unchanged
    union { double d; uint64_t u; } c;
    c.d = v;
    return (c.u >> 63) ? ~c.u : (c.u | 0x8000000000000000ull);
}
__host__ __device__ inline double hm_unkey(uint64_t k) {
    union { double d; uint64_t u; } c;
    c.u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return c.d;
}

struct HmScan {                            // one pass over the matrix
    const double *x;                       // element (g, c) at x[c * ld + g]
    int64_t ld, G, C;
    int64_t chunks_per_row, n_chunks;
    double exclude;                        // values equal to it (IEEE ==) are skipped; NaN skips nothing
    int32_t n_prefix;                      // tracked prefixes, ascending and distinct (0: every kept value matches, slot 0)
    int32_t match_shift;                   // a key matches prefix j when key >> match_shift == prefix[j]
    int32_t digit_shift;                   // histogram pass: digit = (key >> digit_shift) & 255
    uint64_t prefix[HM_MAX_PREFIX];
    unsigned long long *hist;              // histogram pass: [max(n_prefix, 1)][256] counts
    unsigned long long *summary;           // first pass: {min key, max key, non-finite flag}
    uint64_t *cand;                        // compaction pass: [HM_CAND] keys ...
    uint32_t *n_cand;                      // ... and their count
};

struct HmBins {                            // the binning shared by the colour key's counts and the raster
    const double *x;
    int64_t ld, G;
    const int32_t *rows;                   // device: the cell of list position i
    int64_t n_rows;
    const double *breaks;                  // device [nb]
    int32_t nb;
    uint32_t *flag;                        // set to 1 when a binned value is NaN
    // counts
    int64_t chunks_per_row, n_chunks;
    unsigned long long *counts;            // [nb - 1]
    // raster
    int64_t H, W;
    uint8_t *image;                        // [H * W]
};

int hm_grid(int64_t n_chunks);
int launch_hm_hist(const HmScan &a, bool first, hipStream_t s);
int launch_hm_compact(const HmScan &a, hipStream_t s);
int launch_hm_sort(uint64_t *cand, const uint32_t *n_cand, hipStream_t s);
int launch_hm_bins(const HmBins &a, hipStream_t s);
int launch_hm_raster(const HmBins &a, hipStream_t s);

}  // namespace icnv
