// Shared between de_api.hip (validation, wave planning, exact tables, stats) and de_kernels.hip (K12, the per-gene rank-sum and
// Welch tests of mask_non_DE_genes_basic).  DESIGN.md section 4 K12.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace icnv {

constexpr int DE_CHUNK = 4096;       // segment piece one workgroup sorts in LDS (32 KiB); longer segments merge through HBM
constexpr int DE_EXACT_MAX = 49;     // exact Mann-Whitney p-values for n.x, n.y <= 49 (wilcox.test: n < 50)

// Segments of one sort: `count` segments of `n` keys each, segment s at base + s * n.  Keys are finite or +inf (non-finite
// values and padding), so the finite values of a sorted segment are its prefix.
struct DeSegs {
    int64_t base;
    int32_t n, count;
};

// The exact two-sided p-values min(2 P, 1) of (n.x, n.y) at offset tab_off[(n.x - 1) * 49 + n.y - 1], one per W = 0 .. n.x n.y.
int de_exact_table_host(std::vector<int64_t> &off, std::vector<double> &p);

struct DeGather {                    // one wave: the involved groups' cells, genes g0 .. g0 + gw - 1
    const double *x;
    int64_t ld;
    const int32_t *cell_idx;         // per involved group: its cells at cell_off[k]
    const int64_t *cell_off;
    const int64_t *seg_base;         // per involved group: its segments' first key in `keys` (gene j at + j n_k)
    const int64_t *tile_off;         // per involved group: first tile (64 cells x 64 genes) [n_groups + 1]
    int32_t n_groups, g0, gw;
    int32_t jitter;
    uint64_t seed;
    double *keys;
};

struct DeWilcox {                    // one wave of the merge: comparison k, gene j
    const double *buf[2];
    const int64_t *seg_base;         // per group (as DeGather)
    const int32_t *n;                // per group
    const int8_t *which;             // per group: the buffer its sorted segments ended in
    const int32_t *cmp;              // per comparison: (x group, y group)
    const double *exact_p;           // the exact table (device) and its offsets
    const int64_t *exact_off;
    int32_t n_cmp, g0, gw, G;
    double *stat, *p;                // [n_cmp x G]
    unsigned long long *err;         // min over (k G + g) of an empty sample
};

struct DeWelch {
    const double *x;
    int64_t ld;
    const int32_t *cell_idx;
    const int64_t *cell_off;
    int32_t n_groups, G;
    double *mom;                     // [n_groups x 4 x G]: mean, var, n (non-NaN), has +-Inf
    const int32_t *cmp;
    int32_t n_cmp;
    double *stat, *p;
};

int launch_de_gather(const DeGather &a, int64_t n_tiles, hipStream_t s);
int launch_de_sort_chunks(double *keys, const DeSegs *segs_dev, const int64_t *chunk_off_dev, int32_t n_sets, int64_t n_chunks,
                          hipStream_t s);
int launch_de_merge_pass(const double *src, double *dst, const DeSegs &g, int64_t run, hipStream_t s);
int launch_de_wilcox(const DeWilcox &a, hipStream_t s);
int launch_de_welch(const DeWelch &a, hipStream_t s);
// BH of every comparison row of p [n_cmp x G]; sorted: the rows sorted (+inf for NaN); sm scratch [n_cmp x G]
int launch_de_bh_keys(const double *p, double *keys, int64_t n, hipStream_t s);
int launch_de_bh_finish(const double *p, const double *sorted, double *sm, double *padj, int32_t n_cmp, int32_t G, hipStream_t s);
// mean of the C x G matrix (ld): correctly rounded; part scratch of de_mean_parts() * 3 doubles
int de_mean_parts();
int launch_de_mean(const double *x, int64_t ld, int32_t G, int32_t C, double *part, double *mean_out, hipStream_t s);
struct DeMask {
    const double *x;
    int64_t ld;
    double *out;
    int64_t ld_out;
    int32_t G, C;
    const double *padj;              // [n_cmp x G]
    double thresh;
    const int32_t *base;             // per cell
    const int32_t *cc_off;           // per cell + 1: its comparisons in cc_idx
    const int32_t *cc_idx;
    int32_t n_normal, rule;
    int32_t use_mean;                // 1: the mask value is *mean (device), 0: value
    double value;
    const double *mean;
};
int launch_de_mask(const DeMask &a, hipStream_t s);

}  // namespace icnv
