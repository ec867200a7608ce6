// Shared between bayes_api.hip (validation, region classes, stats) and bayes_kernels.hip (K13, the mixture model of the
// HMM-predicted CNV regions: likelihood pass and Gibbs sampler).  DESIGN.md section 4 K13; the contract is in include/icnv.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace icnv {

constexpr int BAYES_MAX_K = 8;          // states of the mixture (i6: 6, i3: 3); more: ICNV_ERR_UNSUPPORTED
constexpr int BAYES_LDS_CELLS = 512;    // undecided cells of a region whose L rows and counts stay in LDS; more stream from L2 / HBM
constexpr int BAYES_PACKED_CELLS = 8;   // at most as many undecided cells (and n_cells > 0): an 8-lane group samples a (region, chain)
constexpr int BAYES_THREADS = 256;

struct BayesRegion {
    int64_t row0;                       // first row of the region's cells in cell_idx / ll / L / freq
    int32_t n_cells;
    int32_t g0, ng;                     // its gene run: rows g0 .. g0 + ng - 1 of the matrix
    int32_t pad;
    uint64_t token;                     // second key word of its random streams
};

struct BayesLoglik {
    const double *x;
    int64_t ld;
    const int32_t *cell_idx;            // [rows] matrix column of every row
    const BayesRegion *regions;
    const int64_t *tile_off;            // [n_regions + 1]: region r's 64-cell tiles are blocks tile_off[r] .. tile_off[r + 1] - 1
    int32_t n_regions, K;
    const double *mu_tau;               // [2 K]: mu | tau
    double *ll, *L;                     // [rows x K]
};

struct BayesSample {
    const double *L;
    const BayesRegion *regions;
    const int32_t *list;                // the regions of this launch
    int32_t n_list, K;
    int32_t n_discard, n_keep;
    uint64_t seed;
    const int32_t *und;                 // [rows]: per region, the positions of its undecided cells (prep kernel)
    const int32_t *n_und;               // [n_regions]
    const int32_t *nfix;                // [n_regions x BAYES_MAX_K]: decided cells per state
    double *theta_sum;                  // [n_regions x K chains x K]
    double *theta_samples;              // nullable [n_regions x K chains x n_keep x K]
    int32_t *freq;                      // [rows x K]
};

int launch_bayes_loglik(const BayesLoglik &a, int64_t n_tiles, hipStream_t s);
// und / n_und / nfix of every region, and freq of the decided cells (= K n_keep at their state); freq is zero on entry
int launch_bayes_prep(const double *L, const BayesRegion *regions, int32_t n_regions, int32_t K, int32_t skip_decided, int32_t n_keep,
                      int32_t *und, int32_t *n_und, int32_t *nfix, int32_t *freq, hipStream_t s);
// lds_cells: 0 = stream L, else the largest n_und of the list (<= BAYES_LDS_CELLS)
int launch_bayes_sample(const BayesSample &a, int32_t lds_cells, hipStream_t s);
// every region of the list has n_cells > 0 and n_und <= BAYES_PACKED_CELLS
int launch_bayes_sample_packed(const BayesSample &a, hipStream_t s);

}  // namespace icnv
