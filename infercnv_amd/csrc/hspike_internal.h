// Shared between hspike_api.hip (validation, chunk planning, uploads) and hspike_kernels.hip (K15, the group gene tables and
// the simulation of the hidden spike-in).  DESIGN.md section 4 K15.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace icnv {

constexpr int HS_CHUNK = 512;        // cells of one group one workgroup sums for its 256 genes
constexpr int HS_SIM_BLOCK = 64;     // one wavefront per workgroup of the simulation: one lane per gene

struct HsChunk {                     // cells cell_idx[begin .. end) of group q
    int32_t q;
    int64_t begin, end;
};

struct HsTables {
    const double *x;
    int64_t ld;
    const int32_t *cell_idx;
    const HsChunk *chunks;           // the chunks of group q are chunk_off[q] .. chunk_off[q + 1] - 1
    const int64_t *chunk_off;
    const int64_t *cell_off;
    int32_t G, n_grp;
    int64_t n_chunks;
    double *part;                    // [n_chunks x 3 x G]: hi, lo of the double-double sum, the plain sum
    int32_t *part_nz;                // [n_chunks x G]
    double *m, *v;                   // [n_grp x G]
    int32_t *nzero;
};

int launch_hs_tables(const HsTables &a, hipStream_t s);

struct HsSpline {                    // device pointers: knots [nk + 4], coef [nk]
    const double *knots, *coef;
    int32_t nk;
    double xmin, range;
};

struct HsSim {
    const double *means;             // [n_mat x n_genes]
    const uint64_t *tokens;          // [n_mat]
    int32_t n_genes, num_cells, n_mat;
    HsSpline var, p0;
    uint64_t seed;
    double *out;                     // [n_mat x num_cells x n_genes]: element (g, c) of matrix k at (k num_cells + c) n_genes + g
};

int launch_hs_simulate(const HsSim &a, hipStream_t s);

}  // namespace icnv
