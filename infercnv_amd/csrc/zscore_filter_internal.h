// K32: the reference z-score gene filter (include/icnv.h "reference z-score gene filter"): the launch geometry shared by the
// kernels (zscore_filter_kernels.hip) and the entry point (zscore_filter_api.hip).  DESIGN.md section 4 K32.
#pragma once
#include "icnv_internal.h"

namespace icnv {

constexpr int ZS_GENES = 64;      // genes of a workgroup: one per lane of a wavefront, 512 contiguous bytes of a row
constexpr int ZS_WAVES = 4;       // wavefronts of a workgroup: wavefront w takes the list positions w, w + 4, ... of its chunk
constexpr int ZS_NT = ZS_GENES * ZS_WAVES;
constexpr int ZS_CHUNK = 256;     // list positions of a workgroup: the geometry, and so the order of every sum, depends on
                                  // (G, n_ref) alone
constexpr int ZS_FINISH_NT = 256;

enum ZsPass { ZS_SUM = 0, ZS_SQUARES = 1, ZS_ABS_Z = 2 };

inline int64_t zs_chunks(int64_t n_ref) { return (n_ref + ZS_CHUNK - 1) / ZS_CHUNK; }

// One pass over the listed rows: per (chunk, gene) the double-double sum of the pass's term goes to part_hi / part_lo
// [chunk * G + g]; ZS_SUM also writes the largest |value| to part_max.  params (device, 4 doubles): {mean, sd, scale, 0}.
int launch_zscore_pass(int pass, const double *x, int64_t ld, int64_t G, const int32_t *rows_dev, int64_t n_ref, const double *params,
                       double *part_hi, double *part_lo, double *part_max, hipStream_t s);
// The sum of all n_chunks * G partials in one fixed order, by one workgroup: ZS_SUM writes params[0] = mean and params[2] = the
// scale of the squares; ZS_SQUARES writes params[1] = sd.
int launch_zscore_finish_total(int pass, const double *part_hi, const double *part_lo, const double *part_max, int64_t n_part, int64_t n_values,
                               double *params, hipStream_t s);
// row_mean[g] = the sum of gene g's chunks, in chunk order, divided by n_ref and rounded once
int launch_zscore_finish_genes(const double *part_hi, const double *part_lo, int64_t G, int64_t n_chunks, int64_t n_ref, double *row_mean,
                               hipStream_t s);

}  // namespace icnv
