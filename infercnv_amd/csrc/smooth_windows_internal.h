// Shared between smooth_windows_api.hip (validation, the tile plan, uploads) and smooth_windows_kernels.hip (K16, the banded
// window operator behind smooth_method = "runmeans" and "coordinates").  DESIGN.md section 4 K16.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace icnv {

constexpr int SW_NT = 256;           // lanes of a workgroup
constexpr int SW_U = 4;              // adjacent output genes of one lane: the rows their windows share are read once
constexpr int SW_CB = 4;             // cells of one workgroup: a weight is fetched once for all of them
constexpr int SW_TILE = SW_NT * SW_U;        // output genes of a full tile
constexpr int SW_MIN_TILE = SW_NT;           // a tile whose span does not fit is halved down to this many genes, then spilled
constexpr int SW_LDS_ROWS = 1280;    // staged rows per cell, skew included: 4 x 1280 x 8 B = 40 KiB, four workgroups per CU
// row r of the staged span sits at r + r / 32: the lanes of a 32-lane group read rows 4 apart, which would share 8 of the 32
// bank pairs without the skew
__host__ __device__ inline int sw_skew(int r) { return r + (r >> 5); }

struct SwTile {                      // output genes [g0, g1); staged rows [span_lo, span_lo + span_len) (unused when spilled)
    int32_t g0, g1, span_lo, span_len;
};

struct SwArgs {
    const double *x;                 // element (g, c) at x[c * ldx + g]
    double *out;                     // element (g, c) at out[c * ldo + g]
    int64_t ldx, ldo, C;
    const int32_t *lo, *len;         // [G]
    const int64_t *w_off;            // [G + 1], null without weights
    const double *w;                 // null: all ones
    const double *denom;             // [G]
    const SwTile *tiles;             // LDS tiles first, then the spilled ones
    int32_t n_lds, n_spill;
    uint32_t *flag;                  // set to 1 when a staged or summed value is not finite
};

int launch_smooth_windows(const SwArgs &a, hipStream_t s);

}  // namespace icnv
