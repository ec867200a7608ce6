// Shared between hclust_api.hip (validation, planning, R labelling, stats), hclust_kernels.hip (K9, the nearest-neighbour
// chain of hclust) and random_trees_api.hip (K10 clusters its trees with K9's host helpers).  DESIGN.md section 4 K9.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "icnv_internal.h"

namespace icnv {

// LDS path: the condensed matrix (n (n-1) / 2 doubles), the chain, the sizes and the active bitmask of one problem in the
// 160 KiB of one workgroup.  201 cells would still fit (162 436 B); 200 is the documented limit.
constexpr int HC_LDS_MAX_N = 200;
constexpr size_t hc_lds_bytes(int n) { return (size_t)n * (n - 1) / 2 * 8 + (size_t)n * 8 + ((size_t)n + 31) / 32 * 4; }
static_assert(hc_lds_bytes(HC_LDS_MAX_N) + 256 <= 160 * 1024, "the LDS path must fit one workgroup");
// HBM path: the active bitmask stays in LDS (n / 8 bytes <= 64 KiB)
constexpr int HC_HBM_MAX_N = 1 << 19;

struct HclustArgs {           // one launch; every pointer is device memory
    int32_t n_run;            // problems of this launch (one workgroup each)
    const int32_t *run;       // [n_run] problem ids
    const int32_t *n;         // per problem: cells
    const int64_t *d_off;     // per problem: its n x n row-major matrix at D + d_off[p]
    double *D;                // mutated by the HBM path, read by the LDS path
    const int64_t *m_off;     // per problem: its n - 1 raw merges (= cell offset - p)
    int32_t *mx, *my;         // raw merges in chain order: positions x < y (the cluster lives on at y) ...
    double *mh;               // ... and their dissimilarity (squared distances for ward.D2)
    const int64_t *c_off;     // per problem: cell offset; HBM path: chain at work + 2 c_off[p], sizes after it
    int32_t *work;
    int64_t *steps;           // per problem: chain steps
    int32_t method;           // ICNV_HCLUST_*
};

int launch_hclust_prep(double *D, int64_t total, bool square, uint32_t *bad, hipStream_t s);
int launch_hclust_lds(const HclustArgs &a, int max_n, hipStream_t s);
int launch_hclust_hbm(const HclustArgs &a, int max_n, hipStream_t s);

// ---- host helpers of hclust_api.hip that K10 (random_trees_api.hip) calls too ----
// The raw merges of a batch of problems, left on the device (K9's chain; K10 keeps only the maximum of most trees).
struct HclustRaw {
    DevBuf d_n, d_moff, d_mx, d_my, d_mh;   // per problem: cells, first raw merge; the raw merges in chain order
    std::vector<int64_t> m_off;
    int n_lds = 0, n_hbm = 0;
    int64_t steps = 0;
};
int hclust_method_check(int32_t method);
void hclust_label(int n, const int32_t *rx, const int32_t *ry, const double *rh, bool root, int32_t *merge, double *height,
                  int32_t *order);
int hclust_raw(double *D, const std::vector<int32_t> &n, const std::vector<int64_t> &c_off, int32_t method, hipStream_t s,
               HclustRaw &out);

}  // namespace icnv
