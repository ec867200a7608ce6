// Shared between knn_api.hip (planning, validation, stats) and knn_kernels.hip (K8, the exact kNN).  DESIGN.md section 4 K8.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace icnv {

constexpr int KNN_MAX_K = 128;           // larger k: ICNV_ERR_UNSUPPORTED
constexpr int KNN_DEFAULT_CAP = 256;     // candidates per query row before the row takes the exhaustive pass
constexpr int KNN_MAX_CAP = 1024;
constexpr int KNN_GC = 32;               // genes per LDS stage of the exact sums
constexpr int KNN_SHIFT_CELLS = 256;     // cells whose mean is the per-gene shift of the screen

// device counters (int64) behind icnv_knn_stats
enum { KNN_STAT_CANDIDATES = 0, KNN_STAT_OVERFLOW_ROWS = 1, KNN_STAT_EXACT_ROWS = 2, KNN_STAT_DEVICE_N = 4 };

struct KnnArgs {                 // one call; every pointer is device memory
    const double *x;             // G x C column-major expression matrix
    int32_t G;
    const int32_t *gene_idx;     // packed gene lists
    const int64_t *gene_off;     // [n_prob + 1]
    const int32_t *cell_idx;     // packed cell lists
    const int64_t *cell_off;     // [n_prob + 1]; query row = position in the packed cell lists
    int32_t n_prob, k;
    int64_t total_genes, total_rows;
    double *shift;               // [total_genes]
    double *Y;                   // compact centred cells: problem p at y_off[p], one row of ld[p] doubles per cell
    const int64_t *y_off;
    const int32_t *ld;           // G_p rounded up to even
    double *norm;                // [total_rows] ||y_i||^2
    int32_t *nn_idx;             // [total_rows * k]
    double *nn_dist;             // [total_rows * k]
    int64_t *stats;              // [KNN_STAT_DEVICE_N]
};

struct KnnBlock {                // one row block: pieces = (problem, rows [r0, r0 + nr)) against all n_p cells of the problem
    int32_t n_pieces;
    const int32_t *piece_prob, *piece_r0, *piece_nr;
    const int64_t *tile_off;     // [n_pieces + 1] screen tiles
    const int64_t *row_off;      // [n_pieces + 1] query rows of the block
    const int64_t *piece_scr;    // [n_pieces] offset of the piece's n_r x n_p entries (8 bytes each) in `screen`
    int64_t n_tiles, n_rows;
    uint32_t *screen;            // per row: n_p upper keys, n_p lower keys -- or n_p exact d2 (exhaustive pass)
    int32_t *cand;               // [n_rows * cap]
    int32_t *ncand;              // [n_rows]
    int32_t cap;
    int32_t all_exact;           // every row through the exhaustive pass (ICNV_KNN_EXHAUSTIVE)
};

int launch_knn_prepare(const KnnArgs &a, hipStream_t s);
int launch_knn_block(const KnnArgs &a, const KnnBlock &b, int wm, hipStream_t s);
size_t knn_refine_lds_bytes(int cap);

}  // namespace icnv
