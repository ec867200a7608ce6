// Shared between leiden_api.hip (validation, scratch, stats) and leiden_kernels.hip (K11, the Leiden community detection of
// the Leiden subclustering).  DESIGN.md section 4 K11.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "lib_math.h"

namespace icnv {

constexpr int LEIDEN_MAX_K = 128;          // larger k: ICNV_ERR_UNSUPPORTED (K8's own limit)
constexpr int LEIDEN_MAX_ITERATIONS = 1000;
constexpr int LEIDEN_MAX_LEVELS = 512;     // levels of one iteration; more: ICNV_ERR_UNSUPPORTED
// queue pops of one move phase over n nodes; more: ICNV_ERR_UNSUPPORTED
__host__ __device__ constexpr int64_t leiden_move_cap(int64_t n) { return 256 * n + 1024; }

// per-problem status words written by the kernels
enum { LEIDEN_OK = 0, LEIDEN_MOVE_CAP = 1, LEIDEN_LEVEL_CAP = 2, LEIDEN_INTERNAL = 3 };
// per-problem counters (int64) written by leiden_kernel
enum { LEIDEN_CNT_LEVELS = 0, LEIDEN_CNT_MOVE = 1, LEIDEN_CNT_REFINE = 2, LEIDEN_CNT_DRAWS = 3, LEIDEN_CNT_N = 4 };

struct LeidenGraph {              // the graphs of a batch: problem p's nodes at node_off[p], its CSR offsets at node_off[p] + p
    const int32_t *nn;            // (sum n_p) x k, positions within the problem
    int32_t k, n_prob;
    const int64_t *node_off;      // [n_prob + 1]
    int64_t *off;                 // CSR offsets within the problem's edge region (edge region of p at 2 k node_off[p])
    int32_t *col;                 // neighbours, ascending, positions within the problem
    int64_t *strength;            // [sum n_p]
    int64_t *strength_sum;        // [n_prob]
    int32_t *raw;                 // scratch: 2 k per node
    int64_t *raw_off;             // scratch: per node + 1 per problem
    int32_t *cnt, *loop;          // scratch: per node
    uint32_t *bad;                // nn_idx entry out of range (check kernel)
};

struct LeidenArgs {               // one call; every pointer device memory, per-node arrays indexed like the graph
    LeidenGraph g;
    const int64_t *edge_off;      // [n_prob] first entry of problem p's edge region (null: 2 k node_off[p])
    const int64_t *ew0;           // level-0 edge weights, indexed like g.col (null: every weight 1)
    int64_t total_e;              // entries of all edge regions together: the stride of the A / B edge arrays
    int32_t objective;            // ICNV_LEIDEN_CPM / ICNV_LEIDEN_MODULARITY
    const double *r;              // [n_prob] resolution (gamma, or gamma / sum s for modularity)
    double beta;
    int32_t n_iterations;
    uint64_t seed;
    const uint64_t *token;        // [n_prob]
    int64_t *i64;                 // 7 per-node arrays: W, acc, Wr, ext, wA, wB, T
    int64_t *offs;                // 2 offset arrays (per node + 1 per problem): A, B
    int32_t *i32;                 // LEIDEN_I32_ARRAYS per-node arrays
    double *cum;                  // per node
    int32_t *nbr;                 // 2 edge arrays (total_e entries each): A, B
    int64_t *ew;                  // 2 edge weight arrays: A, B
    int64_t total_n;
    int32_t *membership;          // [sum n_p] 1-based
    int32_t *n_clusters;          // [n_prob]
    int32_t *status;              // [n_prob]
    int64_t *counters;            // [n_prob * LEIDEN_CNT_N]
};
constexpr int LEIDEN_I64_ARRAYS = 7;
constexpr int LEIDEN_I32_ARRAYS = 17;

int launch_leiden_check(const LeidenGraph &g, hipStream_t s);
int launch_leiden_graph(const LeidenGraph &g, hipStream_t s);
int launch_leiden(const LeidenArgs &a, hipStream_t s);

}  // namespace icnv
