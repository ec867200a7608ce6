// Shared between leiden_pca_api.hip (validation, scratch) and leiden_pca_kernels.hip (K18, the PCA route of the Leiden
// subclustering: .leiden_seurat_preprocess_routine, R/inferCNV_tumor_subclusters.R:699-723).  DESIGN.md section 4 K18.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace icnv {

constexpr int LPCA_MAX_NPCS = 64;             // components of one projection; more: ICNV_ERR_ARG (the route uses <= 10)
constexpr int64_t LPCA_WEIGHT_ONE = 1 << 24;  // the 24-bit fixed-point 1 of the SNN weights (a node's loop)

struct LpProb {                   // one problem of a batch (device array, one entry per problem)
    int64_t cell_off;             // its cells in cell_idx
    int64_t gene_off;             // its genes (features) in gene_idx / mean / sd / v_std
    int64_t z_off;                // its Z block: n_gene rows of ldz doubles
    int64_t m_off;                // its Gram block (n_gene x n_gene) or its V block (n_gene x npcs)
    int64_t e_off;                // its first row in E
    int32_t n, n_gene, ldz, npcs;
};

struct LpArgs {
    const double *x;              // (C, G) expression matrix, a cell's genes contiguous, rows ld apart
    int64_t ld;
    const int32_t *cell_idx, *gene_idx;
    const LpProb *prob;
    int32_t n_prob;
    const double *mean, *sd;      // per (problem, gene)
    double *v_std;                // per (problem, gene)
    double *Z;                    // feature-major blocks
    double *M;                    // Gram blocks
    const double *V;              // eigenvector blocks (n_gene x npcs, row-major)
    double *E;                    // (sum n, e_ld) embeddings
    int32_t e_ld;
};

struct SnnArgs {                  // the SNN graph of a batch of (n, k) kNN blocks
    const int32_t *nn;            // (sum n_p) x k, positions within the problem
    int32_t k, n_prob;
    const int64_t *node_off;      // [n_prob + 1]
    int32_t *t_cnt;               // per node: length of its transposed list; then the fill cursor
    int64_t *t_off;               // per node + 1 per problem: offsets within the problem's region (k n_p entries at k node_off[p])
    int32_t *t_list;              // (sum n_p) x k entries
    int32_t *mark, *touched;      // scratch: n_waves x max n
    int64_t max_n;
    int32_t *row_cnt;             // per node (+ 1): kept entries of its row
    int64_t *row_off;             // [sum n_p + 1], batch-wide
    int32_t *col;                 // outputs of the fill pass
    int32_t *shared;
    int64_t *weight;
    int32_t *loop;                // per node
    uint32_t *bad;                // SNN_BAD_* bits
};

constexpr uint32_t SNN_BAD_RANGE = 1u;    // an nn_idx entry outside [0, n_p)
constexpr uint32_t SNN_BAD_REPEAT = 2u;   // an nn_idx row that repeats an entry

struct LgCheck {                  // device check of a caller's CSR (icnv_leiden_graph_dev)
    const int64_t *node_off, *row_off;
    const int32_t *col, *loop;
    const int64_t *weight;
    int64_t loop_weight;
    int32_t n_prob;
    int64_t *off;                 // per node + 1 per problem: offsets within the problem's edge region
    int64_t *edge_off;            // [n_prob + 1]
    int64_t *strength, *strength_sum;
    uint32_t *bad;
};

int launch_lpca_vstd(const LpArgs &a, int32_t max_genes, hipStream_t s);
int launch_lpca_scale(const LpArgs &a, int32_t max_genes, int32_t max_ldz, hipStream_t s);
int launch_lpca_gram(const LpArgs &a, int32_t max_genes, hipStream_t s);
int launch_lpca_project(const LpArgs &a, int32_t max_n, hipStream_t s);
int snn_blocks(int64_t total_n);
int launch_snn_transpose(const SnnArgs &a, hipStream_t s);
int launch_snn_lists(const SnnArgs &a, hipStream_t s);
int launch_snn_rows(const SnnArgs &a, bool fill, hipStream_t s);
int launch_snn_scan(const SnnArgs &a, int64_t total_n, hipStream_t s);
int launch_lg_check(const LgCheck &c, hipStream_t s);

}  // namespace icnv
