// C ABI of K18 (include/icnv.h "PCA route of the Leiden subclustering"): validation, the problems' descriptors and the
// scratch of the SNN graph.  Kernels: leiden_pca_kernels.hip.  icnv_leiden_graph_dev lives in leiden_api.hip with K11's run.
// DESIGN.md section 4 K18.
#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "icnv_internal.h"
#include "leiden_internal.h"
#include "leiden_pca_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

namespace {

int lists_validate(const char *who, const int32_t *idx, const int32_t *off, int32_t n_prob, int64_t limit, const char *what) {
    const std::string w = std::string(who) + ": ";
    if (!idx || !off) ICNV_FAIL(ICNV_ERR_ARG, w + "null argument");
    if (off[0] != 0) ICNV_FAIL(ICNV_ERR_ARG, w + "offsets must start at 0");
    for (int32_t p = 0; p < n_prob; ++p)
        if (off[p + 1] <= off[p]) ICNV_FAIL(ICNV_ERR_ARG, w + "problem " + std::to_string(p) + " has no " + what);
    for (int64_t i = 0; i < off[n_prob]; ++i)
        if (idx[i] < 0 || idx[i] >= limit) ICNV_FAIL(ICNV_ERR_ARG, w + what + " index out of range");
    return ICNV_OK;
}

// the checks shared by the two entry points that read the expression matrix
int matrix_validate(const char *who, const void *expr, int64_t G, int64_t C, int64_t ld, const int32_t *gene_idx, const int32_t *gene_off,
                    const int32_t *cell_idx, const int32_t *cell_off, int32_t n_prob) {
    const std::string w = std::string(who) + ": ";
    if (!expr) ICNV_FAIL(ICNV_ERR_ARG, w + "null argument");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff || ld < G) ICNV_FAIL(ICNV_ERR_ARG, w + "bad matrix dimensions");
    if (n_prob < 1 || n_prob > 65535) ICNV_FAIL(ICNV_ERR_ARG, w + "n_prob must be in 1 .. 65535");
    int rc = lists_validate(who, gene_idx, gene_off, n_prob, G, "gene");
    if (rc || (rc = lists_validate(who, cell_idx, cell_off, n_prob, C, "cell"))) return rc;
    return ICNV_OK;
}

int ldz_of(int32_t n) { return n + (n & 1); }

// after the argument checks, before the first allocation: without a device the call is ICNV_ERR_HIP, not an allocation failure
int need_device() {
    int n = 0;
    ICNV_HIP(hipGetDeviceCount(&n));
    if (n < 1) ICNV_HIP(hipErrorNoDevice);
    return ICNV_OK;
}

struct Batch {                    // the descriptors of a batch on the device
    std::vector<LpProb> prob;
    DevBuf d_prob, d_gene, d_cell;
    int32_t max_genes = 0, max_n = 0, max_ldz = 0;
};

int batch_sizes(const char *who, const int32_t *n_feat, const int32_t *n_cells, const int32_t *npcs, int32_t n_prob, Batch &b) {
    const std::string w = std::string(who) + ": ";
    if (!n_feat || !n_cells) ICNV_FAIL(ICNV_ERR_ARG, w + "null argument");
    if (n_prob < 1 || n_prob > 65535) ICNV_FAIL(ICNV_ERR_ARG, w + "n_prob must be in 1 .. 65535");
    b.prob.assign((size_t)n_prob, LpProb{});
    int64_t z = 0, m = 0, e = 0;
    for (int32_t p = 0; p < n_prob; ++p) {
        if (n_feat[p] < 1 || n_cells[p] < 1 || n_cells[p] > 0x7ffffffe) ICNV_FAIL(ICNV_ERR_ARG, w + "problem " + std::to_string(p) + " is empty");
        if (npcs && (npcs[p] < 1 || npcs[p] > LPCA_MAX_NPCS)) ICNV_FAIL(ICNV_ERR_ARG, w + "npcs must be in 1 .. 64");
        LpProb &q = b.prob[p];
        q.n = n_cells[p]; q.n_gene = n_feat[p]; q.ldz = ldz_of(q.n); q.npcs = npcs ? npcs[p] : 0;
        q.z_off = z; q.m_off = m; q.e_off = e;
        z += (int64_t)q.n_gene * q.ldz;
        m += npcs ? (int64_t)q.n_gene * q.npcs : (int64_t)q.n_gene * q.n_gene;
        e += q.n;
        b.max_genes = std::max(b.max_genes, q.n_gene); b.max_n = std::max(b.max_n, q.n); b.max_ldz = std::max(b.max_ldz, q.ldz);
    }
    return ICNV_OK;
}

}  // namespace

struct icnv_snn {                 // the state between icnv_snn_begin_dev and icnv_snn_fill_dev
    SnnArgs a{};
    DevBuf d_noff, d_tcnt, d_toff, d_tlist, d_mark, d_touched, d_rowcnt, d_rowoff, d_loop, d_bad;
    int64_t total_n = 0, nnz = 0;
};

extern "C" {

int icnv_lpca_vstd_dev(const double *expr, int64_t G, int64_t C, int64_t ld, const int32_t *gene_idx, const int32_t *gene_off,
                       const int32_t *cell_idx, const int32_t *cell_off, int32_t n_prob, const double *mean, const double *sd,
                       double *v_std, void *stream) {
    int rc = matrix_validate("lpca_vstd", expr, G, C, ld, gene_idx, gene_off, cell_idx, cell_off, n_prob);
    if (rc) return rc;
    if (!mean || !sd || !v_std) ICNV_FAIL(ICNV_ERR_ARG, "lpca_vstd: null argument");
    for (int32_t p = 0; p < n_prob; ++p)
        if (cell_off[p + 1] - cell_off[p] < 2) ICNV_FAIL(ICNV_ERR_ARG, "lpca_vstd: problem " + std::to_string(p) + " has fewer than 2 cells");
    if ((rc = need_device())) return rc;
    hipStream_t s = (hipStream_t)stream;
    Batch b;
    b.prob.assign((size_t)n_prob, LpProb{});
    for (int32_t p = 0; p < n_prob; ++p) {
        LpProb &q = b.prob[p];
        q.cell_off = cell_off[p]; q.gene_off = gene_off[p]; q.n = cell_off[p + 1] - cell_off[p]; q.n_gene = gene_off[p + 1] - gene_off[p];
        b.max_genes = std::max(b.max_genes, q.n_gene);
    }
    if ((rc = upload(b.d_prob, b.prob.data(), b.prob.size(), s)) || (rc = upload(b.d_gene, gene_idx, (size_t)gene_off[n_prob], s)) ||
        (rc = upload(b.d_cell, cell_idx, (size_t)cell_off[n_prob], s)))
        return rc;
    LpArgs a{};
    a.x = expr; a.ld = ld; a.cell_idx = b.d_cell.as<int32_t>(); a.gene_idx = b.d_gene.as<int32_t>(); a.prob = b.d_prob.as<LpProb>();
    a.n_prob = n_prob; a.mean = mean; a.sd = sd; a.v_std = v_std;
    if ((rc = launch_lpca_vstd(a, b.max_genes, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));   // the host vectors and the pool blocks outlive the kernel
    return ICNV_OK;
}

int icnv_lpca_scale_dev(const double *expr, int64_t G, int64_t C, int64_t ld, const int32_t *gene_idx, const int32_t *gene_off,
                        const int32_t *cell_idx, const int32_t *cell_off, int32_t n_prob, const double *mean, const double *sd,
                        double *Z, void *stream) {
    int rc = matrix_validate("lpca_scale", expr, G, C, ld, gene_idx, gene_off, cell_idx, cell_off, n_prob);
    if (rc) return rc;
    if (!mean || !sd || !Z) ICNV_FAIL(ICNV_ERR_ARG, "lpca_scale: null argument");
    if ((rc = need_device())) return rc;
    hipStream_t s = (hipStream_t)stream;
    Batch b;
    b.prob.assign((size_t)n_prob, LpProb{});
    int64_t z = 0;
    for (int32_t p = 0; p < n_prob; ++p) {
        LpProb &q = b.prob[p];
        q.cell_off = cell_off[p]; q.gene_off = gene_off[p]; q.n = cell_off[p + 1] - cell_off[p]; q.n_gene = gene_off[p + 1] - gene_off[p];
        q.ldz = ldz_of(q.n); q.z_off = z;
        z += (int64_t)q.n_gene * q.ldz;
        b.max_genes = std::max(b.max_genes, q.n_gene); b.max_ldz = std::max(b.max_ldz, q.ldz);
    }
    if ((b.max_ldz + 31) / 32 > 65535) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "lpca_scale: more than 2 097 120 cells in one problem");
    if ((rc = upload(b.d_prob, b.prob.data(), b.prob.size(), s)) || (rc = upload(b.d_gene, gene_idx, (size_t)gene_off[n_prob], s)) ||
        (rc = upload(b.d_cell, cell_idx, (size_t)cell_off[n_prob], s)))
        return rc;
    LpArgs a{};
    a.x = expr; a.ld = ld; a.cell_idx = b.d_cell.as<int32_t>(); a.gene_idx = b.d_gene.as<int32_t>(); a.prob = b.d_prob.as<LpProb>();
    a.n_prob = n_prob; a.mean = mean; a.sd = sd; a.Z = Z;
    if ((rc = launch_lpca_scale(a, b.max_genes, b.max_ldz, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));
    return ICNV_OK;
}

int icnv_lpca_gram_dev(const double *Z, const int32_t *n_feat, const int32_t *n_cells, int32_t n_prob, double *M, void *stream) {
    Batch b;
    int rc = batch_sizes("lpca_gram", n_feat, n_cells, nullptr, n_prob, b);
    if (rc) return rc;
    if (!Z || !M) ICNV_FAIL(ICNV_ERR_ARG, "lpca_gram: null argument");
    const int64_t nt = (b.max_genes + 63) / 64;
    if (nt * nt > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "lpca_gram: too many features");
    if ((rc = need_device())) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = upload(b.d_prob, b.prob.data(), b.prob.size(), s))) return rc;
    LpArgs a{};
    a.prob = b.d_prob.as<LpProb>(); a.n_prob = n_prob; a.Z = const_cast<double *>(Z); a.M = M;
    if ((rc = launch_lpca_gram(a, b.max_genes, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));
    return ICNV_OK;
}

int icnv_lpca_project_dev(const double *Z, const double *V, const int32_t *n_feat, const int32_t *n_cells, const int32_t *npcs,
                          int32_t n_prob, double *E, int32_t e_ld, void *stream) {
    Batch b;
    if (!npcs) ICNV_FAIL(ICNV_ERR_ARG, "lpca_project: null argument");
    int rc = batch_sizes("lpca_project", n_feat, n_cells, npcs, n_prob, b);
    if (rc) return rc;
    if (!Z || !V || !E) ICNV_FAIL(ICNV_ERR_ARG, "lpca_project: null argument");
    if (e_ld < 1 || e_ld > LPCA_MAX_NPCS) ICNV_FAIL(ICNV_ERR_ARG, "lpca_project: e_ld must be in 1 .. 64");
    int64_t tn = 0;
    for (int32_t p = 0; p < n_prob; ++p) {
        if (npcs[p] > e_ld) ICNV_FAIL(ICNV_ERR_ARG, "lpca_project: npcs exceeds e_ld");
        tn += n_cells[p];
    }
    if ((rc = need_device())) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = upload(b.d_prob, b.prob.data(), b.prob.size(), s))) return rc;
    ICNV_HIP(hipMemsetAsync(E, 0, (size_t)tn * e_ld * sizeof(double), s));   // the components a problem does not have
    LpArgs a{};
    a.prob = b.d_prob.as<LpProb>(); a.n_prob = n_prob; a.Z = const_cast<double *>(Z); a.V = V; a.E = E; a.e_ld = e_ld;
    if ((rc = launch_lpca_project(a, b.max_n, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));
    return ICNV_OK;
}

int icnv_snn_begin_dev(const int32_t *nn_idx, int32_t k, const int32_t *node_off, int32_t n_prob, icnv_snn_t **out, int64_t *nnz,
                       void *stream) {
    if (!out) ICNV_FAIL(ICNV_ERR_ARG, "snn: null argument");
    *out = nullptr;
    if (!nn_idx || !node_off || !nnz) ICNV_FAIL(ICNV_ERR_ARG, "snn: null argument");
    if (n_prob < 1 || n_prob > 65535) ICNV_FAIL(ICNV_ERR_ARG, "snn: n_prob must be in 1 .. 65535");
    if (k < 1) ICNV_FAIL(ICNV_ERR_ARG, "snn: k must be >= 1");
    if (node_off[0] != 0) ICNV_FAIL(ICNV_ERR_ARG, "snn: offsets must start at 0");
    int64_t max_n = 0;
    for (int32_t p = 0; p < n_prob; ++p) {
        if (node_off[p + 1] < node_off[p]) ICNV_FAIL(ICNV_ERR_ARG, "snn: offsets must be monotone");
        if (k > node_off[p + 1] - node_off[p]) ICNV_FAIL(ICNV_ERR_ARG, "snn: k exceeds the nodes of problem " + std::to_string(p));
        max_n = std::max<int64_t>(max_n, node_off[p + 1] - node_off[p]);
    }
    if (k > LEIDEN_MAX_K) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "snn: k > 128 is not supported");
    const int64_t tn = node_off[n_prob];
    if (tn * k > ((int64_t)1 << 31) - 1) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "snn: batch too large (k sum n_p must stay below 2^31)");
    int rc = need_device();
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    std::unique_ptr<icnv_snn> h(new icnv_snn);
    std::vector<int64_t> noff(node_off, node_off + n_prob + 1);
    const size_t scr = (size_t)n_prob * snn_blocks(max_n) * max_n;
    if ((rc = upload(h->d_noff, noff.data(), noff.size(), s)) || (rc = h->d_tcnt.alloc((size_t)tn * 4)) ||
        (rc = h->d_toff.alloc((size_t)(tn + n_prob) * 8)) || (rc = h->d_tlist.alloc((size_t)tn * k * 4)) ||
        (rc = h->d_mark.alloc(scr * 4)) || (rc = h->d_touched.alloc(scr * 4)) || (rc = h->d_rowcnt.alloc((size_t)(tn + 1) * 4)) ||
        (rc = h->d_rowoff.alloc((size_t)(tn + 1) * 8)) || (rc = h->d_loop.alloc((size_t)tn * 4)) || (rc = h->d_bad.alloc(sizeof(uint32_t))))
        return rc;
    SnnArgs &a = h->a;
    a.nn = nn_idx; a.k = k; a.n_prob = n_prob; a.node_off = h->d_noff.as<int64_t>(); a.t_cnt = h->d_tcnt.as<int32_t>();
    a.t_off = h->d_toff.as<int64_t>(); a.t_list = h->d_tlist.as<int32_t>(); a.mark = h->d_mark.as<int32_t>();
    a.touched = h->d_touched.as<int32_t>(); a.max_n = max_n; a.row_cnt = h->d_rowcnt.as<int32_t>(); a.row_off = h->d_rowoff.as<int64_t>();
    a.loop = h->d_loop.as<int32_t>(); a.bad = h->d_bad.as<uint32_t>();
    h->total_n = tn;
    uint32_t bad = 0;
    ICNV_HIP(hipMemsetAsync(h->d_bad.p, 0, sizeof(uint32_t), s));
    ICNV_HIP(hipMemsetAsync(h->d_tcnt.p, 0, (size_t)tn * 4, s));
    ICNV_HIP(hipMemsetAsync(h->d_mark.p, 0, scr * 4, s));
    if ((rc = launch_snn_transpose(a, s))) return rc;
    ICNV_HIP(hipMemcpyAsync(&bad, h->d_bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (bad) ICNV_FAIL(ICNV_ERR_ARG, "snn: nn_idx entry outside [0, n_p)");
    if ((rc = launch_snn_lists(a, s))) return rc;
    ICNV_HIP(hipMemcpyAsync(&bad, h->d_bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (bad) ICNV_FAIL(ICNV_ERR_ARG, "snn: an nn_idx row repeats an entry");   // N(i) is a set: no row is counted
    if ((rc = launch_snn_rows(a, false, s)) || (rc = launch_snn_scan(a, tn, s))) return rc;
    ICNV_HIP(hipMemcpyAsync(&h->nnz, a.row_off + tn, 8, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    *nnz = h->nnz;
    *out = h.release();
    return ICNV_OK;
}

int icnv_snn_fill_dev(icnv_snn_t *h, int64_t *row_off, int32_t *col, int32_t *shared, int64_t *weight, int32_t *loop, void *stream) {
    if (!h || !row_off || !col || !shared || !weight || !loop) ICNV_FAIL(ICNV_ERR_ARG, "snn: null argument");
    hipStream_t s = (hipStream_t)stream;
    SnnArgs a = h->a;
    a.col = col; a.shared = shared; a.weight = weight;
    int rc;
    if (h->nnz > 0 && (rc = launch_snn_rows(a, true, s))) return rc;
    ICNV_HIP(hipMemcpyAsync(row_off, a.row_off, (size_t)(h->total_n + 1) * 8, hipMemcpyDeviceToDevice, s));
    ICNV_HIP(hipMemcpyAsync(loop, a.loop, (size_t)h->total_n * 4, hipMemcpyDeviceToDevice, s));
    ICNV_HIP(hipStreamSynchronize(s));
    return ICNV_OK;
}

void icnv_snn_end(icnv_snn_t *h) { delete h; }

}  // extern "C"
