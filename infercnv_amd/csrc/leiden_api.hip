// C ABI of K11 (include/icnv.h "Leiden"): cluster_leiden of .leiden_simple_snn (R/inferCNV_tumor_subclusters.R:726-741) --
// validation, the graph and run scratch, stats; and K18's icnv_leiden_graph_dev, which shares leiden_run.  Kernels:
// leiden_kernels.hip (the CSR check of icnv_leiden_graph_dev: leiden_pca_kernels.hip).  DESIGN.md section 4 K11.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "icnv_internal.h"
#include "leiden_internal.h"
#include "leiden_pca_internal.h"

using namespace icnv;

namespace {
std::atomic<int64_t> g_ld[7];   // calls, problems, levels, move visits, refinement visits, draws, wall microseconds

// every host check before any device work (R/inferCNV_tumor_subclusters.R:726: nn2's k = k_nn <= ncol)
int leiden_validate(const int32_t *nn_idx, int32_t k, const int32_t *node_off, int32_t n_prob) {
    if (!nn_idx || !node_off) ICNV_FAIL(ICNV_ERR_ARG, "leiden: null argument");
    if (n_prob < 1) ICNV_FAIL(ICNV_ERR_ARG, "leiden: n_prob must be >= 1");
    if (k < 1) ICNV_FAIL(ICNV_ERR_ARG, "leiden: k must be >= 1");
    if (node_off[0] != 0) ICNV_FAIL(ICNV_ERR_ARG, "leiden: offsets must start at 0");
    for (int32_t p = 0; p < n_prob; ++p) {
        if (node_off[p + 1] < node_off[p]) ICNV_FAIL(ICNV_ERR_ARG, "leiden: offsets must be monotone");
        if (k > node_off[p + 1] - node_off[p]) ICNV_FAIL(ICNV_ERR_ARG, "leiden: k exceeds the nodes of problem " + std::to_string(p));
    }
    if (k > LEIDEN_MAX_K) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "leiden: k > 128 is not supported");
    if ((int64_t)node_off[n_prob] * 2 * k > ((int64_t)1 << 31) - 1)
        ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "leiden: batch too large (2 k sum n_p must stay below 2^31)");
    return ICNV_OK;
}

int leiden_validate_run(int32_t n_prob, int32_t objective, const double *resolution, double beta, int32_t n_iterations,
                        const void *membership, const void *n_clusters) {
    if (!resolution || !membership || !n_clusters) ICNV_FAIL(ICNV_ERR_ARG, "leiden: null argument");
    if (objective != ICNV_LEIDEN_CPM && objective != ICNV_LEIDEN_MODULARITY) ICNV_FAIL(ICNV_ERR_ARG, "leiden: unknown objective");
    for (int32_t p = 0; p < n_prob; ++p)
        if (!std::isfinite(resolution[p]) || resolution[p] < 0) ICNV_FAIL(ICNV_ERR_ARG, "leiden: resolution must be finite and >= 0");
    if (!std::isfinite(beta) || !(beta > 0)) ICNV_FAIL(ICNV_ERR_ARG, "leiden: beta must be finite and > 0");
    if (n_iterations < 1 || n_iterations > LEIDEN_MAX_ITERATIONS) ICNV_FAIL(ICNV_ERR_ARG, "leiden: n_iterations must be in [1, 1000]");
    return ICNV_OK;
}

// the graphs of a batch on the device (after the device check of nn_idx): g's arrays live in the buffers
struct LeidenGraphBufs {
    DevBuf d_off, d_noff, d_col, d_strength, d_ssum, d_raw, d_raw_off, d_cnt, d_loop, d_bad;
    std::vector<int64_t> noff;
    LeidenGraph g{};
};

int leiden_build_graph(const int32_t *nn_idx, int32_t k, const int32_t *node_off, int32_t n_prob, hipStream_t s, LeidenGraphBufs &b) {
    int rc;
    b.noff.assign(node_off, node_off + n_prob + 1);
    const int64_t tn = b.noff[n_prob], E = 2 * (int64_t)k * tn, to = tn + n_prob;
    if ((rc = upload(b.d_noff, b.noff.data(), b.noff.size(), s)) || (rc = b.d_off.alloc((size_t)to * 8)) ||
        (rc = b.d_col.alloc((size_t)std::max<int64_t>(E, 1) * 4)) || (rc = b.d_strength.alloc((size_t)tn * 8)) ||
        (rc = b.d_ssum.alloc((size_t)n_prob * 8)) || (rc = b.d_raw.alloc((size_t)std::max<int64_t>(E, 1) * 4)) ||
        (rc = b.d_raw_off.alloc((size_t)to * 8)) || (rc = b.d_cnt.alloc((size_t)tn * 4)) || (rc = b.d_loop.alloc((size_t)tn * 4)) ||
        (rc = b.d_bad.alloc(sizeof(uint32_t))))
        return rc;
    LeidenGraph &g = b.g;
    g.nn = nn_idx; g.k = k; g.n_prob = n_prob; g.node_off = b.d_noff.as<int64_t>();
    g.off = b.d_off.as<int64_t>(); g.col = b.d_col.as<int32_t>(); g.strength = b.d_strength.as<int64_t>();
    g.strength_sum = b.d_ssum.as<int64_t>(); g.raw = b.d_raw.as<int32_t>(); g.raw_off = b.d_raw_off.as<int64_t>();
    g.cnt = b.d_cnt.as<int32_t>(); g.loop = b.d_loop.as<int32_t>(); g.bad = b.d_bad.as<uint32_t>();
    uint32_t bad = 0;
    ICNV_HIP(hipMemsetAsync(b.d_bad.p, 0, sizeof(uint32_t), s));
    if ((rc = launch_leiden_check(g, s))) return rc;
    ICNV_HIP(hipMemcpyAsync(&bad, b.d_bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (bad) ICNV_FAIL(ICNV_ERR_ARG, "leiden: nn_idx entry outside [0, n_p)");
    return launch_leiden_graph(g, s);
}
}  // namespace

extern "C" {

int icnv_snn_graph_dev(const int32_t *nn_idx, int32_t k, const int32_t *node_off, int32_t n_prob, int64_t *row_off,
                       int32_t *col, int64_t *strength, void *stream) {
    int rc = leiden_validate(nn_idx, k, node_off, n_prob);
    if (rc) return rc;
    if (!row_off || !col || !strength) ICNV_FAIL(ICNV_ERR_ARG, "leiden: null argument");
    hipStream_t s = (hipStream_t)stream;
    LeidenGraphBufs b;
    if ((rc = leiden_build_graph(nn_idx, k, node_off, n_prob, s, b))) return rc;
    const int64_t tn = b.noff[n_prob];
    std::vector<int64_t> off(tn + n_prob), out(tn + 1);
    ICNV_HIP(hipMemcpyAsync(off.data(), b.d_off.p, off.size() * 8, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    int64_t base = 0;
    for (int32_t p = 0; p < n_prob; ++p) {   // problem p's rows after the ones before it
        const int64_t n0 = b.noff[p], n = b.noff[p + 1] - n0;
        for (int64_t i = 0; i <= n; ++i) out[n0 + i] = base + off[n0 + p + i];
        const int64_t nnz = off[n0 + p + n];
        if (nnz) ICNV_HIP(hipMemcpyAsync(col + base, b.d_col.as<int32_t>() + 2 * (int64_t)k * n0, (size_t)nnz * 4, hipMemcpyDeviceToDevice, s));
        base += nnz;
    }
    ICNV_HIP(hipMemcpyAsync(row_off, out.data(), out.size() * 8, hipMemcpyHostToDevice, s));
    ICNV_HIP(hipMemcpyAsync(strength, b.d_strength.p, (size_t)tn * 8, hipMemcpyDeviceToDevice, s));
    ICNV_HIP(hipStreamSynchronize(s));
    return ICNV_OK;
}

// the Leiden run of a batch whose graphs are on the device: g (CSR, strengths), the problems' edge regions (edge_off null:
// 2 k node_off[p], icnv_leiden_dev's), the level-0 edge weights (ew0 null: 1) and E, the entries of all regions together
static int leiden_run(const LeidenGraph &g, const std::vector<int64_t> &noff, const int64_t *edge_off, const int64_t *ew0, int64_t E,
                      int32_t n_prob, int32_t objective, const double *resolution, double beta, int32_t n_iterations, uint64_t seed,
                      const uint64_t *token, int32_t *membership, int32_t *n_clusters, hipStream_t s,
                      std::chrono::steady_clock::time_point t0) {
    int rc;
    const int64_t tn = noff[n_prob], to = tn + n_prob;
    std::vector<int64_t> ssum(n_prob);
    ICNV_HIP(hipMemcpyAsync(ssum.data(), g.strength_sum, ssum.size() * 8, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    std::vector<double> r(n_prob);
    for (int32_t p = 0; p < n_prob; ++p)   // R's wrapper: resolution_parameter / sum(strength) for modularity
        r[p] = objective == ICNV_LEIDEN_MODULARITY ? resolution[p] / (double)ssum[p] : resolution[p];
    std::vector<uint64_t> tok(n_prob, 0);
    if (token) tok.assign(token, token + n_prob);
    DevBuf d_r, d_tok, d_i64, d_offs, d_i32, d_cum, d_nbr, d_ew, d_memb, d_ncl, d_status, d_cnt;
    if ((rc = upload(d_r, r.data(), r.size(), s)) || (rc = upload(d_tok, tok.data(), tok.size(), s)) ||
        (rc = d_i64.alloc((size_t)LEIDEN_I64_ARRAYS * tn * 8)) || (rc = d_offs.alloc((size_t)2 * to * 8)) ||
        (rc = d_i32.alloc((size_t)LEIDEN_I32_ARRAYS * to * 4)) || (rc = d_cum.alloc((size_t)tn * 8)) ||
        (rc = d_nbr.alloc((size_t)std::max<int64_t>(2 * E, 1) * 4)) || (rc = d_ew.alloc((size_t)std::max<int64_t>(2 * E, 1) * 8)) ||
        (rc = d_memb.alloc((size_t)tn * 4)) || (rc = d_ncl.alloc((size_t)n_prob * 4)) || (rc = d_status.alloc((size_t)n_prob * 4)) ||
        (rc = d_cnt.alloc((size_t)n_prob * LEIDEN_CNT_N * 8)))
        return rc;
    LeidenArgs a;
    a.g = g; a.edge_off = edge_off; a.ew0 = ew0; a.total_e = E; a.objective = objective; a.r = d_r.as<double>(); a.beta = beta; a.n_iterations = n_iterations; a.seed = seed;
    a.token = d_tok.as<uint64_t>(); a.i64 = d_i64.as<int64_t>(); a.offs = d_offs.as<int64_t>(); a.i32 = d_i32.as<int32_t>();
    a.cum = d_cum.as<double>(); a.nbr = d_nbr.as<int32_t>(); a.ew = d_ew.as<int64_t>(); a.total_n = tn;
    a.membership = d_memb.as<int32_t>(); a.n_clusters = d_ncl.as<int32_t>(); a.status = d_status.as<int32_t>();
    a.counters = d_cnt.as<int64_t>();
    if ((rc = launch_leiden(a, s))) return rc;
    std::vector<int32_t> status(n_prob), ncl(n_prob);
    std::vector<int64_t> cnt((size_t)n_prob * LEIDEN_CNT_N);
    ICNV_HIP(hipMemcpyAsync(status.data(), d_status.p, status.size() * 4, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipMemcpyAsync(ncl.data(), d_ncl.p, ncl.size() * 4, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipMemcpyAsync(cnt.data(), d_cnt.p, cnt.size() * 8, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    for (int32_t p = 0; p < n_prob; ++p) {
        if (status[p] == LEIDEN_MOVE_CAP)
            ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "leiden: problem " + std::to_string(p) + " exceeded the queue pops of a move phase (256 n + 1024)");
        if (status[p] == LEIDEN_LEVEL_CAP)
            ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "leiden: problem " + std::to_string(p) + " exceeded 512 levels in one iteration");
        if (status[p] != LEIDEN_OK) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "leiden: internal error in problem " + std::to_string(p));
    }
    ICNV_HIP(hipMemcpyAsync(membership, d_memb.p, (size_t)tn * 4, hipMemcpyDeviceToDevice, s));
    ICNV_HIP(hipStreamSynchronize(s));
    std::copy(ncl.begin(), ncl.end(), n_clusters);
    g_ld[0] += 1;
    g_ld[1] += n_prob;
    for (int32_t p = 0; p < n_prob; ++p)
        for (int c = 0; c < LEIDEN_CNT_N; ++c) g_ld[2 + c] += cnt[(size_t)p * LEIDEN_CNT_N + c];
    g_ld[6] += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return ICNV_OK;
}


int icnv_leiden_dev(const int32_t *nn_idx, int32_t k, const int32_t *node_off, int32_t n_prob, int32_t objective,
                    const double *resolution, double beta, int32_t n_iterations, uint64_t seed, const uint64_t *token,
                    int32_t *membership, int32_t *n_clusters, void *stream) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc = leiden_validate(nn_idx, k, node_off, n_prob);
    if (rc || (rc = leiden_validate_run(n_prob, objective, resolution, beta, n_iterations, membership, n_clusters))) return rc;
    hipStream_t s = (hipStream_t)stream;
    LeidenGraphBufs b;
    if ((rc = leiden_build_graph(nn_idx, k, node_off, n_prob, s, b))) return rc;
    const int64_t tn = b.noff[n_prob];
    return leiden_run(b.g, b.noff, nullptr, nullptr, 2 * (int64_t)k * tn, n_prob, objective, resolution, beta, n_iterations, seed, token,
                      membership, n_clusters, s, t0);
}

int icnv_leiden_graph_dev(const int64_t *row_off, const int32_t *col, const int64_t *weight, const int32_t *loop, int64_t loop_weight,
                          const int32_t *node_off, int32_t n_prob, int32_t objective, const double *resolution, double beta,
                          int32_t n_iterations, uint64_t seed, const uint64_t *token, int32_t *membership, int32_t *n_clusters,
                          void *stream) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!row_off || !col || !weight || !loop || !node_off) ICNV_FAIL(ICNV_ERR_ARG, "leiden_graph: null argument");
    if (n_prob < 1) ICNV_FAIL(ICNV_ERR_ARG, "leiden_graph: n_prob must be >= 1");
    if (loop_weight < 1 || loop_weight > ((int64_t)1 << 53)) ICNV_FAIL(ICNV_ERR_ARG, "leiden_graph: loop_weight must be in [1, 2^53]");
    if (node_off[0] != 0) ICNV_FAIL(ICNV_ERR_ARG, "leiden_graph: offsets must start at 0");
    for (int32_t p = 0; p < n_prob; ++p)
        if (node_off[p + 1] <= node_off[p]) ICNV_FAIL(ICNV_ERR_ARG, "leiden_graph: problem " + std::to_string(p) + " has no node");
    int rc = leiden_validate_run(n_prob, objective, resolution, beta, n_iterations, membership, n_clusters);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int64_t tn = node_off[n_prob], to = tn + n_prob;
    std::vector<int64_t> roff((size_t)tn + 1), noff(node_off, node_off + n_prob + 1), off((size_t)to), eoff((size_t)n_prob + 1);
    ICNV_HIP(hipMemcpyAsync(roff.data(), row_off, roff.size() * 8, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (roff[0] != 0) ICNV_FAIL(ICNV_ERR_ARG, "leiden_graph: row_off must start at 0");
    for (int64_t i = 0; i < tn; ++i)
        if (roff[i + 1] < roff[i]) ICNV_FAIL(ICNV_ERR_ARG, "leiden_graph: row_off must be monotone");
    const int64_t E = roff[tn];
    if (E > ((int64_t)1 << 31) - 1) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "leiden_graph: batch too large (the entries must stay below 2^31)");
    for (int32_t p = 0; p < n_prob; ++p) {   // problem p's offsets within its own edge region, n_p + 1 of them
        const int64_t n0 = noff[p], n = noff[p + 1] - n0;
        eoff[p] = roff[n0];
        for (int64_t i = 0; i <= n; ++i) off[n0 + p + i] = roff[n0 + i] - roff[n0];
    }
    eoff[n_prob] = E;
    DevBuf d_noff, d_off, d_eoff, d_strength, d_ssum, d_bad;
    if ((rc = upload(d_noff, noff.data(), noff.size(), s)) || (rc = upload(d_off, off.data(), off.size(), s)) ||
        (rc = upload(d_eoff, eoff.data(), eoff.size(), s)) || (rc = d_strength.alloc((size_t)tn * 8)) ||
        (rc = d_ssum.alloc((size_t)n_prob * 8)) || (rc = d_bad.alloc(sizeof(uint32_t))))
        return rc;
    LgCheck c{};
    c.node_off = d_noff.as<int64_t>(); c.row_off = row_off; c.col = col; c.loop = loop; c.weight = weight; c.loop_weight = loop_weight;
    c.n_prob = n_prob; c.off = d_off.as<int64_t>(); c.edge_off = d_eoff.as<int64_t>(); c.strength = d_strength.as<int64_t>();
    c.strength_sum = d_ssum.as<int64_t>(); c.bad = d_bad.as<uint32_t>();
    uint32_t bad = 0;
    std::vector<int64_t> ssum(n_prob);
    ICNV_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), s));
    if ((rc = launch_lg_check(c, s))) return rc;
    ICNV_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipMemcpyAsync(ssum.data(), d_ssum.p, ssum.size() * 8, hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (bad) ICNV_FAIL(ICNV_ERR_ARG, "leiden_graph: a row is not ascending within [0, n_p) without its own node, a weight is < 1, or a loop flag is not 0 / 1");
    for (int32_t p = 0; p < n_prob; ++p)   // the int64 -> double conversions of the gain must be exact
        if (ssum[p] / 2 >= ((int64_t)1 << 53))
            ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "leiden_graph: the total edge weight of problem " + std::to_string(p) + " reaches 2^53");
    LeidenGraph g{};
    g.k = 0; g.n_prob = n_prob; g.node_off = d_noff.as<int64_t>(); g.off = d_off.as<int64_t>(); g.col = const_cast<int32_t *>(col);
    g.strength = d_strength.as<int64_t>(); g.strength_sum = d_ssum.as<int64_t>();
    return leiden_run(g, noff, d_eoff.as<int64_t>(), weight, E, n_prob, objective, resolution, beta, n_iterations, seed, token, membership,
                      n_clusters, s, t0);
}

int icnv_leiden(const int32_t *nn_idx, int32_t k, const int32_t *node_off, int32_t n_prob, int32_t objective,
                const double *resolution, double beta, int32_t n_iterations, uint64_t seed, const uint64_t *token,
                int32_t *membership, int32_t *n_clusters) {
    int rc = leiden_validate(nn_idx, k, node_off, n_prob);
    if (rc || (rc = leiden_validate_run(n_prob, objective, resolution, beta, n_iterations, membership, n_clusters))) return rc;
    const size_t tn = (size_t)node_off[n_prob];
    DevBuf d_nn, d_memb;
    if ((rc = upload(d_nn, nn_idx, tn * k, nullptr)) || (rc = d_memb.alloc(tn * 4))) return rc;
    std::vector<int32_t> ncl(n_prob);
    if ((rc = icnv_leiden_dev(d_nn.as<int32_t>(), k, node_off, n_prob, objective, resolution, beta, n_iterations, seed, token,
                              d_memb.as<int32_t>(), ncl.data(), nullptr)))
        return rc;
    ICNV_HIP(hipMemcpy(membership, d_memb.p, tn * 4, hipMemcpyDeviceToHost));
    std::copy(ncl.begin(), ncl.end(), n_clusters);
    return ICNV_OK;
}

int icnv_leiden_stats(int64_t *out, int32_t n) {
    if (!out || n < 1) ICNV_FAIL(ICNV_ERR_ARG, "bad argument");
    for (int i = 0; i < n && i < 7; ++i) out[i] = g_ld[i].load();
    return ICNV_OK;
}

void icnv_leiden_stats_reset(void) {
    for (auto &c : g_ld) c.store(0);
}

}  // extern "C"
