// C ABI of K9 (include/icnv.h "hierarchical clustering"): fastcluster::hclust(as.dist(D), method) (R/inferCNV_tumor_subclusters.R:191,
// 582, 609, R/inferCNV_ops.R:1930, 3242, R/inferCNV_heatmap.R:719, 755, 1062, 1079) -- validation, the LDS / HBM split, R's
// labelling of the raw merges and stats.  Kernels: hclust_kernels.hip.  DESIGN.md section 4 K9.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <numeric>
#include <string>
#include <vector>

#include "icnv_internal.h"
#include "hclust_internal.h"

using namespace icnv;

namespace {
std::atomic<int64_t> g_hc[6];   // calls, problems, LDS problems, HBM problems, chain steps, wall microseconds
}  // namespace

namespace icnv {   // shared with K10 (hclust_internal.h)

int hclust_method_check(int32_t method) {
    if (method < ICNV_HCLUST_WARD_D || method > ICNV_HCLUST_MCQUITTY)
        ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "hclust: unsupported method (centroid and median are not reducible)");
    return ICNV_OK;
}

// R's hclust object from one problem's raw merges (chain order): stable sort by dissimilarity, union-find relabelling
// (singletons -(i+1), clusters by sorted step, the smaller internal node first) and the left-first depth-first order
void hclust_label(int n, const int32_t *rx, const int32_t *ry, const double *rh, bool root, int32_t *merge, double *height,
                  int32_t *order) {
    const int nm = n - 1;
    std::vector<int> perm(nm), parent(2 * (size_t)n - 1);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return rh[a] < rh[b]; });
    std::iota(parent.begin(), parent.end(), 0);
    auto find = [&](int i) {
        int r = i;
        while (parent[r] != r) r = parent[r];
        while (parent[i] != r) { const int q = parent[i]; parent[i] = r; i = q; }
        return r;
    };
    for (int i = 0; i < nm; ++i) {
        const int q = perm[i];
        int a = find(rx[q]), b = find(ry[q]);
        parent[a] = parent[b] = n + i;
        if (a > b) std::swap(a, b);
        merge[i] = a < n ? -(a + 1) : a - n + 1;
        merge[i + nm] = b < n ? -(b + 1) : b - n + 1;
        height[i] = root ? std::sqrt(rh[q]) : rh[q];
    }
    std::vector<int> stack{nm};   // R labels: > 0 a merge row (1-based), < 0 a singleton
    int o = 0;
    while (!stack.empty()) {
        const int v = stack.back();
        stack.pop_back();
        if (v < 0) { order[o++] = -v; continue; }
        stack.push_back(merge[v - 1 + nm]);
        stack.push_back(merge[v - 1]);
    }
}

// Every problem's n_p x n_p matrix is at D + d_off[p] (row-major, consecutive).  Checks it and clusters every problem;
// problem p's raw merges start at m_off[p] = c_off[p] - p.  Synchronises s.
int hclust_raw(double *D, const std::vector<int32_t> &n, const std::vector<int64_t> &c_off, int32_t method, hipStream_t s,
               HclustRaw &out) {
    const int P = (int)n.size();
    std::vector<int64_t> d_off(P + 1), &m_off = out.m_off;
    m_off.assign(P + 1, 0);
    d_off[0] = 0;
    for (int p = 0; p < P; ++p) d_off[p + 1] = d_off[p] + (int64_t)n[p] * n[p];
    for (int p = 0; p <= P; ++p) m_off[p] = c_off[p] - p;
    const int64_t total_cells = c_off[P], total_merges = m_off[P];
    int rc;
    DevBuf d_bad;
    uint32_t bad = 0;
    if ((rc = d_bad.alloc(sizeof(uint32_t)))) return rc;
    ICNV_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), s));
    if ((rc = launch_hclust_prep(D, d_off[P], method == ICNV_HCLUST_WARD_D2, d_bad.as<uint32_t>(), s))) return rc;
    ICNV_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (bad) ICNV_FAIL(ICNV_ERR_ARG, "hclust: NaN or infinite distance");

    const bool force_hbm = env_int("ICNV_HCLUST_FORCE_HBM", 0) != 0;
    std::vector<int32_t> run;   // LDS problems, then HBM problems
    int max_lds = 0, max_hbm = 0;
    for (int p = 0; p < P; ++p)
        if (!force_hbm && n[p] <= HC_LDS_MAX_N) { run.push_back(p); max_lds = std::max(max_lds, n[p]); }
    const int n_lds = (int)run.size();
    for (int p = 0; p < P; ++p)
        if (force_hbm || n[p] > HC_LDS_MAX_N) { run.push_back(p); max_hbm = std::max(max_hbm, n[p]); }
    const int n_hbm = P - n_lds;

    DevBuf d_doff, d_coff, d_run, d_steps, d_work;
    if ((rc = upload(out.d_n, n.data(), n.size(), s)) || (rc = upload(d_doff, d_off.data(), d_off.size(), s)) ||
        (rc = upload(out.d_moff, m_off.data(), m_off.size(), s)) || (rc = upload(d_coff, c_off.data(), c_off.size(), s)) ||
        (rc = upload(d_run, run.data(), run.size(), s)) || (rc = out.d_mx.alloc((size_t)total_merges * sizeof(int32_t))) ||
        (rc = out.d_my.alloc((size_t)total_merges * sizeof(int32_t))) || (rc = out.d_mh.alloc((size_t)total_merges * sizeof(double))) ||
        (rc = d_steps.alloc((size_t)P * sizeof(int64_t))))
        return rc;
    if (n_hbm && (rc = d_work.alloc((size_t)total_cells * 2 * sizeof(int32_t)))) return rc;
    HclustArgs a;
    a.n = out.d_n.as<int32_t>(); a.d_off = d_doff.as<int64_t>(); a.D = D; a.m_off = out.d_moff.as<int64_t>();
    a.mx = out.d_mx.as<int32_t>(); a.my = out.d_my.as<int32_t>(); a.mh = out.d_mh.as<double>();
    a.c_off = d_coff.as<int64_t>(); a.work = d_work.as<int32_t>(); a.steps = d_steps.as<int64_t>(); a.method = method;
    a.n_run = n_lds; a.run = d_run.as<int32_t>();
    if ((rc = launch_hclust_lds(a, max_lds, s))) return rc;
    a.n_run = n_hbm; a.run = d_run.as<int32_t>() + n_lds;
    if ((rc = launch_hclust_hbm(a, max_hbm, s))) return rc;

    std::vector<int64_t> steps(P);
    ICNV_HIP(hipMemcpyAsync(steps.data(), d_steps.p, steps.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    out.steps = 0;
    for (int p = 0; p < P; ++p) {
        if (steps[p] < 0) ICNV_FAIL(ICNV_ERR_ARG, "hclust: a dissimilarity overflowed to a non-finite value");
        out.steps += steps[p];
    }
    out.n_lds = n_lds;
    out.n_hbm = n_hbm;
    return ICNV_OK;
}
}  // namespace icnv

namespace {
// hclust_raw, then R's objects written to the DEVICE outputs, problem p's at 2 (c_off[p] - p), c_off[p] - p and c_off[p].
// Synchronises s.
int hclust_run(double *D, const std::vector<int32_t> &n, const std::vector<int64_t> &c_off, int32_t method, int32_t *merge,
               double *height, int32_t *order, hipStream_t s, std::chrono::steady_clock::time_point t0) {
    const int P = (int)n.size();
    HclustRaw raw;
    int rc = hclust_raw(D, n, c_off, method, s, raw);
    if (rc) return rc;
    const std::vector<int64_t> &m_off = raw.m_off;
    const int64_t total_cells = c_off[P], total_merges = m_off[P];
    std::vector<int32_t> mx(total_merges), my(total_merges), hm(2 * total_merges), ho(total_cells);
    std::vector<double> mh(total_merges), hh(total_merges);
    ICNV_HIP(hipMemcpyAsync(mx.data(), raw.d_mx.p, mx.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipMemcpyAsync(my.data(), raw.d_my.p, my.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipMemcpyAsync(mh.data(), raw.d_mh.p, mh.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    for (int p = 0; p < P; ++p) {
        const int64_t m0 = m_off[p];
        hclust_label(n[p], mx.data() + m0, my.data() + m0, mh.data() + m0, method == ICNV_HCLUST_WARD_D2, hm.data() + 2 * m0,
                     hh.data() + m0, ho.data() + c_off[p]);
    }
    ICNV_HIP(hipMemcpyAsync(merge, hm.data(), hm.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    ICNV_HIP(hipMemcpyAsync(height, hh.data(), hh.size() * sizeof(double), hipMemcpyHostToDevice, s));
    ICNV_HIP(hipMemcpyAsync(order, ho.data(), ho.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    ICNV_HIP(hipStreamSynchronize(s));
    const int n_lds = raw.n_lds, n_hbm = raw.n_hbm;
    const int64_t all_steps = raw.steps;
    g_hc[0] += 1;
    g_hc[1] += P;
    g_hc[2] += n_lds;
    g_hc[3] += n_hbm;
    g_hc[4] += all_steps;
    g_hc[5] += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return ICNV_OK;
}

int hclust_cells_validate(const double *expr, int64_t G, int64_t C, const int32_t *gene_idx, const int32_t *gene_off,
                          const int32_t *cell_idx, const int32_t *cell_off, int32_t n_prob, int32_t method, const void *merge,
                          const void *height, const void *order) {
    if (!expr || !gene_idx || !gene_off || !cell_idx || !cell_off || !merge || !height || !order)
        ICNV_FAIL(ICNV_ERR_ARG, "hclust: null argument");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "hclust: bad matrix dimensions");
    if (n_prob < 1) ICNV_FAIL(ICNV_ERR_ARG, "hclust: n_prob must be >= 1");
    if (gene_off[0] != 0 || cell_off[0] != 0) ICNV_FAIL(ICNV_ERR_ARG, "hclust: offsets must start at 0");
    for (int32_t p = 0; p < n_prob; ++p) {
        if (gene_off[p + 1] <= gene_off[p]) ICNV_FAIL(ICNV_ERR_ARG, "hclust: every problem needs at least one gene");
        const int64_t np = (int64_t)cell_off[p + 1] - cell_off[p];
        if (np < 2) ICNV_FAIL(ICNV_ERR_ARG, "hclust: every problem needs at least two cells (problem " + std::to_string(p) + ")");
        if (np > HC_HBM_MAX_N) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "hclust: more than 524288 cells in one problem");
    }
    for (int64_t i = 0; i < gene_off[n_prob]; ++i)
        if (gene_idx[i] < 0 || gene_idx[i] >= G) ICNV_FAIL(ICNV_ERR_ARG, "hclust: gene index out of range");
    for (int64_t i = 0; i < cell_off[n_prob]; ++i)
        if (cell_idx[i] < 0 || cell_idx[i] >= C) ICNV_FAIL(ICNV_ERR_ARG, "hclust: cell index out of range");
    return hclust_method_check(method);
}
}  // namespace

extern "C" {

int icnv_hclust_dev(const double *dist, int64_t ld, int32_t n, int32_t method, int32_t *merge, double *height, int32_t *order,
                    void *stream) {
    const auto t0 = std::chrono::steady_clock::now();
    if (!dist || !merge || !height || !order) ICNV_FAIL(ICNV_ERR_ARG, "hclust: null argument");
    if (n < 2) ICNV_FAIL(ICNV_ERR_ARG, "hclust: must have n >= 2 objects to cluster");
    if (ld < n) ICNV_FAIL(ICNV_ERR_ARG, "hclust: ld must be >= n");
    if (n > HC_HBM_MAX_N) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "hclust: more than 524288 objects");
    int rc = hclust_method_check(method);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    DevBuf ws;   // the chain updates its matrix in place: a private copy
    if ((rc = ws.alloc((size_t)n * n * sizeof(double)))) return rc;
    ICNV_HIP(hipMemcpy2DAsync(ws.p, (size_t)n * sizeof(double), dist, (size_t)ld * sizeof(double), (size_t)n * sizeof(double), n,
                              hipMemcpyDeviceToDevice, s));
    return hclust_run(ws.as<double>(), {n}, {0, n}, method, merge, height, order, s, t0);
}

int icnv_hclust_cells_dev(const double *expr, int64_t G, int64_t C, const int32_t *gene_idx, const int32_t *gene_off,
                          const int32_t *cell_idx, const int32_t *cell_off, int32_t n_prob, int32_t method, int32_t *merge,
                          double *height, int32_t *order, void *stream) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc = hclust_cells_validate(expr, G, C, gene_idx, gene_off, cell_idx, cell_off, n_prob, method, merge, height, order);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    // every problem's distances straight into the workspace, R's sequential dist over the problem's genes (distance_kernels.hip)
    std::vector<int64_t> goff(n_prob + 1), coff(n_prob + 1), doff(n_prob + 1), toff;
    std::vector<int32_t> n(n_prob);
    for (int32_t p = 0; p <= n_prob; ++p) { goff[p] = gene_off[p]; coff[p] = cell_off[p]; }
    doff[0] = 0;
    for (int32_t p = 0; p < n_prob; ++p) {
        n[p] = (int32_t)(coff[p + 1] - coff[p]);
        doff[p + 1] = doff[p] + (int64_t)n[p] * n[p];
    }
    const int dt = exact_dist_plan(n.data(), n_prob, toff);
    if (toff[n_prob] > 0x7fffffff || coff[n_prob] > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "hclust: batch too large");
    DevBuf d_gidx, d_goff, d_cidx, d_coff, d_toff, d_n, d_doff, d_D;
    if ((rc = upload(d_gidx, gene_idx, (size_t)goff[n_prob], s)) || (rc = upload(d_goff, goff.data(), goff.size(), s)) ||
        (rc = upload(d_cidx, cell_idx, (size_t)coff[n_prob], s)) || (rc = upload(d_coff, coff.data(), coff.size(), s)) ||
        (rc = upload(d_toff, toff.data(), toff.size(), s)) || (rc = upload(d_n, n.data(), n.size(), s)) ||
        (rc = upload(d_doff, doff.data(), doff.size(), s)) || (rc = d_D.alloc((size_t)doff[n_prob] * sizeof(double))))
        return rc;
    DistArgs a{};
    a.x = expr; a.ldx = G; a.G = (int32_t)G;
    a.gene_idx = d_gidx.as<int32_t>(); a.gene_off = d_goff.as<int64_t>();
    a.cell_idx = d_cidx.as<int32_t>(); a.cell_off = d_coff.as<int64_t>(); a.n = d_n.as<int32_t>();
    a.n_prob = n_prob; a.tile_off = d_toff.as<int64_t>(); a.d_off = d_doff.as<int64_t>(); a.D = d_D.as<double>();
    if ((rc = launch_exact_dist(a, dt, toff[n_prob], s))) return rc;
    return hclust_run(d_D.as<double>(), n, coff, method, merge, height, order, s, t0);
}

int icnv_hclust_cells(const double *expr, int64_t G, int64_t C, const int32_t *gene_idx, const int32_t *gene_off,
                      const int32_t *cell_idx, const int32_t *cell_off, int32_t n_prob, int32_t method, int32_t *merge,
                      double *height, int32_t *order) {
    int rc = hclust_cells_validate(expr, G, C, gene_idx, gene_off, cell_idx, cell_off, n_prob, method, merge, height, order);
    if (rc) return rc;
    const size_t cells = (size_t)cell_off[n_prob], merges = cells - (size_t)n_prob;
    MatrixLease in;
    DevBuf d_merge, d_height, d_order;
    if ((rc = acquire_input(expr, G * C, nullptr, in)) || (rc = d_merge.alloc(2 * merges * sizeof(int32_t))) ||
        (rc = d_height.alloc(merges * sizeof(double))) || (rc = d_order.alloc(cells * sizeof(int32_t))))
        return rc;
    if ((rc = icnv_hclust_cells_dev(in.dev, G, C, gene_idx, gene_off, cell_idx, cell_off, n_prob, method, d_merge.as<int32_t>(),
                                    d_height.as<double>(), d_order.as<int32_t>(), nullptr)))
        return rc;
    ICNV_HIP(hipMemcpy(merge, d_merge.p, 2 * merges * sizeof(int32_t), hipMemcpyDeviceToHost));
    ICNV_HIP(hipMemcpy(height, d_height.p, merges * sizeof(double), hipMemcpyDeviceToHost));
    ICNV_HIP(hipMemcpy(order, d_order.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost));
    return ICNV_OK;
}

int icnv_hclust_stats(int64_t *out, int32_t n) {
    if (!out || n < 1) ICNV_FAIL(ICNV_ERR_ARG, "bad argument");
    for (int i = 0; i < n && i < 6; ++i) out[i] = g_hc[i].load();
    return ICNV_OK;
}

void icnv_hclust_stats_reset(void) {
    for (auto &c : g_hc) c.store(0);
}

}  // extern "C"
