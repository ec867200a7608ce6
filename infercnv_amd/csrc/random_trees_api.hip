// C ABI of K10 (include/icnv.h "random trees"): .parameterize_random_cluster_heights_smoothed_trees
// (R/inferCNV_tumor_subclusters.random_smoothed_trees.R:217-298) for every clade of a recursion level in one call -- validation,
// the waves under ICNV_RT_SCRATCH_MB and stats.  Kernels: random_trees_kernels.hip; the trees are K9's (hclust_api.hip).
// DESIGN.md section 4 K10.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <numeric>
#include <string>
#include <vector>

#include "icnv_internal.h"
#include "hclust_internal.h"
#include "random_trees_internal.h"

using namespace icnv;

namespace {
std::atomic<int64_t> g_rt[6];   // calls, clades, permuted matrices, waves, chain steps, wall microseconds

int rt_validate(const double *expr, int64_t G, int64_t C, const int32_t *cell_idx, const int32_t *cell_off, int32_t n_prob,
                int32_t window) {
    if (!expr || !cell_idx || !cell_off) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: null argument");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: bad matrix dimensions");
    if (n_prob < 1) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: n_prob must be >= 1");
    if (window < 1) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: window must be >= 1");
    if (cell_off[0] != 0) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: offsets must start at 0");
    for (int32_t p = 0; p < n_prob; ++p) {
        const int64_t np = (int64_t)cell_off[p + 1] - cell_off[p];
        if (np < 2) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: every clade needs at least two cells (clade " + std::to_string(p) + ")");
        if (np > HC_HBM_MAX_N) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "random_trees: more than 524288 cells in one clade");
    }
    for (int64_t i = 0; i < cell_off[n_prob]; ++i)
        if (cell_idx[i] < 0 || cell_idx[i] >= C) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: cell index out of range");
    return ICNV_OK;
}

// The clades' cell lists and tokens on the device, checked for non-finite values (ICNV_ERR_ARG) before anything else runs.
struct RtClades {
    DevBuf d_cidx, d_coff, d_tok;
    std::vector<int64_t> coff;
};

int rt_upload_clades(const double *expr, int32_t G, const int32_t *cell_idx, const int32_t *cell_off, const uint64_t *token,
                     int32_t n_prob, hipStream_t s, RtClades &cl) {
    cl.coff.resize(n_prob + 1);
    for (int32_t p = 0; p <= n_prob; ++p) cl.coff[p] = cell_off[p];
    std::vector<uint64_t> tok(token, token + n_prob);
    int rc;
    DevBuf d_bad;
    uint32_t bad = 0;
    if ((rc = upload(cl.d_cidx, cell_idx, (size_t)cl.coff[n_prob], s)) || (rc = upload(cl.d_coff, cl.coff.data(), cl.coff.size(), s)) ||
        (rc = upload(cl.d_tok, tok.data(), tok.size(), s)) || (rc = d_bad.alloc(sizeof(uint32_t))))
        return rc;
    ICNV_HIP(hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), s));
    if ((rc = launch_rt_check(expr, G, cl.d_cidx.as<int32_t>(), cl.coff[n_prob], d_bad.as<uint32_t>(), s))) return rc;
    ICNV_HIP(hipMemcpyAsync(&bad, d_bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (bad) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: NaN or infinite value among the clades' cells");
    return ICNV_OK;
}

// Items (clade, iteration; -1 = the observed matrix) -> their rows after the stages: m gets the gathered (permuted) rows,
// ld_m doubles apart; z (rows of G doubles) the smoothed and centred ones.
int rt_stage(const double *expr, int32_t G, const RtClades &cl, uint64_t seed, int32_t window, const std::vector<int32_t> &clade,
             const std::vector<int32_t> &iter, const std::vector<int64_t> &row, uint32_t stages, double *m, int64_t ld_m, double *z,
             hipStream_t s) {
    const int n_items = (int)clade.size();
    const int64_t rows = row[n_items];
    int rc;
    DevBuf d_clade, d_iter, d_row;
    if ((rc = upload(d_clade, clade.data(), clade.size(), s)) || (rc = upload(d_iter, iter.data(), iter.size(), s)) ||
        (rc = upload(d_row, row.data(), row.size(), s)))
        return rc;
    RtItems a;
    a.n_items = n_items; a.G = G; a.x = expr;
    a.cell_idx = cl.d_cidx.as<int32_t>(); a.cell_off = cl.d_coff.as<int64_t>();
    a.item_clade = d_clade.as<int32_t>(); a.item_iter = d_iter.as<int32_t>(); a.item_row = d_row.as<int64_t>();
    a.token = cl.d_tok.as<uint64_t>(); a.seed = seed;
    a.m = m; a.ld_m = ld_m; a.z = z; a.window = window;
    if ((rc = launch_rt_permute(a, s))) return rc;
    if (stages & ICNV_RT_SMOOTH) {
        if ((rc = launch_rt_smooth(a, rows, s))) return rc;
    } else {
        ICNV_HIP(hipMemcpy2DAsync(z, (size_t)G * sizeof(double), m, (size_t)ld_m * sizeof(double), (size_t)G * sizeof(double),
                                  (size_t)rows, hipMemcpyDeviceToDevice, s));
    }
    if (stages & ICNV_RT_CENTER) {   // step 11's own median centring (R/inferCNV_ops.R:2098)
        LargeChainArgs c{};
        c.out = z; c.G = G; c.n_rows = (int32_t)rows; c.mask = ICNV_ST_CENTER;
        if ((rc = launch_chain_large_center(c, s))) return rc;
    }
    // the device buffers above are freed when this returns: the stream must be done with them
    ICNV_HIP(hipStreamSynchronize(s));
    return ICNV_OK;
}
}  // namespace

extern "C" {

int icnv_random_trees_dev(const double *expr, int64_t G, int64_t C, const int32_t *cell_idx, const int32_t *cell_off,
                          const uint64_t *token, int32_t n_prob, int32_t window, int32_t n_iter, uint64_t seed, int32_t method,
                          int32_t *merge, double *height, int32_t *order, double *rand_max_height, void *stream) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc = rt_validate(expr, G, C, cell_idx, cell_off, n_prob, window);
    if (rc) return rc;
    if (!token || !merge || !height || !order || !rand_max_height) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: null argument");
    if (n_iter < 1) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: n_iter must be >= 1");
    if ((int64_t)n_prob * (n_iter + 1) > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "random_trees: too many matrices");
    if ((rc = hclust_method_check(method))) return rc;
    hipStream_t s = (hipStream_t)stream;
    RtClades cl;
    if ((rc = rt_upload_clades(expr, (int32_t)G, cell_idx, cell_off, token, n_prob, s, cl))) return rc;

    // waves: the distance matrices of a wave within half the cap (at least one), its matrices built in sub-waves within the other
    // half; every item is computed on its own, so no cap and no batch composition changes a bit
    const int64_t cap = std::max<int64_t>(1, env_int("ICNV_RT_SCRATCH_MB", 8192)) * ((int64_t)1 << 20);
    const int64_t ld = G + (G & 1);
    auto d_bytes = [&](int64_t n) { return n * n * 8 + n * 24 + 64; };
    auto m_bytes = [&](int64_t n) { return n * (ld + G) * 8 + G * 12 + n * 16 + 64; };
    const int64_t total_cells = cl.coff[n_prob], total_merges = total_cells - n_prob;
    std::vector<int32_t> hm(2 * total_merges), ho(total_cells);
    std::vector<double> hh(total_merges);
    const int64_t n_items = (int64_t)n_prob * (n_iter + 1);   // item q: clade q / (n_iter + 1), iteration q % (n_iter + 1) - 1
    auto item_n = [&](int64_t q) { const int64_t p = q / (n_iter + 1); return cl.coff[p + 1] - cl.coff[p]; };
    const bool root = method == ICNV_HCLUST_WARD_D2;
    int64_t waves = 0, steps = 0;
    for (int64_t q0 = 0; q0 < n_items;) {
        int64_t q1 = q0, used = 0;
        while (q1 < n_items && (q1 == q0 || (used + d_bytes(item_n(q1)) <= cap / 2 && q1 - q0 < 65535))) used += d_bytes(item_n(q1++));
        const int nw = (int)(q1 - q0);
        std::vector<int32_t> n(nw);
        std::vector<int64_t> c_off(nw + 1), d_off(nw + 1);
        c_off[0] = d_off[0] = 0;
        for (int i = 0; i < nw; ++i) {
            n[i] = (int32_t)item_n(q0 + i);
            c_off[i + 1] = c_off[i] + n[i];
            d_off[i + 1] = d_off[i] + (int64_t)n[i] * n[i];
        }
        DevBuf d_D;
        if ((rc = d_D.alloc((size_t)d_off[nw] * sizeof(double)))) return rc;
        for (int i0 = 0; i0 < nw;) {   // sub-waves: matrices -> R's sequential dist into D (distance_kernels.hip)
            int i1 = i0;
            int64_t mused = 0;
            while (i1 < nw && (i1 == i0 || mused + m_bytes(n[i1]) <= cap / 2)) mused += m_bytes(n[i1++]);
            const int ns = i1 - i0;
            std::vector<int32_t> clade(ns), iter(ns), ids;
            std::vector<int64_t> row(ns + 1), doff(ns + 1), toff;
            row[0] = 0;
            for (int i = 0; i < ns; ++i) {
                const int64_t q = q0 + i0 + i;
                clade[i] = (int32_t)(q / (n_iter + 1));
                iter[i] = (int32_t)(q % (n_iter + 1)) - 1;
                row[i + 1] = row[i] + n[i0 + i];
                doff[i] = d_off[i0 + i] - d_off[i0];
            }
            const int64_t rows = row[ns];
            if (rows > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "random_trees: sub-wave too large");
            ids.resize(rows);
            std::iota(ids.begin(), ids.end(), 0);
            const int dt = exact_dist_plan(n.data() + i0, ns, toff);
            if (toff[ns] > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "random_trees: sub-wave too large");
            DevBuf d_m, d_z, d_ids, d_row, d_toff, d_n, d_doff;
            if ((rc = d_m.alloc((size_t)rows * ld * sizeof(double))) || (rc = d_z.alloc((size_t)rows * G * sizeof(double))))
                return rc;
            if ((rc = rt_stage(expr, (int32_t)G, cl, seed, window, clade, iter, row, ICNV_RT_PERMUTE | ICNV_RT_SMOOTH | ICNV_RT_CENTER,
                               d_m.as<double>(), ld, d_z.as<double>(), s)))
                return rc;
            if ((rc = upload(d_ids, ids.data(), ids.size(), s)) || (rc = upload(d_row, row.data(), row.size(), s)) ||
                (rc = upload(d_toff, toff.data(), toff.size(), s)) || (rc = upload(d_n, n.data() + i0, (size_t)ns, s)) ||
                (rc = upload(d_doff, doff.data(), doff.size(), s)))
                return rc;
            DistArgs da{};   // the staged cells: row r of the sub-wave at d_z + r G, every gene in order
            da.x = d_z.as<double>(); da.ldx = G; da.G = (int32_t)G;
            da.cell_idx = d_ids.as<int32_t>(); da.cell_off = d_row.as<int64_t>(); da.n = d_n.as<int32_t>();
            da.n_prob = ns; da.tile_off = d_toff.as<int64_t>(); da.d_off = d_doff.as<int64_t>(); da.D = d_D.as<double>() + d_off[i0];
            if ((rc = launch_exact_dist(da, dt, toff[ns], s))) return rc;
            ICNV_HIP(hipStreamSynchronize(s));   // (the sub-wave's buffers go back to the pool here)
            i0 = i1;
        }
        HclustRaw raw;
        if ((rc = hclust_raw(d_D.as<double>(), n, c_off, method, s, raw))) return rc;
        d_D.release();
        // observed trees: labelled as R does (K9); permuted trees: only their maximum height, on the device
        std::vector<int64_t> pm_off, p_out;
        std::vector<int32_t> p_n;
        std::vector<int> obs;
        for (int i = 0; i < nw; ++i) {
            const int64_t q = q0 + i;
            const int64_t p = q / (n_iter + 1), r = q % (n_iter + 1) - 1;
            if (r < 0) {
                obs.push_back(i);
            } else {
                pm_off.push_back(raw.m_off[i]);
                p_n.push_back(n[i]);
                p_out.push_back(p * n_iter + r);
            }
        }
        if (!p_n.empty()) {
            DevBuf d_pm, d_pn, d_po;
            if ((rc = upload(d_pm, pm_off.data(), pm_off.size(), s)) || (rc = upload(d_pn, p_n.data(), p_n.size(), s)) ||
                (rc = upload(d_po, p_out.data(), p_out.size(), s)))
                return rc;
            if ((rc = launch_rt_max_height(raw.d_mh.as<double>(), d_pm.as<int64_t>(), d_pn.as<int32_t>(), d_po.as<int64_t>(),
                                           (int32_t)p_n.size(), root, rand_max_height, s)))
                return rc;
            ICNV_HIP(hipStreamSynchronize(s));
        }
        if (!obs.empty()) {
            std::vector<std::vector<int32_t>> mx(obs.size()), my(obs.size());
            std::vector<std::vector<double>> mh(obs.size());
            for (size_t k = 0; k < obs.size(); ++k) {
                const int i = obs[k];
                const size_t nm = (size_t)n[i] - 1;
                mx[k].resize(nm); my[k].resize(nm); mh[k].resize(nm);
                ICNV_HIP(hipMemcpyAsync(mx[k].data(), raw.d_mx.as<int32_t>() + raw.m_off[i], nm * sizeof(int32_t), hipMemcpyDeviceToHost, s));
                ICNV_HIP(hipMemcpyAsync(my[k].data(), raw.d_my.as<int32_t>() + raw.m_off[i], nm * sizeof(int32_t), hipMemcpyDeviceToHost, s));
                ICNV_HIP(hipMemcpyAsync(mh[k].data(), raw.d_mh.as<double>() + raw.m_off[i], nm * sizeof(double), hipMemcpyDeviceToHost, s));
            }
            ICNV_HIP(hipStreamSynchronize(s));
            for (size_t k = 0; k < obs.size(); ++k) {
                const int64_t p = (q0 + obs[k]) / (n_iter + 1), m0 = cl.coff[p] - p;
                hclust_label(n[obs[k]], mx[k].data(), my[k].data(), mh[k].data(), root, hm.data() + 2 * m0, hh.data() + m0,
                             ho.data() + cl.coff[p]);
            }
        }
        steps += raw.steps;
        ++waves;
        q0 = q1;
    }
    ICNV_HIP(hipMemcpyAsync(merge, hm.data(), hm.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    ICNV_HIP(hipMemcpyAsync(height, hh.data(), hh.size() * sizeof(double), hipMemcpyHostToDevice, s));
    ICNV_HIP(hipMemcpyAsync(order, ho.data(), ho.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    ICNV_HIP(hipStreamSynchronize(s));
    g_rt[0] += 1;
    g_rt[1] += n_prob;
    g_rt[2] += (int64_t)n_prob * n_iter;
    g_rt[3] += waves;
    g_rt[4] += steps;
    g_rt[5] += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return ICNV_OK;
}

int icnv_random_trees(const double *expr, int64_t G, int64_t C, const int32_t *cell_idx, const int32_t *cell_off,
                      const uint64_t *token, int32_t n_prob, int32_t window, int32_t n_iter, uint64_t seed, int32_t method,
                      int32_t *merge, double *height, int32_t *order, double *rand_max_height) {
    int rc = rt_validate(expr, G, C, cell_idx, cell_off, n_prob, window);
    if (rc) return rc;
    if (!token || !merge || !height || !order || !rand_max_height) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: null argument");
    if (n_iter < 1) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: n_iter must be >= 1");
    if ((rc = hclust_method_check(method))) return rc;
    const size_t cells = (size_t)cell_off[n_prob], merges = cells - (size_t)n_prob, nr = (size_t)n_prob * n_iter;
    MatrixLease in;
    DevBuf d_merge, d_height, d_order, d_rand;
    if ((rc = acquire_input(expr, G * C, nullptr, in)) || (rc = d_merge.alloc(2 * merges * sizeof(int32_t))) ||
        (rc = d_height.alloc(merges * sizeof(double))) || (rc = d_order.alloc(cells * sizeof(int32_t))) ||
        (rc = d_rand.alloc(nr * sizeof(double))))
        return rc;
    if ((rc = icnv_random_trees_dev(in.dev, G, C, cell_idx, cell_off, token, n_prob, window, n_iter, seed, method,
                                    d_merge.as<int32_t>(), d_height.as<double>(), d_order.as<int32_t>(), d_rand.as<double>(), nullptr)))
        return rc;
    ICNV_HIP(hipMemcpy(merge, d_merge.p, 2 * merges * sizeof(int32_t), hipMemcpyDeviceToHost));
    ICNV_HIP(hipMemcpy(height, d_height.p, merges * sizeof(double), hipMemcpyDeviceToHost));
    ICNV_HIP(hipMemcpy(order, d_order.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost));
    ICNV_HIP(hipMemcpy(rand_max_height, d_rand.p, nr * sizeof(double), hipMemcpyDeviceToHost));
    return ICNV_OK;
}

int icnv_random_trees_matrix_dev(const double *expr, int64_t G, int64_t C, const int32_t *cells, int32_t n, int32_t window,
                                 uint64_t seed, uint64_t token, int32_t iter, uint32_t stages, double *out, void *stream) {
    const int32_t off[2] = {0, n};
    int rc = rt_validate(expr, G, C, cells, off, 1, window);
    if (rc) return rc;
    if (!out) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: null argument");
    if (iter < -1) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: iter must be >= -1");
    if (stages & ~(uint32_t)(ICNV_RT_PERMUTE | ICNV_RT_SMOOTH | ICNV_RT_CENTER)) ICNV_FAIL(ICNV_ERR_ARG, "random_trees: unknown stage bits");
    hipStream_t s = (hipStream_t)stream;
    RtClades cl;
    if ((rc = rt_upload_clades(expr, (int32_t)G, cells, off, &token, 1, s, cl))) return rc;
    const int64_t ld = G + (G & 1);
    DevBuf d_m;
    if ((rc = d_m.alloc((size_t)n * ld * sizeof(double)))) return rc;
    const int32_t it = (stages & ICNV_RT_PERMUTE) ? iter : -1;
    return rt_stage(expr, (int32_t)G, cl, seed, window, {0}, {it}, {0, n}, stages, d_m.as<double>(), ld, out, s);
}

int icnv_random_trees_stats(int64_t *out, int32_t n) {
    if (!out || n < 1) ICNV_FAIL(ICNV_ERR_ARG, "bad argument");
    for (int i = 0; i < n && i < 6; ++i) out[i] = g_rt[i].load();
    return ICNV_OK;
}

void icnv_random_trees_stats_reset(void) {
    for (auto &c : g_rt) c.store(0);
}

}  // extern "C"
