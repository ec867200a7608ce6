// C ABI of K8 (include/icnv.h "exact kNN"): RANN::nn2(t(expr_data), k = k_nn) per problem (R/inferCNV_tumor_subclusters.R:726) --
// validation, the row blocks under ICNV_KNN_SCRATCH_MB, the per-device counters and stats.  Kernels: knn_kernels.hip.
// DESIGN.md section 4 K8.
#include <algorithm>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "icnv_internal.h"
#include "knn_internal.h"

using namespace icnv;

namespace {
std::atomic<int64_t> g_knn_host[6];   // calls, problems, query rows, row blocks, screened rows, forced-exhaustive rows
std::mutex g_knn_mu;
std::map<int, int64_t *> g_knn_dev;   // per device: KNN_STAT_DEVICE_N counters

int knn_device_counters(int64_t **out) {
    int dev = 0;
    ICNV_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_knn_mu);
    int64_t *&p = g_knn_dev[dev];
    if (!p) {
        ICNV_HIP(hipMalloc(&p, KNN_STAT_DEVICE_N * sizeof(int64_t)));
        ICNV_HIP(hipMemset(p, 0, KNN_STAT_DEVICE_N * sizeof(int64_t)));
    }
    *out = p;
    return ICNV_OK;
}

// every check before any device work: offsets, sizes, k, every gene and cell index
int knn_validate(const double *expr, int64_t G, int64_t C, const int32_t *gene_idx, const int32_t *gene_off, const int32_t *cell_idx,
                 const int32_t *cell_off, int32_t n_prob, int32_t k, const void *nn_idx, const void *nn_dist) {
    if (!expr || !nn_idx || !nn_dist || !gene_idx || !gene_off || !cell_idx || !cell_off) ICNV_FAIL(ICNV_ERR_ARG, "knn: null argument");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "knn: bad matrix dimensions");
    if (n_prob < 1) ICNV_FAIL(ICNV_ERR_ARG, "knn: n_prob must be >= 1");
    if (k < 1) ICNV_FAIL(ICNV_ERR_ARG, "knn: k must be >= 1");
    if (gene_off[0] != 0 || cell_off[0] != 0) ICNV_FAIL(ICNV_ERR_ARG, "knn: offsets must start at 0");
    for (int32_t p = 0; p < n_prob; ++p) {
        if (gene_off[p + 1] <= gene_off[p]) ICNV_FAIL(ICNV_ERR_ARG, "knn: every problem needs at least one gene");
        if (cell_off[p + 1] <= cell_off[p]) ICNV_FAIL(ICNV_ERR_ARG, "knn: every problem needs at least one cell");
        if (k > cell_off[p + 1] - cell_off[p]) ICNV_FAIL(ICNV_ERR_ARG, "knn: k exceeds the cells of problem " + std::to_string(p));
    }
    if (k > KNN_MAX_K) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "knn: k > 128 is not supported");
    for (int64_t i = 0; i < gene_off[n_prob]; ++i)
        if (gene_idx[i] < 0 || gene_idx[i] >= G) ICNV_FAIL(ICNV_ERR_ARG, "knn: gene index out of range");
    for (int64_t i = 0; i < cell_off[n_prob]; ++i)
        if (cell_idx[i] < 0 || cell_idx[i] >= C) ICNV_FAIL(ICNV_ERR_ARG, "knn: cell index out of range");
    return ICNV_OK;
}

struct KnnPlanBlock {
    std::vector<int32_t> i32;   // piece_prob | piece_r0 | piece_nr
    std::vector<int64_t> i64;   // tile_off (n + 1) | row_off (n + 1) | piece_scr (n)
    int64_t n_tiles = 0, n_rows = 0, entries = 0;
    int wm = 2;
    DevBuf d_i32, d_i64;
};
}  // namespace

extern "C" {

int icnv_knn_dev(const double *expr, int64_t G, int64_t C, const int32_t *gene_idx, const int32_t *gene_off, const int32_t *cell_idx,
                 const int32_t *cell_off, int32_t n_prob, int32_t k, int32_t *nn_idx, double *nn_dist, void *stream) {
    int rc = knn_validate(expr, G, C, gene_idx, gene_off, cell_idx, cell_off, n_prob, k, nn_idx, nn_dist);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool all_exact = env_int("ICNV_KNN_EXHAUSTIVE", 0) != 0;
    const int64_t budget = std::max<int64_t>(1, env_int("ICNV_KNN_SCRATCH_MB", 4096)) * ((int64_t)1 << 20) / 8;   // 8-byte screen entries
    const int cap = (int)std::max<int64_t>(1, std::min<int64_t>(KNN_MAX_CAP, env_int("ICNV_KNN_CAP", KNN_DEFAULT_CAP)));
    const int64_t max_block_rows = ((int64_t)256 << 20) / ((int64_t)cap * 4);   // candidate lists <= 256 MB

    // problems: 64-bit offsets, padded row length, compact-matrix offsets
    std::vector<int64_t> goff(n_prob + 1), coff(n_prob + 1), yoff(n_prob + 1);
    std::vector<int32_t> ld(n_prob);
    for (int32_t p = 0; p <= n_prob; ++p) { goff[p] = gene_off[p]; coff[p] = cell_off[p]; }
    yoff[0] = 0;
    for (int32_t p = 0; p < n_prob; ++p) {
        const int64_t Gp = goff[p + 1] - goff[p];
        ld[p] = (int32_t)(Gp + (Gp & 1));
        yoff[p + 1] = yoff[p] + (coff[p + 1] - coff[p]) * ld[p];
    }
    const int64_t total_rows = coff[n_prob], total_genes = goff[n_prob];

    // row blocks: pieces (problem, rows) whose screens together fit the budget (at least one row per block)
    std::vector<std::unique_ptr<KnnPlanBlock>> blocks;
    {
        std::vector<int32_t> pp, pr0, pnr;
        int64_t used = 0, rows = 0;
        auto close = [&]() {
            if (pp.empty()) return;
            auto b = std::make_unique<KnnPlanBlock>();
            const int n = (int)pp.size();
            int64_t t128 = 0;
            for (int i = 0; i < n; ++i) {
                const int64_t np = coff[pp[i] + 1] - coff[pp[i]];
                t128 += ((pnr[i] + 127) / 128) * ((np + 127) / 128);
            }
            b->wm = t128 >= 2 * (int64_t)num_cus() ? 4 : 2;
            const int DT = 32 * b->wm;
            b->i32.insert(b->i32.end(), pp.begin(), pp.end());
            b->i32.insert(b->i32.end(), pr0.begin(), pr0.end());
            b->i32.insert(b->i32.end(), pnr.begin(), pnr.end());
            b->i64.assign(3 * (size_t)n + 2, 0);
            int64_t *toff = b->i64.data(), *roff = toff + n + 1, *soff = roff + n + 1;
            for (int i = 0; i < n; ++i) {
                const int64_t np = coff[pp[i] + 1] - coff[pp[i]];
                toff[i + 1] = toff[i] + ((pnr[i] + DT - 1) / DT) * ((np + DT - 1) / DT);
                roff[i + 1] = roff[i] + pnr[i];
                soff[i] = b->entries;
                b->entries += (int64_t)pnr[i] * np;
            }
            b->n_tiles = toff[n];
            b->n_rows = roff[n];
            blocks.push_back(std::move(b));
            pp.clear(); pr0.clear(); pnr.clear();
            used = rows = 0;
        };
        for (int32_t p = 0; p < n_prob; ++p) {
            const int64_t np = coff[p + 1] - coff[p];
            int64_t r = 0;
            while (r < np) {
                int64_t nr = std::min({np - r, (budget - used) / np, max_block_rows - rows});
                if (nr < 1) {
                    if (!pp.empty()) { close(); continue; }
                    nr = 1;
                }
                pp.push_back(p); pr0.push_back((int32_t)r); pnr.push_back((int32_t)nr);
                used += nr * np; rows += nr; r += nr;
            }
        }
        close();
    }
    for (auto &b : blocks)
        if (b->n_tiles > 0x7fffffff || b->n_rows > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "knn: row block too large");
    if (total_genes > ((int64_t)1 << 31) * 255 || total_rows > 0x7fffffff) ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "knn: batch too large");

    int64_t *stats = nullptr;
    if ((rc = knn_device_counters(&stats))) return rc;
    DevBuf d_gidx, d_goff, d_cidx, d_coff, d_yoff, d_ld, d_shift, d_Y, d_norm, d_screen, d_cand, d_ncand;
    int64_t max_entries = 0, max_rows = 0;
    for (auto &b : blocks) { max_entries = std::max(max_entries, b->entries); max_rows = std::max(max_rows, b->n_rows); }
    if ((rc = upload(d_gidx, gene_idx, (size_t)total_genes, s)) || (rc = upload(d_goff, goff.data(), goff.size(), s)) ||
        (rc = upload(d_cidx, cell_idx, (size_t)total_rows, s)) || (rc = upload(d_coff, coff.data(), coff.size(), s)) ||
        (rc = upload(d_yoff, yoff.data(), yoff.size(), s)) || (rc = upload(d_ld, ld.data(), ld.size(), s)) ||
        (rc = d_norm.alloc((size_t)total_rows * sizeof(double))) || (rc = d_screen.alloc((size_t)max_entries * 8)) ||
        (rc = d_cand.alloc((size_t)max_rows * cap * sizeof(int32_t))) || (rc = d_ncand.alloc((size_t)max_rows * sizeof(int32_t))))
        return rc;
    if (!all_exact && ((rc = d_shift.alloc((size_t)total_genes * sizeof(double))) || (rc = d_Y.alloc((size_t)yoff[n_prob] * sizeof(double)))))
        return rc;
    for (auto &b : blocks)
        if ((rc = upload(b->d_i32, b->i32.data(), b->i32.size(), s)) || (rc = upload(b->d_i64, b->i64.data(), b->i64.size(), s))) return rc;

    KnnArgs a;
    a.x = expr; a.G = (int32_t)G;
    a.gene_idx = d_gidx.as<int32_t>(); a.gene_off = d_goff.as<int64_t>();
    a.cell_idx = d_cidx.as<int32_t>(); a.cell_off = d_coff.as<int64_t>();
    a.n_prob = n_prob; a.k = k; a.total_genes = total_genes; a.total_rows = total_rows;
    a.shift = d_shift.as<double>(); a.Y = d_Y.as<double>(); a.y_off = d_yoff.as<int64_t>(); a.ld = d_ld.as<int32_t>();
    a.norm = d_norm.as<double>(); a.nn_idx = nn_idx; a.nn_dist = nn_dist; a.stats = stats;
    if (!all_exact && (rc = launch_knn_prepare(a, s))) return rc;
    for (auto &pb : blocks) {
        KnnBlock b;
        const int n = (int)(pb->i32.size() / 3);
        b.n_pieces = n;
        b.piece_prob = pb->d_i32.as<int32_t>(); b.piece_r0 = b.piece_prob + n; b.piece_nr = b.piece_r0 + n;
        b.tile_off = pb->d_i64.as<int64_t>(); b.row_off = b.tile_off + n + 1; b.piece_scr = b.row_off + n + 1;
        b.n_tiles = pb->n_tiles; b.n_rows = pb->n_rows;
        b.screen = d_screen.as<uint32_t>(); b.cand = d_cand.as<int32_t>(); b.ncand = d_ncand.as<int32_t>();
        b.cap = cap; b.all_exact = all_exact ? 1 : 0;
        if ((rc = launch_knn_block(a, b, pb->wm, s))) return rc;
    }
    g_knn_host[0] += 1;
    g_knn_host[1] += n_prob;
    g_knn_host[2] += total_rows;
    g_knn_host[3] += (int64_t)blocks.size();
    g_knn_host[all_exact ? 5 : 4] += total_rows;
    return ICNV_OK;
}

int icnv_knn(const double *expr, int64_t G, int64_t C, const int32_t *gene_idx, const int32_t *gene_off, const int32_t *cell_idx,
             const int32_t *cell_off, int32_t n_prob, int32_t k, int32_t *nn_idx, double *nn_dist) {
    int rc = knn_validate(expr, G, C, gene_idx, gene_off, cell_idx, cell_off, n_prob, k, nn_idx, nn_dist);
    if (rc) return rc;
    const size_t n_out = (size_t)cell_off[n_prob] * k;
    MatrixLease in;
    DevBuf d_idx, d_dist;
    if ((rc = acquire_input(expr, G * C, nullptr, in)) || (rc = d_idx.alloc(n_out * sizeof(int32_t))) ||
        (rc = d_dist.alloc(n_out * sizeof(double))))
        return rc;
    if ((rc = icnv_knn_dev(in.dev, G, C, gene_idx, gene_off, cell_idx, cell_off, n_prob, k, d_idx.as<int32_t>(), d_dist.as<double>(),
                           nullptr)))
        return rc;
    ICNV_HIP(hipMemcpy(nn_idx, d_idx.p, n_out * sizeof(int32_t), hipMemcpyDeviceToHost));
    ICNV_HIP(hipMemcpy(nn_dist, d_dist.p, n_out * sizeof(double), hipMemcpyDeviceToHost));
    return ICNV_OK;
}

int icnv_knn_stats(int64_t *out, int32_t n) {
    if (!out || n < 1) ICNV_FAIL(ICNV_ERR_ARG, "bad argument");
    int64_t v[9] = {g_knn_host[0].load(), g_knn_host[1].load(), g_knn_host[2].load(), g_knn_host[3].load(), g_knn_host[4].load(), 0, 0,
                    0, g_knn_host[5].load()};
    std::lock_guard<std::mutex> lk(g_knn_mu);
    if (!g_knn_dev.empty()) {
        int cur = 0;
        ICNV_HIP(hipGetDevice(&cur));
        for (auto &kv : g_knn_dev) {
            int64_t h[KNN_STAT_DEVICE_N];
            ICNV_HIP(hipSetDevice(kv.first));
            ICNV_HIP(hipDeviceSynchronize());
            ICNV_HIP(hipMemcpy(h, kv.second, sizeof(h), hipMemcpyDeviceToHost));
            v[5] += h[KNN_STAT_CANDIDATES];
            v[6] += h[KNN_STAT_OVERFLOW_ROWS];
            v[7] += h[KNN_STAT_EXACT_ROWS];
        }
        ICNV_HIP(hipSetDevice(cur));
    }
    for (int i = 0; i < n && i < 9; ++i) out[i] = v[i];
    return ICNV_OK;
}

void icnv_knn_stats_reset(void) {
    for (auto &c : g_knn_host) c.store(0);
    std::lock_guard<std::mutex> lk(g_knn_mu);
    int cur = 0;
    if (hipGetDevice(&cur) != hipSuccess) { (void)hipGetLastError(); return; }
    for (auto &kv : g_knn_dev) {
        if (hipSetDevice(kv.first) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
            hipMemset(kv.second, 0, KNN_STAT_DEVICE_N * sizeof(int64_t)) != hipSuccess)
            (void)hipGetLastError();
    }
    (void)hipSetDevice(cur);
}

}  // extern "C"
