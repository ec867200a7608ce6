// C ABI of K12 (include/icnv.h "non-DE gene masking"): validation, the involved groups, waves of genes under
// ICNV_DE_SCRATCH_MB, the cached exact Mann-Whitney table, BH and the mask.  Kernels: de_kernels.hip.  DESIGN.md section 4 K12.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "icnv_internal.h"
#include "de_internal.h"

using namespace icnv;

namespace {

std::atomic<int64_t> g_de[7];   // calls, comparisons, genes, LDS segments, HBM segments, waves, wall microseconds

// the exact two-sided p-values of every (n.x, n.y) <= 49: built once on the host, one device copy per device
struct ExactDev { double *p = nullptr; int64_t *off = nullptr; };
std::mutex g_exact_mu;
std::map<int, ExactDev> g_exact_dev;

int exact_table(ExactDev &out) {
    static std::vector<int64_t> off;
    static std::vector<double> p;
    static std::once_flag once;
    std::call_once(once, [] { de_exact_table_host(off, p); });
    int dev = 0;
    ICNV_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lk(g_exact_mu);
    auto it = g_exact_dev.find(dev);
    if (it != g_exact_dev.end()) { out = it->second; return ICNV_OK; }
    ExactDev e;
    ICNV_HIP(hipMalloc((void **)&e.p, p.size() * sizeof(double)));
    ICNV_HIP(hipMalloc((void **)&e.off, off.size() * sizeof(int64_t)));
    ICNV_HIP(hipMemcpy(e.p, p.data(), p.size() * sizeof(double), hipMemcpyHostToDevice));
    ICNV_HIP(hipMemcpy(e.off, off.data(), off.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    g_exact_dev[dev] = e;
    out = e;
    return ICNV_OK;
}

int64_t scratch_cap_bytes() {
    const char *e = std::getenv("ICNV_DE_SCRATCH_MB");
    const int64_t mb = (e && *e) ? std::atoll(e) : 8192;
    return std::max<int64_t>(1, mb) << 20;
}

int de_validate(const double *expr, int64_t G, int64_t C, int64_t ld, const int32_t *cell_idx, const int32_t *cell_off,
                int32_t n_groups, const int32_t *cmp, int32_t n_cmp, int32_t test, const void *stat, const void *p, const void *padj) {
    if (!expr || !cell_idx || !cell_off || !cmp || !stat || !p || !padj) ICNV_FAIL(ICNV_ERR_ARG, "de_tests: null argument");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff || ld < G) ICNV_FAIL(ICNV_ERR_ARG, "de_tests: bad matrix dimensions");
    if (n_groups < 1 || n_cmp < 1) ICNV_FAIL(ICNV_ERR_ARG, "de_tests: n_groups and n_cmp must be >= 1");
    if (test != ICNV_DE_WILCOXON && test != ICNV_DE_T) ICNV_FAIL(ICNV_ERR_ARG, "de_tests: unknown test " + std::to_string(test));
    if (cell_off[0] != 0) ICNV_FAIL(ICNV_ERR_ARG, "de_tests: offsets must start at 0");
    for (int32_t q = 0; q < n_groups; ++q)
        if (cell_off[q + 1] < cell_off[q]) ICNV_FAIL(ICNV_ERR_ARG, "de_tests: offsets must be monotone");
    for (int64_t i = 0; i < cell_off[n_groups]; ++i)
        if (cell_idx[i] < 0 || cell_idx[i] >= C) ICNV_FAIL(ICNV_ERR_ARG, "de_tests: cell index out of range");
    for (int32_t k = 0; k < 2 * n_cmp; ++k)
        if (cmp[k] < 0 || cmp[k] >= n_groups) ICNV_FAIL(ICNV_ERR_ARG, "de_tests: comparison group out of range");
    return ICNV_OK;
}

// sorts `count` segments of n keys at keys + base in place or into `other`; returns the buffer they end in
int sort_segments(double *keys, double *other, const DeSegs &g, hipStream_t s, double **result) {
    int rc;
    DevBuf d_seg, d_off;
    const int64_t chunks[2] = {0, (int64_t)g.count * (((int64_t)g.n + DE_CHUNK - 1) / DE_CHUNK)};
    if ((rc = upload(d_seg, &g, 1, s)) || (rc = upload(d_off, chunks, 2, s))) return rc;
    if ((rc = launch_de_sort_chunks(keys, d_seg.as<DeSegs>(), d_off.as<int64_t>(), 1, chunks[1], s))) return rc;
    double *src = keys, *dst = other;
    for (int64_t run = DE_CHUNK; run < g.n; run *= 2) {
        if ((rc = launch_de_merge_pass(src, dst, g, run, s))) return rc;
        std::swap(src, dst);
    }
    *result = src;
    ICNV_HIP(hipStreamSynchronize(s));
    return ICNV_OK;
}

}  // namespace

extern "C" {

int icnv_de_tests_dev(const double *expr, int64_t G, int64_t C, int64_t ld, const int32_t *cell_idx, const int32_t *cell_off,
                      int32_t n_groups, const int32_t *cmp, int32_t n_cmp, int32_t test, int32_t jitter, uint64_t seed,
                      double *stat, double *p, double *padj, void *stream) {
    const auto t0 = std::chrono::steady_clock::now();
    int rc = de_validate(expr, G, C, ld, cell_idx, cell_off, n_groups, cmp, n_cmp, test, stat, p, padj);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;

    // the groups some comparison uses, numbered by first use
    std::vector<int32_t> gid((size_t)n_groups, -1), used, cmp2((size_t)2 * n_cmp);
    for (int32_t k = 0; k < 2 * n_cmp; ++k) {
        if (gid[cmp[k]] < 0) { gid[cmp[k]] = (int32_t)used.size(); used.push_back(cmp[k]); }
        cmp2[k] = gid[cmp[k]];
    }
    const int32_t ng = (int32_t)used.size();
    std::vector<int32_t> cidx, nk((size_t)ng);
    std::vector<int64_t> coff((size_t)ng + 1, 0);
    for (int32_t q = 0; q < ng; ++q) {
        const int32_t b = cell_off[used[q]], e = cell_off[used[q] + 1];
        cidx.insert(cidx.end(), cell_idx + b, cell_idx + e);
        nk[q] = e - b;
        coff[q + 1] = coff[q] + nk[q];
    }
    DevBuf d_cidx, d_coff, d_cmp;
    if ((rc = upload(d_cidx, cidx.data(), cidx.size(), s)) || (rc = upload(d_coff, coff.data(), coff.size(), s)) ||
        (rc = upload(d_cmp, cmp2.data(), cmp2.size(), s)))
        return rc;

    int64_t n_lds = 0, n_hbm = 0, waves = 0;
    if (test == ICNV_DE_T) {
        DevBuf d_mom;
        if ((rc = d_mom.alloc((size_t)ng * 4 * G * sizeof(double)))) return rc;
        DeWelch a{};
        a.x = expr; a.ld = ld; a.cell_idx = d_cidx.as<int32_t>(); a.cell_off = d_coff.as<int64_t>();
        a.n_groups = ng; a.G = (int32_t)G; a.mom = d_mom.as<double>(); a.cmp = d_cmp.as<int32_t>(); a.n_cmp = n_cmp;
        a.stat = stat; a.p = p;
        if ((rc = launch_de_welch(a, s))) return rc;
        ICNV_HIP(hipStreamSynchronize(s));
    } else {
        ExactDev ex;
        if ((rc = exact_table(ex))) return rc;
        const int64_t per_gene = std::max<int64_t>(coff[ng], 1) * 16;   // two key buffers
        const int64_t gw_max = std::max<int64_t>(1, std::min<int64_t>(G, scratch_cap_bytes() / per_gene));
        DevBuf d_a, d_b, d_err, d_n, d_which;
        if ((rc = d_a.alloc((size_t)std::max<int64_t>(coff[ng], 1) * gw_max * sizeof(double))) ||
            (rc = d_b.alloc((size_t)std::max<int64_t>(coff[ng], 1) * gw_max * sizeof(double))) || (rc = d_err.alloc(sizeof(uint64_t))) ||
            (rc = upload(d_n, nk.data(), nk.size(), s)))
            return rc;
        ICNV_HIP(hipMemsetAsync(d_err.p, 0xff, sizeof(uint64_t), s));
        for (int32_t q = 0; q < ng; ++q) (nk[q] <= DE_CHUNK ? n_lds : n_hbm) += G;
        for (int64_t g0 = 0; g0 < G; g0 += gw_max) {
            const int64_t gw = std::min<int64_t>(gw_max, G - g0);
            std::vector<int64_t> seg_base((size_t)ng), tile_off((size_t)ng + 1, 0), chunk_off((size_t)ng + 1, 0);
            std::vector<DeSegs> segs((size_t)ng);
            std::vector<int8_t> which((size_t)ng, 0);
            for (int32_t q = 0; q < ng; ++q) {
                seg_base[q] = coff[q] * gw;
                tile_off[q + 1] = tile_off[q] + ((int64_t)nk[q] + 63) / 64 * ((gw + 63) / 64);
                chunk_off[q + 1] = chunk_off[q] + gw * (((int64_t)nk[q] + DE_CHUNK - 1) / DE_CHUNK);
                segs[q].base = seg_base[q]; segs[q].n = nk[q]; segs[q].count = (int32_t)gw;
            }
            if (tile_off[ng] > 0x7fffffff || chunk_off[ng] > 0x7fffffff || (coff[ng] * gw + 255) / 256 > 0x7fffffff)
                ICNV_FAIL(ICNV_ERR_UNSUPPORTED, "de_tests: wave too large (lower ICNV_DE_SCRATCH_MB)");
            DevBuf d_base, d_tile, d_chunk, d_segs;
            if ((rc = upload(d_base, seg_base.data(), seg_base.size(), s)) || (rc = upload(d_tile, tile_off.data(), tile_off.size(), s)) ||
                (rc = upload(d_chunk, chunk_off.data(), chunk_off.size(), s)) || (rc = upload(d_segs, segs.data(), segs.size(), s)))
                return rc;
            DeGather ga{};
            ga.x = expr; ga.ld = ld; ga.cell_idx = d_cidx.as<int32_t>(); ga.cell_off = d_coff.as<int64_t>();
            ga.seg_base = d_base.as<int64_t>(); ga.tile_off = d_tile.as<int64_t>(); ga.n_groups = ng; ga.g0 = (int32_t)g0;
            ga.gw = (int32_t)gw; ga.jitter = jitter ? 1 : 0; ga.seed = seed; ga.keys = d_a.as<double>();
            if ((rc = launch_de_gather(ga, tile_off[ng], s))) return rc;
            if ((rc = launch_de_sort_chunks(d_a.as<double>(), d_segs.as<DeSegs>(), d_chunk.as<int64_t>(), ng, chunk_off[ng], s))) return rc;
            for (int32_t q = 0; q < ng; ++q) {   // segments beyond one LDS chunk: merge passes through HBM
                double *src = d_a.as<double>(), *dst = d_b.as<double>();
                for (int64_t run = DE_CHUNK; run < nk[q]; run *= 2) {
                    if ((rc = launch_de_merge_pass(src, dst, segs[q], run, s))) return rc;
                    std::swap(src, dst);
                    which[q] ^= 1;
                }
            }
            if ((rc = upload(d_which, which.data(), which.size(), s))) return rc;
            DeWilcox wa{};
            wa.buf[0] = d_a.as<double>(); wa.buf[1] = d_b.as<double>();
            wa.seg_base = d_base.as<int64_t>(); wa.n = d_n.as<int32_t>(); wa.which = d_which.as<int8_t>(); wa.cmp = d_cmp.as<int32_t>();
            wa.exact_p = ex.p; wa.exact_off = ex.off; wa.n_cmp = n_cmp; wa.g0 = (int32_t)g0; wa.gw = (int32_t)gw; wa.G = (int32_t)G;
            wa.stat = stat; wa.p = p; wa.err = d_err.as<unsigned long long>();
            if ((rc = launch_de_wilcox(wa, s))) return rc;
            ICNV_HIP(hipStreamSynchronize(s));   // the wave's small buffers go back to the pool
            ++waves;
        }
        uint64_t err = 0;
        ICNV_HIP(hipMemcpy(&err, d_err.p, sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (err != ~(uint64_t)0) {
            const int64_t k = (int64_t)(err / (uint64_t)G), g = (int64_t)(err % (uint64_t)G);
            ICNV_FAIL(ICNV_ERR_ARG, "de_tests: comparison " + std::to_string(k) + " (groups " + std::to_string(cmp[2 * k]) + ", " +
                                        std::to_string(cmp[2 * k + 1]) + "), gene " + std::to_string(g) +
                                        ": not enough (non-missing) observations (a sample without finite values)");
        }
    }

    // BH per comparison row
    {
        const int64_t n = (int64_t)n_cmp * G;
        DevBuf d_k0, d_k1, d_sm;
        if ((rc = d_k0.alloc((size_t)n * sizeof(double))) || (rc = d_k1.alloc((size_t)n * sizeof(double))) ||
            (rc = d_sm.alloc((size_t)n * sizeof(double))))
            return rc;
        if ((rc = launch_de_bh_keys(p, d_k0.as<double>(), n, s))) return rc;
        DeSegs rows{0, (int32_t)G, n_cmp};
        double *sorted = nullptr;
        if ((rc = sort_segments(d_k0.as<double>(), d_k1.as<double>(), rows, s, &sorted))) return rc;
        if ((rc = launch_de_bh_finish(p, sorted, d_sm.as<double>(), padj, n_cmp, (int32_t)G, s))) return rc;
        ICNV_HIP(hipStreamSynchronize(s));
    }
    g_de[0] += 1;
    g_de[1] += n_cmp;
    g_de[2] += G;
    g_de[3] += n_lds;
    g_de[4] += n_hbm;
    g_de[5] += waves;
    g_de[6] += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    return ICNV_OK;
}

int icnv_de_tests(const double *expr, int64_t G, int64_t C, const int32_t *cell_idx, const int32_t *cell_off, int32_t n_groups,
                  const int32_t *cmp, int32_t n_cmp, int32_t test, int32_t jitter, uint64_t seed, double *stat, double *p,
                  double *padj) {
    int rc = de_validate(expr, G, C, G, cell_idx, cell_off, n_groups, cmp, n_cmp, test, stat, p, padj);
    if (rc) return rc;
    const size_t n = (size_t)n_cmp * G;
    MatrixLease in;
    DevBuf d_stat, d_p, d_padj;
    if ((rc = acquire_input(expr, G * C, nullptr, in)) || (rc = d_stat.alloc(n * sizeof(double))) || (rc = d_p.alloc(n * sizeof(double))) ||
        (rc = d_padj.alloc(n * sizeof(double))))
        return rc;
    if ((rc = icnv_de_tests_dev(in.dev, G, C, G, cell_idx, cell_off, n_groups, cmp, n_cmp, test, jitter, seed, d_stat.as<double>(),
                                d_p.as<double>(), d_padj.as<double>(), nullptr)))
        return rc;
    ICNV_HIP(hipMemcpy(stat, d_stat.p, n * sizeof(double), hipMemcpyDeviceToHost));
    ICNV_HIP(hipMemcpy(p, d_p.p, n * sizeof(double), hipMemcpyDeviceToHost));
    ICNV_HIP(hipMemcpy(padj, d_padj.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return ICNV_OK;
}

int icnv_mask_non_de_dev(const double *expr, int64_t G, int64_t C, int64_t ld, const double *padj, int32_t n_cmp,
                         double p_val_thresh, const int32_t *base, const int32_t *cc_off, const int32_t *cc_idx, int32_t n_normal,
                         int32_t rule, int32_t use_mean, double mask_val, double *out, int64_t ld_out, double *mean_out,
                         void *stream) {
    if (!expr || !base || !cc_off || !out || (n_cmp > 0 && !padj)) ICNV_FAIL(ICNV_ERR_ARG, "mask_non_de: null argument");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff || ld < G || ld_out < G) ICNV_FAIL(ICNV_ERR_ARG, "mask_non_de: bad matrix dimensions");
    if (n_cmp < 0) ICNV_FAIL(ICNV_ERR_ARG, "mask_non_de: n_cmp must be >= 0");
    if (rule != ICNV_DE_MASK_ANY && rule != ICNV_DE_MASK_MOST && rule != ICNV_DE_MASK_ALL)
        ICNV_FAIL(ICNV_ERR_ARG, "mask_non_de: unknown rule " + std::to_string(rule));
    if (out == expr && ld_out != ld) ICNV_FAIL(ICNV_ERR_ARG, "mask_non_de: in place needs ld_out == ld");
    if (cc_off[0] != 0) ICNV_FAIL(ICNV_ERR_ARG, "mask_non_de: offsets must start at 0");
    for (int64_t c = 0; c < C; ++c)
        if (cc_off[c + 1] < cc_off[c]) ICNV_FAIL(ICNV_ERR_ARG, "mask_non_de: offsets must be monotone");
    if (cc_off[C] > 0 && !cc_idx) ICNV_FAIL(ICNV_ERR_ARG, "mask_non_de: null argument");
    for (int64_t i = 0; i < cc_off[C]; ++i)
        if (cc_idx[i] < 0 || cc_idx[i] >= n_cmp) ICNV_FAIL(ICNV_ERR_ARG, "mask_non_de: comparison index out of range");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    DevBuf d_base, d_off, d_idx, d_part, d_mean;
    if ((rc = upload(d_base, base, (size_t)C, s)) || (rc = upload(d_off, cc_off, (size_t)C + 1, s)) || (rc = upload(d_idx, cc_idx, (size_t)cc_off[C], s)) ||
        (rc = d_mean.alloc(sizeof(double))))
        return rc;
    if (use_mean) {
        if ((rc = d_part.alloc((size_t)de_mean_parts() * 3 * sizeof(double)))) return rc;
        if ((rc = launch_de_mean(expr, ld, (int32_t)G, (int32_t)C, d_part.as<double>(), d_mean.as<double>(), s))) return rc;
    }
    double used = mask_val;
    if (use_mean) {   // the mean first: an in-place mask must not change what it is taken over
        ICNV_HIP(hipMemcpyAsync(&used, d_mean.p, sizeof(double), hipMemcpyDeviceToHost, s));
        ICNV_HIP(hipStreamSynchronize(s));
    }
    DeMask m{};
    m.x = expr; m.ld = ld; m.out = out; m.ld_out = ld_out; m.G = (int32_t)G; m.C = (int32_t)C; m.padj = padj;
    m.thresh = p_val_thresh; m.base = d_base.as<int32_t>(); m.cc_off = d_off.as<int32_t>(); m.cc_idx = d_idx.as<int32_t>();
    m.n_normal = n_normal; m.rule = rule; m.use_mean = 0; m.value = used; m.mean = d_mean.as<double>();
    if ((rc = launch_de_mask(m, s))) return rc;
    ICNV_HIP(hipStreamSynchronize(s));
    if (mean_out) *mean_out = used;
    return ICNV_OK;
}

int icnv_mask_non_de(const double *expr, int64_t G, int64_t C, const double *padj, int32_t n_cmp, double p_val_thresh,
                     const int32_t *base, const int32_t *cc_off, const int32_t *cc_idx, int32_t n_normal, int32_t rule,
                     int32_t use_mean, double mask_val, double *out, double *mean_out) {
    if (!expr || !out || (n_cmp > 0 && !padj)) ICNV_FAIL(ICNV_ERR_ARG, "mask_non_de: null argument");
    if (G < 1 || C < 1) ICNV_FAIL(ICNV_ERR_ARG, "mask_non_de: bad matrix dimensions");
    int rc;
    MatrixLease in;
    DevBuf d_padj, d_out;
    const size_t n = (size_t)G * C;
    if ((rc = acquire_input(expr, G * C, nullptr, in)) || (rc = upload(d_padj, padj, (size_t)n_cmp * G, nullptr)) ||
        (rc = d_out.alloc(n * sizeof(double))))
        return rc;
    if ((rc = icnv_mask_non_de_dev(in.dev, G, C, G, d_padj.as<double>(), n_cmp, p_val_thresh, base, cc_off, cc_idx, n_normal, rule,
                                   use_mean, mask_val, d_out.as<double>(), G, mean_out, nullptr)))
        return rc;
    ICNV_HIP(hipMemcpy(out, d_out.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return ICNV_OK;
}

int icnv_de_stats(int64_t *out, int32_t n) {
    if (!out || n < 1) ICNV_FAIL(ICNV_ERR_ARG, "bad argument");
    for (int i = 0; i < n && i < 7; ++i) out[i] = g_de[i].load();
    return ICNV_OK;
}

void icnv_de_stats_reset(void) {
    for (auto &c : g_de) c.store(0);
}

}  // extern "C"
