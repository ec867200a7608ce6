// C ABI of K17 (include/icnv.h "data layer of plot_cnv"): validation, the radix driver of the exact quantiles, uploads.
// Kernels: heatmap_kernels.hip.  DESIGN.md section 4 K17.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "icnv_internal.h"
#include "heatmap_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

namespace {

std::atomic<int64_t> g_hm[4];   // calls, radix passes, compacted candidates, wall microseconds

struct HmClock {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~HmClock() {
        g_hm[0] += 1;
        g_hm[3] += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    }
};

int hm_check_matrix(const char *who, const double *x, int64_t ld, int64_t G, int64_t C) {
    if (!x) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": null argument");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff || ld < G) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": bad matrix dimensions");
    return ICNV_OK;
}

int hm_check_breaks(const char *who, const double *breaks, int32_t nb) {
    if (!breaks) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": null argument");
    if (nb < 2 || nb > HM_MAX_BREAKS) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": the number of breaks must be 2 .. 257");
    for (int32_t i = 0; i < nb; ++i) {
        if (!std::isfinite(breaks[i])) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": a break is not finite");
        if (i && !(breaks[i] > breaks[i - 1])) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": the breaks must be strictly ascending");
    }
    return ICNV_OK;
}

int hm_check_rows(const char *who, const int32_t *rows, int64_t n, int64_t C) {
    if (!rows) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": null argument");
    if (n < 1 || n > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": the cell list must have 1 .. 2^31 - 1 entries");
    for (int64_t i = 0; i < n; ++i)
        if (rows[i] < 0 || rows[i] >= C) ICNV_FAIL(ICNV_ERR_ARG, std::string(who) + ": entry " + std::to_string(i) + " of the cell list is not a cell");
    return ICNV_OK;
}

int hm_check_probs(const double *probs, int32_t n_probs, const double *quantiles) {
    if (!probs || !quantiles) ICNV_FAIL(ICNV_ERR_ARG, "quantiles_excluding: null argument");
    if (n_probs < 1 || n_probs > HM_MAX_PROBS) ICNV_FAIL(ICNV_ERR_ARG, "quantiles_excluding: 1 .. 8 probabilities per call");
    for (int32_t i = 0; i < n_probs; ++i)
        if (!(probs[i] >= 0.0 && probs[i] <= 1.0)) ICNV_FAIL(ICNV_ERR_ARG, "quantiles_excluding: a probability outside [0, 1]");
    return ICNV_OK;
}

struct HmRank {
    int64_t r;          // wanted order statistic (0-based) of the kept values
    uint64_t prefix;    // the key bits known so far
    int64_t below;      // kept values whose key lies below every key with this prefix
    int64_t cnt;        // kept values with this prefix
};

}  // namespace

extern "C" {

int icnv_quantiles_excluding_dev(const double *x, int64_t ld, int64_t G, int64_t C, double exclude, const double *probs,
                                 int32_t n_probs, double *quantiles, double *order_stats, int64_t *counts, double *minmax,
                                 void *stream) {
    HmClock clock;
    int rc;
    if ((rc = hm_check_matrix("quantiles_excluding", x, ld, G, C)) || (rc = hm_check_probs(probs, n_probs, quantiles))) return rc;
    hipStream_t s = (hipStream_t)stream;

    HmScan a{};
    a.x = x; a.exclude = exclude;
    if (ld == G) { a.ld = G * C; a.G = G * C; a.C = 1; }   // contiguous: one long row, one ragged chunk instead of C
    else { a.ld = ld; a.G = G; a.C = C; }
    a.chunks_per_row = (a.G + HM_CHUNK - 1) / HM_CHUNK;
    a.n_chunks = a.chunks_per_row * a.C;

    // workspace: [HM_MAX_PREFIX][256] counts | {min key, max key, flag} | candidates | their count
    constexpr size_t N_HIST = (size_t)HM_MAX_PREFIX * HM_BINS;
    DevBuf ws;
    if ((rc = ws.alloc((N_HIST + 3 + HM_CAND + 1) * sizeof(uint64_t)))) return rc;
    a.hist = ws.as<unsigned long long>();
    a.summary = a.hist + N_HIST;
    a.cand = reinterpret_cast<uint64_t *>(a.summary + 3);
    a.n_cand = reinterpret_cast<uint32_t *>(a.cand + HM_CAND);
    const unsigned long long summary0[3] = {~0ull, 0ull, 0ull};
    ICNV_HIP(hipMemcpyAsync(a.summary, summary0, sizeof(summary0), hipMemcpyHostToDevice, s));
    ICNV_HIP(hipMemsetAsync(a.n_cand, 0, sizeof(uint64_t), s));

    std::vector<unsigned long long> hist(N_HIST);
    std::vector<HmRank> ranks;
    std::vector<uint64_t> plist;          // distinct prefixes, ascending
    std::vector<int64_t> pcnt;
    std::vector<double> stat(2 * (size_t)n_probs);
    unsigned long long summary[3] = {0, 0, 0};
    int64_t n_kept = 0, passes = 0, n_cand = 0;

    for (int shift = 64 - HM_DIGIT_BITS;; shift -= HM_DIGIT_BITS) {
        const bool first = shift == 64 - HM_DIGIT_BITS;
        const size_t slots = std::max<size_t>(plist.size(), 1) * HM_BINS;
        a.n_prefix = (int32_t)plist.size();
        a.match_shift = shift + HM_DIGIT_BITS;
        a.digit_shift = shift;
        for (size_t j = 0; j < plist.size(); ++j) a.prefix[j] = plist[j];
        ICNV_HIP(hipMemsetAsync(a.hist, 0, slots * sizeof(uint64_t), s));
        if ((rc = launch_hm_hist(a, first, s))) return rc;
        ICNV_HIP(hipMemcpyAsync(hist.data(), a.hist, slots * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
        if (first) ICNV_HIP(hipMemcpyAsync(summary, a.summary, sizeof(summary), hipMemcpyDeviceToHost, s));
        ICNV_HIP(hipStreamSynchronize(s));
        ++passes;
        if (first) {
            if (summary[2]) ICNV_FAIL(ICNV_ERR_ARG, "quantiles_excluding: the matrix holds a value that is not finite");
            for (int d = 0; d < HM_BINS; ++d) n_kept += (int64_t)hist[d];
            if (n_kept == 0) ICNV_FAIL(ICNV_ERR_ARG, "quantiles_excluding: every value equals `exclude`");
            for (int32_t i = 0; i < n_probs; ++i) {
                const double index = (double)(n_kept - 1) * probs[i];
                ranks.push_back(HmRank{(int64_t)std::floor(index), 0, 0, n_kept});
                ranks.push_back(HmRank{(int64_t)std::ceil(index), 0, 0, n_kept});
            }
        }
        for (HmRank &k : ranks) {
            const size_t j = first ? 0 : (size_t)(std::lower_bound(plist.begin(), plist.end(), k.prefix) - plist.begin());
            const unsigned long long *h = hist.data() + j * HM_BINS;
            const int64_t rel = k.r - k.below;
            int64_t cum = 0;
            int d = 0;
            for (; d < HM_BINS - 1 && rel >= cum + (int64_t)h[d]; ++d) cum += (int64_t)h[d];
            if (rel < cum || rel >= cum + (int64_t)h[d]) ICNV_FAIL(ICNV_ERR_HIP, "quantiles_excluding: the digit counts do not add up (internal error)");
            k.below += cum;
            k.prefix = (k.prefix << HM_DIGIT_BITS) | (uint64_t)d;
            k.cnt = (int64_t)h[d];
        }
        plist.clear();
        for (const HmRank &k : ranks) plist.push_back(k.prefix);
        std::sort(plist.begin(), plist.end());
        plist.erase(std::unique(plist.begin(), plist.end()), plist.end());
        pcnt.assign(plist.size(), 0);
        int64_t total = 0;
        for (const HmRank &k : ranks) pcnt[(size_t)(std::lower_bound(plist.begin(), plist.end(), k.prefix) - plist.begin())] = k.cnt;
        for (int64_t c : pcnt) total += c;

        if (shift == 0) {                 // every bit is known: the prefix is the key
            for (size_t i = 0; i < ranks.size(); ++i) stat[i] = hm_unkey(ranks[i].prefix);
            break;
        }
        if (total <= HM_CAND) {           // few enough: compact them, sort them in one workgroup, pick by rank
            a.n_prefix = (int32_t)plist.size();
            a.match_shift = shift;
            for (size_t j = 0; j < plist.size(); ++j) a.prefix[j] = plist[j];
            std::vector<uint64_t> sorted((size_t)total);
            uint32_t got = 0;
            if ((rc = launch_hm_compact(a, s)) || (rc = launch_hm_sort(a.cand, a.n_cand, s))) return rc;
            ICNV_HIP(hipMemcpyAsync(&got, a.n_cand, sizeof(got), hipMemcpyDeviceToHost, s));
            ICNV_HIP(hipMemcpyAsync(sorted.data(), a.cand, (size_t)total * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
            ICNV_HIP(hipStreamSynchronize(s));
            if ((int64_t)got != total) ICNV_FAIL(ICNV_ERR_HIP, "quantiles_excluding: the candidate list does not match the counts (internal error)");
            n_cand = total;
            for (size_t i = 0; i < ranks.size(); ++i) {
                const size_t j = (size_t)(std::lower_bound(plist.begin(), plist.end(), ranks[i].prefix) - plist.begin());
                int64_t off = 0;
                for (size_t q = 0; q < j; ++q) off += pcnt[q];
                stat[i] = hm_unkey(sorted[(size_t)(off + ranks[i].r - ranks[i].below)]);
            }
            break;
        }
    }
    g_hm[1] += passes; g_hm[2] += n_cand;

    // quantile(type = 7), R/src/library/stats/R/quantile.R, in this operation order
    for (int32_t i = 0; i < n_probs; ++i) {
        const double index = (double)(n_kept - 1) * probs[i], lo = std::floor(index), h = index - lo;
        const double xl = stat[2 * i], xh = stat[2 * i + 1];
        quantiles[i] = (index == lo || xh == xl) ? xl : (1.0 - h) * xl + h * xh;
    }
    if (order_stats) std::copy(stat.begin(), stat.end(), order_stats);
    if (counts) { counts[0] = n_kept; counts[1] = G * C - n_kept; }
    if (minmax) { minmax[0] = hm_unkey(summary[0]); minmax[1] = hm_unkey(summary[1]); }
    return ICNV_OK;
}

int icnv_quantiles_excluding(const double *x, int64_t G, int64_t C, double exclude, const double *probs, int32_t n_probs,
                             double *quantiles, double *order_stats, int64_t *counts, double *minmax) {
    int rc;
    if ((rc = hm_check_matrix("quantiles_excluding", x, G, G, C)) || (rc = hm_check_probs(probs, n_probs, quantiles))) return rc;
    MatrixLease in;
    if ((rc = acquire_input(x, G * C, nullptr, in))) return rc;
    return icnv_quantiles_excluding_dev(in.dev, G, G, C, exclude, probs, n_probs, quantiles, order_stats, counts, minmax, nullptr);
}

int icnv_heatmap_bins_dev(const double *x, int64_t ld, int64_t G, int64_t C, const int32_t *rows, int64_t n_rows,
                          const double *breaks, int32_t nb, int64_t *counts, void *stream) {
    HmClock clock;
    int rc;
    if (!counts) ICNV_FAIL(ICNV_ERR_ARG, "heatmap_bins: null argument");
    if ((rc = hm_check_matrix("heatmap_bins", x, ld, G, C)) || (rc = hm_check_breaks("heatmap_bins", breaks, nb)) ||
        (rc = hm_check_rows("heatmap_bins", rows, n_rows, C)))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    DevBuf d_rows, d_br, d_out;
    if ((rc = upload(d_rows, rows, (size_t)n_rows, s)) || (rc = upload(d_br, breaks, (size_t)nb, s)) ||
        (rc = d_out.alloc((HM_MAX_BREAKS + 1) * sizeof(uint64_t))))
        return rc;
    ICNV_HIP(hipMemsetAsync(d_out.p, 0, (HM_MAX_BREAKS + 1) * sizeof(uint64_t), s));
    HmBins a{};
    a.x = x; a.ld = ld; a.G = G; a.rows = d_rows.as<int32_t>(); a.n_rows = n_rows; a.breaks = d_br.as<double>(); a.nb = nb;
    a.counts = d_out.as<unsigned long long>();
    a.flag = reinterpret_cast<uint32_t *>(a.counts + HM_MAX_BREAKS);
    a.chunks_per_row = (G + HM_CHUNK - 1) / HM_CHUNK;
    a.n_chunks = a.chunks_per_row * n_rows;
    if ((rc = launch_hm_bins(a, s))) return rc;
    unsigned long long host[HM_MAX_BREAKS + 1];
    ICNV_HIP(hipMemcpyAsync(host, d_out.p, sizeof(host), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (host[HM_MAX_BREAKS] & 0xffffffffull) ICNV_FAIL(ICNV_ERR_ARG, "heatmap_bins: a listed cell holds a NaN");
    for (int32_t b = 0; b < nb - 1; ++b) counts[b] = (int64_t)host[b];
    return ICNV_OK;
}

int icnv_heatmap_bins(const double *x, int64_t G, int64_t C, const int32_t *rows, int64_t n_rows, const double *breaks, int32_t nb,
                      int64_t *counts) {
    int rc;
    if ((rc = hm_check_matrix("heatmap_bins", x, G, G, C))) return rc;
    MatrixLease in;
    if ((rc = acquire_input(x, G * C, nullptr, in))) return rc;
    return icnv_heatmap_bins_dev(in.dev, G, G, C, rows, n_rows, breaks, nb, counts, nullptr);
}

int icnv_heatmap_raster_dev(const double *x, int64_t ld, int64_t G, int64_t C, const int32_t *order, int64_t n,
                            const double *breaks, int32_t nb, int64_t H, int64_t W, uint8_t *image, void *stream) {
    HmClock clock;
    int rc;
    if (!image) ICNV_FAIL(ICNV_ERR_ARG, "heatmap_raster: null argument");
    if (H < 1 || H > 0x7fffffff || W < 1 || W > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "heatmap_raster: H and W must be 1 .. 2^31 - 1");
    if ((rc = hm_check_matrix("heatmap_raster", x, ld, G, C)) || (rc = hm_check_breaks("heatmap_raster", breaks, nb)) ||
        (rc = hm_check_rows("heatmap_raster", order, n, C)))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    DevBuf d_rows, d_br, d_img, d_flag;   // rendered aside: a NaN found by the kernel must leave `image` as it was
    if ((rc = upload(d_rows, order, (size_t)n, s)) || (rc = upload(d_br, breaks, (size_t)nb, s)) ||
        (rc = d_img.alloc((size_t)H * (size_t)W)) || (rc = d_flag.alloc(sizeof(uint32_t))))
        return rc;
    ICNV_HIP(hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), s));
    HmBins a{};
    a.x = x; a.ld = ld; a.G = G; a.rows = d_rows.as<int32_t>(); a.n_rows = n; a.breaks = d_br.as<double>(); a.nb = nb;
    a.flag = d_flag.as<uint32_t>(); a.H = H; a.W = W; a.image = d_img.as<uint8_t>();
    if ((rc = launch_hm_raster(a, s))) return rc;
    uint32_t flag = 0;
    ICNV_HIP(hipMemcpyAsync(&flag, d_flag.p, sizeof(flag), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));
    if (flag) ICNV_FAIL(ICNV_ERR_ARG, "heatmap_raster: a sampled value is NaN");
    ICNV_HIP(hipMemcpyAsync(image, d_img.p, (size_t)H * (size_t)W, hipMemcpyDeviceToDevice, s));
    ICNV_HIP(hipStreamSynchronize(s));   // the pool block outlives the copy
    return ICNV_OK;
}

int icnv_heatmap_raster(const double *x, int64_t G, int64_t C, const int32_t *order, int64_t n, const double *breaks, int32_t nb,
                        int64_t H, int64_t W, uint8_t *image) {
    int rc;
    if (!image) ICNV_FAIL(ICNV_ERR_ARG, "heatmap_raster: null argument");
    if (H < 1 || H > 0x7fffffff || W < 1 || W > 0x7fffffff) ICNV_FAIL(ICNV_ERR_ARG, "heatmap_raster: H and W must be 1 .. 2^31 - 1");
    if ((rc = hm_check_matrix("heatmap_raster", x, G, G, C))) return rc;
    MatrixLease in;
    DevBuf d_img;
    if ((rc = acquire_input(x, G * C, nullptr, in)) || (rc = d_img.alloc((size_t)H * (size_t)W))) return rc;
    if ((rc = icnv_heatmap_raster_dev(in.dev, G, G, C, order, n, breaks, nb, H, W, d_img.as<uint8_t>(), nullptr))) return rc;
    ICNV_HIP(hipMemcpy(image, d_img.p, (size_t)H * (size_t)W, hipMemcpyDeviceToHost));
    return ICNV_OK;
}

int icnv_heatmap_stats(int64_t *out, int32_t n) {
    if (!out || n < 1) ICNV_FAIL(ICNV_ERR_ARG, "bad argument");
    for (int i = 0; i < n && i < 4; ++i) out[i] = g_hm[i].load();
    return ICNV_OK;
}

void icnv_heatmap_stats_reset(void) {
    for (auto &c : g_hm) c.store(0);
}

}  // extern "C"
