// C ABI of K16 (include/icnv.h "window smoothers of step 10"): validation, the tile plan and the uploads of the window
// tables.  Kernel: smooth_windows_kernels.hip.  DESIGN.md section 4 K16.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "icnv_internal.h"
#include "smooth_windows_internal.h"
#include "../../include/icnv.h"

using namespace icnv;

namespace {

std::atomic<int64_t> g_sw[6];   // calls, LDS tiles, spilled tiles, weighted calls, window rows (sum of len), wall microseconds

// every check of the contract that needs no device work; `rows` receives the sum of len
int sw_validate(const double *in, int64_t ld_in, const double *out, int64_t ld_out, int64_t G, int64_t C, const int32_t *lo,
                const int32_t *len, const int64_t *w_off, const double *w, const double *denom, int64_t &rows) {
    if (!in || !out || !lo || !len || !denom) ICNV_FAIL(ICNV_ERR_ARG, "smooth_windows: null argument");
    if (w && !w_off) ICNV_FAIL(ICNV_ERR_ARG, "smooth_windows: weights without w_off");
    if (G < 1 || G > 0x7fffffff || C < 1 || C > 0x7fffffff || ld_in < G || ld_out < G)
        ICNV_FAIL(ICNV_ERR_ARG, "smooth_windows: bad matrix dimensions");
    rows = 0;
    for (int64_t g = 0; g < G; ++g) {
        const std::string who = "smooth_windows: gene " + std::to_string(g) + ": ";
        if (lo[g] < 0) ICNV_FAIL(ICNV_ERR_ARG, who + "lo < 0");
        if (len[g] < 1) ICNV_FAIL(ICNV_ERR_ARG, who + "len < 1");
        if ((int64_t)lo[g] + len[g] > G) ICNV_FAIL(ICNV_ERR_ARG, who + "lo + len > G");
        if (!std::isfinite(denom[g]) || denom[g] == 0.0) ICNV_FAIL(ICNV_ERR_ARG, who + "denom must be finite and not zero");
        if (w && (w_off[g] < 0 || w_off[g + 1] < w_off[g] + len[g]))
            ICNV_FAIL(ICNV_ERR_ARG, who + "w_off must be monotone with room for len weights");
        rows += len[g];
    }
    const uintptr_t i0 = (uintptr_t)in, i1 = (uintptr_t)(in + (C - 1) * ld_in + G), o0 = (uintptr_t)out,
                    o1 = (uintptr_t)(out + (C - 1) * ld_out + G);
    if (i0 < o1 && o0 < i1) ICNV_FAIL(ICNV_ERR_ARG, "smooth_windows: expr_out overlaps expr_in (a window reads its neighbours: not in place)");
    return ICNV_OK;
}

// tiles of up to SW_TILE output genes whose windows' span fits the LDS budget; a span that does not fit halves the tile down to
// SW_MIN_TILE genes, and what still does not fit is spilled (read from HBM)
void sw_plan(int64_t G, const int32_t *lo, const int32_t *len, std::vector<SwTile> &lds, std::vector<SwTile> &spill) {
    for (int64_t g0 = 0; g0 < G;) {
        const int64_t full = std::min<int64_t>(SW_TILE, G - g0);
        int64_t n = full;
        for (;;) {
            int32_t a = 0x7fffffff, b = 0;
            for (int64_t g = g0; g < g0 + n; ++g) {
                a = std::min(a, lo[g]);
                b = std::max(b, lo[g] + len[g]);
            }
            if (sw_skew(b - a - 1) < SW_LDS_ROWS) {
                lds.push_back(SwTile{(int32_t)g0, (int32_t)(g0 + n), a, b - a});
                break;
            }
            if (n > SW_MIN_TILE) {
                n = std::max<int64_t>(SW_MIN_TILE, n / 2);
                continue;
            }
            n = full;
            spill.push_back(SwTile{(int32_t)g0, (int32_t)(g0 + n), 0, 0});
            break;
        }
        g0 += n;
    }
}

}  // namespace

extern "C" {

int icnv_smooth_windows_dev(const double *expr_in, int64_t ld_in, double *expr_out, int64_t ld_out, int64_t G, int64_t C,
                            const int32_t *lo, const int32_t *len, const int64_t *w_off, const double *w, const double *denom,
                            void *stream) {
    const auto t0 = std::chrono::steady_clock::now();
    int64_t rows = 0;
    int rc = sw_validate(expr_in, ld_in, expr_out, ld_out, G, C, lo, len, w_off, w, denom, rows);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;
    std::vector<SwTile> tiles, spill;
    sw_plan(G, lo, len, tiles, spill);
    const int32_t n_lds = (int32_t)tiles.size(), n_spill = (int32_t)spill.size();
    tiles.insert(tiles.end(), spill.begin(), spill.end());
    DevBuf d_lo, d_len, d_off, d_w, d_den, d_tiles, d_flag;
    if ((rc = upload(d_lo, lo, (size_t)G, s)) || (rc = upload(d_len, len, (size_t)G, s)) || (rc = upload(d_den, denom, (size_t)G, s)) ||
        (rc = upload(d_tiles, tiles.data(), tiles.size(), s)) || (rc = d_flag.alloc(sizeof(uint32_t))))
        return rc;
    if (w && ((rc = upload(d_off, w_off, (size_t)G + 1, s)) || (rc = upload(d_w, w, (size_t)w_off[G], s)))) return rc;
    ICNV_HIP(hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), s));
    SwArgs a{};
    a.x = expr_in; a.out = expr_out; a.ldx = ld_in; a.ldo = ld_out; a.C = C;
    a.lo = d_lo.as<int32_t>(); a.len = d_len.as<int32_t>(); a.denom = d_den.as<double>();
    a.w_off = w ? d_off.as<int64_t>() : nullptr; a.w = w ? d_w.as<double>() : nullptr;
    a.tiles = d_tiles.as<SwTile>(); a.n_lds = n_lds; a.n_spill = n_spill; a.flag = d_flag.as<uint32_t>();
    if ((rc = launch_smooth_windows(a, s))) return rc;
    uint32_t flag = 0;
    ICNV_HIP(hipMemcpyAsync(&flag, d_flag.p, sizeof(flag), hipMemcpyDeviceToHost, s));
    ICNV_HIP(hipStreamSynchronize(s));   // the host tables and the pool blocks outlive the kernel
    g_sw[0] += 1; g_sw[1] += n_lds; g_sw[2] += n_spill; g_sw[3] += w ? 1 : 0; g_sw[4] += rows;
    g_sw[5] += std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    if (flag) ICNV_FAIL(ICNV_ERR_ARG, "smooth_windows: the input holds a value that is not finite (the reference's smoothers have no NA handling here)");
    return ICNV_OK;
}

int icnv_smooth_windows(const double *expr_in, double *expr_out, int64_t G, int64_t C, const int32_t *lo, const int32_t *len,
                        const int64_t *w_off, const double *w, const double *denom) {
    int64_t rows = 0;
    int rc = sw_validate(expr_in, G, expr_out, G, G, C, lo, len, w_off, w, denom, rows);
    if (rc) return rc;
    MatrixLease in;
    DevBuf d_out;
    if ((rc = acquire_input(expr_in, G * C, nullptr, in)) || (rc = d_out.alloc((size_t)G * C * sizeof(double)))) return rc;
    if ((rc = icnv_smooth_windows_dev(in.dev, G, d_out.as<double>(), G, G, C, lo, len, w_off, w, denom, nullptr))) return rc;
    ICNV_HIP(hipMemcpy(expr_out, d_out.p, (size_t)G * C * sizeof(double), hipMemcpyDeviceToHost));
    return ICNV_OK;
}

int icnv_smooth_windows_stats(int64_t *out, int32_t n) {
    if (!out || n < 1) ICNV_FAIL(ICNV_ERR_ARG, "bad argument");
    for (int i = 0; i < n && i < 6; ++i) out[i] = g_sw[i].load();
    return ICNV_OK;
}

void icnv_smooth_windows_stats_reset(void) {
    for (auto &c : g_sw) c.store(0);
}

}  // extern "C"
