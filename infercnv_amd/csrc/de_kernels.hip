// K12: the per-gene tests of mask_non_DE_genes_basic (R/inferCNV_mask_non_DE.R:28-258) for every (subcluster, normal type)
// comparison at once.  DESIGN.md section 4 K12; the contract is in include/icnv.h and restated in tests/de_restate.py.
//
// wilcoxon, per wave of genes:
//   de_gather_kernel       the involved groups' values (with the jitter of the (gene, cell) stream) gene-major per group,
//                          -0 -> +0, non-finite -> +inf: one segment per (group, gene), its finite values sort first
//   de_sort_chunks_kernel  bitonic sort of every segment piece of <= DE_CHUNK keys in LDS
//   de_merge_pass_kernel   longer segments: runs of DE_CHUNK << p merged pairwise through HBM (rank of every key in the
//                          other run: ties go A first, so the output is a permutation)
//   de_wilcox_kernel       per (comparison, gene) one sequential merge of the two sorted finite prefixes: 2W, the tie sum
//                          T = sum(t^3 - t), the branch and p
// t: de_moments_kernel per (group, gene), de_welch_kernel per (comparison, gene).
// BH: the p rows sorted by the same two kernels, de_bh_finish_kernel (suffix minimum per row, then every p looks up its
// adjusted value by rank).  Mask: de_mean_* and de_mask_kernel.
// Every value is an individually rounded IEEE-754 double operation in the documented order: -ffp-contract=off.
#include <algorithm>
#include <vector>

#include "icnv_internal.h"
#include "lib_math.h"
#include "random_trees_internal.h"
#include "leiden_internal.h"
#include "de_internal.h"
#include "../../include/icnv.h"

#pragma clang fp contract(off)

namespace icnv {

namespace {

// the jitter of (gene g, cell c): Generator(Philox(key = [seed, token], counter = [0, g, c, 0])), two random() draws, R's
// INVERSION rule, then rnorm's mean + sd z
__device__ inline double de_jitter(uint64_t seed, int64_t g, int64_t c) {
    RtPhilox ph(seed, ICNV_DE_JITTER_TOKEN, (uint64_t)g, (uint64_t)c);
    const double u1 = ph.random();
    const double u2 = ph.random();
    const double z = lib_qnorm((floor(134217728.0 * u1) + u2) / 134217728.0);
    return 1e-4 + 1e-4 * z;
}

// 2 min(pnorm(z), pnorm(z, lower.tail = FALSE)): pnorm_both's non-log branches (R nmath/pnorm.c), exp = exp_lib
__device__ inline double de_pnorm2(double z) {
    if (z != z) return z;
    const double y = fabs(z);
    if (y <= 0.67448975) {
        const double q = y * y;
        double num = 0.065682337918207449113 * q, den = q;
        num = (num + 2.2352520354606839287) * q;  den = (den + 47.20258190468824187) * q;
        num = (num + 161.02823106855587881) * q;  den = (den + 976.09855173777669322) * q;
        num = (num + 1067.6894854603709582) * q;  den = (den + 10260.932208618978205) * q;
        const double t = y * (num + 18154.981253343561249) / (den + 45507.789335026729956);
        return 2.0 * (0.5 - t);
    }
    if (!(y < 37.5193)) return 0.0;
    double t;
    if (y <= 5.656854249492380195206754896838) {
        double num = 1.0765576773720192317e-8 * y, den = y;
        num = (num + 0.39894151208813466764) * y;  den = (den + 22.266688044328115691) * y;
        num = (num + 8.8831497943883759412) * y;   den = (den + 235.38790178262499861) * y;
        num = (num + 93.506656132177855979) * y;   den = (den + 1519.377599407554805) * y;
        num = (num + 597.27027639480026226) * y;   den = (den + 6485.558298266760755) * y;
        num = (num + 2494.5375852903726711) * y;   den = (den + 18615.571640885098091) * y;
        num = (num + 6848.1904505362823326) * y;   den = (den + 34900.952721145977266) * y;
        num = (num + 11602.651437647350124) * y;   den = (den + 38912.003286093271411) * y;
        t = (num + 9842.7148383839780218) / (den + 19685.429676859990727);
    } else {
        const double q = 1.0 / (y * y);
        double num = 0.02307344176494017303 * q, den = q;
        num = (num + 0.21589853405795699) * q;       den = (den + 1.28426009614491121) * q;
        num = (num + 0.1274011611602473639) * q;     den = (den + 0.468238212480865118) * q;
        num = (num + 0.022235277870649807) * q;      den = (den + 0.0659881378689285515) * q;
        num = (num + 0.001421619193227893466) * q;   den = (den + 0.00378239633202758244) * q;
        t = q * (num + 2.9112874951168792e-5) / (den + 7.29751555083966205e-5);
        t = (0.398942280401432677939946059934 - t) / y;
    }
    const double xs = trunc(y * 16.0) / 16.0;
    const double del = (y - xs) * (y + xs);
    const double small = lib_exp(-xs * xs * 0.5) * lib_exp(-del * 0.5) * t;
    return 2.0 * fmin(small, 1.0 - small);
}

// lgamma(a) - lgamma(a + 1/2), a > 0: shifted to a >= 10 by the exact ratio product, then Stirling's series
__device__ inline double de_stirling_corr(double a) {
    const double x = 1.0 / a;
    const double x2 = x * x;
    const double c[8] = {1.0 / 12.0, -1.0 / 360.0, 1.0 / 1260.0, -1.0 / 1680.0, 1.0 / 1188.0, -691.0 / 360360.0, 1.0 / 156.0,
                         -3617.0 / 122400.0};
    double h = c[7];
    for (int j = 6; j >= 0; --j) h = h * x2 + c[j];
    return h * x;
}
__device__ inline double de_lgamma_diff_half(double a) {
    double r = 1.0;
    while (a < 10.0) {
        r = r * ((a + 0.5) / a);
        a = a + 1.0;
    }
    const double d = (((-0.5 * lib_log(a)) - (a * lib_log1p(0.5 / a))) + 0.5) + (de_stirling_corr(a) - de_stirling_corr(a + 0.5));
    return r == 1.0 ? d : d + lib_log(r);
}

// the continued fraction of I_x(a, b) (modified Lentz)
__device__ inline double de_betacf(double a, double b, double x) {
    const double FPMIN = 1e-300;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - (qab * x) / qap;
    if (fabs(d) < FPMIN) d = FPMIN;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= ICNV_DE_CF_MAX_ITER; ++m) {
        const double md = (double)m, m2 = 2.0 * md;
        double aa = ((md * (b - md)) * x) / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < FPMIN) d = FPMIN;
        c = 1.0 + aa / c;
        if (fabs(c) < FPMIN) c = FPMIN;
        d = 1.0 / d;
        h = h * (d * c);
        aa = (((-(a + md)) * (qab + md)) * x) / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < FPMIN) d = FPMIN;
        c = 1.0 + aa / c;
        if (fabs(c) < FPMIN) c = FPMIN;
        d = 1.0 / d;
        const double del = d * c;
        h = h * del;
        if (fabs(del - 1.0) <= 4.440892098500626e-16) break;
    }
    return h;
}

// 2 pt(-|t|, df) = I_{df / (df + t^2)}(df / 2, 1 / 2)
__device__ inline double de_pt2(double t, double df) {
    if (t != t || df != df) return t + df;
    if (__builtin_isinf(t)) return 0.0;
    const double a = df * 0.5, b = 0.5;
    const double t2 = t * t;
    const double x = df / (df + t2), xc = t2 / (df + t2);
    const double lx = -lib_log1p(t2 / df), lxc = lib_log(xc);
    const double lfront = ((a * lx) + (b * lxc)) - (0.57236494292470008707 + de_lgamma_diff_half(a));
    const double front = lib_exp(lfront);
    if (x < (a + 1.0) / (a + b + 2.0)) return (front * de_betacf(a, b, x)) / a;
    return 1.0 - (front * de_betacf(b, a, xc)) / b;
}

__device__ inline void dd_add(double &hi, double &lo, double x) {
    const double s = hi + x;
    const double bb = s - hi;
    lo += (hi - (s - bb)) + (x - bb);
    hi = s;
}
// (hi + lo) / n, correctly rounded (viterbi_kernels.hip group_means_finish_kernel)
__device__ inline double dd_div(double hi, double lo, double n) {
    const double s = hi + lo;
    const double e = lo - (s - hi);
    const double q0 = s / n;
    const double r = __builtin_fma(-q0, n, s);
    return q0 + (r + e) / n;
}
__device__ inline double dd_round(double hi, double lo) { return hi + lo; }

__device__ inline int64_t lower_bound(const double *a, int64_t n, double v) {   // # a[i] < v
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (a[m] < v) lo = m + 1; else hi = m;
    }
    return lo;
}
__device__ inline int64_t upper_bound(const double *a, int64_t n, double v) {   // # a[i] <= v
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (a[m] <= v) lo = m + 1; else hi = m;
    }
    return lo;
}

template <typename T>
__device__ inline int find_set(const T *off, int n_sets, T b) {   // off[s] <= b < off[s + 1]
    int lo = 0, hi = n_sets;
    while (hi - lo > 1) {
        const int m = (lo + hi) >> 1;
        if (off[m] <= b) lo = m; else hi = m;
    }
    return lo;
}

// one 64-cell x 64-gene tile per workgroup: coalesced reads along the genes of a cell, coalesced writes along a segment
__global__ void __launch_bounds__(256) de_gather_kernel(DeGather a) {
    __shared__ double tile[64][65];
    const int64_t b = blockIdx.x;
    const int k = find_set(a.tile_off, a.n_groups, b);
    const int64_t c0 = a.cell_off[k], nk = a.cell_off[k + 1] - c0;
    const int64_t gtiles = (a.gw + 63) / 64;
    const int64_t t = b - a.tile_off[k];
    const int64_t ct = t / gtiles, gt = t - ct * gtiles;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t j = gt * 64 + tx;
    for (int r = ty; r < 64; r += 4) {
        const int64_t i = ct * 64 + r;
        double v = __builtin_inf();
        if (i < nk && j < a.gw) {
            const int64_t c = a.cell_idx[c0 + i], g = a.g0 + j;
            v = a.x[c * a.ld + g];
            if (a.jitter) v = v + de_jitter(a.seed, g, c);
            if (v == 0.0) v = 0.0;
            if (!(fabs(v) <= 1.7976931348623157e308)) v = __builtin_inf();
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < 64; r += 4) {
        const int64_t jj = gt * 64 + r, i = ct * 64 + tx;
        if (jj < a.gw && i < nk) a.keys[a.seg_base[k] + jj * nk + i] = tile[tx][r];
    }
}

__global__ void __launch_bounds__(256) de_sort_chunks_kernel(double *keys, const DeSegs *segs, const int64_t *chunk_off, int n_sets) {
    __shared__ double s[DE_CHUNK];
    const int64_t b = blockIdx.x;
    const int set = find_set(chunk_off, n_sets, b);
    const DeSegs g = segs[set];
    const int64_t nch = ((int64_t)g.n + DE_CHUNK - 1) / DE_CHUNK;
    const int64_t local = b - chunk_off[set];
    const int64_t seg = local / nch, piece = local - seg * nch;
    const int64_t start = piece * DE_CHUNK;
    const int len = (int)min((int64_t)DE_CHUNK, (int64_t)g.n - start);
    int P = 2;
    while (P < len) P <<= 1;
    double *src = keys + g.base + seg * g.n + start;
    for (int i = threadIdx.x; i < P; i += 256) s[i] = i < len ? src[i] : __builtin_inf();
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
        for (int j2 = k2 >> 1; j2 > 0; j2 >>= 1) {
            for (int i = threadIdx.x; i < (P >> 1); i += 256) {
                const int lo = ((i & ~(j2 - 1)) << 1) | (i & (j2 - 1));
                const int hi = lo + j2;
                const bool up = (lo & k2) == 0;
                const double u = s[lo], v = s[hi];
                if ((u > v) == up) { s[lo] = v; s[hi] = u; }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < len; i += 256) src[i] = s[i];
}

__global__ void __launch_bounds__(256) de_merge_pass_kernel(const double *__restrict__ src, double *__restrict__ dst, DeSegs g, int64_t run) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n = g.n;
    if (e >= n * g.count) return;
    const int64_t seg = e / n, i = e - seg * n;
    const double *sp = src + g.base + seg * n;
    double *dp = dst + g.base + seg * n;
    const int64_t base = i - i % (2 * run);
    const int64_t a_len = min(run, n - base);
    const int64_t b_start = base + a_len;
    const int64_t b_len = min(run, n - b_start);
    const double v = sp[i];
    int64_t pos;
    if (i < b_start) pos = (i - base) + (b_len > 0 ? lower_bound(sp + b_start, b_len, v) : 0);
    else pos = (i - b_start) + upper_bound(sp + base, a_len, v);
    dp[base + pos] = v;
}

__global__ void __launch_bounds__(256) de_wilcox_kernel(DeWilcox a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)a.n_cmp * a.gw) return;
    const int k = (int)(e / a.gw);
    const int64_t j = e - (int64_t)k * a.gw, g = a.g0 + j;
    const int gx = a.cmp[2 * k], gy = a.cmp[2 * k + 1];
    const int64_t nxa = a.n[gx], nya = a.n[gy];
    const double *X = a.buf[a.which[gx]] + a.seg_base[gx] + j * nxa;
    const double *Y = a.buf[a.which[gy]] + a.seg_base[gy] + j * nya;
    const int64_t nx = lower_bound(X, nxa, __builtin_inf()), ny = lower_bound(Y, nya, __builtin_inf());
    const int64_t o = (int64_t)k * a.G + g;
    if (nx == 0 || ny == 0) {
        atomicMin(a.err, (unsigned long long)o);
        a.stat[o] = __builtin_nan("");
        a.p[o] = __builtin_nan("");
        return;
    }
    // one merge: tie groups in ascending order; x's ranks in half units, r the values already ranked
    int64_t i = 0, jj = 0, r = 0, sx2 = 0, T = 0;
    while (i < nx || jj < ny) {
        const double xv = i < nx ? X[i] : __builtin_inf(), yv = jj < ny ? Y[jj] : __builtin_inf();
        const double v = xv < yv ? xv : yv;
        int64_t cx = 0, cy = 0;
        while (i < nx && X[i] == v) { ++cx; ++i; }
        while (jj < ny && Y[jj] == v) { ++cy; ++jj; }
        const int64_t t = cx + cy;
        sx2 += cx * (2 * r + t + 1);
        r += t;
        T += t * t * t - t;
    }
    const int64_t w2 = sx2 - nx * (nx + 1);   // 2 W
    const double W = (double)w2 * 0.5;
    double p;
    if (nx <= DE_EXACT_MAX && ny <= DE_EXACT_MAX && T == 0) {
        p = a.exact_p[a.exact_off[(nx - 1) * DE_EXACT_MAX + (ny - 1)] + w2 / 2];
    } else {
        const double dx = (double)nx, dy = (double)ny;
        const double z0 = W - dx * dy / 2.0;
        const double sigma = sqrt((dx * dy / 12.0) * ((dx + dy + 1.0) - (double)T / ((dx + dy) * (dx + dy - 1.0))));
        const double corr = z0 > 0.0 ? 0.5 : (z0 < 0.0 ? -0.5 : 0.0);
        p = de_pnorm2((z0 - corr) / sigma);
    }
    a.stat[o] = W;
    a.p[o] = p;
}

// per (group q, gene g): mean (correctly rounded), var = cr(sum round(round(x - m)^2)) / (n - 1), n without NaN, +-Inf seen
__global__ void __launch_bounds__(256) de_moments_kernel(DeWelch a) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.G) return;
    for (int q = blockIdx.y; q < a.n_groups; q += gridDim.y) {
    const int64_t b = a.cell_off[q], e = a.cell_off[q + 1];
    double hi = 0.0, lo = 0.0;
    int64_t n = 0;
    bool inf = false;
    for (int64_t i = b; i < e; ++i) {
        const double v = a.x[(int64_t)a.cell_idx[i] * a.ld + g];
        if (v != v) continue;
        ++n;
        if (__builtin_isinf(v)) inf = true;
        else dd_add(hi, lo, v);
    }
    double m = __builtin_nan(""), var = __builtin_nan("");
    if (!inf && n > 0) {
        m = dd_div(hi, lo, (double)n);
        hi = 0.0; lo = 0.0;
        for (int64_t i = b; i < e; ++i) {
            const double v = a.x[(int64_t)a.cell_idx[i] * a.ld + g];
            if (v != v) continue;
            const double d = v - m;
            dd_add(hi, lo, d * d);
        }
        var = dd_round(hi, lo) / ((double)n - 1.0);
    }
    double *dst = a.mom + (int64_t)q * 4 * a.G + g;
    dst[0] = m;
    dst[a.G] = var;
    dst[2 * (int64_t)a.G] = (double)n;
    dst[3 * (int64_t)a.G] = inf ? 1.0 : 0.0;
    }
}

// t.test(x, y) (Welch) per (comparison, gene); NA where R's try() catches a stop()
__global__ void __launch_bounds__(256) de_welch_kernel(DeWelch a) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)a.n_cmp * a.G) return;
    const int k = (int)(e / a.G);
    const int64_t g = e - (int64_t)k * a.G;
    const double *mx_ = a.mom + (int64_t)a.cmp[2 * k] * 4 * a.G + g, *my_ = a.mom + (int64_t)a.cmp[2 * k + 1] * 4 * a.G + g;
    const double mx = mx_[0], vx = mx_[a.G], nx = mx_[2 * (int64_t)a.G], ix = mx_[3 * (int64_t)a.G];
    const double my = my_[0], vy = my_[a.G], ny = my_[2 * (int64_t)a.G], iy = my_[3 * (int64_t)a.G];
    double t = __builtin_nan(""), p = __builtin_nan("");
    if (nx >= 2.0 && ny >= 2.0 && ix == 0.0 && iy == 0.0) {
        const double sx = sqrt(vx / nx), sy = sqrt(vy / ny);
        const double se = sqrt(sx * sx + sy * sy);
        const double eps10 = 10.0 * 2.220446049250313e-16;
        if (se == se && !(se < eps10 * fmax(fabs(mx), fabs(my)))) {
            const double sx2 = sx * sx, sy2 = sy * sy, se2 = se * se;
            const double df = (se2 * se2) / ((sx2 * sx2) / (nx - 1.0) + (sy2 * sy2) / (ny - 1.0));
            t = (mx - my) / se;
            p = de_pt2(-fabs(t), df);
        }
    }
    a.stat[e] = t;
    a.p[e] = p;
}

__global__ void de_bh_keys_kernel(const double *__restrict__ p, double *__restrict__ keys, int64_t n) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e < n) {
        const double v = p[e];
        keys[e] = v == v ? v : __builtin_inf();
    }
}

// one workgroup per comparison row: sm[i] = min over sorted positions >= i of (n / #(p <= q_i)) * q_i; then every p's
// adjusted value is min(1, sm[rank of p])
__global__ void __launch_bounds__(256) de_bh_finish_kernel(const double *__restrict__ p, const double *__restrict__ sorted,
                                                           double *__restrict__ sm, double *__restrict__ padj, int G) {
    __shared__ double s[256];
    const int64_t k = blockIdx.x;
    const double *row = sorted + k * G;
    double *smr = sm + k * G;
    const int64_t n = lower_bound(row, G, __builtin_inf());
    const double nd = (double)n;
    double carry = __builtin_inf();
    for (int64_t end = n; end > 0; end -= 256) {
        const int64_t i = end - 256 + threadIdx.x;
        double v = __builtin_inf();
        if (i >= 0) {
            const double q = row[i];
            v = (nd / (double)upper_bound(row, n, q)) * q;
        }
        s[threadIdx.x] = v;
        for (int off = 1; off < 256; off <<= 1) {
            __syncthreads();
            const double o = threadIdx.x + off < 256 ? s[threadIdx.x + off] : __builtin_inf();
            __syncthreads();
            s[threadIdx.x] = fmin(s[threadIdx.x], o);
        }
        __syncthreads();
        if (i >= 0) smr[i] = fmin(s[threadIdx.x], carry);
        carry = fmin(carry, s[0]);
        __syncthreads();
    }
    __syncthreads();
    for (int64_t g = threadIdx.x; g < G; g += 256) {
        const double v = p[k * G + g];
        padj[k * G + g] = v == v ? fmin(1.0, smr[lower_bound(row, n, v)]) : v;
    }
}

constexpr int DE_MEAN_BLOCKS = 1024;

// per workgroup: double-double sum of its cells' values and their plain sum
__global__ void __launch_bounds__(256) de_mean_partial_kernel(const double *__restrict__ x, int64_t ld, int G, int C, double *part) {
    __shared__ double red[3][4];
    double hi = 0.0, lo = 0.0, plain = 0.0;
    for (int64_t c = blockIdx.x; c < C; c += gridDim.x)
        for (int64_t g = threadIdx.x; g < G; g += 256) {
            const double v = x[c * ld + g];
            dd_add(hi, lo, v);
            plain += v;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double oh = __shfl_xor(hi, o, 64), ol = __shfl_xor(lo, o, 64), op = __shfl_xor(plain, o, 64);
        dd_add(hi, lo, oh);
        lo += ol;
        plain += op;
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = hi; red[1][threadIdx.x >> 6] = lo; red[2][threadIdx.x >> 6] = plain; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double h = red[0][0], l = red[1][0], pl = red[2][0];
        for (int w = 1; w < 4; ++w) { dd_add(h, l, red[0][w]); l += red[1][w]; pl += red[2][w]; }
        part[3 * blockIdx.x] = h;
        part[3 * blockIdx.x + 1] = l;
        part[3 * blockIdx.x + 2] = pl;
    }
}
__global__ void de_mean_finish_kernel(const double *part, int n_parts, double n, double *mean) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double hi = 0.0, lo = 0.0, plain = 0.0;
    for (int i = 0; i < n_parts; ++i) { dd_add(hi, lo, part[3 * i]); lo += part[3 * i + 1]; plain += part[3 * i + 2]; }
    const double m = dd_div(hi, lo, n);
    *mean = (m == m && fabs(m) <= 1.7976931348623157e308) ? m : plain / n;
}

__global__ void __launch_bounds__(256) de_mask_kernel(DeMask a) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.G) return;
    for (int64_t c = blockIdx.y; c < a.C; c += gridDim.y) {
    int cnt = a.base[c];
    for (int i = a.cc_off[c]; i < a.cc_off[c + 1]; ++i) cnt += a.padj[(int64_t)a.cc_idx[i] * a.G + g] < a.thresh ? 1 : 0;
    bool m;
    if (a.rule == ICNV_DE_MASK_ANY) m = cnt == 0;
    else if (a.rule == ICNV_DE_MASK_MOST) m = (double)cnt < (double)a.n_normal / 2.0;
    else m = cnt != a.n_normal;
    const double v = a.x[c * a.ld + g];
    a.out[c * a.ld_out + g] = m ? (a.use_mean ? *a.mean : a.value) : v;
    }
}

}  // namespace

typedef unsigned __int128 u128;

// a / b correctly rounded, 0 <= a <= b, b > 0 (long division, round half to even)
static double u128_ratio(u128 a, u128 b) {
    if (a == 0) return 0.0;
    if (a == b) return 1.0;
    u128 r = a;
    uint64_t mant = 0;
    int e = 0, nb = 0;
    while (nb < 53) {
        r <<= 1;
        --e;
        mant <<= 1;
        if (r >= b) { r -= b; mant |= 1; }
        if (mant) ++nb;
    }
    r <<= 1;
    const bool half = r >= b;
    if (half) r -= b;
    if (half && (r != 0 || (mant & 1))) ++mant;
    return ldexp((double)mant, e);
}

int de_exact_table_host(std::vector<int64_t> &off, std::vector<double> &p) {
    const int M = DE_EXACT_MAX;
    // f[m][n][k]: arrangements of m x's and n y's with k (x, y) pairs x > y
    std::vector<std::vector<u128>> f((M + 1) * (M + 1));
    for (int m = 0; m <= M; ++m)
        for (int n = 0; n <= M; ++n) {
            std::vector<u128> &v = f[m * (M + 1) + n];
            v.assign((size_t)m * n + 1, 0);
            if (m == 0 || n == 0) { v[0] = 1; continue; }
            const std::vector<u128> &a = f[(m - 1) * (M + 1) + n], &b = f[m * (M + 1) + n - 1];
            for (size_t k = 0; k < a.size(); ++k) v[k + n] += a[k];
            for (size_t k = 0; k < b.size(); ++k) v[k] += b[k];
        }
    off.assign((size_t)M * M, 0);
    p.clear();
    for (int m = 1; m <= M; ++m)
        for (int n = 1; n <= M; ++n) {
            const std::vector<u128> &v = f[m * (M + 1) + n];
            off[(m - 1) * M + n - 1] = (int64_t)p.size();
            std::vector<u128> cum(v.size());
            u128 s = 0;
            for (size_t k = 0; k < v.size(); ++k) { s += v[k]; cum[k] = s; }
            const u128 total = s;
            for (int64_t w = 0; w <= (int64_t)m * n; ++w) {
                const u128 tail = 2 * w > (int64_t)m * n ? total - cum[w - 1] : cum[w];
                const double pp = 2.0 * u128_ratio(tail, total);
                p.push_back(pp < 1.0 ? pp : 1.0);
            }
        }
    return ICNV_OK;
}

#define DE_LAUNCH_CHECK() ICNV_HIP(hipGetLastError())

int launch_de_gather(const DeGather &a, int64_t n_tiles, hipStream_t s) {
    if (n_tiles <= 0) return ICNV_OK;
    hipLaunchKernelGGL(de_gather_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, a);
    DE_LAUNCH_CHECK();
    return ICNV_OK;
}

int launch_de_sort_chunks(double *keys, const DeSegs *segs_dev, const int64_t *chunk_off_dev, int32_t n_sets, int64_t n_chunks,
                          hipStream_t s) {
    if (n_chunks <= 0) return ICNV_OK;
    hipLaunchKernelGGL(de_sort_chunks_kernel, dim3((unsigned)n_chunks), dim3(256), 0, s, keys, segs_dev, chunk_off_dev, n_sets);
    DE_LAUNCH_CHECK();
    return ICNV_OK;
}

int launch_de_merge_pass(const double *src, double *dst, const DeSegs &g, int64_t run, hipStream_t s) {
    const int64_t n = (int64_t)g.n * g.count;
    if (n <= 0) return ICNV_OK;
    hipLaunchKernelGGL(de_merge_pass_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, g, run);
    DE_LAUNCH_CHECK();
    return ICNV_OK;
}

int launch_de_wilcox(const DeWilcox &a, hipStream_t s) {
    const int64_t n = (int64_t)a.n_cmp * a.gw;
    if (n <= 0) return ICNV_OK;
    hipLaunchKernelGGL(de_wilcox_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    DE_LAUNCH_CHECK();
    return ICNV_OK;
}

int launch_de_welch(const DeWelch &a, hipStream_t s) {
    hipLaunchKernelGGL(de_moments_kernel, dim3((unsigned)((a.G + 255) / 256), (unsigned)std::min(a.n_groups, 65535)), dim3(256), 0, s, a);
    DE_LAUNCH_CHECK();
    const int64_t n = (int64_t)a.n_cmp * a.G;
    hipLaunchKernelGGL(de_welch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    DE_LAUNCH_CHECK();
    return ICNV_OK;
}

int launch_de_bh_keys(const double *p, double *keys, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(de_bh_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, keys, n);
    DE_LAUNCH_CHECK();
    return ICNV_OK;
}

int launch_de_bh_finish(const double *p, const double *sorted, double *sm, double *padj, int32_t n_cmp, int32_t G, hipStream_t s) {
    hipLaunchKernelGGL(de_bh_finish_kernel, dim3((unsigned)n_cmp), dim3(256), 0, s, p, sorted, sm, padj, G);
    DE_LAUNCH_CHECK();
    return ICNV_OK;
}

int de_mean_parts() { return DE_MEAN_BLOCKS; }

int launch_de_mean(const double *x, int64_t ld, int32_t G, int32_t C, double *part, double *mean_out, hipStream_t s) {
    hipLaunchKernelGGL(de_mean_partial_kernel, dim3(DE_MEAN_BLOCKS), dim3(256), 0, s, x, ld, G, C, part);
    DE_LAUNCH_CHECK();
    hipLaunchKernelGGL(de_mean_finish_kernel, dim3(1), dim3(64), 0, s, part, DE_MEAN_BLOCKS, (double)G * (double)C, mean_out);
    DE_LAUNCH_CHECK();
    return ICNV_OK;
}

int launch_de_mask(const DeMask &a, hipStream_t s) {
    hipLaunchKernelGGL(de_mask_kernel, dim3((unsigned)((a.G + 255) / 256), (unsigned)std::min(a.C, 65535)), dim3(256), 0, s, a);
    DE_LAUNCH_CHECK();
    return ICNV_OK;
}

}  // namespace icnv
