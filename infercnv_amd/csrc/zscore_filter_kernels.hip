// K32: the reference z-score gene filter (include/icnv.h "reference z-score gene filter").  DESIGN.md section 4 K32.
//
// Three passes over the rows of the listed reference cells of a (C, G) matrix, all of one geometry: a workgroup takes 64
// neighbouring genes (a lane per gene: a wavefront reads 512 contiguous bytes of a row) and a chunk of ZS_CHUNK list positions,
// which its four wavefronts take in turn.  A lane adds its gene's terms into a double-double number in list order; LDS is used
// once, to add the four wavefronts' numbers in wavefront order.  The (chunk, gene) partials go to HBM with plain stores and a
// second small kernel adds them in one fixed order: no atomics, and the same bits for the same (G, n_ref) on every run.
//   ZS_SUM      term v                           -> mean = sum / N, and the largest |v|, which sets the scale of the squares
//   ZS_SQUARES  term ((v - mean) * scale)^2      -> sd = sqrt(sum / (N - 1)) / scale   ((v - mean) is kept as an exact pair)
//   ZS_ABS_Z    term |(v - mean) / sd| (two fp64 operations, as R evaluates it)        -> per gene: sum / n_ref
// Compiled with -ffp-contract=off: the error-free transformations below are sequences of individually rounded operations.
#include <cmath>

#include "zscore_filter_internal.h"

namespace icnv {
namespace {

struct Dd { double hi, lo; };

__device__ __forceinline__ Dd fast_two_sum(double a, double b) {   // |a| >= |b| (or a == 0)
    const double s = a + b;
    return {s, b - (s - a)};
}

__device__ __forceinline__ Dd two_sum(double a, double b) {
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}

__device__ __forceinline__ Dd dd_add_d(Dd a, double v) {
    Dd s = two_sum(a.hi, v);
    s.lo += a.lo;
    return fast_two_sum(s.hi, s.lo);
}

__device__ __forceinline__ Dd dd_add(Dd a, Dd b) {
    Dd s = two_sum(a.hi, b.hi);
    const Dd t = two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = fast_two_sum(s.hi, s.lo);
    s.lo += t.lo;
    return fast_two_sum(s.hi, s.lo);
}

__device__ __forceinline__ Dd dd_div_n(Dd a, double n) {   // n: an integer below 2^53
    const double q1 = a.hi / n;
    const double r = fma(-q1, n, a.hi) + a.lo;
    return fast_two_sum(q1, r / n);
}

__device__ __forceinline__ Dd dd_sqrt(Dd a) {
    const double x = sqrt(a.hi);
    if (!(a.hi > 0.0) || isinf(a.hi)) return {x, 0.0};   // 0, NaN, +Inf (and NaN for a negative number)
    const double p = x * x, e = fma(x, x, -p);
    const double r = ((a.hi - p) - e) + a.lo;
    return fast_two_sum(x, r / (2.0 * x));
}

template <int PASS>
__global__ __launch_bounds__(ZS_NT) void zscore_pass_kernel(const double *__restrict__ x, int64_t ld, int64_t G,
                                                            const int32_t *__restrict__ rows, int64_t n_ref,
                                                            const double *__restrict__ params, double *__restrict__ part_hi,
                                                            double *__restrict__ part_lo, double *__restrict__ part_max) {
    __shared__ double s_hi[ZS_WAVES][ZS_GENES], s_lo[ZS_WAVES][ZS_GENES], s_mx[ZS_WAVES][ZS_GENES];
    const int lane = threadIdx.x & (ZS_GENES - 1), wave = threadIdx.x / ZS_GENES;
    const int64_t g = (int64_t)blockIdx.x * ZS_GENES + lane;
    const int64_t r0 = (int64_t)blockIdx.y * ZS_CHUNK;
    const int64_t r1 = r0 + ZS_CHUNK < n_ref ? r0 + ZS_CHUNK : n_ref;
    double mean = 0.0, sd = 0.0, scale = 1.0;
    if (PASS != ZS_SUM) { mean = params[0]; sd = params[1]; scale = params[2]; }
    Dd acc = {0.0, 0.0};
    double mx = 0.0;
    if (g < G) {
#pragma unroll 4
        for (int64_t r = r0 + wave; r < r1; r += ZS_WAVES) {
            const double v = x[(int64_t)rows[r] * ld + g];
            if (PASS == ZS_SUM) {
                acc = dd_add_d(acc, v);
                mx = fmax(mx, fabs(v));
            } else if (PASS == ZS_SQUARES) {
                const Dd d = two_sum(v, -mean);             // v - mean, exactly
                const double h = d.hi * scale, l = d.lo * scale;
                const double p = h * h;
                const Dd sq = {p, fma(h, h, -p) + 2.0 * (h * l)};
                acc = dd_add(acc, sq);
            } else {
                acc = dd_add_d(acc, fabs((v - mean) / sd));
            }
        }
    }
    s_hi[wave][lane] = acc.hi;
    s_lo[wave][lane] = acc.lo;
    s_mx[wave][lane] = mx;
    __syncthreads();
    if (wave == 0 && g < G) {
#pragma unroll
        for (int w = 1; w < ZS_WAVES; ++w) {
            acc = dd_add(acc, Dd{s_hi[w][lane], s_lo[w][lane]});
            mx = fmax(mx, s_mx[w][lane]);
        }
        const int64_t o = (int64_t)blockIdx.y * G + g;
        part_hi[o] = acc.hi;
        part_lo[o] = acc.lo;
        if (PASS == ZS_SUM) part_max[o] = mx;
    }
}

// one workgroup: thread t adds the partials t, t + 256, ... in that order, then a tree over the threads
__global__ __launch_bounds__(ZS_FINISH_NT) void zscore_finish_total_kernel(int pass, const double *__restrict__ part_hi,
                                                                           const double *__restrict__ part_lo,
                                                                           const double *__restrict__ part_max, int64_t n_part,
                                                                           double n_values, double *params) {
    __shared__ double s_hi[ZS_FINISH_NT], s_lo[ZS_FINISH_NT], s_mx[ZS_FINISH_NT];
    const int t = threadIdx.x;
    Dd acc = {0.0, 0.0};
    double mx = 0.0;
    for (int64_t i = t; i < n_part; i += ZS_FINISH_NT) {
        acc = dd_add(acc, Dd{part_hi[i], part_lo[i]});
        if (pass == ZS_SUM) mx = fmax(mx, part_max[i]);
    }
    s_hi[t] = acc.hi;
    s_lo[t] = acc.lo;
    s_mx[t] = mx;
    __syncthreads();
    for (int stride = ZS_FINISH_NT / 2; stride > 0; stride >>= 1) {
        if (t < stride) {
            const Dd a = dd_add(Dd{s_hi[t], s_lo[t]}, Dd{s_hi[t + stride], s_lo[t + stride]});
            s_hi[t] = a.hi;
            s_lo[t] = a.lo;
            s_mx[t] = fmax(s_mx[t], s_mx[t + stride]);
        }
        __syncthreads();
    }
    if (t != 0) return;
    acc = Dd{s_hi[0], s_lo[0]};
    if (pass == ZS_SUM) {
        params[0] = dd_div_n(acc, n_values).hi;
        // the squares are taken of (v - mean) * 2^k: k = 0 unless the largest |v| lies outside 2^-400 .. 2^400, where a square
        // could leave the double range; then the largest |v| is brought to [1, 2) (a subnormal one as near to it as 2^1000 goes)
        mx = s_mx[0];
        int k = 0;
        if (mx > 0.0 && !isinf(mx)) {
            const int e = ilogb(mx);
            if (e > 400) k = -e;
            else if (e < -400) k = -e < 1000 ? -e : 1000;
        }
        params[2] = ldexp(1.0, k);
        params[3] = ldexp(1.0, -k);
    } else {
        const Dd var = dd_div_n(acc, n_values - 1.0);       // N = 1: 0 / 0, NaN as R's sd of one value
        params[1] = dd_sqrt(var).hi * params[3];
    }
}

__global__ __launch_bounds__(ZS_FINISH_NT) void zscore_finish_genes_kernel(const double *__restrict__ part_hi,
                                                                           const double *__restrict__ part_lo, int64_t G,
                                                                           int64_t n_chunks, double n_ref, double *__restrict__ row_mean) {
    const int64_t g = (int64_t)blockIdx.x * ZS_FINISH_NT + threadIdx.x;
    if (g >= G) return;
    Dd acc = {0.0, 0.0};
    for (int64_t c = 0; c < n_chunks; ++c) acc = dd_add(acc, Dd{part_hi[c * G + g], part_lo[c * G + g]});
    row_mean[g] = dd_div_n(acc, n_ref).hi;
}

}  // namespace

int launch_zscore_pass(int pass, const double *x, int64_t ld, int64_t G, const int32_t *rows_dev, int64_t n_ref, const double *params,
                       double *part_hi, double *part_lo, double *part_max, hipStream_t s) {
    KernelTimer kt("zscore_filter_pass", s);
    const dim3 grid((unsigned)((G + ZS_GENES - 1) / ZS_GENES), (unsigned)zs_chunks(n_ref));
    if (pass == ZS_SUM)
        hipLaunchKernelGGL(zscore_pass_kernel<ZS_SUM>, grid, dim3(ZS_NT), 0, s, x, ld, G, rows_dev, n_ref, params, part_hi, part_lo, part_max);
    else if (pass == ZS_SQUARES)
        hipLaunchKernelGGL(zscore_pass_kernel<ZS_SQUARES>, grid, dim3(ZS_NT), 0, s, x, ld, G, rows_dev, n_ref, params, part_hi, part_lo, part_max);
    else
        hipLaunchKernelGGL(zscore_pass_kernel<ZS_ABS_Z>, grid, dim3(ZS_NT), 0, s, x, ld, G, rows_dev, n_ref, params, part_hi, part_lo, part_max);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_zscore_finish_total(int pass, const double *part_hi, const double *part_lo, const double *part_max, int64_t n_part, int64_t n_values,
                               double *params, hipStream_t s) {
    KernelTimer kt("zscore_filter_finish", s);
    hipLaunchKernelGGL(zscore_finish_total_kernel, dim3(1), dim3(ZS_FINISH_NT), 0, s, pass, part_hi, part_lo, part_max, n_part, (double)n_values,
                       params);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

int launch_zscore_finish_genes(const double *part_hi, const double *part_lo, int64_t G, int64_t n_chunks, int64_t n_ref, double *row_mean,
                               hipStream_t s) {
    KernelTimer kt("zscore_filter_finish", s);
    hipLaunchKernelGGL(zscore_finish_genes_kernel, dim3((unsigned)((G + ZS_FINISH_NT - 1) / ZS_FINISH_NT)), dim3(ZS_FINISH_NT), 0, s, part_hi,
                       part_lo, G, n_chunks, (double)n_ref, row_mean);
    ICNV_HIP(hipGetLastError());
    return ICNV_OK;
}

}  // namespace icnv
