// The library's own elementary functions, shared by the kernels whose results are held to a sequential restatement bit for
// bit (K11 Leiden, K12 non-DE masking, K13 Bayesian filter): separately rounded IEEE-754 double operations in one fixed
// order.  Every file that includes this header is built with -ffp-contract=off.  Restated operation by operation in
// tests/leiden_restate.py and tests/de_restate.py (exp_lib, log_lib, qnorm_lib, log1p_lib).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "icnv_log_table.h"

namespace icnv {

// exp_lib(x):
//   k = floor(x * (1/ln2) + 0.5);  t = (x - k * ln2_hi) - k * ln2_lo;  p = Horner of sum_{j<=11} t^j / j!;  ldexp(p, k)
// x > 709 (and NaN) gives +inf: the threshold keeps p * 2^k finite (k <= 1023, p < 1).  x < -708 gives 0 (K12's pnorm and pt,
// K13's likelihood ratios; K11 only passes x >= 0): from -708 on, k >= -1021 and p * 2^k stays a normal number.
constexpr double LIB_EXP_MAX = 709.0;
constexpr double LIB_EXP_MIN = -708.0;
__host__ __device__ inline double lib_exp(double x) {
    if (!(x <= LIB_EXP_MAX)) return INFINITY;
    if (x < LIB_EXP_MIN) return 0.0;
    const double kd = floor(x * 1.4426950408889634 + 0.5);
    const double t = (x - kd * 6.93147180369123816490e-01) - kd * 1.90821492927058770002e-10;
    const double c[12] = {1.0, 1.0, 1.0 / 2, 1.0 / 6, 1.0 / 24, 1.0 / 120, 1.0 / 720, 1.0 / 5040, 1.0 / 40320, 1.0 / 362880,
                          1.0 / 3628800, 1.0 / 39916800};
    double p = c[11];
    for (int j = 10; j >= 0; --j) p = p * t + c[j];
    return ldexp(p, (int)kd);
}

#if defined(__HIPCC__)
static __device__ const double g_lib_log_tab[ICNV_LOG_N][3] = ICNV_LOG_TABLE_INIT;

// the library's table log (viterbi_kernels.hip dev_log, the same operation sequence), its table read from global memory
__device__ inline double lib_log(double x) {
    uint64_t ix = (uint64_t)__double_as_longlong(x);
    if (ix - 0x0010000000000000ull >= 0x7fe0000000000000ull) {
        if ((ix << 1) == 0) return -__builtin_inf();
        if (ix == 0x7ff0000000000000ull) return x;
        if ((ix >> 63) || (ix & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) return __builtin_nan("");
        ix = (uint64_t)__double_as_longlong(x * 0x1p52) - (52ull << 52);
    }
    const uint64_t tmp = ix - ICNV_LOG_OFF;
    const int i = (int)((tmp >> 45) & 127);
    const int k = (int)((int64_t)tmp >> 52);
    const double z = __longlong_as_double((long long)(ix - (tmp & 0xfff0000000000000ull)));
    const double r = __builtin_fma(z, g_lib_log_tab[i][0], -1.0);
    const double kd = (double)k;
    const double w = __builtin_fma(kd, ICNV_LOG_LN2HI, g_lib_log_tab[i][1]);
    const double hi = w + r;
    const double lo = ((w - hi) + r) + (kd * ICNV_LOG_LN2LO + g_lib_log_tab[i][2]);
    const double r2 = r * r;
    double q = __builtin_fma(r, ICNV_LOG_B6, ICNV_LOG_B5);
    q = __builtin_fma(r, q, ICNV_LOG_B4);
    q = __builtin_fma(r, q, ICNV_LOG_B3);
    q = __builtin_fma(r, q, ICNV_LOG_B2);
    q = __builtin_fma(r, q, ICNV_LOG_B1);
    q = __builtin_fma(r, q, ICNV_LOG_B0);
    return hi + __builtin_fma(r2, q, lo);
}

template <int N>
__device__ inline double lib_horner(const double (&c)[N], double r) {
    double p = c[N - 1];
#pragma unroll
    for (int j = N - 2; j >= 0; --j) p = p * r + c[j];
    return p;
}

// qnorm5(p, 0, 1) by AS 241 (PPND16) as infercnv_amd/r_rng.qnorm restates it, with the table log
__device__ inline double lib_qnorm(double p) {
    const double A[8] = {3.3871328727963666080e0, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
                         4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3};
    const double B[8] = {1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3, 2.1213794301586595867e+4,
                         3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3};
    const double Cc[8] = {1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
                          1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4};
    const double D[8] = {1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
                         1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9};
    const double E[8] = {6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
                         2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7};
    const double F[8] = {1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
                         1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15};
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return q * lib_horner(A, r) / lib_horner(B, r);
    }
    double r = sqrt(-lib_log(q < 0 ? p : 1.0 - p));
    double val;
    if (r <= 5.0) {
        r = r - 1.6;
        val = lib_horner(Cc, r) / lib_horner(D, r);
    } else {
        r = r - 5.0;
        val = lib_horner(E, r) / lib_horner(F, r);
    }
    return q < 0 ? -val : val;
}

// log1p(y), y >= 0: 2 atanh(s), s = y / (2 + y), by Horner in s^2 for y <= 1/2, the table log of 1 + y above
__device__ inline double lib_log1p(double y) {
    if (!(y <= 0.5)) return lib_log(1.0 + y);
    const double s = y / (2.0 + y);
    const double s2 = s * s;
    double h = 1.0 / 29.0;
    for (int k = 13; k >= 1; --k) h = h * s2 + 1.0 / (double)(2 * k + 1);
    h = h * s2 + 1.0;
    return (2.0 * s) * h;
}
#endif

}  // namespace icnv
