// lf_gammainc.h - the upper incomplete gamma function Gamma(a, x) = int_x^inf t^(a-1) e^-t dt in fp64, for the integrated
// luminosity function (lf_bands_integ in lf_bands.h).  lumfuncmcmc_amd/lfintegrals.py holds the
// NumPy twin: the same algorithm, operation for operation (no contraction here, so the IEEE operations agree to the bit;
// the device library's exp, log, expm1 and pow differ from the C library's in the last bits).
//
// Domain: real a in [GI_A_MIN, GI_A_MAX] = [-5, 7] (alpha + 1 and alpha + 2 for alpha in [-6, 5]), x >= 0.  x = 0 gives
// Gamma(a) for a > 0 and +inf otherwise; x = +inf, and every x whose exp(-x / 2) is 0, gives 0.  A NaN, a negative x or an a
// outside the domain gives NaN before any loop is entered; inside the domain the result is never NaN, and a Gamma(a, x) above
// the largest double (a < 0, x below 1e-61 and less) is +inf.
//
// With m = rint(a), a0 = a - m in [-1/2, 1/2] (exact), w(a0) the polynomial of lf_gammainc_coef.h and
// r = 1 + a0 w = 1 / Gamma(1 + a0):
//   x < GI_XSW = 1, m >= 1:  Gamma(b, x) = 1 / r - x^b e^-x sum_n x^n / (b (b + 1) .. (b + n)) at b = a - (m - 1) in
//       [1/2, 3/2] (all terms positive; the difference loses a factor of at most Gamma(1/2) / Gamma(1/2, 1) = 6.4), then
//       m - 1 steps of Gamma(c + 1, x) = c Gamma(c, x) + x^c e^-x, sums of positive terms.
//   x < 1, m <= 0:  Gautschi's form at the base order a0,
//       Gamma(a0, x) = [ -w / r - expm1(a0 ln x) / a0 ] - x^a0 sum_{n >= 1} (-x)^n / (n! (a0 + n)),
//       whose bracket is Gamma(a0) - x^a0 / a0 without its cancellation and tends to -euler - ln x as a0 -> 0 (taken
//       below |a0| = GI_A0_TINY); then -m steps of Gamma(c - 1, x) = (Gamma(c, x) - x^(c-1) e^-x) / (c - 1), which never
//       divides by 0 (c - 1 <= -1/2) and is stable for x < 1.  a = 0, -1, -2, .. take this path with a0 = 0 exactly.
//       Where |a0 ln x| > GI_AL_POW = 1 the bracket takes (x^a0 - 1) / a0 from the pow the series needs anyway: expm1 would
//       amplify the rounding of the product a0 ln x by |a0 ln x|, up to 370 at the smallest doubles, while x^a0 is then
//       outside [1 / e, e] and the difference loses a factor of 1.6 at the most.  The recurrence runs on
//       GI_REC_SCALE = 2^-8 of its two terms (exact: both stay normal numbers) and a step whose x^(c-1) e^-x is +inf even
//       so gives +inf: Gamma(c - 1, x) = (x^(c-1) e^-x - Gamma(c, x)) / (1 - c), 1 - c <= 5 and Gamma(c, x) smaller by a
//       factor x < 1e-61, is above 2^8 / 5 of the largest double there, and the next step would otherwise take inf - inf.
//       The product with 2^8 at the end overflows exactly when the result does.
//   x >= 1:  Legendre's continued fraction x^c e^-x / (x + 1 - c - 1 (1 - c) / (x + 3 - c - 2 (2 - c) / ..)) evaluated
//       bottom-up from term N = GI_CF_N0 + int(GI_CF_K / x) (one division per term; its error falls like exp(-4 sqrt(N x)),
//       N x >= 120 leaves 1e-19), at c = a for m <= 0 (every partial denominator positive) or at c = b followed by the
//       upward recurrence in the scaled form q' = (c q + 1) / x, q = Gamma(c, x) / (x^c e^-x); the result is
//       ((x^a e^(-x/2)) e^(-x/2)) q so that only the last product can leave the normal range.
//
// Trip caps, all hard: either series GI_SER_CAP = 40 (x < 1: 18 is the most any input takes), the continued fraction
// GI_CF_CAP = 136 (the formula gives at most 8 + 120), either recurrence GI_REC_CAP = 6 (|m| <= 7).  The series leave
// their loops when a term is NOT larger than 2^-54 of the sum, a test a NaN fails.
#pragma once

#include <hip/hip_runtime.h>

#include "lf_gammainc_coef.h"

namespace lf {

constexpr double GI_A_MIN = -5.0, GI_A_MAX = 7.0;
constexpr double GI_XSW = 1.0;
constexpr int GI_SER_CAP = 40;
constexpr int GI_CF_N0 = 8;
constexpr double GI_CF_K = 120.0;
constexpr int GI_CF_CAP = 136;
constexpr int GI_REC_CAP = 6;
constexpr double GI_EPS = 0x1p-54;
constexpr double GI_A0_TINY = 0x1p-500;
constexpr double GI_AL_POW = 1.0;
constexpr double GI_REC_SCALE = 0x1p-8, GI_REC_UNSCALE = 0x1p8;

// 10^t from IEEE operations alone (lfintegrals.exp10 is the same to the bit): Gamma(a, x) ~ e^-x turns one ulp of
// x = 10^t into x ulp of the result, more than the device and the C library's exp10 may differ by.
__device__ __forceinline__ double gi_exp10(double t) {
#pragma clang fp contract(off)
    if (t >= 309.0) return __builtin_inf();
    if (t < -330.0) return 0.0;
    if (!(t == t)) return t;
    const double k = rint(t * GI_LOG2_10);
    const double r = (t - k * GI_LG2_HI) - k * GI_LG2_LO;
    double p = GI_E10[GI_NE10 - 1];
#pragma unroll
    for (int j = GI_NE10 - 2; j >= 0; --j) p = p * r + GI_E10[j];
    return ldexp(p, (int)k);
}

__device__ __forceinline__ double gammainc_upper(double a, double x) {
#pragma clang fp contract(off)
    if (!(x >= 0.0) || !(a >= GI_A_MIN && a <= GI_A_MAX)) return __builtin_nan("");
    const double m = rint(a);
    const int mi = (int)m;
    const double a0 = a - m;
    double w = GI_W[GI_NW - 1];
#pragma unroll
    for (int k = GI_NW - 2; k >= 0; --k) w = w * a0 + GI_W[k];
    const double r = 1.0 + a0 * w;                          // 1 / Gamma(1 + a0)
    const bool up = mi >= 1;
    const double b = a - (m - 1.0);                         // base order of the upward side, in [1/2, 3/2]
    if (x == 0.0) {
        if (!(a > 0.0)) return __builtin_inf();
        double g = 1.0 / r;
        if (!up) return g / a0;
        for (int k = 1; k <= GI_REC_CAP; ++k)
            if (k <= mi - 1) g = g * (a - (double)k);
        return g;
    }
    const bool small = x < GI_XSW;
    const double eh = exp(small ? -x : -0.5 * x);
    if (eh == 0.0) return 0.0;
    const double pw = pow(x, small ? (up ? b : a0) : a);
    if (small && up) {
        double term = 1.0 / b, tot = term;
        for (int k = 1; k <= GI_SER_CAP; ++k) {
            term = term * (x / (b + (double)k));
            tot = tot + term;
            if (!(term > tot * GI_EPS)) break;
        }
        double f = pw * eh;
        double g = 1.0 / r - f * tot;
        for (int k = 0; k < GI_REC_CAP; ++k)
            if (k <= mi - 2) {
                g = (b + (double)k) * g + f;
                f = f * x;
            }
        return g;
    }
    if (small) {
        double t = 1.0, tot = 0.0;
        for (int k = 1; k <= GI_SER_CAP; ++k) {
            t = t * (-x / (double)k);
            const double term = t / (a0 + (double)k);
            tot = tot + term;
            if (!(fabs(term) > fabs(tot) * GI_EPS)) break;
        }
        const double lx = log(x);
        const double al = a0 * lx;
        const double brk = fabs(al) > GI_AL_POW ? (pw - 1.0) / a0 : expm1(al) / a0;
        const double sing = fabs(a0) < GI_A0_TINY ? -GI_W[0] - lx : -w / r - brk;
        double g = (sing - pw * tot) * GI_REC_SCALE;
        double f = (pw * eh) * GI_REC_SCALE;
        for (int k = 1; k <= GI_REC_CAP; ++k)
            if (k <= -mi) {
                f = f / x;
                g = f == __builtin_inf() ? __builtin_inf() : (g - f) / (a + (-m - (double)k));
            }
        return g * GI_REC_UNSCALE;
    }
    const double c = up ? b : a;
    int nt = GI_CF_N0 + (int)(GI_CF_K / x);
    nt = nt < GI_CF_CAP ? nt : GI_CF_CAP;
    double f = x + (2.0 * (double)nt + 1.0) - c;
    for (int k = nt; k >= 1; --k) {
        const double kd = (double)k;
        f = (x + (2.0 * kd - 1.0) - c) + (-kd * (kd - c)) / f;
    }
    double q = 1.0 / f;
    for (int k = 0; k < GI_REC_CAP; ++k)
        if (k <= mi - 2) q = ((b + (double)k) * q + 1.0) / x;
    return ((pw * eh) * eh) * q;
}

}  // namespace lf
