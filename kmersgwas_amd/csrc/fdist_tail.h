// fdist_tail.h — Q(F; 1, df), the upper tail of the F distribution with (1, df) degrees of freedom: the p-value of lmm_lrt's Wald and
// score statistics ("-lmm 4"). One double function for the host (kgwas_fdist_tail) and for the device
// (lmm_refine_all_kernel), so that the CPU suite pins the code the GPU runs.
//
// Q = I_x(a, 1/2), a = df / 2, x = df / (df + F): the two-sided Student-t tail of sqrt(F). I_x is taken from the continued
// fraction of the incomplete beta function (modified Lentz), whose front factor is x^a (1 - x)^(1/2) / (a B(a, 1/2)):
//   - a tiny p keeps its relative accuracy: the front factor is exp(a log x + log r(a)), log x = -log1p(F / df), and 1 - x comes
//     in as F / (df + F), never as a difference;
//   - past x = (a + 1) / (a + 5/2) the fraction converges slowly and p is no longer small: there Q = 1 - I_(1-x)(1/2, a);
//   - r(a) = Gamma(a + 1/2) / Gamma(a), so that B(a, 1/2) = sqrt(pi) / r(a), is never a difference of two lgamma values (at
//     a = 32766 those are 3e5 each and their difference 5): a is raised to >= 20 by r(a) = r(a + 1) a / (a + 1/2), and there
//     log r(a) = 1/2 log a - 1/(8a) + 1/(192a^3) - 1/(640a^5) + 17/(14336a^7) - 31/(18432a^9) + 691/(180224a^11), the Stirling
//     series of log Gamma(a + h) - log Gamma(a) at h = 1/2 (coefficients (2^(1-m) - 2) B_m / (m (m - 1)), m = 2, 4, ..); the first
//     term left out is below 1e-18 at a = 20.
// The fraction's value h is about 1 / (1 - x + 1 / df) and is reached through differences of that size, so its relative error grows
// like h eps: 5e-12 at df = 65533 and F = 3, 2e-13 at df = 1133 (measured against 40-digit arithmetic), below that elsewhere.
#pragma once
#include <cmath>

#if defined(__HIP__) || defined(__HIPCC__)
#define KGWAS_HD __host__ __device__
#else
#define KGWAS_HD
#endif

namespace kgwas {

// log(Gamma(a + 1/2) / Gamma(a)), a > 0
KGWAS_HD inline double log_gamma_half_ratio(double a) {
    double shift = 1.0;  // r(a) = shift * r(a raised)
    while (a < 20.0) {
        shift *= a / (a + 0.5);
        a += 1.0;
    }
    const double z = 1.0 / a, z2 = z * z;
    const double series =
        z * (-1.0 / 8.0 + z2 * (1.0 / 192.0 + z2 * (-1.0 / 640.0 + z2 * (17.0 / 14336.0 + z2 * (-31.0 / 18432.0 + z2 * (691.0 / 180224.0))))));
    return 0.5 * log(a) + series + log(shift);
}

// the continued fraction of I_x(a, b) without its front factor (x below (a + 1) / (a + b + 2) for a quick end)
KGWAS_HD inline double beta_fraction(double a, double b, double x) {
    const double tiny = 1e-300, eps = 2.3e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 4000; m++) {  // (about sqrt(max(a, b)) steps are needed: 181 at a = 32766)
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) <= eps) break;
    }
    return h;
}

// Q(F; 1, df), df > 0. F <= 0 gives 1, F = +inf gives 0, a NaN gives NaN.
KGWAS_HD inline double fdist_tail(double F, double df) {
    if (!(F == F) || !(df > 0.0)) return __builtin_nan("");
    if (F <= 0.0) return 1.0;
    if (F > 1.7e308) return 0.0;
    const double a = 0.5 * df;
    const double omx = F / (df + F);      // 1 - x
    const double logx = -log1p(F / df);   // log x
    const double x = df / (df + F);
    // x^a (1 - x)^(1/2) / B(a, 1/2)
    const double front = exp(a * logx + log_gamma_half_ratio(a)) * sqrt(omx) * 0.5641895835477562869;  // 1 / sqrt(pi)
    if (x < (a + 1.0) / (a + 2.5)) return front * beta_fraction(a, 0.5, x) / a;
    return 1.0 - front * beta_fraction(0.5, a, omx) * 2.0;
}

}  // namespace kgwas
