// bfhip_igamc.h -- Q(a, x) = Gamma(a, x) / Gamma(a), the regularised upper incomplete gamma function in double precision: the survival
// function of a chi-square with 2 a degrees of freedom at 2 x.  Plain C++, so that a host build can test the same text.
//
//   prefactor  F = x^a e^-x / Gamma(a).  For a >= 8 through Stirling's series s(a), Gamma(a) = sqrt(2 pi / a) (a / e)^a e^s(a):
//              F = sqrt(a / 2 pi) exp(a (log1p(mu) - mu) - s(a)), mu = (x - a) / a, with log1p(mu) - mu from its own series near 0, so
//              that nothing of size a log a is ever rounded; below 8 as exp(a log x - x - lgamma(a)), whose terms are small.
//   x < max(a, 1)   P = F sum_k x^k / (a (a + 1) ... (a + k)), Q = 1 - P (Q > 0.15 there, so the difference costs no digits)
//   elsewhere       Q = F / (x + 1 - a - 1 (1 - a) / (x + 3 - a - 2 (2 - a) / (x + 5 - a - ...))), evaluated forward with rescaling
// Either sum stops at the first term below the rounding of the total, or after BF_IGAMC_MAXIT terms: about 9 sqrt(a) are needed at
// x = a, so the cap holds to a of a few hundred thousand, far beyond the half-integers up to 1024 this is used for.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define BF_IGAMC_FN __host__ __device__ inline
#else
#define BF_IGAMC_FN inline
#endif
#define BF_IGAMC_MAXIT 5000

// log1p(mu) - mu
BF_IGAMC_FN double bf_log1pmx(double mu) {
    if (fabs(mu) > 0.4) return log1p(mu) - mu;
    // -mu^2 / 2 + mu^3 / 3 - ...: at most 40 terms at 0.4
    double p = mu, s = 0.;
    for (int k = 2; k < 64; ++k) {
        p *= -mu;
        const double t = p / (double)k;
        s += t;
        if (fabs(t) < 1e-17 * fabs(s)) break;
    }
    return s;
}

// x^a e^-x / Gamma(a), a > 0, 0 < x < inf
BF_IGAMC_FN double bf_igam_fac(double a, double x) {
    if (a < 8.) return exp(a * log(x) - x - lgamma(a));
    const double r = 1. / a, r2 = r * r;
    const double s = r * (1. / 12. + r2 * (-1. / 360. + r2 * (1. / 1260. + r2 * (-1. / 1680. + r2 * (1. / 1188. + r2 * (-691. / 360360. +
                     r2 * (1. / 156. + r2 * (-3617. / 122400.))))))));
    return sqrt(a * 0.15915494309189533577) * exp(a * bf_log1pmx((x - a) / a) - s);
}

BF_IGAMC_FN double bf_igamc(double a, double x) {
    if (!(a > 0.) || !(x >= 0.)) return __builtin_nan("");   // (a NaN argument fails both)
    if (x == 0.) return 1.;
    if (a == __builtin_inf()) return __builtin_nan("");
    if (x == __builtin_inf()) return 0.;
    const double fac = bf_igam_fac(a, x);
    if (x < 1. || x < a) {
        if (fac == 0.) return 1.;
        double r = a, c = 1., sum = 1.;
        for (int k = 0; k < BF_IGAMC_MAXIT; ++k) {
            r += 1.;
            c *= x / r;
            sum += c;
            if (c <= 1.1e-16 * sum) break;
        }
        return 1. - fac * sum / a;
    }
    if (fac == 0.) return 0.;
    const double big = 4503599627370496., biginv = 2.22044604925031308085e-16;
    double y = 1. - a, z = x + y + 1., c = 0.;
    double pkm2 = 1., qkm2 = x, pkm1 = x + 1., qkm1 = z * x, ans = pkm1 / qkm1;
    for (int k = 0; k < BF_IGAMC_MAXIT; ++k) {
        c += 1.;
        y += 1.;
        z += 2.;
        const double yc = y * c, pk = pkm1 * z - pkm2 * yc, qk = qkm1 * z - qkm2 * yc;
        double t = 1.;
        if (qk != 0.) {
            const double q = pk / qk;
            t = fabs((ans - q) / q);
            ans = q;
        }
        pkm2 = pkm1;
        pkm1 = pk;
        qkm2 = qkm1;
        qkm1 = qk;
        if (fabs(pk) > big) {
            pkm2 *= biginv;
            pkm1 *= biginv;
            qkm2 *= biginv;
            qkm1 *= biginv;
        }
        if (t <= 1.1e-16) break;
    }
    return ans * fac;
}
