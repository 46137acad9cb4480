// bfhip_constraint.h -- the constraint transform of one coordinate (transforms/_constraint.pyx:133-215), the ONE copy every
// kernel family and the Hessian code evaluate.  Plain arithmetic, host and device (tests/test_constraint_host.py sweeps it on the CPU through tests/hess_host).
//
//   kind 0 (none):      T = lo + rg x
//   kind 1 (two-sided): T = lo + rg t,          t = 1 / (1 + exp(-x))
//   kind 2 (lower):     T = lo + rg exp(x)
//   kind 3 (upper):     T = lo + rg (1 - exp(x))
//
// What the density needs of T is J = T', log|J| (density.py:748) and J2 / J = d log|J| / dx (density.py:749-750); the Hessian also
// d2 log|J| / dx2.  The reference's statements form the logistic kind's J as t (1 - t), and J2 / J by a division of two such
// products; 1 - t cancels once exp(-x) nears the rounding of 1 (x of a few tens), and is 0 from x = 37: log|J| = -inf where the
// true value is about -x.  Here the logistic kind is taken on the side where nothing cancels, with a = exp(-|x|) <= 1 and
// s = 1 / (1 + a) in [1/2, 1]:
//
//   t = s (x >= 0),  a s (x < 0)           J = a s^2 rg
//   J2 / J = 1 - 2 t = -+ (1 - a) s         (1 - a is exact or harmless: the result is then near 0 against a gradient of order 1)
//   log|J| = -|x| + log(s^2 |rg|)           d2 log|J| / dx2 = -2 a s^2
//
// so every kind has log|J| = lin + log(c) with lin linear in x and c of the size of the range: one exponential per coordinate,
// and the logarithm is the caller's -- a lane that owns several coordinates may take one logarithm of the product of their c
// (bfhip_group.h), which cannot underflow the way a product of Jacobians does.  Where J itself underflows to zero (|x| beyond
// about 745) c is zero: log|J| is -inf there, with J, rather than a number that no longer belongs to the J returned.
#pragma once
#include <math.h>
#include "bfhip_model.h"

struct BfConstraint {
    double xo;       // T(x)
    double J;        // T'(x)
    double jt;       // T'(x) / rg
    double gj;       // T''(x) / T'(x) = d log|J| / dx
    double lin, c;   // log|J| = lin + log(c)
};

struct BfLibmExp {
    __host__ __device__ double operator()(double x) const { return exp(x); }
};
struct BfLibmLog {
    __host__ __device__ double operator()(double x) const { return log(x); }
};

// (one exponential serves every kind and no kind branches: lanes of a wave hold coordinates of different kinds)
// UF: report log|J| = -inf where J has underflowed to zero.  The sampler kernels leave the test out (UF = false: two instructions
// per coordinate and leapfrog step; a chain has no way to |x| > 745, and lin + log(c) is the true value there anyway).
template <bool UF = true, typename EXP = BfLibmExp>
__host__ __device__ inline __attribute__((always_inline)) BfConstraint bf_constraint(double x, int kind, double lo, double rg,
                                                                                     EXP ex = EXP()) {
    const double ax = fabs(x);
    const double arg = kind == 1 ? -ax : x;
    const double a = ex(arg);
    // (s serves the logistic kind only; for the other kinds a = exp(x) may be inf and s zero or NaN: computed for every lane, selected
    // by none)
    const double s = 1. / (1. + a), as = a * s;
    const double ar = fabs(rg);
    double tmp = x, jt = 1., g = 0., c = ar;
    if (kind == 1) {
        tmp = x >= 0. ? s : as;
        jt = as * s;
        g = copysign((1. - a) * s, -x);
        c = (s * s) * ar;
    }
    if (kind == 2) { tmp = a; jt = a; g = 1.; }
    if (kind == 3) { tmp = 1. - a; jt = -a; g = 1.; }
    BfConstraint r;
    r.xo = lo + tmp * rg;
    r.J = jt * rg;
    r.jt = jt;
    r.gj = g;
    r.lin = kind == 0 ? 0. : arg;   // -|x| for the logistic kind, x for the one-sided kinds
    r.c = (UF && r.J == 0.) ? 0. : c;
    return r;
}

// the form most callers want: T(x), J, log|J| and J2 / J
template <bool UF = true, typename EXP = BfLibmExp, typename LOG = BfLibmLog>
__host__ __device__ inline __attribute__((always_inline)) void bf_to_original(double x, int kind, double lo, double rg, double &xo,
                                                                              double &J, double &lj, double &gj, EXP ex = EXP(),
                                                                              LOG lg = LOG()) {
    const BfConstraint r = bf_constraint<UF>(x, kind, lo, rg, ex);
    xo = r.xo;
    J = r.J;
    lj = r.lin + lg(r.c);
    gj = r.gj;
}

// second derivative of log|J|: the logistic kind's -2 t (1 - t); the other kinds' log|J| is linear in x
__host__ __device__ inline double bf_constraint_lj2(const BfConstraint &r, int kind) { return kind == 1 ? -2. * r.jt : 0.; }
