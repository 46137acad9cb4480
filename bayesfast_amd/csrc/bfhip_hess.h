// bfhip_hess.h -- value, gradient and Hessian of the uploaded scalar surrogate density at ONE point, as arithmetic.
//
// The function is the one bfhip_logp_grad returns (bf_eval_w1, bfhip_eval.h; Density.logp_and_grad, core/density.py:724-754); the
// Hessian is the symmetrised Jacobian of that gradient, closed form in every term (the density is a polynomial seen through
// per-coordinate maps):
//
//   xs_i = (T_i(x_i) - su_lo_i) / su_diff_i,  a_i = dxs_i/dx_i,  b_i = d2xs_i/dx_i^2     (T the constraint transform, or the identity)
//   p(xs) the polynomial, gp its gradient, F = S + (cubic terms, linear in xs) its Hessian
//   outside the bound (beta > alpha; xm = xs - mu, h = H xm, beta^2 = xm.h, x0 = mu + (alpha/beta) xm, j0, F at x0, u = F xm, q = xm.u,
//   coef = (f(x0) - f_mu)/alpha - (j0.xm)/beta):
//       Hp = (alpha/beta) [F - (u h^T + h u^T)/beta^2 + q h h^T/beta^4] + (coef/beta) [sym(H) - h h^T/beta^2],   gp = j0 + coef h/beta
//   m(x) = p(xs(x)):  gm_i = gp_i a_i,  Hm_ij = a_i Hp_ij a_j + delta_ij gp_i b_i
//   Gaussian link:    dphi = -prec (m - y);  H = dphi Hm - prec gm gm^T      (no link: dphi = 1, prec = 0)
//   decay term, where beta_d^2 > alpha_2: the gradient is -2 gamma H_d^T (xo - mu_d) WITHOUT the transform's Jacobian (density.py:745),
//       so its Jacobian is -2 gamma H_d[j][i] J_j; symmetrised: -gamma (H_d[j][i] J_j + H_d[i][j] J_i)
//   transform (original_space = 0): + delta_ij d2/dx_i^2 log|T'_i|    (logit: -2 s (1 - s); the one-sided kinds and the affine one: 0)
//
// On the surfaces beta = alpha and beta_d^2 = alpha_2 the function is C^1 only; the Hessian takes the gradient's branch.
//
// The code is written for a team of nt cooperating threads (tid = 0 .. nt - 1) that share the work arrays and meet at BF_HESS_SYNC():
// a workgroup with the arrays in LDS on the device, one thread (nt = 1, no barrier) on the host -- tests/hess_host compiles this
// header with BF_HOST_EMU.  Matrix-vector products are parallel over rows; every scalar reduction is taken by every thread over the
// shared vectors in index order, so all threads hold the same scalars bit for bit and branch alike.  No HIP-only construct here.
#pragma once
#include <math.h>
#include "bfhip_model.h"
#include "bfhip_constraint.h"

#ifdef BF_HOST_EMU
#define BF_HESS_SYNC() ((void)0)
#else
#define BF_HESS_SYNC() __syncthreads()
#endif

// entry (r, c) of a DP x DP matrix stored as MFMA A-operand fragments (bfhip_model.h: DevModel)
__host__ __device__ inline double bf_frag_at(const double *f, int DP, int r, int c) {
    return f[((size_t)(r >> 4) * (DP >> 2) + (c >> 2)) * 64 + ((c & 3) << 4) + (r & 15)];
}

// sum_k M[i][k] (v[k] - c[k]) over k < d in index order (c may be NULL)
__host__ __device__ inline double bf_frag_row_dot(const double *f, int DP, int i, const double *v, const double *c, int d) {
    double acc = 0.;
    for (int k = 0; k < d; ++k) acc += bf_frag_at(f, DP, i, k) * (c ? v[k] - c[k] : v[k]);
    return acc;
}

// Pair number idx of the lower triangle (i >= j) of an n x n matrix, rows a and n - 1 - a folded into one line of n + 1 slots:
// idx < bf_tri_slots(n); false for the slots that fall off (the middle row's second half when n is odd).
__host__ __device__ inline int bf_tri_slots(int n) { return ((n + 1) / 2) * (n + 1); }
__host__ __device__ inline bool bf_tri_pair(int n, int idx, int &i, int &j) {
    const int a = idx / (n + 1), b = idx - a * (n + 1);
    if (b <= a) {
        i = a;
        j = b;
        return true;
    }
    i = n - 1 - a;
    j = b - a - 1;
    return i > a;
}

#define BF_HESS_NVEC 17   // work vectors of d doubles each (BfHessWork)

struct BfHessWork {
    double *xo, *xs, *a, *b, *J, *lj, *lj2, *gj;   // original-space point, scaled point, dxs/dx, d2xs/dx2, T', log|T'|, its 2nd derivative, T''/T'
    double *sx, *fc, *gp, *xm, *h, *x0, *u, *dg;   // S xe, cubic value terms, polynomial gradient, xs - mu, H xm, projected point, F xm, decay H_d^T xd
    double *g;                                     // the gradient of logp (result)
    const double *xe;                              // where F is evaluated: x0 outside the bound, xs inside
};

__host__ __device__ inline void bf_hess_work_bind(BfHessWork &w, double *buf, int d) {
    double **p[BF_HESS_NVEC] = {&w.xo, &w.xs, &w.a, &w.b, &w.J, &w.lj, &w.lj2, &w.gj, &w.sx, &w.fc, &w.gp, &w.xm, &w.h, &w.x0, &w.u, &w.dg, &w.g};
    for (int i = 0; i < BF_HESS_NVEC; ++i) *p[i] = buf + (size_t)i * d;
    w.xe = w.xs;
}

// the scalars of one evaluation (every thread holds its own, identical copy)
struct BfHessPt {
    double logp;
    int oob, dec, tr;
    double ab, cb, ib2, q;   // alpha/beta, coef/beta, 1/beta^2, xm.F xm
    double dphi, prec;
};

// constraint transform of one coordinate with the derivatives the Hessian needs (bfhip_constraint.h): T, T', T'', log|T'| and
// the first two derivatives of log|T'|
__host__ __device__ inline void bf_hess_transform(double x, int kind, double lo, double rg, double &xo, double &J, double &J2, double &lj,
                                                  double &gj, double &lj2) {
    const BfConstraint tc = bf_constraint(x, kind, lo, rg);
    xo = tc.xo;
    J = tc.J;
    J2 = tc.gj * tc.J;
    lj = tc.lin + log(tc.c);
    gj = tc.gj;
    lj2 = bf_constraint_lj2(tc, kind);
}

// cubic-2 and cubic-3 contributions to gradient component i at the point x (modules/_poly.pyx:49-137; bf_cubic_grad of bfhip_eval.h)
__host__ __device__ inline void bf_hess_cubic_grad(const DevModel &m, int i, const double *x, double &gc, double &fc) {
    gc = 0.;
    fc = 0.;
    const int p2 = m.n2 > 0 ? m.pos2[i] : -1;
    if (p2 >= 0) {
        double v1 = 0., v2 = 0.;
        for (int k = 0; k < m.n2; ++k) {
            const double xk = x[m.mask2[k]];
            v1 += m.A2t[k * m.n2 + p2] * xk;
            v2 += m.A2[k * m.n2 + p2] * (xk * xk);
        }
        gc += 2. * x[i] * v1 + v2;
        fc += x[i] * x[i] * v1;
    }
    const int p3 = m.n3 > 0 ? m.pos3[i] : -1;
    if (p3 >= 0) {
        double s = 0.;
        for (int k = 0; k < m.n3; ++k) {
            double t = 0.;
            for (int l = 0; l < m.n3; ++l) t += m.T3t[((size_t)k * m.n3 + l) * m.n3 + p3] * x[m.mask3[l]];
            s += t * x[m.mask3[k]];
        }
        gc += 0.5 * s;
        fc += x[i] * (0.5 * s) * (1. / 3.);
    }
}

// entry (i, j), i <= j, of the polynomial's Hessian F at the point x:
//   cubic-2  f = sum_j x_j^2 (a x)_j:   F_jl = 2 delta_jl (a x)_j + 2 x_j a[j][l] + 2 a[l][j] x_l
//   cubic-3  f = 1/6 sum T[j,k,l] x_j x_k x_l (T the symmetric fill):   F_jm = sum_l T[j,m,l] x_l
__host__ __device__ inline double bf_hess_poly_entry(const DevModel &m, const double *x, int i, int j) {
    double F = m.has_quad ? bf_frag_at(m.Sf, m.DP, i, j) : 0.;
    if (!m.has_cubic) return F;
    const int pi = m.n2 > 0 ? m.pos2[i] : -1, pj = m.n2 > 0 ? m.pos2[j] : -1;
    if (pi >= 0 && pj >= 0) {
        double c = 2. * (x[i] * m.A2[pi * m.n2 + pj]) + 2. * (m.A2[pj * m.n2 + pi] * x[j]);
        if (i == j) {
            double v1 = 0.;
            for (int k = 0; k < m.n2; ++k) v1 += m.A2t[k * m.n2 + pi] * x[m.mask2[k]];
            c += 2. * v1;
        }
        F += c;
    }
    const int qi = m.n3 > 0 ? m.pos3[i] : -1, qj = m.n3 > 0 ? m.pos3[j] : -1;
    if (qi >= 0 && qj >= 0 && qi != qj) {
        const double *T = m.T3t + ((size_t)qi * m.n3 + qj) * m.n3;
        double s = 0.;
        for (int l = 0; l < m.n3; ++l) s += T[l] * x[m.mask3[l]];
        F += s;
    }
    return F;
}

// Value and gradient at x (d doubles, any address space), and every vector bf_hess_entry needs.  All nt threads call it; on return
// (after its last barrier) w.g holds the gradient and the returned scalars are the same in every thread.  want_hess = 0 skips the one
// product only the Hessian uses (u = F xm).
__host__ __device__ inline BfHessPt bf_hess_eval(const DevModel &m, const double *x, int original_space, BfHessWork &w, int tid, int nt,
                                                 int want_hess) {
    const int d = m.d, DP = m.DP;
    const double *pd = m.pd;
    BfHessPt r;
    r.tr = m.has_transform && !original_space;
    r.oob = 0;
    r.dec = 0;
    r.ab = r.cb = r.ib2 = r.q = 0.;
    r.dphi = 1.;
    r.prec = 0.;
    BF_HESS_SYNC();   // the previous evaluation's readers are done
    for (int i = tid; i < d; i += nt) {
        double xo = x[i], J = 1., J2 = 0., lj = 0., gj = 0., lj2 = 0.;
        if (r.tr) bf_hess_transform(x[i], (int)pd[PD_KIND * DP + i], pd[PD_LO * DP + i], pd[PD_RG * DP + i], xo, J, J2, lj, gj, lj2);
        const double diff = m.has_su ? pd[PD_SU_DIFF * DP + i] : 1.;
        w.xo[i] = xo;
        w.xs[i] = m.has_su ? (xo - pd[PD_SU_LO * DP + i]) / diff : xo;
        w.J[i] = J;
        w.a[i] = J / diff;
        w.b[i] = J2 / diff;
        w.lj[i] = lj;
        w.lj2[i] = lj2;
        w.gj[i] = gj;
    }
    BF_HESS_SYNC();
    for (int i = tid; i < d; i += nt) {
        double sx = 0., gc = 0., fc = 0.;
        if (m.has_quad)
            sx = bf_frag_row_dot(m.Sf, DP, i, w.xs, NULL, d);
        if (m.has_cubic) bf_hess_cubic_grad(m, i, w.xs, gc, fc);
        w.sx[i] = sx;
        w.fc[i] = fc;
        w.gp[i] = (sx + pd[PD_LIN * DP + i]) + gc;
        if (m.use_bound) {
            const double hv = bf_frag_row_dot(m.Hf, DP, i, w.xs, pd + PD_MU * DP, d);
            w.xm[i] = w.xs[i] - pd[PD_MU * DP + i];
            w.h[i] = hv;
        }
        if (m.use_decay) {   // (Hdf holds H_d^T: the gradient is (xo - mu_d) H_d, core/density.py:745)
            w.dg[i] = bf_frag_row_dot(m.Hdf, DP, i, w.xo, pd + PD_DMU * DP, d);
        }
    }
    BF_HESS_SYNC();
    double quad = 0., lin = 0., fcub = 0., b2 = 0., bd2 = 0., logdet = 0.;
    for (int i = 0; i < d; ++i) {
        quad += w.xs[i] * w.sx[i];
        lin += pd[PD_LIN * DP + i] * w.xs[i];
        fcub += w.fc[i];
        if (m.use_bound) b2 += w.xm[i] * w.h[i];
        if (m.use_decay) bd2 += (w.xo[i] - pd[PD_DMU * DP + i]) * w.dg[i];
        logdet += w.lj[i];
    }
    double f = ((m.c0 + lin) + 0.5 * quad) + fcub;
    w.xe = w.xs;
    const double beta = m.use_bound ? sqrt(b2) : 0.;
    if (m.use_bound && beta > m.alpha) {   // linear extrapolation outside the alpha-ellipsoid (modules/poly.py:480-503)
        r.oob = 1;
        for (int i = tid; i < d; i += nt) w.x0[i] = (m.alpha * w.xs[i] + (beta - m.alpha) * pd[PD_MU * DP + i]) / beta;
        BF_HESS_SYNC();   // (also: every thread has taken the sums above before sx and fc are overwritten)
        w.xe = w.x0;
        for (int i = tid; i < d; i += nt) {
            double sx = 0., gc = 0., fc = 0.;
            if (m.has_quad)
                sx = bf_frag_row_dot(m.Sf, DP, i, w.x0, NULL, d);
            if (m.has_cubic) bf_hess_cubic_grad(m, i, w.x0, gc, fc);
            w.sx[i] = sx;
            w.fc[i] = fc;
            w.gp[i] = (sx + pd[PD_LIN * DP + i]) + gc;   // j0
            if (want_hess) {
                double uv = 0.;
                for (int k = 0; k < d; ++k) uv += bf_hess_poly_entry(m, w.x0, i < k ? i : k, i < k ? k : i) * w.xm[k];
                w.u[i] = uv;
            }
        }
        BF_HESS_SYNC();
        double quad0 = 0., lin0 = 0., fcub0 = 0., dotj = 0., q = 0.;
        for (int i = 0; i < d; ++i) {
            quad0 += w.x0[i] * w.sx[i];
            lin0 += pd[PD_LIN * DP + i] * w.x0[i];
            fcub0 += w.fc[i];
            dotj += w.gp[i] * w.xm[i];
            if (want_hess) q += w.xm[i] * w.u[i];
        }
        const double f0 = ((m.c0 + lin0) + 0.5 * quad0) + fcub0;
        f = (beta * f0 - (beta - m.alpha) * m.f_mu) / m.alpha;
        const double coef = (f0 - m.f_mu) / m.alpha - dotj / beta;
        r.ab = m.alpha / beta;
        r.cb = coef / beta;
        r.ib2 = 1. / b2;
        r.q = q;
        BF_HESS_SYNC();   // every thread has read j0 before it becomes the gradient
        for (int i = tid; i < d; i += nt) w.gp[i] = w.gp[i] + coef * (w.h[i] / beta);
    }
    if (m.has_link) {   // logp = phi(m), phi the Gaussian log likelihood of the surrogate's output (core/density.py:552-560)
        const double res = f - m.link_y;
        r.dphi = -(m.link_prec * res);
        r.prec = m.link_prec;
        f = m.link_logp0 - 0.5 * (res * (m.link_prec * res));
    }
    if (m.use_decay) {
        const double ex = bd2 - m.decay_alpha2;
        f -= m.decay_gamma * (ex > 0. ? ex : (ex != ex ? ex : 0.));   // np.clip keeps NaN
        r.dec = bd2 > m.decay_alpha2;
    }
    if (r.tr) f += logdet;
    for (int i = tid; i < d; i += nt) {   // (gp_i is this thread's own element)
        double gv = r.dphi * (w.gp[i] * w.a[i]);
        if (r.dec) gv -= 2. * m.decay_gamma * w.dg[i];
        w.g[i] = gv + w.gj[i];
    }
    r.logp = f;
    BF_HESS_SYNC();
    return r;
}

// entry (i, j) of the Hessian of logp at the point of the last bf_hess_eval(.., want_hess = 1).  Computed from the ordered pair
// (min, max), so that entry(i, j) == entry(j, i) bit for bit whichever thread takes which.
__host__ __device__ inline double bf_hess_entry(const DevModel &m, const BfHessWork &w, const BfHessPt &r, int i, int j) {
    if (i > j) {
        const int t = i;
        i = j;
        j = t;
    }
    const int DP = m.DP;
    double Hp = bf_hess_poly_entry(m, w.xe, i, j);
    if (r.oob) {
        const double hh = w.h[i] * w.h[j] * r.ib2;
        const double Hs = 0.5 * (bf_frag_at(m.Hf, DP, i, j) + bf_frag_at(m.Hf, DP, j, i));
        Hp = r.ab * ((Hp - (w.u[i] * w.h[j] + w.h[i] * w.u[j]) * r.ib2) + r.q * r.ib2 * hh) + r.cb * (Hs - hh);
    }
    const double gmi = w.gp[i] * w.a[i], gmj = w.gp[j] * w.a[j];
    double v = r.dphi * ((w.a[i] * w.a[j]) * Hp) - r.prec * (gmi * gmj);
    if (r.dec) v -= m.decay_gamma * (bf_frag_at(m.Hdf, DP, i, j) * w.J[j] + bf_frag_at(m.Hdf, DP, j, i) * w.J[i]);
    if (i == j) v += r.dphi * (w.gp[i] * w.b[i]) + w.lj2[i];
    return v;
}

// ---- damped Newton maximiser of logp in the sampling space (original_space = 0), one team per start -------------------------------
// Per iteration: A = -H + lambda I, Cholesky in place, step = A^-1 g.  The iteration first tries lambda = 0 (Newton's own step); if
// -H does not factor or the step does not increase logp, lambda restarts at max(lambda_prev / 10, 1e-3 max|H_ii|) and grows tenfold
// until a step ascends (Levenberg).  A start ends when sum|step| / d <= xtol: status 0 if that step was undamped, 3 if it was damped
// (a damped step is shorter than Newton's: its length says nothing about the distance to the maximum).  The symmetric Hessian lives
// in the strict upper triangle of M plus the vector hd, the factor in the lower triangle and the diagonal: a retry needs no second
// matrix and no second evaluation.
#define BF_NEWTON_NVEC 6
#define BF_NEWTON_MAX_RAISE 400   // (1e-3 .. overflow: lambda is non-finite long before; a bound on the loop, never reached by a finite problem)

struct BfNewtonWork {
    double *M;     // [d][ld]
    int ld;
    double *x, *xt, *gc, *r, *st, *hd;   // current point, trial point, gradient at x, solve scratch / step, solve scratch, diag(H)
};

__host__ __device__ inline void bf_newton_work_bind(BfNewtonWork &nw, double *M, int ld, double *buf, int d) {
    nw.M = M;
    nw.ld = ld;
    nw.x = buf;
    nw.xt = buf + d;
    nw.gc = buf + 2 * (size_t)d;
    nw.r = buf + 3 * (size_t)d;
    nw.st = buf + 4 * (size_t)d;
    nw.hd = buf + 5 * (size_t)d;
}

__host__ __device__ inline bool bf_finite(double v) { return (v - v) == 0.; }

// H of the last evaluation -> upper triangle of M and hd; the gradient -> gc
__host__ __device__ inline void bf_newton_store(const DevModel &m, const BfHessWork &w, const BfHessPt &pt, BfNewtonWork &nw, int tid, int nt) {
    const int d = m.d;
    for (int idx = tid; idx < bf_tri_slots(d); idx += nt) {
        int i, j;
        if (!bf_tri_pair(d, idx, i, j)) continue;   // (i >= j)
        const double v = bf_hess_entry(m, w, pt, j, i);
        if (i == j) nw.hd[i] = v;
        else nw.M[(size_t)j * nw.ld + i] = v;
    }
    for (int i = tid; i < d; i += nt) nw.gc[i] = w.g[i];
    BF_HESS_SYNC();
}

// lower triangle and diagonal of M <- Cholesky factor of -H + lam I; 0 when a pivot is not positive and finite
__host__ __device__ inline int bf_newton_chol(BfNewtonWork &nw, int d, double lam, int tid, int nt) {
    const int ld = nw.ld;
    double *M = nw.M;
    for (int idx = tid; idx < bf_tri_slots(d); idx += nt) {
        int i, j;
        if (!bf_tri_pair(d, idx, i, j)) continue;
        M[(size_t)i * ld + j] = i == j ? lam - nw.hd[i] : -M[(size_t)j * ld + i];
    }
    BF_HESS_SYNC();
    for (int k = 0; k < d; ++k) {
        const double p = M[(size_t)k * ld + k];
        if (!(p > 0.) || !bf_finite(p)) return 0;   // (the same value in every thread)
        const double sp = sqrt(p);
        BF_HESS_SYNC();   // every thread has read the pivot
        for (int i = k + tid; i < d; i += nt) M[(size_t)i * ld + k] = (i == k) ? sp : M[(size_t)i * ld + k] / sp;
        BF_HESS_SYNC();
        const int mm = d - k - 1;
        for (int idx = tid; idx < bf_tri_slots(mm); idx += nt) {   // the trailing lower triangle, one pair per slot
            int i, j;
            if (!bf_tri_pair(mm, idx, i, j)) continue;
            i += k + 1;
            j += k + 1;
            M[(size_t)i * ld + j] -= M[(size_t)i * ld + k] * M[(size_t)j * ld + k];
        }
        BF_HESS_SYNC();
    }
    return 1;
}

// r <- (L L^T)^-1 gc
__host__ __device__ inline void bf_newton_solve(BfNewtonWork &nw, int d, int tid, int nt) {
    const int ld = nw.ld;
    const double *M = nw.M;
    for (int i = tid; i < d; i += nt) nw.r[i] = nw.gc[i];
    for (int k = 0; k < d; ++k) {
        BF_HESS_SYNC();
        const double yk = nw.r[k] / M[(size_t)k * ld + k];
        for (int i = k + 1 + tid; i < d; i += nt) nw.r[i] -= M[(size_t)i * ld + k] * yk;
        if (tid == 0) nw.st[k] = yk;
    }
    for (int k = d - 1; k >= 0; --k) {
        BF_HESS_SYNC();
        const double sk = nw.st[k] / M[(size_t)k * ld + k];
        for (int i = tid; i < k; i += nt) nw.st[i] -= M[(size_t)k * ld + i] * sk;
        if (tid == 0) nw.r[k] = sk;   // (r is free: the forward pass is over)
    }
    BF_HESS_SYNC();
}

// what the iteration itself returns; the evaluation (below) keeps the rest
struct BfNewtonStat {
    double logp;
    int n_iter, status;
    double last_step, lam;
};

// The iteration on any evaluation Ev of a team:
//   double Ev::eval(const double *x, int tid, int nt)   logp at x, and whatever store needs, left in the evaluation's own work arrays;
//                                                       all threads call it, its last barrier passed on return
//   void Ev::store(BfNewtonWork &nw, int tid, int nt)   H of the LAST eval -> upper triangle of nw.M and nw.hd, its gradient -> nw.gc,
//                                                       then a barrier
// On return the last eval was taken at the returned point nw.x and stored.
//
// fixed (d bytes, any address space; NULL: none) holds coordinates in place: the step of a fixed coordinate is exactly zero and its
// x leaves with the bits it came in with.  After every store, row and column i of the stored matrix become an identity row (hd_i = -1:
// the pivot of -H + lambda I is lambda + 1) and gc_i = 0, so the factor's entries in that row are exactly zero and all indexing stays
// as it is.  The convergence measure, the damping scale and hence the Levenberg shift range over the free coordinates only.  With
// no free coordinate the call evaluates once: status 0 (2 for a non-finite value), 0 iterations.
__host__ __device__ inline void bf_newton_mask(BfNewtonWork &nw, int d, const uint8_t *fixed, int tid, int nt) {
    for (int idx = tid; idx < bf_tri_slots(d); idx += nt) {
        int i, j;
        if (!bf_tri_pair(d, idx, i, j)) continue;   // (i >= j)
        if (!fixed[i] && !fixed[j]) continue;
        if (i == j) {
            nw.hd[i] = -1.;
            nw.gc[i] = 0.;
        } else {
            nw.M[(size_t)j * nw.ld + i] = 0.;
        }
    }
    BF_HESS_SYNC();
}

template <class Ev>
__host__ __device__ inline BfNewtonStat bf_newton_run(Ev &ev, int d, const double *x0, int max_iter, double xtol, BfNewtonWork &nw, int tid,
                                                      int nt, const uint8_t *fixed = NULL) {
    BfNewtonStat res;
    res.n_iter = 0;
    res.status = 1;
    res.last_step = 0.;
    res.lam = 0.;
    int n_free = d;
    if (fixed)
        for (int i = 0; i < d; ++i) n_free -= fixed[i] ? 1 : 0;
    BF_HESS_SYNC();
    for (int i = tid; i < d; i += nt) nw.x[i] = x0[i];
    BF_HESS_SYNC();
    double f = ev.eval(nw.x, tid, nt), lam_prev = 0.;
    ev.store(nw, tid, nt);
    if (fixed) bf_newton_mask(nw, d, fixed, tid, nt);
    if (!bf_finite(f)) res.status = 2;
    else if (n_free == 0) res.status = 0;
    for (int it = 0; it < max_iter && res.status == 1; ++it) {
        double hmax = 0.;
        for (int i = 0; i < d; ++i)
            if (!fixed || !fixed[i]) hmax = fmax(hmax, fabs(nw.hd[i]));
        const double lam0 = hmax > 0. ? 1e-3 * hmax : 1e-3;
        double lam = 0., ms = 0., ft = f;
        int accepted = 0;
        for (int n_try = 0; n_try < BF_NEWTON_MAX_RAISE; ++n_try) {
            if (bf_newton_chol(nw, d, lam, tid, nt)) {
                bf_newton_solve(nw, d, tid, nt);
                ms = 0.;
                for (int i = 0; i < d; ++i)
                    if (!fixed || !fixed[i]) ms += fabs(nw.r[i]);
                ms /= (double)n_free;
                if (!bf_finite(ms)) {
                    res.status = 2;
                    break;
                }
                if (lam > 0. && ms <= xtol) {   // a damped step this short: stay, and say so
                    res.status = 3;
                    res.last_step = ms;
                    res.lam = lam;
                    break;
                }
                for (int i = tid; i < d; i += nt) nw.xt[i] = (fixed && fixed[i]) ? nw.x[i] : nw.x[i] + nw.r[i];
                BF_HESS_SYNC();
                ft = ev.eval(nw.xt, tid, nt);
                // (near the maximum the increase falls below the rounding of logp itself)
                if (bf_finite(ft) && ft >= f - 1e-13 * fmax(1., fabs(f))) {
                    accepted = 1;
                    break;
                }
            }
            BF_HESS_SYNC();
            lam = lam > 0. ? 10. * lam : fmax(0.1 * lam_prev, lam0);
        }
        if (!accepted) {
            if (res.status == 1) res.status = 3;   // (BF_NEWTON_MAX_RAISE)
            if (res.status == 3 && !(res.lam > 0.)) res.lam = lam;
            // the work vectors may hold a rejected trial point: evaluate the point that is returned
            (void)ev.eval(nw.x, tid, nt);   // (f is logp at nw.x already)
            ev.store(nw, tid, nt);
            if (fixed) bf_newton_mask(nw, d, fixed, tid, nt);
            break;
        }
        for (int i = tid; i < d; i += nt) nw.x[i] = nw.xt[i];
        f = ft;
        ev.store(nw, tid, nt);   // (its barrier also publishes x)
        if (fixed) bf_newton_mask(nw, d, fixed, tid, nt);
        res.n_iter = it + 1;
        res.last_step = ms;
        res.lam = lam;
        lam_prev = lam;
        if (lam == 0. && ms <= xtol) res.status = 0;
    }
    res.logp = f;
    return res;
}

// ---- the objective of a profile: an evaluation Ev (one with the members w and pt: BfScalarNewtonEval, PldNewtonEval) seen as ------
//   BFHIP_PROFILE_SAMPLING (0)   Ev itself, the function the maximiser climbs
//   BFHIP_PROFILE_ORIGINAL (1)   logp_orig(T(x)): Ev minus sum_i log|T'_i(x_i)|, its gradient minus d log|T'_i| / dx_i, its Hessian's
//                                diagonal minus d2 log|T'_i| / dx_i^2 -- the three vectors lj, gj, lj2 the evaluation leaves behind.
// The sum is taken by every thread in index order.  Without a transform the two are the same function and the same instructions.
// Where the decay term is on, the original objective also takes that term's true derivatives (store, below).
template <class Ev>
struct BfProfileEval {
    Ev &ev;
    int objective;
    __host__ __device__ bool shifted() const { return objective == 1 && ev.pt.tr; }
    __host__ __device__ double eval(const double *x, int tid, int nt) {
        double f = ev.eval(x, tid, nt);
        if (shifted()) {
            double logdet = 0.;
            for (int i = 0; i < ev.m.d; ++i) logdet += ev.w.lj[i];
            f -= logdet;
        }
        return f;
    }
    __host__ __device__ void store(BfNewtonWork &nw, int tid, int nt) {
        ev.store(nw, tid, nt);
        if (!shifted()) return;
        const int d = ev.m.d, DP = ev.m.DP;
        const double gam = ev.m.decay_gamma;
        if (ev.pt.dec) {
            // The sampling-space gradient carries the decay term WITHOUT the transform's Jacobian (bfhip_hess.h, top), so it is not
            // the derivative of the value, and its zero is not the value's maximum.  A profile is a statement about the value: here
            // the decay term -gamma (xo - mu_d)^T H_d (xo - mu_d) is chained through T like every other term,
            //   gradient  -2 gamma dg_i J_i,   Hessian  -gamma (H_d[j][i] + H_d[i][j]) J_i J_j - delta_ij 2 gamma dg_i T''_i    (T'' = gj J)
            // in place of -2 gamma dg_i and -gamma (H_d[j][i] J_j + H_d[i][j] J_i).
            // dg = H_d^T (xo - mu_d) is the term's gradient only for a symmetric H_d, which it is (the inverse covariance of the fit
            // points); the Hessian is written with H_d + H_d^T so that it stays symmetric bit for bit.
            for (int idx = tid; idx < bf_tri_slots(d); idx += nt) {
                int i, j;
                if (!bf_tri_pair(d, idx, i, j)) continue;   // (i >= j)
                const double hji = bf_frag_at(ev.m.Hdf, DP, j, i), hij = bf_frag_at(ev.m.Hdf, DP, i, j);
                const double Ji = ev.w.J[i], Jj = ev.w.J[j];
                const double c = -gam * (((hji + hij) * (Ji * Jj) - hji * Ji) - hij * Jj);
                if (i == j) nw.hd[i] += c - 2. * gam * (ev.w.dg[i] * (ev.w.gj[i] * Ji));
                else nw.M[(size_t)j * nw.ld + i] += c;
            }
        }
        for (int i = tid; i < d; i += nt) {
            double g = nw.gc[i] - ev.w.gj[i];
            if (ev.pt.dec) g -= 2. * gam * (ev.w.dg[i] * (ev.w.J[i] - 1.));
            nw.gc[i] = g;
        }
        BF_HESS_SYNC();
        for (int i = tid; i < d; i += nt) nw.hd[i] -= ev.w.lj2[i];   // (behind the barrier: hd_i may have been another thread's above)
        BF_HESS_SYNC();
    }
};

// ---- the scalar surrogate density as that evaluation ----
struct BfScalarNewtonEval {
    const DevModel &m;
    BfHessWork &w;
    BfHessPt pt;
    __host__ __device__ double eval(const double *x, int tid, int nt) {
        pt = bf_hess_eval(m, x, 0, w, tid, nt, 1);
        return pt.logp;
    }
    __host__ __device__ void store(BfNewtonWork &nw, int tid, int nt) { bf_newton_store(m, w, pt, nw, tid, nt); }
};

struct BfNewtonResult {
    double logp;
    int n_iter, status;
    double last_step, lam;
    BfHessPt pt;   // the evaluation at the returned point: nw.x, with H in the upper triangle of M and hd, the gradient in gc
};

__host__ __device__ inline BfNewtonResult bf_newton_max(const DevModel &m, const double *x0, int max_iter, double xtol, BfHessWork &w,
                                                        BfNewtonWork &nw, int tid, int nt) {
    BfScalarNewtonEval ev = {m, w, BfHessPt()};
    const BfNewtonStat st = bf_newton_run(ev, m.d, x0, max_iter, xtol, nw, tid, nt);
    BfNewtonResult res;
    res.logp = st.logp;
    res.n_iter = st.n_iter;
    res.status = st.status;
    res.last_step = st.last_step;
    res.lam = st.lam;
    res.pt = ev.pt;
    return res;
}
