// bfhip_pld_hess.h -- value, gradient and Hessian of the uploaded PIPELINE density (bfhip_pld.h: multi-output surrogate, Gaussian
// likelihood, optional prior) at ONE point, for a workgroup of PLDH_TH threads.
//
// The function is the one bfhip_logp_grad returns for a pipeline density (bf_pld_logp_grad_kernel, bfhip_pld.hip); the Hessian is the
// symmetrised Jacobian of that gradient, closed form in every term.  Notation as in bfhip_hess.h, per output where that header has
// one polynomial:
//
//   xs_i = (T_i(x_i) - su_lo_i) / su_diff_i,  a_i = dxs_i/dx_i,  b_i = d2xs_i/dx_i^2,  J_i = T'_i,  J2_i = T''_i
//   phi(xs) the nf monomials, Dphi (nf x d) their derivatives, C' (MP x nf) the whitened (and compressed) coefficients
//   L(xs) = logp0 - |r|^2 / 2 the likelihood, r the residual, W = C'^T r
//
//   inside the bound:   r = C' phi - y',  Jm = C' Dphi,   grad_xs L = -Jm^T r
//       H_L = -Jm^T Jm - sum_o r_o d2 f_o = -Jm^T Jm - sum_p W_p d2 phi_p                  (d2 phi_p: at most three index pairs)
//
//   outside (beta > alpha; xm = xs - mu, h = H xm, beta^2 = xm.h, x0 = mu + (alpha/beta) xm; f0 = C' phi, J0 = C' Dphi at x0):
//       every output o is extrapolated as the scalar surrogate is:  f_o = (beta f0_o - (beta - alpha) f_mu'_o) / alpha,
//           grad f_o = J0_o + c_o h / beta,          c_o = (f0_o - f_mu'_o) / alpha - (J0 xm)_o / beta,
//           d2 f_o = (alpha/beta) [F_o - (u_o h^T + h u_o^T)/beta^2 + q_o h h^T/beta^4] + (c_o/beta) [sym(H) - h h^T/beta^2]
//       with F_o the Hessian of output o's polynomial at x0, u_o = F_o xm, q_o = xm.u_o.  Summed with the weights r_o = f_o - y'_o:
//           G = J0 + c h^T / beta                    (the Jacobian of the extrapolated outputs)
//           F_r = sum_o r_o F_o = sum_p W_p d2 phi_p(x0),   u_r = F_r xm,   q_r = xm.u_r
//           H_L = -G^T G - (alpha/beta) [F_r - (u_r h^T + h u_r^T)/beta^2 + q_r h h^T/beta^4] - (c.r/beta) [sym(H) - h h^T/beta^2]
//           grad_xs L = -G^T r = -(J0^T r + (c.r) h / beta),      J0^T r = Dphi^T W
//
//   compressed outputs (m > nf; C' = Q [R; 0], the device holds R and the heads of Q^T y', Q^T f_mu'): in the rotated output space the
//   tail rows of f0 and J0 are zero, those of f_mu' and y' are not.  Outside the bound, with bb = (beta - alpha) / alpha:
//       c_tail = -f_mu'_tail / alpha,                r_tail = -bb f_mu'_tail - y'_tail
//       c.c  += k_ff / alpha^2           so   G^T G += (k_ff / alpha^2) h h^T / beta^2           (G_tail = c_tail h^T / beta)
//       c.r  += (bb k_ff + k_fy) / alpha                                                        (as the gradient kernel adds it)
//       r.r  += bb (bb k_ff + 2 k_fy)    (|y'_tail|^2 is in logp0)
//   W and F_r see the head rows only (the tail rows of C' are zero).  Inside the bound the tails are constants.
//
//   the chain, the decay term and the transform exactly as bf_hess_entry (bfhip_hess.h), gp = grad_xs L:
//       H_ij = a_i H_L,ij a_j + delta_ij gp_i b_i - [decay on] gamma (H_d[j][i] J_j + H_d[i][j] J_i) + delta_ij d2/dx_i^2 log|T'_i|
//   prior (diagonal, original space):                - delta_ij prec_i (J_i^2 + (xo_i - mu_i) J2_i)
//
//   hess_kind = BFHIP_HESS_GAUSS_NEWTON keeps what carries no residual: -a_i (G^T G)_ij a_j, the prior's -prec_i J_i^2, the decay
//   term and the transform's log-Jacobian term.  Dropped: F_r, u_r, q_r, the c.r term (sum_o r_o times the extrapolation's own
//   curvature; c.r contains xm.Dphi^T W), gp_i b_i and the prior's (xo_i - mu_i) J2_i.  The likelihood part, -a G^T G a, is negative
//   semi-definite by construction.
//
// On the surfaces beta = alpha and beta_d^2 = alpha_2 the Hessian takes the gradient's branch.
//
// The two dense contractions run on v_mfma_f64_16x16x4 with the COORDINATES as the sixteen columns:
//   GEMM1  [F0 | J0 xm | J0] (MP x (d + 2)) = C' [phi | Dphi xm | dphi/dx_1 .. dphi/dx_d], in column tiles of 16.  A = the CF fragments
//          of the upload; the B tile (PP x 16, PLD_XS layout) is built sparsely in LDS from the monomial table (a monomial has at most
//          three non-zero derivatives).  Tile 0 carries F0 and J0 xm, from which its epilogue takes c and r per row (a lane fetches
//          its row's two values from the lanes of columns 0 and 1); every tile's epilogue adds c h^T / beta and stores G.
//   GEMM2  G^T G (d x d, K = MP), the upper 16 x 16 tiles.  A and B are both read from G, row-major [MP][DG], DG = d rounded up to 16:
//          lane l of k-step s reads G[4 s + (l >> 4)][16 t + (l & 15)] for either operand.
// G (MP x DG doubles: 256 KB at 500 x 64) does not fit LDS beside the rest, so it and the Gram matrix live in a per-workgroup slot of
// a work buffer in global memory (bfhip_ctx::hess_work); at these sizes it stays in L2.  A workgroup reads back only what it wrote
// itself, behind a barrier.  W = C'^T r is one matrix-vector pass over CTF; sum_p W_p d2 phi_p is a gather per ordered pair from the
// CSR table of the upload (PldDev::h2ptr, h2ent), in increasing monomial index.
//
// Invariants: no atomics; every sum in a fixed order; entry (i, j) computed from the ordered pair (and from the upper tiles of
// G^T G only), so H == H^T bit for bit; a point's result depends on the point and the density only.
#pragma once
#include "bfhip_hess.h"
#include "bfhip_pld.h"

#define PLDH_TH 256     // threads of the workgroup (four waves)
#define PLDH_NVEC 17    // work vectors of d doubles (PldHessWork)

struct PldHessWork {
    double *xo, *xs, *a, *b, *J, *J2, *lj, *lj2, *gj;   // as BfHessWork; J2 = T''
    double *xm, *h, *hb, *dg, *u, *gn, *gp, *g;         // xs - mu, H xm, h / beta, decay H_d^T xd, F_r xm, J0^T r, grad_xs L, the gradient
    double *xe;    // [DP + 2]  the point the polynomials are taken at (x0 outside the bound), then 1 and 0
    double *W;     // [PP]      C'^T r
    double *CV;    // [MP]      c
    double *RV;    // [MP]      r
    double *FD;    // [MP]      f0 - f_mu'
    double *B;     // [PP / 4][PLD_XS]  one column tile of the B operand of GEMM1
    double *G;     // global: [MP][DG]
    double *HG;    // global: [DG][DG]  G^T G, upper tiles
    int DG;
};

__host__ __device__ inline int pldh_dg(int d) { return (d + 15) / 16 * 16; }
__host__ __device__ inline size_t pldh_lds_doubles(int d, int DP, int MP, int PP) {
    return (size_t)PLDH_NVEC * d + (DP + 2) + PP + (size_t)3 * MP + (size_t)(PP / 4) * PLD_XS;
}
__host__ __device__ inline size_t pldh_slot_doubles(int d, int MP) { return (size_t)(MP + pldh_dg(d)) * pldh_dg(d); }

#ifndef BF_HOST_EMU
__device__ inline void pldh_work_bind(PldHessWork &w, double *lds, double *slot, const DevModel &m) {
    const int d = m.d;
    double **p[PLDH_NVEC] = {&w.xo, &w.xs, &w.a, &w.b, &w.J, &w.J2, &w.lj, &w.lj2, &w.gj, &w.xm, &w.h, &w.hb, &w.dg, &w.u, &w.gn, &w.gp, &w.g};
    for (int i = 0; i < PLDH_NVEC; ++i) *p[i] = lds + (size_t)i * d;
    w.xe = lds + (size_t)PLDH_NVEC * d;
    w.W = w.xe + (m.DP + 2);
    w.CV = w.W + m.pld.PP;
    w.RV = w.CV + m.pld.MP;
    w.FD = w.RV + m.pld.MP;
    w.B = w.FD + m.pld.MP;
    w.DG = pldh_dg(d);
    w.G = slot;
    w.HG = slot + (size_t)m.pld.MP * w.DG;
}

// once per launch, all threads: the columns of G between d and DG are zero (GEMM1 never writes them, GEMM2 reads whole tiles)
__device__ inline void pldh_work_init(const PldHessWork &w, const DevModel &m, int tid) {
    const int pad = w.DG - m.d;
    for (int i = tid; i < m.pld.MP * pad; i += PLDH_TH) w.G[(size_t)(i / pad) * w.DG + m.d + i % pad] = 0.;
}

// the scalars of one evaluation (every thread holds its own, identical copy)
struct PldHessPt {
    double logp;
    int oob, dec, tr, full;
    double ab, cb, ib2, q, tailc;   // alpha/beta, (c.r)/beta, 1/beta^2, xm.F_r xm, k_ff / alpha^2
};

// one 16 x 16 tile of G^T G: rows 16 ti .., columns 16 tj .., over n_steps k-steps (a multiple of 4); both operands from G
__device__ inline d4_t pldh_gram_tile(const double *G, int DG, int ti, int tj, int n_steps, int lane) {
    d4_t acc = {0., 0., 0., 0.};
    const double *ap = G + (size_t)(lane >> 4) * DG + 16 * ti + (lane & 15);
    const double *bp = G + (size_t)(lane >> 4) * DG + 16 * tj + (lane & 15);
    const size_t st = (size_t)4 * DG;
    double a0[4], b0[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) { a0[q] = ap[q * st]; b0[q] = bp[q * st]; }
    for (int s = 4; s < n_steps; s += 4) {
        double a1[4], b1[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { a1[q] = ap[(s + q) * st]; b1[q] = bp[(s + q) * st]; }
#pragma unroll
        for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[q], b0[q], acc, 0, 0, 0);
#pragma unroll
        for (int q = 0; q < 4; ++q) { a0[q] = a1[q]; b0[q] = b1[q]; }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[q], b0[q], acc, 0, 0, 0);
    return acc;
}

// entry (i, j), i <= j, of F_r = sum_p W_p d2 phi_p at w.xe, in increasing p
__device__ inline double pldh_second(const PldDev &pl, const PldHessWork &w, int d, int i, int j) {
    const int pi = i * (2 * d - i + 1) / 2 + (j - i);
    double s = 0.;
    for (int e = pl.h2ptr[pi]; e < pl.h2ptr[pi + 1]; ++e) {
        const unsigned long long en = pl.h2ent[e];
        const unsigned hi = (unsigned)(en >> 32);
        s += ((double)((hi >> 8) & 255u) * w.W[(unsigned)en]) * w.xe[hi & 255u];
    }
    return s;
}

// Value and gradient at x (d doubles, any address space), G^T G in w.HG and every vector pldh_entry needs.  All PLDH_TH threads call
// it; on return (after its last barrier) w.g holds the gradient and the returned scalars are the same in every thread.
__device__ inline PldHessPt pldh_eval(const DevModel &m, const double *x, int original_space, int hess_kind, PldHessWork &w, int tid) {
    const PldDev &pl = m.pld;
    const int d = m.d, DP = m.DP, nt = PLDH_TH, lane = tid & 63, wv = tid >> 6, nwv = PLDH_TH / 64;
    const int MP = pl.MP, PP = pl.PP, DG = w.DG;
    const double *pd = m.pd;
    PldHessPt r;
    r.tr = m.has_transform && !original_space;
    r.full = hess_kind == BFHIP_HESS_FULL;
    r.oob = 0;
    r.dec = 0;
    r.ab = r.cb = r.ib2 = r.q = r.tailc = 0.;
    __syncthreads();   // the previous evaluation's readers are done
    for (int i = tid; i < d; i += nt) {
        double xo = x[i], J = 1., J2 = 0., lj = 0., gj = 0., lj2 = 0.;
        if (r.tr) bf_hess_transform(x[i], (int)pd[PD_KIND * DP + i], pd[PD_LO * DP + i], pd[PD_RG * DP + i], xo, J, J2, lj, gj, lj2);
        const double diff = m.has_su ? pd[PD_SU_DIFF * DP + i] : 1.;
        const double xs = m.has_su ? (xo - pd[PD_SU_LO * DP + i]) / diff : xo;
        w.xo[i] = xo;
        w.xs[i] = xs;
        w.J[i] = J;
        w.J2[i] = J2;
        w.a[i] = J / diff;
        w.b[i] = J2 / diff;
        w.lj[i] = lj;
        w.lj2[i] = lj2;
        w.gj[i] = gj;
        w.xm[i] = m.use_bound ? xs - pd[PD_MU * DP + i] : 0.;
    }
    __syncthreads();
    for (int i = tid; i < d; i += nt) {
        w.h[i] = m.use_bound ? bf_frag_row_dot(m.Hf, DP, i, w.xs, pd + PD_MU * DP, d) : 0.;
        w.dg[i] = m.use_decay ? bf_frag_row_dot(m.Hdf, DP, i, w.xo, pd + PD_DMU * DP, d) : 0.;
    }
    __syncthreads();
    double b2 = 0., bd2 = 0., logdet = 0., pr = 0.;
    for (int i = 0; i < d; ++i) {
        b2 += w.xm[i] * w.h[i];
        if (m.use_decay) bd2 += (w.xo[i] - pd[PD_DMU * DP + i]) * w.dg[i];
        logdet += w.lj[i];
        if (pl.has_prior) {
            const double dx = w.xo[i] - pl.prior_mu[i];
            pr += pl.prior_prec[i] * dx * dx;
        }
    }
    const double alpha = m.alpha, beta = m.use_bound ? sqrt(b2) : 0.;
    r.oob = m.use_bound && beta > alpha;
    for (int i = tid; i < DP + 2; i += nt) {
        double v = i == DP ? 1. : 0.;
        if (i < d) v = r.oob ? (alpha * w.xs[i] + (beta - alpha) * pd[PD_MU * DP + i]) / beta : w.xs[i];
        w.xe[i] = v;
        if (i < d) w.hb[i] = r.oob ? w.h[i] / beta : 0.;
    }
    __syncthreads();

    // ---- GEMM1, column tile by column tile: columns 0 = phi, 1 = Dphi xm, 2 + v = dphi / dx_v ----
    const int n_ct = (d + 2 + 15) / 16, n_b = pl.NS1 * PLD_XS;
    for (int ct = 0; ct < n_ct; ++ct) {
        for (int i = tid; i < n_b; i += nt) w.B[i] = 0.;
        __syncthreads();
        for (int p = tid; p < PP; p += nt) {
            const unsigned mo = pl.mono[p];
            const int ix[3] = {(int)(mo & 255u), (int)((mo >> 8) & 255u), (int)((mo >> 16) & 255u)};
            const double xv[3] = {w.xe[ix[0]], w.xe[ix[1]], w.xe[ix[2]]};
            const double term[3] = {xv[1] * xv[2], xv[0] * xv[2], xv[0] * xv[1]};   // the product without factor q
            double *bp = w.B + (p >> 2) * PLD_XS + 16 * (p & 3);
            double dxm = 0.;
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                const int v = ix[q];
                bool first = v < d;
                for (int q2 = 0; q2 < q; ++q2) first = first && ix[q2] != v;
                if (!first) continue;
                double val = term[q];   // the product rule over the positions that hold x_v
                for (int q2 = q + 1; q2 < 3; ++q2)
                    if (ix[q2] == v) val += term[q2];
                dxm += val * w.xm[v];
                const int cg = 2 + v;
                if ((cg >> 4) == ct) bp[cg & 15] = val;
            }
            if (ct == 0) {
                bp[0] = (xv[0] * xv[1]) * xv[2];
                bp[1] = dxm;
            }
        }
        __syncthreads();
        for (int t = wv; t < pl.NT1; t += nwv) {
            const d4_t acc = pld_tile(pl.CF + (size_t)t * pl.NS1 * 64, w.B, pl.NS1, lane);
            const int col = lane & 15, j = 16 * ct + col - 2;
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const int row = 16 * t + 4 * r4 + (lane >> 4);
                double cv;
                if (ct == 0) {   // (uniform over the workgroup)
                    const double f0 = __shfl(acc[r4], lane & 48, 64), jx = __shfl(acc[r4], (lane & 48) | 1, 64);
                    const double fmu = pl.fmuw[row], y = pl.yw[row];
                    cv = r.oob ? (f0 - fmu) / alpha - jx / beta : 0.;
                    const double fv = r.oob ? (beta * f0 - (beta - alpha) * fmu) / alpha : f0;   // modules/poly.py:487
                    if (col == 0) {
                        w.CV[row] = cv;
                        w.RV[row] = fv - y;
                        w.FD[row] = f0 - fmu;
                    }
                } else {
                    cv = w.CV[row];
                }
                if (j >= 0 && j < d) w.G[(size_t)row * DG + j] = r.oob ? acc[r4] + cv * w.hb[j] : acc[r4];
            }
        }
        __syncthreads();   // the tile is consumed; c and r are visible
    }

    // ---- GEMM2: the upper tiles of G^T G (the columns of G at or beyond d are zero: pldh_work_init) ----
    const int n_dt = DG / 16;
    for (int job = wv; job < n_dt * n_dt; job += nwv) {
        const int ti = job / n_dt, tj = job - ti * n_dt;
        if (ti > tj) continue;
        const d4_t acc = pldh_gram_tile(w.G, DG, ti, tj, pl.NS2, lane);
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) w.HG[(size_t)(16 * ti + 4 * r4 + (lane >> 4)) * DG + 16 * tj + (lane & 15)] = acc[r4];
    }
    // ---- W = C'^T r: CTF[(u NS2 + s) 64 + l] = C'[4 s + (l >> 4)][16 u + (l & 15)] ----
    for (int p = tid; p < PP; p += nt) {
        const double *cp = pl.CTF + (size_t)(p >> 4) * pl.NS2 * 64 + (p & 15);
        double acc = 0.;
        for (int o = 0; o < MP; ++o) acc += cp[(o >> 2) * 64 + ((o & 3) << 4)] * w.RV[o];
        w.W[p] = acc;
    }
    double s_rr = 0., s_fr = 0.;
    for (int o = 0; o < MP; ++o) {
        s_rr += w.RV[o] * w.RV[o];
        s_fr += w.FD[o] * w.RV[o];
    }
    __syncthreads();
    for (int j = tid; j < d; j += nt) {   // (J0^T r)_j: the monomials that contain x_j, each times its cofactor (pld_grad)
        double g = 0.;
        for (int i = 0; i < pl.n_ent; ++i) {
            const unsigned long long en = pl.gtab[(size_t)i * DP + j];
            const unsigned eh = (unsigned)(en >> 32);
            g += ((double)((eh >> 16) & 255u) * w.W[(unsigned)en]) * (w.xe[eh & 255u] * w.xe[(eh >> 8) & 255u]);
        }
        w.gn[j] = g;
        double uv = 0.;
        if (r.oob && r.full)
            for (int k = 0; k < d; ++k) uv += pldh_second(pl, w, d, j < k ? j : k, j < k ? k : j) * w.xm[k];
        w.u[j] = uv;
    }
    __syncthreads();
    double crd = 0.;
    if (r.oob) {
        const double bb = (beta - alpha) / alpha;
        s_rr += bb * (bb * pl.k_ff + 2. * pl.k_fy);
        s_fr += bb * pl.k_ff + pl.k_fy;
        double dj = 0., q = 0.;
        for (int i = 0; i < d; ++i) {
            dj += w.gn[i] * w.xm[i];
            q += w.xm[i] * w.u[i];
        }
        crd = s_fr / alpha - dj / beta;   // c.r
        r.ab = alpha / beta;
        r.cb = crd / beta;
        r.ib2 = 1. / b2;
        r.q = q;
        r.tailc = pl.k_ff / (alpha * alpha);
    }
    double f = pl.logp0 - 0.5 * s_rr;
    if (pl.has_prior) f += pl.prior_c0 - 0.5 * pr;
    if (m.use_decay) {
        const double ex = bd2 - m.decay_alpha2;
        f -= m.decay_gamma * (ex > 0. ? ex : (ex != ex ? ex : 0.));   // np.clip keeps NaN
        r.dec = bd2 > m.decay_alpha2;
    }
    if (r.tr) f += logdet;
    for (int i = tid; i < d; i += nt) {
        const double gp = -(r.oob ? w.gn[i] + crd * w.hb[i] : w.gn[i]);
        w.gp[i] = gp;
        double gv = gp * w.a[i];
        if (pl.has_prior) gv += -(pl.prior_prec[i] * (w.xo[i] - pl.prior_mu[i])) * w.J[i];
        if (r.dec) gv -= 2. * m.decay_gamma * w.dg[i];
        w.g[i] = gv + w.gj[i];
    }
    r.logp = f;
    __syncthreads();
    return r;
}

// entry (i, j) of the Hessian of logp at the point of the last pldh_eval.  Computed from the ordered pair (min, max), so that
// entry(i, j) == entry(j, i) bit for bit whichever thread takes which.
__device__ inline double pldh_entry(const DevModel &m, const PldHessWork &w, const PldHessPt &r, int i, int j) {
    if (i > j) {
        const int t = i;
        i = j;
        j = t;
    }
    const PldDev &pl = m.pld;
    const int DP = m.DP;
    double Hp = -w.HG[(size_t)i * w.DG + j];
    if (r.oob) Hp -= r.tailc * (w.hb[i] * w.hb[j]);
    if (r.full) {
        const double Fr = pldh_second(pl, w, m.d, i, j);
        if (r.oob) {
            const double hh = w.h[i] * w.h[j] * r.ib2;
            const double Hs = 0.5 * (bf_frag_at(m.Hf, DP, i, j) + bf_frag_at(m.Hf, DP, j, i));
            Hp -= r.ab * ((Fr - (w.u[i] * w.h[j] + w.h[i] * w.u[j]) * r.ib2) + r.q * r.ib2 * hh) + r.cb * (Hs - hh);
        } else {
            Hp -= Fr;
        }
    }
    double v = (w.a[i] * w.a[j]) * Hp;
    if (r.dec) v -= m.decay_gamma * (bf_frag_at(m.Hdf, DP, i, j) * w.J[j] + bf_frag_at(m.Hdf, DP, j, i) * w.J[i]);
    if (i == j) {
        if (r.full) v += w.gp[i] * w.b[i];
        v += w.lj2[i];
        if (pl.has_prior) {
            double c = w.J[i] * w.J[i];
            if (r.full) c += (w.xo[i] - pl.prior_mu[i]) * w.J2[i];
            v -= pl.prior_prec[i] * c;
        }
    }
    return v;
}

// the pipeline density as the evaluation of bf_newton_run (bfhip_hess.h), in the sampling space
struct PldNewtonEval {
    const DevModel &m;
    PldHessWork &w;
    int hess_kind;
    PldHessPt pt;
    __device__ double eval(const double *x, int tid, int nt) {
        (void)nt;
        pt = pldh_eval(m, x, 0, hess_kind, w, tid);
        return pt.logp;
    }
    __device__ void store(BfNewtonWork &nw, int tid, int nt) {
        const int d = m.d;
        for (int idx = tid; idx < bf_tri_slots(d); idx += nt) {
            int i, j;
            if (!bf_tri_pair(d, idx, i, j)) continue;   // (i >= j)
            const double v = pldh_entry(m, w, pt, j, i);
            if (i == j) nw.hd[i] = v;
            else nw.M[(size_t)j * nw.ld + i] = v;
        }
        for (int i = tid; i < d; i += nt) nw.gc[i] = w.g[i];
        __syncthreads();
    }
};

// host side (bfhip_pld_hess.hip): the refusals, the LDS need (pldh_lds_doubles + lds_extra_doubles), the grid and the work buffer of
// a launch of n points on this evaluation
struct bfhip_ctx;
int plh_prepare(bfhip_ctx *ctx, const char *who, int hess_kind, int n, size_t lds_extra_doubles, size_t *lds_bytes, int *grid);
#endif  // BF_HOST_EMU
