// The per-point arithmetic of bayesfast_amd/csrc/bfhip_hess.h -- the analytic Hessian of the surrogate density and the damped Newton
// maximiser -- compiled for the host with a team of one thread (BF_HOST_EMU: no barriers), on the tables bf_pack_density builds.
// TEST INFRASTRUCTURE ONLY: it lets the CPU suite check the formulas against differences of the oracle's gradient.
// Also the host entry points of two helpers every sampler kernel shares: bfhip_constraint.h and bfhip_adapt.h (end of the file).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#define BF_HOST_EMU 1
#include "bfhip_hess.h"
#include "bfhip_adapt.h"
#include "bfhip_pack.h"

BfTune &bf_tune() {
    static BfTune t;
    return t;
}

namespace {
// the host copy of what bfhip_density_upload puts on the device
struct HostModel {
    DevModel m;
    std::vector<double> h, A2, A2t, T3;
    std::vector<int> mask2, mask3, pos2, pos3;
};

int build(const bfhip_density_desc *ds, HostModel &hm) {
    const int d = ds->d;
    if (d < 1 || d > BFHIP_MAX_DIM) return -1;
    const int DP = bf_pack_density(ds, hm.h);
    const size_t MAT = (size_t)DP * DP;
    DevModel &m = hm.m;
    memset(&m, 0, sizeof(m));
    m.d = d;
    m.DP = DP;
    m.has_transform = ds->ranges != NULL;
    m.has_su = ds->su_lo != NULL;
    m.has_quad = ds->quad != NULL;
    m.use_bound = ds->use_bound != 0;
    m.use_decay = ds->use_decay != 0;
    m.pd = hm.h.data();
    m.Sf = m.pd + (size_t)PD_N * DP;
    m.Hf = m.Sf + MAT;
    m.Hdf = m.Hf + MAT;
    m.c0 = ds->c0;
    m.alpha = ds->alpha;
    m.f_mu = ds->f_mu;
    m.decay_alpha2 = ds->decay_alpha2;
    m.decay_gamma = ds->decay_gamma;
    m.has_link = ds->link_kind == 1;
    m.link_y = ds->link_y;
    m.link_prec = ds->link_prec;
    m.link_logp0 = ds->link_logp0;
    m.has_cubic = (ds->cubic2 || ds->cubic3) ? 1 : 0;
    if (m.has_cubic) {   // compact tables over the dimensions the cubic terms touch (DevModel: A2, A2t, T3t)
        hm.pos2.assign(DP, -1);
        hm.pos3.assign(DP, -1);
        if (ds->cubic2)
            for (int i = 0; i < d; ++i) {
                bool used = false;
                for (int k = 0; k < d; ++k) used = used || ds->cubic2[(size_t)i * d + k] != 0. || ds->cubic2[(size_t)k * d + i] != 0.;
                if (used) {
                    hm.pos2[i] = (int)hm.mask2.size();
                    hm.mask2.push_back(i);
                }
            }
        if (ds->cubic3) {
            std::vector<char> used(d, 0);
            for (int j = 0; j < d; ++j)
                for (int k = j + 1; k < d; ++k)
                    for (int l = k + 1; l < d; ++l)
                        if (ds->cubic3[((size_t)j * d + k) * d + l] != 0.) used[j] = used[k] = used[l] = 1;
            for (int i = 0; i < d; ++i)
                if (used[i]) {
                    hm.pos3[i] = (int)hm.mask3.size();
                    hm.mask3.push_back(i);
                }
        }
        const int n2 = (int)hm.mask2.size(), n3 = (int)hm.mask3.size();
        hm.A2.assign((size_t)n2 * n2, 0.);
        hm.A2t.assign((size_t)n2 * n2, 0.);
        hm.T3.assign((size_t)n3 * n3 * n3, 0.);
        for (int a = 0; a < n2; ++a)
            for (int b = 0; b < n2; ++b) {
                hm.A2[(size_t)a * n2 + b] = ds->cubic2[(size_t)hm.mask2[a] * d + hm.mask2[b]];
                hm.A2t[(size_t)b * n2 + a] = hm.A2[(size_t)a * n2 + b];
            }
        for (int a = 0; a < n3; ++a)
            for (int b = a + 1; b < n3; ++b)
                for (int c = b + 1; c < n3; ++c) {
                    const double v = ds->cubic3[((size_t)hm.mask3[a] * d + hm.mask3[b]) * d + hm.mask3[c]];
                    const int p[3] = {a, b, c};
                    for (int q0 = 0; q0 < 3; ++q0)
                        for (int q1 = 0; q1 < 3; ++q1)
                            for (int q2 = 0; q2 < 3; ++q2)
                                if (q0 != q1 && q1 != q2 && q0 != q2) hm.T3[((size_t)p[q0] * n3 + p[q1]) * n3 + p[q2]] = v;
                }
        m.n2 = n2;
        m.n3 = n3;
        m.mask2 = hm.mask2.data();
        m.pos2 = hm.pos2.data();
        m.mask3 = hm.mask3.data();
        m.pos3 = hm.pos3.data();
        m.A2 = hm.A2.data();
        m.A2t = hm.A2t.data();
        m.T3t = hm.T3.data();
    }
    return 0;
}
}  // namespace

extern "C" int bfhost_logp_hess(const bfhip_density_desc *ds, int n, const double *x, int original_space, double *logp, double *grad,
                                double *hess) {
    HostModel hm;
    if (build(ds, hm)) return -1;
    const int d = ds->d;
    std::vector<double> buf((size_t)BF_HESS_NVEC * d);
    BfHessWork w;
    bf_hess_work_bind(w, buf.data(), d);
    for (int p = 0; p < n; ++p) {
        const BfHessPt pt = bf_hess_eval(hm.m, x + (size_t)p * d, original_space, w, 0, 1, 1);
        logp[p] = pt.logp;
        for (int i = 0; i < d; ++i) grad[(size_t)p * d + i] = w.g[i];
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j) hess[((size_t)p * d + i) * d + j] = bf_hess_entry(hm.m, w, pt, i, j);
    }
    return 0;
}

extern "C" int bfhost_laplace_opt(const bfhip_density_desc *ds, int max_iter, double xtol, int n_start, const double *x0, double *x,
                                  double *logp, double *hess, double *info) {
    HostModel hm;
    if (build(ds, hm)) return -1;
    const int d = ds->d, ld = d + 1;
    std::vector<double> M((size_t)d * ld), buf((size_t)(BF_HESS_NVEC + BF_NEWTON_NVEC) * d);
    BfHessWork w;
    BfNewtonWork nw;
    bf_hess_work_bind(w, buf.data(), d);
    bf_newton_work_bind(nw, M.data(), ld, buf.data() + (size_t)BF_HESS_NVEC * d, d);
    for (int s = 0; s < n_start; ++s) {
        const BfNewtonResult res = bf_newton_max(hm.m, x0 + (size_t)s * d, max_iter, xtol, w, nw, 0, 1);
        for (int i = 0; i < d; ++i) x[(size_t)s * d + i] = nw.x[i];
        logp[s] = res.logp;
        info[s * 4 + 0] = res.n_iter;
        info[s * 4 + 1] = res.status;
        info[s * 4 + 2] = res.last_step;
        info[s * 4 + 3] = res.lam;
        if (hess)
            for (int i = 0; i < d; ++i)
                for (int j = 0; j < d; ++j)
                    hess[((size_t)s * d + i) * d + j] = i == j ? nw.hd[i] : (i < j ? M[(size_t)i * ld + j] : M[(size_t)j * ld + i]);
    }
    return 0;
}

// the constraint transform's one helper (bfhip_constraint.h) at n coordinates of one kind: out[5 i ..] = T, T', log|T'|, T''/T',
// d2 log|T'| / dx2
extern "C" int bfhost_constraint(int n, const double *x, int kind, double lo, double rg, double *out) {
    for (int i = 0; i < n; ++i) {
        double xo, J, J2, lj, gj, lj2;
        bf_hess_transform(x[i], kind, lo, rg, xo, J, J2, lj, gj, lj2);
        out[5 * i + 0] = xo;
        out[5 * i + 1] = J;
        out[5 * i + 2] = lj;
        out[5 * i + 3] = gj;
        out[5 * i + 4] = lj2;
    }
    return 0;
}

// ---- the iteration end's one helper (bfhip_adapt.h), both rounding policies ----
namespace {
struct HostMath {
    static double ex(double x) { return exp(x); }
    static double lg(double x) { return log(x); }
    static double sq(double x) { return sqrt(x); }
};

template <bool FUSED>
void step_adapt(const bfhip_sampler_config &cfg, int one_call, int n, const double *accept, double smu, double *state, double *out) {
    double hbar = state[0], log_step = state[1], log_bar = state[2], count = state[3];
    for (int i = 0; i < n; ++i) {
        if (one_call) BfStepAdapt<FUSED>::step(cfg, accept[i], smu, hbar, log_step, log_bar, count, HostMath());
        else BfStepAdapt<FUSED>::update(cfg, BfStepAdapt<FUSED>::consts(cfg, count, HostMath()), accept[i], smu, hbar, log_step, log_bar, count);
        out[4 * i + 0] = hbar;
        out[4 * i + 1] = log_step;
        out[4 * i + 2] = log_bar;
        out[4 * i + 3] = count;
    }
}

template <bool FUSED>
void welford(int n, const double *x, double n0, double mean, double raw, double *out) {
    for (int i = 0; i < n; ++i) {
        n0 += 1.;
        bf_welford_add<FUSED>(x[i], n0, mean, raw);
        out[2 * i + 0] = mean;
        out[2 * i + 1] = raw;
    }
}
}  // namespace

// n successive dual-averaging updates from state = (hbar, log_step, log_bar, count): out[4 i ..] = the state after update i;
// one_call: through step(), else through consts() and update()
extern "C" int bfhost_step_adapt(int fused, int one_call, double target_accept, double gamma, double k, double t_0, int n, const double *accept,
                                 double smu, double *state, double *out) {
    bfhip_sampler_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.target_accept = target_accept;
    cfg.gamma = gamma;
    cfg.k = k;
    cfg.t_0 = t_0;
    if (fused) step_adapt<true>(cfg, one_call, n, accept, smu, state, out);
    else step_adapt<false>(cfg, one_call, n, accept, smu, state, out);
    return 0;
}

// n samples added to one element of a Welford window that starts at (n0, mean, raw): out[2 i ..] = mean, raw after sample i
extern "C" int bfhost_welford(int fused, int n, const double *x, double n0, double mean, double raw, double *out) {
    if (fused) welford<true>(n, x, n0, mean, raw, out);
    else welford<false>(n, x, n0, mean, raw, out);
    return 0;
}

// n_iter iterations of the metric's window logic from state = (fg_n, bg_n, n_samples, prev_upd, adapt_window):
// out[7 i ..] = the five scalars after iteration i, then its refresh and roll flags
extern "C" int bfhost_metric_window(int update_window, int doubling, int n_iter, const double *state, double *out) {
    bfhip_sampler_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.update_window = update_window;
    cfg.doubling = doubling;
    BfMetricWindow mw{state[0], state[1], state[2], state[3], state[4]};
    for (int i = 0; i < n_iter; ++i) {
        const long delta = mw.begin();
        const bool refresh = mw.refresh(cfg, delta), roll = mw.roll(delta);
        mw.end(cfg, roll);
        const double row[7] = {mw.fg_n, mw.bg_n, mw.n_samples, mw.prev_upd, mw.adapt_window, refresh ? 1. : 0., roll ? 1. : 0.};
        memcpy(out + 7 * i, row, sizeof(row));
    }
    return 0;
}
