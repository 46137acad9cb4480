// One grid line of a profile (bayesfast_amd/csrc/bfhip_profile.h: the masked Newton iteration of bfhip_hess.h in continuation)
// compiled for the host with a team of one thread, on the tables bf_pack_density builds.  TEST INFRASTRUCTURE ONLY.
// The host copy of the uploaded density (HostModel, build) is the one tests/hess_host keeps: that translation unit is included
// whole, so that there is one copy of it and the two libraries cannot drift apart.
#include "../hess_host/hess_host.cpp"
#include "bfhip_profile.h"

// as bfhip_profile_lines, on host arrays; -1 for the arguments that call refuses with BFHIP_ERR_ARG
extern "C" int bfhost_profile_lines(const bfhip_density_desc *ds, int max_iter, double xtol, int objective, int n_line, int n_val,
                                    const uint8_t *fixed, const int32_t *walk, const double *x_start, const double *values, double *x,
                                    double *logp, double *info) {
    HostModel hm;
    if (build(ds, hm)) return -1;
    const int d = ds->d, ld = d + 1;
    if ((objective != BFHIP_PROFILE_SAMPLING && objective != BFHIP_PROFILE_ORIGINAL) || n_val < 1 || n_line < 0) return -1;
    for (int l = 0; l < n_line; ++l) {
        const int wk = walk[l];
        if (wk == -1 ? n_val != 1 : (wk < 0 || wk >= d || !fixed[(size_t)l * d + wk])) return -1;
    }
    std::vector<double> M((size_t)d * ld), buf((size_t)(BF_HESS_NVEC + BF_NEWTON_NVEC) * d);
    BfHessWork w;
    BfNewtonWork nw;
    bf_hess_work_bind(w, buf.data(), d);
    bf_newton_work_bind(nw, M.data(), ld, buf.data() + (size_t)BF_HESS_NVEC * d, d);
    for (int l = 0; l < n_line; ++l) {
        BfScalarNewtonEval ev = {hm.m, w, BfHessPt()};
        BfProfileEval<BfScalarNewtonEval> pe = {ev, objective};
        const size_t row = (size_t)l * n_val;
        bf_profile_line(pe, d, n_val, max_iter, xtol, fixed + (size_t)l * d, walk[l], x_start + (size_t)l * d, values ? values + row : NULL,
                        x + row * d, logp + row, info + row * 4, nw, 0, 1);
    }
    return 0;
}

// the objective's value, gradient and Hessian diagonal at n points, as the iteration sees them (before the mask)
extern "C" int bfhost_profile_objective(const bfhip_density_desc *ds, int objective, int n, const double *x, double *f, double *grad,
                                        double *hdiag) {
    HostModel hm;
    if (build(ds, hm)) return -1;
    const int d = ds->d, ld = d + 1;
    std::vector<double> M((size_t)d * ld), buf((size_t)(BF_HESS_NVEC + BF_NEWTON_NVEC) * d);
    BfHessWork w;
    BfNewtonWork nw;
    bf_hess_work_bind(w, buf.data(), d);
    bf_newton_work_bind(nw, M.data(), ld, buf.data() + (size_t)BF_HESS_NVEC * d, d);
    for (int p = 0; p < n; ++p) {
        BfScalarNewtonEval ev = {hm.m, w, BfHessPt()};
        BfProfileEval<BfScalarNewtonEval> pe = {ev, objective};
        f[p] = pe.eval(x + (size_t)p * d, 0, 1);
        pe.store(nw, 0, 1);
        for (int i = 0; i < d; ++i) {
            grad[(size_t)p * d + i] = nw.gc[i];
            hdiag[(size_t)p * d + i] = nw.hd[i];
        }
    }
    return 0;
}
