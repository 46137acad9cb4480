// bfhip_laplace.hip -- the analytic Hessian of the uploaded surrogate density and the device-resident Newton maximiser of the
// OptimizeStep's Laplace approximation (utils/laplace.py:131-183, which differences the gradient and optimises one point per call).
//
//   bfhip_logp_hess     a workgroup per point, a thread per matrix row: bf_hess_eval (bfhip_hess.h) with its work vectors in LDS,
//                       then the threads run over the d x d entries in row-major order (coalesced 8-byte stores).  The output is 8 n d^2 bytes, but the stores are not what bounds the kernel:
//                       the per-point evaluation in front of them is (DESIGN.md section 4.5 has the measurement).  Each entry is
//                       computed from its ordered index pair, so the result is symmetric bit for bit.
//   bfhip_laplace_opt   a workgroup per start, the whole damped Newton iteration inside one launch (bf_newton_max): the matrix
//                       (d (d + 1) doubles, 129 KiB at d = 128) and 23 vectors of d in LDS.  A start's result depends on its x0
//                       row and the density only: no atomics, no cross-workgroup state, every sum in index order.
#include <cmath>
#include "bfhip_common.h"
#include "bfhip_hess.h"

#define LP_TH 256

__global__ __launch_bounds__(LP_TH) void bf_logp_hess_kernel(DevModel m, int n, const double *__restrict__ x, int original_space,
                                                            double *__restrict__ logp, double *__restrict__ grad,
                                                            double *__restrict__ hess) {
    extern __shared__ double lds[];
    const int d = m.d, tid = threadIdx.x, nt = blockDim.x;
    BfHessWork w;
    bf_hess_work_bind(w, lds, d);
    for (int p = blockIdx.x; p < n; p += gridDim.x) {
        const BfHessPt pt = bf_hess_eval(m, x + (size_t)p * d, original_space, w, tid, nt, 1);
        if (tid == 0 && logp) logp[p] = pt.logp;
        if (grad)
            for (int i = tid; i < d; i += nt) grad[(size_t)p * d + i] = w.g[i];
        double *hp = hess + (size_t)p * d * d;
        for (int idx = tid; idx < d * d; idx += nt) {
            const int i = idx / d, j = idx - i * d;
            hp[idx] = bf_hess_entry(m, w, pt, i, j);
        }
    }
}

__global__ __launch_bounds__(LP_TH) void bf_laplace_opt_kernel(DevModel m, int n_start, int max_iter, double xtol,
                                                              const double *__restrict__ x0, double *__restrict__ xout,
                                                              double *__restrict__ logp, double *__restrict__ hess,
                                                              double *__restrict__ info) {
    extern __shared__ double lds[];
    const int d = m.d, ld = d + 1, tid = threadIdx.x, nt = blockDim.x;   // (odd or even, ld = d + 1 keeps a column off a single bank)
    double *vec = lds + (size_t)d * ld;
    BfHessWork w;
    BfNewtonWork nw;
    bf_hess_work_bind(w, vec, d);
    bf_newton_work_bind(nw, lds, ld, vec + (size_t)BF_HESS_NVEC * d, d);
    for (int s = blockIdx.x; s < n_start; s += gridDim.x) {
        const BfNewtonResult res = bf_newton_max(m, x0 + (size_t)s * d, max_iter, xtol, w, nw, tid, nt);
        for (int i = tid; i < d; i += nt) xout[(size_t)s * d + i] = nw.x[i];
        if (tid == 0) {
            logp[s] = res.logp;
            info[(size_t)s * 4 + 0] = (double)res.n_iter;
            info[(size_t)s * 4 + 1] = (double)res.status;
            info[(size_t)s * 4 + 2] = res.last_step;
            info[(size_t)s * 4 + 3] = res.lam;
        }
        if (hess) {
            double *hp = hess + (size_t)s * d * d;
            for (int idx = tid; idx < d * d; idx += nt) {
                const int i = idx / d, j = idx - i * d;
                hp[idx] = i == j ? nw.hd[i] : (i < j ? nw.M[(size_t)i * ld + j] : nw.M[(size_t)j * ld + i]);
            }
        }
        __syncthreads();   // the next start overwrites M and the vectors
    }
}

static int lp_check(bfhip_ctx *ctx, const char *who) {
    if (!ctx->has_model) return bf_set_error(BFHIP_ERR_STATE, "%s: no density uploaded", who);
    if (ctx->model.pld.on)
        return bf_set_error(BFHIP_ERR_UNSUPPORTED, "%s: this call covers the scalar surrogate density, not the pipeline density "
                                                   "(multi-output surrogate + Gaussian likelihood): use bfhip_pipeline_logp_hess / "
                                                   "bfhip_pipeline_laplace_opt", who);
    return 0;
}

extern "C" int bfhip_logp_hess(bfhip_ctx *ctx, int n, const double *x, int original_space, double *logp, double *grad, double *hess) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 0 || (n > 0 && (!x || !hess))) return bf_set_error(BFHIP_ERR_ARG, "bfhip_logp_hess: invalid argument");
    if (int rc = lp_check(ctx, "bfhip_logp_hess")) return rc;
    if (n == 0) return 0;
    const int d = ctx->model.d;
    const size_t lds = (size_t)BF_HESS_NVEC * d * sizeof(double);
    // one thread per row of the matrix-vector products (the evaluation's critical path): more workgroups in flight, none of their waves idle
    const int th = d <= 64 ? 64 : 128;
    hipLaunchKernelGGL(bf_logp_hess_kernel, dim3(n), dim3(th), lds, ctx->stream, ctx->model, n, x, original_space, logp, grad, hess);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int bfhip_laplace_opt(bfhip_ctx *ctx, const bfhip_laplace_opts *opts, int n_start, const double *x0, double *x, double *logp,
                                 double *hess, double *info) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || !opts || n_start < 0 || (n_start > 0 && (!x0 || !x || !logp || !info)) || opts->max_iter < 0 || !(opts->xtol >= 0.))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_laplace_opt: invalid argument");
    if (int rc = lp_check(ctx, "bfhip_laplace_opt")) return rc;
    if (n_start == 0) return 0;
    const int d = ctx->model.d;
    const size_t lds = ((size_t)d * (d + 1) + (size_t)(BF_HESS_NVEC + BF_NEWTON_NVEC) * d) * sizeof(double);
    if (lds > BF_LDS_MAX) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_laplace_opt: %zu KB of LDS", lds / 1024);
    if (int rc = bf_set_lds(bf_laplace_opt_kernel, lds)) return rc;
    const int th = d >= 32 ? LP_TH : 64;
    hipLaunchKernelGGL(bf_laplace_opt_kernel, dim3(n_start), dim3(th), lds, ctx->stream, ctx->model, n_start, opts->max_iter, opts->xtol,
                       x0, x, logp, hess, info);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
