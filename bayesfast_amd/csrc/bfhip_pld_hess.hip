// bfhip_pld_hess.hip -- the analytic Hessian of the uploaded pipeline density and its device-resident Newton maximiser
// (bfhip_pld_hess.h has the arithmetic and the layout of the two contractions).
//
//   bfhip_pipeline_logp_hess     a workgroup of four waves per point: pldh_eval, then the threads run over the d x d entries in
//                                row-major order (coalesced stores), each entry from its ordered index pair.
//   bfhip_pipeline_laplace_opt   a workgroup per start, the whole damped Newton iteration inside one launch: bf_newton_run
//                                (bfhip_hess.h: the scalar density's loop, Cholesky and solve) on PldNewtonEval; the matrix
//                                (d (d + 1) doubles) and the work vectors in LDS beside the evaluation's block.
// Both take a slot of the context's work buffer per workgroup (G and G^T G); the grid is capped so that the buffer stays small, and
// a workgroup walks over its points.  A point's result depends on the point and the density only.
#include <cmath>
#include "bfhip_common.h"
#include "bfhip_pld_hess.h"

#define PLDH_WORK_MAX ((size_t)256 << 20)   // the work buffer's cap: slots are dealt until it is reached

__global__ __launch_bounds__(PLDH_TH) void bf_pld_logp_hess_kernel(DevModel m, int n, const double *__restrict__ x, int original_space,
                                                                   int hess_kind, double *work, double *__restrict__ logp,
                                                                   double *__restrict__ grad, double *__restrict__ hess) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int d = m.d, tid = threadIdx.x, nt = PLDH_TH;
    PldHessWork w;
    pldh_work_bind(w, lds, work + (size_t)blockIdx.x * pldh_slot_doubles(d, m.pld.MP), m);
    pldh_work_init(w, m, tid);
    for (int p = blockIdx.x; p < n; p += gridDim.x) {
        const PldHessPt pt = pldh_eval(m, x + (size_t)p * d, original_space, hess_kind, w, tid);
        if (tid == 0 && logp) logp[p] = pt.logp;
        if (grad)
            for (int i = tid; i < d; i += nt) grad[(size_t)p * d + i] = w.g[i];
        double *hp = hess + (size_t)p * d * d;
        for (int idx = tid; idx < d * d; idx += nt) {
            const int i = idx / d, j = idx - i * d;
            hp[idx] = pldh_entry(m, w, pt, i, j);
        }
    }
}

__global__ __launch_bounds__(PLDH_TH) void bf_pld_laplace_opt_kernel(DevModel m, int n_start, int max_iter, double xtol, int hess_kind,
                                                                     double *work, const double *__restrict__ x0,
                                                                     double *__restrict__ xout, double *__restrict__ logp,
                                                                     double *__restrict__ hess, double *__restrict__ info) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int d = m.d, ld = d + 1, tid = threadIdx.x, nt = PLDH_TH;
    double *vec = lds + (size_t)d * ld;
    PldHessWork w;
    BfNewtonWork nw;
    bf_newton_work_bind(nw, lds, ld, vec, d);
    pldh_work_bind(w, vec + (size_t)BF_NEWTON_NVEC * d, work + (size_t)blockIdx.x * pldh_slot_doubles(d, m.pld.MP), m);
    pldh_work_init(w, m, tid);
    for (int s = blockIdx.x; s < n_start; s += gridDim.x) {
        PldNewtonEval ev = {m, w, hess_kind, PldHessPt()};
        const BfNewtonStat res = bf_newton_run(ev, d, x0 + (size_t)s * d, max_iter, xtol, nw, tid, nt);
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

// the checks every call on the evaluation shares (bfhip_profile.hip too), the grid and the work buffer: *grid workgroups, each with its slot
int plh_prepare(bfhip_ctx *ctx, const char *who, int hess_kind, int n, size_t lds_extra_doubles, size_t *lds_bytes, int *grid) {
    if (!ctx->has_model) return bf_set_error(BFHIP_ERR_STATE, "%s: no density uploaded", who);
    const DevModel &m = ctx->model;
    if (!m.pld.on)
        return bf_set_error(BFHIP_ERR_UNSUPPORTED, "%s takes the pipeline density (bfhip_pipeline_upload); the scalar surrogate density "
                                                   "goes through bfhip_logp_hess / bfhip_laplace_opt", who);
    if (hess_kind != BFHIP_HESS_FULL && hess_kind != BFHIP_HESS_GAUSS_NEWTON)
        return bf_set_error(BFHIP_ERR_ARG, "%s: hess_kind %d is neither BFHIP_HESS_FULL nor BFHIP_HESS_GAUSS_NEWTON", who, hess_kind);
    if (m.pld.stream)
        return bf_set_error(BFHIP_ERR_UNSUPPORTED, "%s: the streamed form of the pipeline density (%d monomials in %d chunks of %d) has no "
                                                   "analytic Hessian; difference bfhip_logp_grad instead", who, m.pld.nf, m.pld.NC, m.pld.KC);
    *lds_bytes = (pldh_lds_doubles(m.d, m.DP, m.pld.MP, m.pld.PP) + lds_extra_doubles) * sizeof(double);
    if (*lds_bytes > BF_LDS_MAX)
        return bf_set_error(BFHIP_ERR_UNSUPPORTED, "%s: %zu KB of LDS per workgroup (%d inputs, %d rows, %d monomials) exceed %zu KB", who,
                            (*lds_bytes + 1023) / 1024, m.d, m.pld.m, m.pld.nf, BF_LDS_MAX / 1024);
    const size_t slot = pldh_slot_doubles(m.d, m.pld.MP) * sizeof(double);
    if (slot > PLDH_WORK_MAX)
        return bf_set_error(BFHIP_ERR_UNSUPPORTED, "%s: %zu KB of work buffer per workgroup exceed %zu KB", who, slot / 1024, PLDH_WORK_MAX / 1024);
    size_t g = (size_t)2 * ctx->n_cu;
    if (g > PLDH_WORK_MAX / slot) g = PLDH_WORK_MAX / slot;
    if (g > (size_t)n) g = (size_t)n;
    *grid = (int)g;
    return bf_grow(ctx, &ctx->hess_work, &ctx->hess_work_bytes, g * slot);
}

extern "C" int bfhip_pipeline_logp_hess(bfhip_ctx *ctx, int n, const double *x, int original_space, int hess_kind, double *logp,
                                        double *grad, double *hess) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 0 || (n > 0 && (!x || !hess))) return bf_set_error(BFHIP_ERR_ARG, "bfhip_pipeline_logp_hess: invalid argument");
    size_t lds = 0;
    int grid = 0;
    if (int rc = plh_prepare(ctx, "bfhip_pipeline_logp_hess", hess_kind, n, 0, &lds, &grid)) return rc;
    if (n == 0) return 0;
    if (int rc = bf_set_lds(bf_pld_logp_hess_kernel, lds)) return rc;
    hipLaunchKernelGGL(bf_pld_logp_hess_kernel, dim3(grid), dim3(PLDH_TH), lds, ctx->stream, ctx->model, n, x, original_space, hess_kind,
                       (double *)ctx->hess_work, logp, grad, hess);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int bfhip_pipeline_laplace_opt(bfhip_ctx *ctx, const bfhip_laplace_opts *opts, int hess_kind, int n_start, const double *x0,
                                          double *x, double *logp, double *hess, double *info) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || !opts || n_start < 0 || (n_start > 0 && (!x0 || !x || !logp || !info)) || opts->max_iter < 0 || !(opts->xtol >= 0.))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_pipeline_laplace_opt: invalid argument");
    size_t lds = 0;
    int grid = 0;
    const int d = ctx->has_model ? ctx->model.d : 0;
    if (int rc = plh_prepare(ctx, "bfhip_pipeline_laplace_opt", hess_kind, n_start, (size_t)d * (d + 1) + (size_t)BF_NEWTON_NVEC * d, &lds, &grid))
        return rc;
    if (n_start == 0) return 0;
    if (int rc = bf_set_lds(bf_pld_laplace_opt_kernel, lds)) return rc;
    hipLaunchKernelGGL(bf_pld_laplace_opt_kernel, dim3(grid), dim3(PLDH_TH), lds, ctx->stream, ctx->model, n_start, opts->max_iter, opts->xtol,
                       hess_kind, (double *)ctx->hess_work, x0, x, logp, hess, info);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
