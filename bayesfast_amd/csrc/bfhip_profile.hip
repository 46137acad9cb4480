// bfhip_profile.hip -- profiles of the uploaded density along grid lines: at every value of one coordinate the maximum over the
// coordinates that are not held fixed (bfhip_profile.h has a line's rules, bfhip_hess.h the masked Newton iteration and the
// objective).
//
//   bfhip_profile_lines            the scalar surrogate density: a workgroup per line, the LDS layout of bfhip_laplace_opt
//   bfhip_pipeline_profile_lines   the pipeline density: the work-buffer slots, the LDS layout, the capped grid and the refusals of
//                                  bfhip_pipeline_laplace_opt; a workgroup walks over its lines
// A line's result depends on its own rows and the density only: no atomics, no cross-workgroup state, every sum in index order.  With
// an all-zero mask, walk = -1 and the sampling objective a line is the maximiser's start, bit for bit.
#include <cmath>
#include <vector>
#include "bfhip_common.h"
#include "bfhip_profile.h"
#include "bfhip_pld_hess.h"

#define PF_TH 256

struct PfLines {
    int n_line, n_val, max_iter, objective;
    double xtol;
    const uint8_t *fixed;     // (n_line, d)
    const int32_t *walk;      // (n_line)
    const double *x_start;    // (n_line, d)
    const double *values;     // (n_line, n_val)
    double *x, *logp, *info;  // (n_line, n_val, d), (n_line, n_val), (n_line, n_val, 4)
};

template <class Ev>
__device__ inline void pf_line(Ev &ev, const PfLines &a, int d, int l, BfNewtonWork &nw, int tid, int nt) {
    BfProfileEval<Ev> pe = {ev, a.objective};
    const size_t row = (size_t)l * a.n_val;
    bf_profile_line(pe, d, a.n_val, a.max_iter, a.xtol, a.fixed + (size_t)l * d, (int)a.walk[l], a.x_start + (size_t)l * d,
                    a.values ? a.values + row : NULL, a.x + row * d, a.logp + row, a.info + row * 4, nw, tid, nt);
    __syncthreads();   // the next line overwrites M and the vectors
}

__global__ __launch_bounds__(PF_TH) void bf_profile_lines_kernel(DevModel m, PfLines a) {
    extern __shared__ double lds[];
    const int d = m.d, ld = d + 1, tid = threadIdx.x, nt = blockDim.x;
    double *vec = lds + (size_t)d * ld;
    BfHessWork w;
    BfNewtonWork nw;
    bf_hess_work_bind(w, vec, d);
    bf_newton_work_bind(nw, lds, ld, vec + (size_t)BF_HESS_NVEC * d, d);
    for (int l = blockIdx.x; l < a.n_line; l += gridDim.x) {
        BfScalarNewtonEval ev = {m, w, BfHessPt()};
        pf_line(ev, a, d, l, nw, tid, nt);
    }
}

__global__ __launch_bounds__(PLDH_TH) void bf_pld_profile_lines_kernel(DevModel m, PfLines a, int hess_kind, double *work) {
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int d = m.d, ld = d + 1, tid = threadIdx.x, nt = PLDH_TH;
    double *vec = lds + (size_t)d * ld;
    PldHessWork w;
    BfNewtonWork nw;
    bf_newton_work_bind(nw, lds, ld, vec, d);
    pldh_work_bind(w, vec + (size_t)BF_NEWTON_NVEC * d, work + (size_t)blockIdx.x * pldh_slot_doubles(d, m.pld.MP), m);
    pldh_work_init(w, m, tid);
    for (int l = blockIdx.x; l < a.n_line; l += gridDim.x) {
        PldNewtonEval ev = {m, w, hess_kind, PldHessPt()};
        pf_line(ev, a, d, l, nw, tid, nt);
    }
}

// The argument checks both calls share.  The mask and the walk coordinates are read back from the device: this synchronises the stream.
static int pf_check(bfhip_ctx *ctx, const char *who, const bfhip_laplace_opts *opts, int objective, int n_line, int n_val,
                    const uint8_t *fixed, const int32_t *walk, const double *x_start, const double *values, double *x, double *logp,
                    double *info) {
    if (!ctx || !opts || n_line < 0 || n_val < 1 || (n_line > 0 && (!fixed || !walk || !x_start || !x || !logp || !info)) ||
        opts->max_iter < 0 || !(opts->xtol >= 0.))
        return bf_set_error(BFHIP_ERR_ARG, "%s: invalid argument", who);
    if (objective != BFHIP_PROFILE_SAMPLING && objective != BFHIP_PROFILE_ORIGINAL)
        return bf_set_error(BFHIP_ERR_ARG, "%s: objective %d is neither BFHIP_PROFILE_SAMPLING nor BFHIP_PROFILE_ORIGINAL", who, objective);
    if (!ctx->has_model) return bf_set_error(BFHIP_ERR_STATE, "%s: no density uploaded", who);
    if (n_line == 0) return 0;
    const int d = ctx->model.d;
    std::vector<int32_t> hw((size_t)n_line);
    std::vector<uint8_t> hf((size_t)n_line * d);
    BF_HIP_CHECK(hipMemcpyAsync(hw.data(), walk, hw.size() * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    BF_HIP_CHECK(hipMemcpyAsync(hf.data(), fixed, hf.size(), hipMemcpyDeviceToHost, ctx->stream));
    BF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    for (int l = 0; l < n_line; ++l) {
        const int wk = hw[l];
        if (wk == -1) {
            if (n_val != 1) return bf_set_error(BFHIP_ERR_ARG, "%s: line %d moves no coordinate (walk = -1), which takes n_val == 1, not %d", who, l, n_val);
            continue;
        }
        if (wk < 0 || wk >= d) return bf_set_error(BFHIP_ERR_ARG, "%s: line %d walks coordinate %d of %d", who, l, wk, d);
        if (!hf[(size_t)l * d + wk])
            return bf_set_error(BFHIP_ERR_ARG, "%s: line %d walks coordinate %d, which is not in the line's mask of fixed coordinates", who, l, wk);
        if (!values) return bf_set_error(BFHIP_ERR_ARG, "%s: line %d walks coordinate %d but values is NULL", who, l, wk);
    }
    return 0;
}

extern "C" int bfhip_profile_lines(bfhip_ctx *ctx, const bfhip_laplace_opts *opts, int objective, int n_line, int n_val,
                                   const uint8_t *fixed, const int32_t *walk, const double *x_start, const double *values, double *x,
                                   double *logp, double *info) {
    BfDeviceGuard dev_guard(ctx);
    const char *who = "bfhip_profile_lines";
    if (ctx && ctx->has_model && ctx->model.pld.on)
        return bf_set_error(BFHIP_ERR_UNSUPPORTED, "%s: this call covers the scalar surrogate density, not the pipeline density "
                                                   "(multi-output surrogate + Gaussian likelihood): use bfhip_pipeline_profile_lines", who);
    if (int rc = pf_check(ctx, who, opts, objective, n_line, n_val, fixed, walk, x_start, values, x, logp, info)) return rc;
    if (n_line == 0) return 0;
    const int d = ctx->model.d;
    const size_t lds = ((size_t)d * (d + 1) + (size_t)(BF_HESS_NVEC + BF_NEWTON_NVEC) * d) * sizeof(double);
    if (lds > BF_LDS_MAX) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "%s: %zu KB of LDS", who, lds / 1024);
    if (int rc = bf_set_lds(bf_profile_lines_kernel, lds)) return rc;
    const int th = d >= 32 ? PF_TH : 64;
    const PfLines a = {n_line, n_val, opts->max_iter, objective, opts->xtol, fixed, walk, x_start, values, x, logp, info};
    hipLaunchKernelGGL(bf_profile_lines_kernel, dim3(n_line), dim3(th), lds, ctx->stream, ctx->model, a);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int bfhip_pipeline_profile_lines(bfhip_ctx *ctx, const bfhip_laplace_opts *opts, int hess_kind, int objective, int n_line,
                                            int n_val, const uint8_t *fixed, const int32_t *walk, const double *x_start,
                                            const double *values, double *x, double *logp, double *info) {
    BfDeviceGuard dev_guard(ctx);
    const char *who = "bfhip_pipeline_profile_lines";
    if (!ctx) return bf_set_error(BFHIP_ERR_ARG, "%s: invalid argument", who);
    size_t lds = 0;
    int grid = 0;
    const int d = ctx->has_model ? ctx->model.d : 0;
    if (int rc = plh_prepare(ctx, who, hess_kind, n_line < 0 ? 0 : n_line, (size_t)d * (d + 1) + (size_t)BF_NEWTON_NVEC * d, &lds, &grid)) return rc;
    if (int rc = pf_check(ctx, who, opts, objective, n_line, n_val, fixed, walk, x_start, values, x, logp, info)) return rc;
    if (n_line == 0) return 0;
    if (int rc = bf_set_lds(bf_pld_profile_lines_kernel, lds)) return rc;
    const PfLines a = {n_line, n_val, opts->max_iter, objective, opts->xtol, fixed, walk, x_start, values, x, logp, info};
    hipLaunchKernelGGL(bf_pld_profile_lines_kernel, dim3(grid), dim3(PLDH_TH), lds, ctx->stream, ctx->model, a, hess_kind,
                       (double *)ctx->hess_work);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
