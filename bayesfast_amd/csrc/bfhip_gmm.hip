// bfhip_gmm.hip -- bfhip_gmm_step and bfhip_gmm_work_bytes: one pass of expectation-maximisation for a mixture of Gaussians over the
// draws (bayesfast_amd/utils/gmm.py).  The kernels and their rules are in bfhip_gmm.h; this file checks the arguments and queues the
// launches on the context's stream: the E kernel over blocks of 64 rows, then, if the statistics are asked for, the moment kernel over
// (part, component) and the merge.
#include "bfhip_gmm.h"

extern "C" size_t bfhip_gmm_work_bytes(long n, int d, int k) {
    if (n < 1 || n > 0x7fffffffL || d < 1 || d > BFHIP_MAX_DIM || k < 1 || k > BFHIP_GMM_MAX_K) return 0;
    return gm_work(nullptr, n, d, k).bytes;
}

struct GmArgs {
    hipStream_t st;
    int d, k;
    long n;
    const double *x;
    long ldx;
    const double *logw, *centre, *mean, *whiten, *logc;
    double *logpdf, *resp;
    long ldr;
    GmWork w;
    int want_stats;
};
template <int NS>
static int gm_launch_e(const GmArgs &a) {
    const size_t lds = gm_e_lds(NS);
    if (int rc = bf_set_lds(gm_e_kernel<NS>, lds)) return rc;
    hipLaunchKernelGGL(gm_e_kernel<NS>, dim3((unsigned)((a.n + GM_RB - 1) / GM_RB)), dim3(GM_T), lds, a.st, a.d, a.k, a.n, a.x, a.ldx, a.logw,
                       a.mean, a.whiten, a.logc, a.logpdf, a.resp, a.ldr, a.w.wr, a.w.esum, a.want_stats);
    return 0;
}
template <int CB>
static void gm_launch_moment(const GmArgs &a, const GmPlan &pl) {
    hipLaunchKernelGGL(gm_moment_kernel<CB>, dim3((unsigned)pl.P, (unsigned)a.k), dim3(GM_T), gm_moment_lds(CB), a.st, a.d, a.k, a.n, a.x, a.ldx,
                       a.centre, (const double *)a.w.wr, pl.R, a.w.part);
}

extern "C" int bfhip_gmm_step(bfhip_ctx *ctx, int d, int k, long n, const double *x, long ldx, const double *logw, const double *centre,
                              const double *mean, const double *whiten, const double *logc, double *stats, double *logpdf, double *resp,
                              long ldr, void *work, size_t work_bytes) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || !x || !centre || !mean || !whiten || !logc || !work || n < 1 || d < 1 || k < 1)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_gmm_step: invalid argument (n = %ld, d = %d, k = %d, or a null pointer)", n, d, k);
    if (!stats && !logpdf && !resp) return bf_set_error(BFHIP_ERR_ARG, "bfhip_gmm_step: invalid argument (stats, logpdf and resp are all NULL)");
    if (d > BFHIP_MAX_DIM) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_gmm_step: d = %d exceeds BFHIP_MAX_DIM = %d", d, BFHIP_MAX_DIM);
    if (k > BFHIP_GMM_MAX_K)
        return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_gmm_step: k = %d components exceed BFHIP_GMM_MAX_K = %d", k, BFHIP_GMM_MAX_K);
    if (n > 0x7fffffffL) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_gmm_step: more than 2^31-1 rows (n = %ld)", n);
    if (ldx < d) return bf_set_error(BFHIP_ERR_ARG, "bfhip_gmm_step: a row stride below d (ldx = %ld, d = %d)", ldx, d);
    if (resp && ldr < k) return bf_set_error(BFHIP_ERR_ARG, "bfhip_gmm_step: a row stride below k (ldr = %ld, k = %d)", ldr, k);
    if ((uintptr_t)work & 255) return bf_set_error(BFHIP_ERR_ARG, "bfhip_gmm_step: the work buffer is not 256-byte aligned");
    const size_t need = bfhip_gmm_work_bytes(n, d, k);
    if (work_bytes < need) return bf_set_error(BFHIP_ERR_ARG, "bfhip_gmm_step: work buffer of %zu bytes, %zu needed", work_bytes, need);
    const GmArgs a = {ctx->stream, d, k, n, x, ldx, logw, centre, mean, whiten, logc, logpdf, resp, ldr, gm_work(work, n, d, k), stats ? 1 : 0};
    int rc = 0;
    switch (gm_steps(d)) {
#define GM_CASE(NS) case NS: rc = gm_launch_e<NS>(a); break
        GM_CASE(1); GM_CASE(2); GM_CASE(4); GM_CASE(8); GM_CASE(12); GM_CASE(16); GM_CASE(24); GM_CASE(32);
#undef GM_CASE
    }
    if (rc) return rc;
    if (stats) {
        const GmPlan pl = gm_plan(n);
        switch ((d + 15) / 16) {
#define GM_CASE(CB) case CB: gm_launch_moment<CB>(a, pl); break
            GM_CASE(1); GM_CASE(2); GM_CASE(3); GM_CASE(4); GM_CASE(5); GM_CASE(6); GM_CASE(7); GM_CASE(8);
#undef GM_CASE
        }
        const size_t total = (size_t)k * gm_stat_size(d);
        hipLaunchKernelGGL(gm_merge_kernel, dim3((unsigned)((total + GM_T - 1) / GM_T + 1)), dim3(GM_T), 0, a.st, d, k, pl.P,
                           (n + GM_RB - 1) / GM_RB, (const double *)a.w.part, (const double2 *)a.w.esum, stats);
    }
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
