// bfhip_kde.hip -- bfhip_kde_logsum and bfhip_kde_work_bytes: the n x m sum of Gaussian kernels behind the multivariate kernel
// density estimate (bayesfast_amd/utils/kde.py) and the parameter-shift test built on it; bfhip_kde_wmean and
// bfhip_kde_wmean_work_bytes: the kernel-weighted means of the same pairs (score, kernel regression, mean shift).  The kernels and
// their rules are in bfhip_kde.h; this file checks the arguments and queues the launches: the data rows' pass once, then per chunk
// of queries the tile pass and the merge, all on the context's stream.
#include "bfhip_kde.h"

extern "C" size_t bfhip_kde_work_bytes(long n, long m, int d) {
    if (n < 1 || m < 1 || n > 0x7fffffffL || m > 0x7fffffffL || d < 1 || d > BFHIP_MAX_DIM) return 0;
    return kd_work(nullptr, n, m).bytes;
}

template <int NS>
static void kd_launch_tiles(hipStream_t st, dim3 grid, int d, long n, const double *z, long ldz, const double *c, long m, const double *zq,
                            long ldq, long q0, long mc, int exclude_self, long R, double2 *part) {
    hipLaunchKernelGGL(kd_tile_kernel<NS>, grid, dim3(KD_T), 0, st, d, n, z, ldz, c, m, zq, ldq, q0, mc, exclude_self, R, part);
}

extern "C" int bfhip_kde_logsum(bfhip_ctx *ctx, int d, long n, const double *z, long ldz, const double *logw, long m, const double *zq,
                                long ldq, int exclude_self, double *out, void *work, size_t work_bytes) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || !z || !zq || !out || !work || n < 1 || m < 1 || d < 1)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_kde_logsum: invalid argument");
    if (d > BFHIP_MAX_DIM) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_kde_logsum: d = %d exceeds BFHIP_MAX_DIM = %d", d, BFHIP_MAX_DIM);
    if (n > 0x7fffffffL || m > 0x7fffffffL) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_kde_logsum: more than 2^31-1 rows");
    if (ldz < d || ldq < d) return bf_set_error(BFHIP_ERR_ARG, "bfhip_kde_logsum: a row stride below d");
    if (exclude_self && (zq != z || m != n || ldq != ldz))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_kde_logsum: exclude_self needs the queries to be the data (zq == z, m == n)");
    if (work_bytes < bfhip_kde_work_bytes(n, m, d)) return bf_set_error(BFHIP_ERR_ARG, "bfhip_kde_logsum: work buffer too small");
    const KdWork w = kd_work(work, n, m);
    const KdPlan pl = kd_plan(n);
    const int ns = kd_steps(d);
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(kd_rows_kernel, dim3((unsigned)((n + KD_T - 1) / KD_T)), dim3(KD_T), 0, st, d, n, z, ldz, logw, w.c);
    for (long q0 = 0; q0 < m; q0 += KD_MCHUNK) {
        const long mc = m - q0 < KD_MCHUNK ? m - q0 : KD_MCHUNK;
        const dim3 grid((unsigned)pl.P, (unsigned)((mc + KD_QB - 1) / KD_QB));
#define KD_CASE(NS) case NS: kd_launch_tiles<NS>(st, grid, d, n, z, ldz, w.c, m, zq, ldq, q0, mc, exclude_self, pl.R, w.part); break
        switch (ns) {
            KD_CASE(1); KD_CASE(2); KD_CASE(4); KD_CASE(8); KD_CASE(12); KD_CASE(16); KD_CASE(24); KD_CASE(32);
        }
#undef KD_CASE
        hipLaunchKernelGGL(kd_merge_kernel, dim3((unsigned)((mc + KD_T - 1) / KD_T)), dim3(KD_T), 0, st, pl.P, mc, (const double2 *)w.part, out + q0);
    }
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- kernel-weighted means ------------------------------------------------------------------------------------------------------------
extern "C" size_t bfhip_kde_wmean_work_bytes(long n, long m, int d, int k) {
    if (n < 1 || m < 1 || n > 0x7fffffffL || m > 0x7fffffffL || d < 1 || d > BFHIP_MAX_DIM || k < 1 || k > BFHIP_MAX_DIM) return 0;
    return kd_wm_work(nullptr, n, m, k).bytes;
}

struct KdWmArgs {
    hipStream_t st;
    dim3 grid;
    size_t lds;
    int d;
    long n;
    const double *z;
    long ldz;
    const double *c;
    int k;
    const double *v;
    long ldv, m;
    const double *zq;
    long ldq, q0, mc;
    int exclude_self;
    long R;
    double *part;
};
template <int NS, int CB, bool SAME>
static int kd_wm_launch(const KdWmArgs &a) {
    if (int rc = bf_set_lds(kd_wm_tile_kernel<NS, CB, SAME>, a.lds)) return rc;
    hipLaunchKernelGGL((kd_wm_tile_kernel<NS, CB, SAME>), a.grid, dim3(KD_T), a.lds, a.st, a.d, a.n, a.z, a.ldz, a.c, a.k, a.v, a.ldv, a.m, a.zq,
                       a.ldq, a.q0, a.mc, a.exclude_self, a.R, a.part);
    return 0;
}
template <int NS>
static int kd_wm_launch_blocks(const KdWmArgs &a, int cb, bool same) {
    if (same) return kd_wm_launch<NS, kd_wm_same_blocks(NS), true>(a);
    switch (cb) {
        case 1: return kd_wm_launch<NS, 1, false>(a);
        case 2: return kd_wm_launch<NS, 2, false>(a);
        case 4: return kd_wm_launch<NS, 4, false>(a);
        default: return kd_wm_launch<NS, 8, false>(a);
    }
}

extern "C" int bfhip_kde_wmean(bfhip_ctx *ctx, int d, long n, const double *z, long ldz, const double *logw, int k, const double *v, long ldv,
                               long m, const double *zq, long ldq, int exclude_self, double *logsum, double *mean, long ldo, void *work,
                               size_t work_bytes) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || !z || !zq || !v || !mean || !work || n < 1 || m < 1 || d < 1 || k < 1)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_kde_wmean: invalid argument (n = %ld, m = %ld, d = %d, k = %d, or a null pointer)", n, m, d, k);
    if (d > BFHIP_MAX_DIM) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_kde_wmean: d = %d exceeds BFHIP_MAX_DIM = %d", d, BFHIP_MAX_DIM);
    if (k > BFHIP_MAX_DIM)
        return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_kde_wmean: k = %d columns exceed BFHIP_MAX_DIM = %d (batch the columns)", k, BFHIP_MAX_DIM);
    if (n > 0x7fffffffL || m > 0x7fffffffL)
        return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_kde_wmean: more than 2^31-1 rows (n = %ld, m = %ld)", n, m);
    if (ldz < d || ldq < d) return bf_set_error(BFHIP_ERR_ARG, "bfhip_kde_wmean: a row stride below d (ldz = %ld, ldq = %ld, d = %d)", ldz, ldq, d);
    if (ldv < k || ldo < k) return bf_set_error(BFHIP_ERR_ARG, "bfhip_kde_wmean: a row stride below k (ldv = %ld, ldo = %ld, k = %d)", ldv, ldo, k);
    if (exclude_self && (zq != z || m != n || ldq != ldz))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_kde_wmean: exclude_self needs the queries to be the data (zq == z, m == n; m = %ld, n = %ld)", m, n);
    const size_t need = bfhip_kde_wmean_work_bytes(n, m, d, k);
    if (work_bytes < need) return bf_set_error(BFHIP_ERR_ARG, "bfhip_kde_wmean: work buffer of %zu bytes, %zu needed", work_bytes, need);
    const KdWmWork w = kd_wm_work(work, n, m, k);
    const KdPlan pl = kd_plan(n);
    const int ns = kd_steps(d);
    const bool same = v == z && ldv == ldz && k == d;
    const int cb = same ? kd_wm_same_blocks(ns) : kd_wm_blocks(k);
    const long chunk = kd_wm_chunk(n, k);
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(kd_rows_kernel, dim3((unsigned)((n + KD_T - 1) / KD_T)), dim3(KD_T), 0, st, d, n, z, ldz, logw, w.c);
    for (long q0 = 0; q0 < m; q0 += chunk) {
        const long mc = m - q0 < chunk ? m - q0 : chunk;
        const KdWmArgs a = {st, dim3((unsigned)pl.P, (unsigned)((mc + KD_QB - 1) / KD_QB)), kd_wm_lds(ns, cb, same), d, n, z, ldz, w.c, k, v, ldv, m,
                            zq, ldq, q0, mc, exclude_self, pl.R, w.part};
        int rc = 0;
#define KD_CASE(NS) case NS: rc = kd_wm_launch_blocks<NS>(a, cb, same); break
        switch (ns) {
            KD_CASE(1); KD_CASE(2); KD_CASE(4); KD_CASE(8); KD_CASE(12); KD_CASE(16); KD_CASE(24); KD_CASE(32);
        }
#undef KD_CASE
        if (rc) return rc;
        hipLaunchKernelGGL(kd_wm_merge_kernel, dim3((unsigned)((mc + KD_T / 64 - 1) / (KD_T / 64))), dim3(KD_T), 0, st, pl.P, mc, k,
                           (const double *)w.part, logsum ? logsum + q0 : nullptr, mean + (size_t)q0 * ldo, ldo);
    }
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
