// bfhip_lgo.h -- leave-group-out cross-validation of a batch of 16 groups of data points (bayesfast_amd/utils/data_lgo.py has the
// definitions); included at the end of bfhip_psis.hip, after bfhip_rw.h.  A group's column holds ell_s = c - q_s / 2, the log of the
// conditional density of the group given the rest of the data at draw s, q_s the conditional chi-square of its dof points.
//
//   bfhip_igamc        Q(a, x) elementwise (bfhip_igamc.h), exported so that the function can be tested on its own
//   bfhip_lgo_accum    folds an (n, <= 16) buffer of whitened residuals z into the (n, 16) buffer of group columns: column j goes to
//                      slot slot[j], acc = acc - 0.5 * (z * z) once per column in column order, not contracted, a slot that starts in
//                      this call from c.  A row is one thread's: the bits of a group's column depend on the order of its columns alone,
//                      not on how they were split over calls, slots or batches.  Vector loads and stores, nothing atomic.
//   bfhip_ploo_moments, bfhip_ploo_tail    run unchanged on that buffer in mode BFHIP_PLOO_ELL
//   bfhip_lgo_finish   the fit per column and the smoothed tail as bfhip_ploo_finish launches them (pl_fit_and_smooth), then one pass
//                      over the rows, and the M tail rows fetched by index, for bfhip_ploo_finish's sums and, with q = 2 (c - ell) and
//                      Q = Q(dof / 2, q / 2), sum e q, sum e Q, sum w q, sum w Q.  The orders are those of bfhip_ploo_finish, set by n
//                      alone; a column never meets its neighbours.
#pragma once
#include "bfhip_igamc.h"

typedef double lg_d2 __attribute__((ext_vector_type(2)));

// ==== Q(a, x) elementwise ============================================================================================================
__global__ __launch_bounds__(PS_T) void lg_igamc_kernel(long n, const double *__restrict__ a, const double *__restrict__ x,
                                                       double *__restrict__ out) {
    for (long i = (long)blockIdx.x * PS_T + threadIdx.x; i < n; i += (long)gridDim.x * PS_T) out[i] = bf_igamc(a[i], x[i]);
}

extern "C" int bfhip_igamc(bfhip_ctx *ctx, long n, const double *a, const double *x, double *out) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || !a || !x || !out) return bf_set_error(BFHIP_ERR_ARG, "bfhip_igamc: invalid argument");
    hipLaunchKernelGGL(lg_igamc_kernel, dim3(ps_grid(n, PS_T)), dim3(PS_T), 0, ctx->stream, n, a, x, out);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ==== accumulate =====================================================================================================================
struct LgMap {          // by value: the kernel's scalar registers hold it
    int slot[PL_B];     // column j of z -> slot of acc, or -1
    double c[PL_B];     // per slot
    unsigned start;     // bit s: slot s starts at c[s] in this call, whatever acc holds
    unsigned touched;   // bit s: slot s starts or takes a column
};

// thread: one row.  VEC: both rows 16-byte aligned (even strides, aligned bases) -- two doubles per load and store
template <bool VEC>
__global__ __launch_bounds__(PS_T) void lg_accum_kernel(long n, const double *__restrict__ z, long ldz, int nb, LgMap mp,
                                                       double *__restrict__ acc, long lda) {
#pragma clang fp contract(off)
    const long row = (long)blockIdx.x * PS_T + threadIdx.x;
    if (row >= n) return;
    const double *zr = z + row * ldz;
    double *ar = acc + row * lda;
    double zv[PL_B], av[PL_B];
#pragma unroll
    for (int p = 0; p < PL_B / 2; ++p) {
        zv[2 * p] = zv[2 * p + 1] = 0.;
        if (2 * p + 1 < nb) {   // (a pair is read only where both columns exist: the buffer may end with the last row's column nb - 1)
            if (VEC) {
                const lg_d2 v = *(const lg_d2 *)(zr + 2 * p);
                zv[2 * p] = v.x;
                zv[2 * p + 1] = v.y;
            } else {
                zv[2 * p] = zr[2 * p];
                zv[2 * p + 1] = zr[2 * p + 1];
            }
        } else if (2 * p < nb) {
            zv[2 * p] = zr[2 * p];
        }
    }
#pragma unroll
    for (int p = 0; p < PL_B / 2; ++p) {
        const unsigned pair = 3u << (2 * p);
        av[2 * p] = mp.c[2 * p];
        av[2 * p + 1] = mp.c[2 * p + 1];
        if (!(mp.touched & pair) || (mp.start & pair) == pair) continue;   // nothing to read: untouched, or both start here
        double lo, hi;
        if (VEC) {
            const lg_d2 v = *(const lg_d2 *)(ar + 2 * p);
            lo = v.x;
            hi = v.y;
        } else {
            lo = ar[2 * p];
            hi = ar[2 * p + 1];
        }
        if (!(mp.start >> (2 * p) & 1u)) av[2 * p] = lo;
        if (!(mp.start >> (2 * p + 1) & 1u)) av[2 * p + 1] = hi;
    }
#pragma unroll
    for (int j = 0; j < PL_B; ++j) {   // column order; the slot is the same in every thread, so the inner test is scalar
        if (j >= nb) continue;
        const double h = 0.5 * (zv[j] * zv[j]);
#pragma unroll
        for (int s = 0; s < PL_B; ++s)
            if (mp.slot[j] == s) av[s] = av[s] - h;
    }
#pragma unroll
    for (int p = 0; p < PL_B / 2; ++p) {
        if (!(mp.touched & (3u << (2 * p)))) continue;
        if (VEC) {
            *(lg_d2 *)(ar + 2 * p) = lg_d2{av[2 * p], av[2 * p + 1]};
        } else {
            ar[2 * p] = av[2 * p];
            ar[2 * p + 1] = av[2 * p + 1];
        }
    }
}

extern "C" int bfhip_lgo_accum(bfhip_ctx *ctx, long n, const double *z, long ldz, int nb, const int *slot, const double *c,
                               unsigned start, double *acc, long lda) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || !z || nb < 1 || nb > PL_B || ldz < nb || !slot || !acc || lda < PL_B || (start >> PL_B) || (start && !c))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_lgo_accum: invalid argument");
    if (n > 0x7fffffffL) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_lgo_accum: more than 2^31-1 rows");
    LgMap mp;
    mp.start = start;
    mp.touched = start;
    for (int j = 0; j < PL_B; ++j) {
        mp.slot[j] = j < nb ? slot[j] : -1;
        mp.c[j] = c ? c[j] : 0.;
        if (mp.slot[j] < -1 || mp.slot[j] >= PL_B) return bf_set_error(BFHIP_ERR_ARG, "bfhip_lgo_accum: invalid argument");
        if (mp.slot[j] >= 0) mp.touched |= 1u << mp.slot[j];
    }
    if (!mp.touched) return 0;
    const bool vec = (ldz & 1) == 0 && (lda & 1) == 0 && ((uintptr_t)z & 15) == 0 && ((uintptr_t)acc & 15) == 0;
    const unsigned g = (unsigned)((n + PS_T - 1) / PS_T);
    if (vec)
        hipLaunchKernelGGL(lg_accum_kernel<true>, dim3(g), dim3(PS_T), 0, ctx->stream, n, z, ldz, nb, mp, acc, lda);
    else
        hipLaunchKernelGGL(lg_accum_kernel<false>, dim3(g), dim3(PS_T), 0, ctx->stream, n, z, ldz, nb, mp, acc, lda);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ==== finish =========================================================================================================================
#define LG_NSUM 5   // sums over the smoothed weights: sum e, sum e^2, sum exp(lb - max lb), sum e q, sum e Q; then sum w q, sum w Q
static_assert(LG_NSUM + 2 <= PL_NPART, "the body's partial results fit the moment passes' part of the work buffer");

struct LgCols {   // by value
    double c[PL_B], a[PL_B];   // per slot: the constant of ell, dof / 2
};

__device__ inline double lg_q(double c, double ell) {
    const double q = 2. * (c - ell);
    return q > 0. ? q : 0.;   // (rounding alone takes it below 0)
}

// the rows not above the cut pair, each with its own ratio, as pl_body_kernel; and every row of the sample under its base weight
__global__ __launch_bounds__(PS_T) void lg_body_kernel(PlCols a, LgCols gc, long M, const double *__restrict__ out,
                                                      const uint64_t *__restrict__ tail_keys, const uint32_t *__restrict__ tail_idx,
                                                      double *__restrict__ part) {
    __shared__ double red[LG_NSUM + 2][PS_T];
    const int b = threadIdx.x & (PL_B - 1), sl = threadIdx.x / PL_B;
    const double lb0 = -log((double)a.n), w0 = 1. / (double)a.n;
    double v[LG_NSUM + 2];
    for (int k = 0; k < LG_NSUM + 2; ++k) v[k] = 0.;
    if (b < a.nb) {
        const double mx = out[PL_MAXR * PL_B + b], mb = out[PL_MAXB * PL_B + b];
        const double cb = gc.c[b], ab = gc.a[b];
        const uint64_t kc = tail_keys[(long)b * (M + 1)];   // the cut pair
        const uint32_t ic = tail_idx[(long)b * (M + 1)];
        for (long r = (long)blockIdx.x * BF_SLICES + sl; r < a.n; r += (long)gridDim.x * BF_SLICES) {
            const double lb = a.lb ? a.lb[r] : lb0;
            if (lb == -__builtin_inf()) continue;
            const double ell = pl_ell(a, r, b);
            const double q = lg_q(cb, ell), big_q = bf_igamc(ab, 0.5 * q), w = a.lb ? exp(lb) : w0;
            v[LG_NSUM] += w * q;
            v[LG_NSUM + 1] += w * big_q;
            const double rs = pl_shifted(a.lb ? lb : 0., ell, mx);
            const uint64_t key = bf_order_key(rs);
            if (key > kc || (key == kc && (uint32_t)r > ic)) continue;   // a tail row: it comes with its smoothed value
            const double e = exp(rs);
            v[0] += e;
            v[1] += e * e;
            v[2] += a.lb ? exp(lb - mb) : 1.;
            v[3] += e * q;
            v[4] += e * big_q;
        }
    }
    for (int k = 0; k < LG_NSUM + 2; ++k) red[k][threadIdx.x] = v[k];
    __syncthreads();
    if (sl == 0)
        for (int k = 0; k < LG_NSUM + 2; ++k) part[((long)k * PS_MAXB + blockIdx.x) * PL_B + b] = bf_slice_fold(v[k], 1, red[k], b, BfSum());
}

// workgroup b: the workgroups' body sums, the M tail rows fetched by index, the column's figures
__global__ __launch_bounds__(PS_T) void lg_finish_kernel(PlCols a, LgCols gc, long M, int nblk, const double *__restrict__ part,
                                                        const uint32_t *__restrict__ tail_idx, const double *__restrict__ sm,
                                                        const double *__restrict__ out8s, double *__restrict__ out, double *__restrict__ lgo) {
    __shared__ double red[PS_T];
    const int b = blockIdx.x;
    const double lb0 = -log((double)a.n);
    const double mx = out[PL_MAXR * PL_B + b], mb = a.lb ? out[PL_MAXB * PL_B + b] : 0., shift = mb - mx;
    const double cb = gc.c[b], ab = gc.a[b];
    double body[LG_NSUM + 2], tail[LG_NSUM];
    for (int k = 0; k < LG_NSUM + 2; ++k) {
        double s = 0.;
        for (int g = threadIdx.x; g < nblk; g += PS_T) s += part[((long)k * PS_MAXB + g) * PL_B + b];
        body[k] = bf_block_reduce<PS_T>(s, red, BfSum());
    }
    for (int k = 0; k < LG_NSUM; ++k) tail[k] = 0.;
    for (long i = threadIdx.x; i < M; i += PS_T) {
        const double v = sm[(long)b * (M + 1) + i], e = exp(v);
        const long row = tail_idx[(long)b * (M + 1) + 1 + i];
        tail[0] += e;
        tail[1] += e * e;
        if (row >= a.n) continue;   // (the caller's array: nothing is read through an index that is no row)
        const double lb = a.lb ? a.lb[row] : lb0;
        if (lb == -__builtin_inf()) continue;   // a row of zero weight in the tail (fewer than M + 1 rows have any): in the normalisation only
        const double ell = pl_ell(a, row, b), q = lg_q(cb, ell);
        tail[2] += exp(v + ell - shift);
        tail[3] += e * q;
        tail[4] += e * bf_igamc(ab, 0.5 * q);
    }
    for (int k = 0; k < LG_NSUM; ++k) tail[k] = bf_block_reduce<PS_T>(tail[k], red, BfSum());
    if (threadIdx.x != 0) return;
    const double *out8 = out8s + 8 * b;
    const double nan = __builtin_nan("");
    const int own = (int)out[PL_FLAGS * PL_B + b];
    const bool bad = (own & 5) != 0;   // (nothing was fitted to such a column that is worth a flag)
    const int flags = bad ? own : own | ((int)out8[7] & 2);
    const double s1 = body[0] + tail[0], s2 = body[1] + tail[1];
    out[PL_ELPD * PL_B + b] = bad ? nan : log(body[2] + tail[2]) + shift - log(s1);
    out[PL_KHAT * PL_B + b] = bad ? nan : out8[0];
    out[PL_SIGMA * PL_B + b] = bad ? nan : out8[1];
    out[PL_M * PL_B + b] = (double)M;
    out[PL_CUT * PL_B + b] = bad ? nan : out8[3];
    out[PL_ESS * PL_B + b] = bad ? nan : s1 * s1 / s2;
    out[PL_PIT * PL_B + b] = nan;
    out[PL_FLAGS * PL_B + b] = (double)flags;
    if (bad) out[PL_LPD * PL_B + b] = out[PL_SWE * PL_B + b] = out[PL_WAIC * PL_B + b] = out[PL_MAXR * PL_B + b] = nan;
    lgo[BFHIP_LGO_CHI2_BASE * PL_B + b] = bad ? nan : body[LG_NSUM];
    lgo[BFHIP_LGO_CHI2 * PL_B + b] = bad ? nan : (body[3] + tail[3]) / s1;
    lgo[BFHIP_LGO_PPP_BASE * PL_B + b] = bad ? nan : body[LG_NSUM + 1];
    lgo[BFHIP_LGO_PPP * PL_B + b] = bad ? nan : (body[4] + tail[4]) / s1;
}

extern "C" int bfhip_lgo_finish(bfhip_ctx *ctx, long n, const double *series, long ld, int nb, const double *c, const double *dof,
                                const double *lb, const uint64_t *tail_keys, const uint32_t *tail_idx, double *out, double *lgo_out,
                                void *work, size_t work_bytes) {
    BfDeviceGuard dev_guard(ctx);
    if (int rc = pl_check("bfhip_lgo_finish", ctx, n, series, ld, nb, BFHIP_PLOO_ELL, nullptr)) return rc;
    if (!c || !dof || !out || !lgo_out || !tail_keys || !tail_idx || !work || work_bytes < bfhip_ploo_work_bytes(n))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_lgo_finish: invalid argument");
    LgCols gc;
    for (int b = 0; b < PL_B; ++b) {
        gc.c[b] = b < nb ? c[b] : 0.;
        gc.a[b] = b < nb ? 0.5 * dof[b] : 1.;
        if (!(gc.a[b] > 0.) || !(gc.a[b] < __builtin_inf()) || gc.c[b] != gc.c[b])
            return bf_set_error(BFHIP_ERR_ARG, "bfhip_lgo_finish: invalid argument");
    }
    const long M = pl_tail_size(n);
    const int m = 30 + (int)floor(sqrt((double)M));
    if (m > PS_MAXM) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_lgo_finish: %d candidate thetas", m);
    const PlWork w = pl_work(work, n);
    const PlCols a = {n, series, ld, nb, BFHIP_PLOO_ELL, nullptr, lb};
    hipStream_t st = ctx->stream;
    pl_fit_and_smooth(st, w, nb, M, m, tail_keys);
    const int g = ps_grid(n, BF_SLICES);
    hipLaunchKernelGGL(lg_body_kernel, dim3(g), dim3(PS_T), 0, st, a, gc, M, (const double *)out, tail_keys, tail_idx, w.part);
    hipLaunchKernelGGL(lg_finish_kernel, dim3(nb), dim3(PS_T), 0, st, a, gc, M, g, (const double *)w.part, tail_idx, (const double *)w.sm,
                       (const double *)w.out8, out, lgo_out);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
