// bfhip_pscale.h -- the smoothed importance weights of a batch of 16 columns of log ratios, written out (bayesfast_amd/utils/
// power_scale.py has the definitions); included at the end of bfhip_psis.hip, after bfhip_rw.h, whose fit it launches again: the
// distance between two weighted ECDFs (bfhip_pscale.hip) needs the weights of every draw, where bfhip_rw_finish keeps their sums.
//
//   bfhip_rw_weights   pl_fit_and_smooth as bfhip_rw_finish launches it (the same kernels on the same tail keys: the same bits), then
//                      u <- e = exp(smoothed shifted r): the rows not above the cut pair with their own ratio in one pass over the batch
//                      (a row above it and a row of zero weight get 0), the M tail rows scattered by index with their smoothed values;
//                      u <- u / sum e over the rows of the sample.
//
// The sum: a thread (slice, column) adds its rows in index order, slice 0 folds the slices in order, the column's workgroup of the tail
// kernel adds the workgroups' sums and the tail's by a halving tree -- every order is set by n alone, and a column's sum sees its own
// column alone.
#pragma once

__global__ __launch_bounds__(PS_T) void pw_body_kernel(PlCols a, long M, const double *__restrict__ out, const uint64_t *__restrict__ tail_keys,
                                                      const uint32_t *__restrict__ tail_idx, double *__restrict__ u, long ld_u,
                                                      double *__restrict__ part) {
    __shared__ double red[PS_T];
    const int b = threadIdx.x & (PL_B - 1), sl = threadIdx.x / PL_B;
    const double lb0 = -log((double)a.n);
    double s = 0.;
    if (b < a.nb) {
        const double mx = out[PL_MAXR * PL_B + b];
        const uint64_t kc = tail_keys[(long)b * (M + 1)];   // the cut pair
        const uint32_t ic = tail_idx[(long)b * (M + 1)];
        for (long r = (long)blockIdx.x * BF_SLICES + sl; r < a.n; r += (long)gridDim.x * BF_SLICES) {
            const double lb = a.lb ? a.lb[r] : lb0;
            double e = 0.;
            if (lb != -__builtin_inf()) {   // (a row of zero weight is not read as a number)
                const double rs = pl_shifted(a.lb ? lb : 0., pl_ell(a, r, b), mx);
                const uint64_t key = bf_order_key(rs);
                if (!(key > kc || (key == kc && (uint32_t)r > ic))) {   // a tail row comes with its smoothed value
                    e = exp(rs);
                    s += e;
                }
            }
            u[r * ld_u + b] = e;
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (sl == 0) part[(long)blockIdx.x * PL_B + b] = bf_slice_fold(s, 1, red, b, BfSum());
}

// workgroup b: the M tail rows of the sample, scattered by index; the column's sum and its figures
__global__ __launch_bounds__(PS_T) void pw_tail_kernel(PlCols a, long M, int nblk, const double *__restrict__ part,
                                                      const uint32_t *__restrict__ tail_idx, const double *__restrict__ sm,
                                                      const double *__restrict__ out8s, const double *__restrict__ out, double *__restrict__ u,
                                                      long ld_u, double *__restrict__ tot, double *__restrict__ wout) {
    __shared__ double red[PS_T];
    const int b = blockIdx.x;
    const double lb0 = -log((double)a.n);
    double body = 0., tail = 0.;
    for (int g = threadIdx.x; g < nblk; g += PS_T) body += part[(long)g * PL_B + b];
    body = bf_block_reduce<PS_T>(body, red, BfSum());
    for (long i = threadIdx.x; i < M; i += PS_T) {
        const long row = tail_idx[(long)b * (M + 1) + 1 + i];
        if (row >= a.n) continue;   // (the caller's array: nothing is written through an index that is no row)
        if ((a.lb ? a.lb[row] : lb0) == -__builtin_inf()) continue;   // a row of zero weight in the tail: not part of the sample
        const double e = exp(sm[(long)b * (M + 1) + i]);
        u[row * ld_u + b] = e;
        tail += e;
    }
    tail = bf_block_reduce<PS_T>(tail, red, BfSum());
    if (threadIdx.x != 0) return;
    const double *out8 = out8s + 8 * b;
    const int own = (int)out[PL_FLAGS * PL_B + b];
    const bool bad = (own & 5) != 0;
    const double nan = __builtin_nan(""), total = body + tail;
    tot[b] = bad ? nan : total;
    wout[BFHIP_RWW_SUM * PL_B + b] = bad ? nan : total;
    wout[BFHIP_RWW_KHAT * PL_B + b] = bad ? nan : out8[0];
    wout[BFHIP_RWW_FLAGS * PL_B + b] = (double)(bad ? own : own | ((int)out8[7] & 2));
    wout[(BFHIP_RWW_NOUT - 1) * PL_B + b] = 0.;
}

// element (row, column): a row of the sample is divided by its column's sum (NaN in a column with flag 1 or 4)
__global__ __launch_bounds__(PS_T) void pw_scale_kernel(long n, int nb, const double *__restrict__ lb, const double *__restrict__ tot,
                                                       double *__restrict__ u, long ld_u) {
    const long e = (long)blockIdx.x * PS_T + threadIdx.x, row = e / PL_B;
    const int b = (int)(e & (PL_B - 1));
    if (row >= n || b >= nb) return;
    if (lb && lb[row] == -__builtin_inf()) return;   // (written as 0 by the body pass)
    u[row * ld_u + b] = u[row * ld_u + b] / tot[b];
}

extern "C" int bfhip_rw_weights(bfhip_ctx *ctx, long n, const double *series, long ld, int nb, int mode, const double *c, const double *lb,
                                const uint64_t *tail_keys, const uint32_t *tail_idx, const double *out, void *work, size_t work_bytes,
                                double *u, long ld_u, double *wout) {
    BfDeviceGuard dev_guard(ctx);
    if (int rc = pl_check("bfhip_rw_weights", ctx, n, series, ld, nb, mode, c)) return rc;
    if (!out || !tail_keys || !tail_idx || !work || work_bytes < bfhip_ploo_work_bytes(n) || !u || ld_u < nb || !wout)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_rw_weights: invalid argument");
    const long M = pl_tail_size(n);
    const int m = 30 + (int)floor(sqrt((double)M));
    if (m > PS_MAXM) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_rw_weights: %d candidate thetas", m);
    const PlWork w = pl_work(work, n);
    const PlCols a = {n, series, ld, nb, mode, c, lb};
    hipStream_t st = ctx->stream;
    pl_fit_and_smooth(st, w, nb, M, m, tail_keys);
    const int g = ps_grid(n, BF_SLICES);
    double *tot = w.part + (size_t)PS_MAXB * PL_B;   // (the body's partial sums take the first PS_MAXB x 16 of the PL_NPART arrays)
    hipLaunchKernelGGL(pw_body_kernel, dim3(g), dim3(PS_T), 0, st, a, M, out, tail_keys, tail_idx, u, ld_u, w.part);
    hipLaunchKernelGGL(pw_tail_kernel, dim3(nb), dim3(PS_T), 0, st, a, M, g, (const double *)w.part, tail_idx, (const double *)w.sm,
                       (const double *)w.out8, out, u, ld_u, tot, wout);
    const long nblk = (n * PL_B + PS_T - 1) / PS_T;   // <= 2^27
    hipLaunchKernelGGL(pw_scale_kernel, dim3((unsigned)nblk), dim3(PS_T), 0, st, n, nb, lb, (const double *)tot, u, ld_u);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
