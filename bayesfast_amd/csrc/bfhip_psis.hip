// bfhip_psis.hip -- what follows the importance weights of PostStep (bayesfast_amd/utils/psis.py): Pareto-smoothed importance
// sampling (Vehtari, Simpson, Gelman, Yao, Gabry 2024; the tail fit of Zhang & Stephens 2009) and the weighted table of mean, sd
// and quantiles, on the device:
//
//   bfhip_psis              log ratios -> shifted, tail-smoothed, normalised log weights and khat, sigma, log mean weight, Kish ESS
//   bfhip_wstat_columns     a batch of columns of the time-major sample tensor -> (n, WS_B), every draw kept, zero-weight rows masked
//   bfhip_wstat_moments     sum w, sum w^2 once; per column sum w x, then sum w (x - mean)^2, sum w^2 (x - mean)^2, min, max
//   bfhip_wstat_cumweights  running sum of the weights in a column's sorted order (three launches, no workgroup waits on another)
//   bfhip_wstat_quantiles   weighted quantiles by bisection in the running sum
//
// Every floating-point reduction has one fixed shape: a thread adds its elements in index order, a workgroup combines its 256
// threads by a halving tree in LDS (or, per column, its 16 row slices one after the other), one workgroup combines the
// workgroups' partial results the same way.  The shape depends on n alone, so the same input gives the same bits, and a column's
// sums never see its neighbours.  All of it is bound by HBM reads (8 to 16 bytes per element and pass); the transcendental work
// of the tail fit is (30 + sqrt M) M log1p, M <= 3 sqrt n.  64-bit offsets throughout.
#include "bfhip_block.h"

#define PS_T 256        // threads per workgroup, everywhere in this file
#define PS_MAXB 1024    // workgroups of a first-level reduction (they stride over the data beyond PS_T * PS_MAXB elements)
#define PS_MAXM 512     // candidate thetas: m = 30 + floor(sqrt M) <= 402 for n <= 2^31 - 1
#define WS_B BFHIP_DIAG_BATCH
#define WS_ROWS (PS_T / WS_B)          // row slices of a workgroup of the column reductions
#define WS_ITEMS 8                     // consecutive sorted positions per thread of the scan
#define WS_TILE (PS_T * WS_ITEMS)      // sorted positions per workgroup of the scan
static_assert(WS_B == 16 && WS_ROWS == BF_SLICES, "the column reductions take the column with a mask and the slice with a shift");
static_assert(BFHIP_WSTAT_WORK >= 4 * PS_MAXB * WS_B, "bfhip_wstat_moments keeps up to four partial arrays");

static inline int ps_grid(long n, long per_block) {
    const long g = (n + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > PS_MAXB ? PS_MAXB : g));
}

// ==== PSIS ===========================================================================================================================
// flags (out8[7]): 1 a NaN or +inf ratio, or no finite ratio at all: every output NaN; 2 no smoothing (M < 5, or a tail without spread)
__global__ __launch_bounds__(PS_T) void ps_ratio_kernel(long n, const double *__restrict__ logp, const double *__restrict__ logq,
                                                       double *__restrict__ lw, double *__restrict__ part) {
    __shared__ double red[PS_T];
    double mx = -__builtin_inf(), bad = 0.;
    for (long i = (long)blockIdx.x * PS_T + threadIdx.x; i < n; i += (long)gridDim.x * PS_T) {
        const double v = logq ? logp[i] - logq[i] : logp[i];
        lw[i] = v;
        if (v != v || v == __builtin_inf()) bad = 1.;
        else mx = fmax(mx, v);
    }
    mx = bf_block_reduce<PS_T>(mx, red, BfMax());
    bad = bf_block_reduce<PS_T>(bad, red, BfMax());
    if (threadIdx.x == 0) {
        part[blockIdx.x] = mx;
        part[PS_MAXB + blockIdx.x] = bad;
    }
}

__global__ __launch_bounds__(PS_T) void ps_max_kernel(int nb, const double *__restrict__ part, double *__restrict__ out8) {
    __shared__ double red[PS_T];
    double mx = -__builtin_inf(), bad = 0.;
    for (int i = threadIdx.x; i < nb; i += PS_T) {
        mx = fmax(mx, part[i]);
        bad = fmax(bad, part[PS_MAXB + i]);
    }
    mx = bf_block_reduce<PS_T>(mx, red, BfMax());
    bad = bf_block_reduce<PS_T>(bad, red, BfMax());
    if (threadIdx.x == 0) {
        out8[6] = mx;
        out8[7] = (bad != 0. || mx == -__builtin_inf()) ? 1. : 0.;
    }
}

__global__ __launch_bounds__(PS_T) void ps_shift_kernel(long n, const double *__restrict__ out8, double *__restrict__ lw) {
    const long i = (long)blockIdx.x * PS_T + threadIdx.x;
    if (i < n) lw[i] -= out8[6];
}

// exceedance of sorted tail position i over the cut
__device__ inline double ps_exceed(const uint64_t *tail, long i, double ecut) { return exp(bf_order_value(tail[i])) - ecut; }

// workgroup j: theta_j and k_j = mean_i log1p(-theta_j x_i)
__global__ __launch_bounds__(PS_T) void ps_theta_kernel(long n, long M, int m, const uint64_t *__restrict__ ks, double *__restrict__ kj,
                                                       double *__restrict__ thj) {
    __shared__ double red[PS_T];
    const uint64_t *tail = ks + (n - M);
    const double ecut = exp(bf_order_value(ks[n - M - 1]));
    const double xn = ps_exceed(tail, M - 1, ecut);
    const double xq = ps_exceed(tail, (long)floor((double)M / 4. + 0.5) - 1, ecut);
    const double th = 1. / xn + (1. - sqrt((double)m / ((double)(blockIdx.x + 1) - 0.5))) / (3. * xq);
    double s = 0.;
    for (long i = threadIdx.x; i < M; i += PS_T) s += log1p(-th * ps_exceed(tail, i, ecut));
    s = bf_block_reduce<PS_T>(s, red, BfSum());
    if (threadIdx.x == 0) {
        kj[blockIdx.x] = s / (double)M;
        thj[blockIdx.x] = th;
    }
}

// one workgroup: the profile likelihoods, their weights, the posterior-mean theta, k, sigma, khat
__global__ __launch_bounds__(PS_T) void ps_fit_kernel(long n, long M, int m, const uint64_t *__restrict__ ks, const double *__restrict__ kj,
                                                     const double *__restrict__ thj, double *__restrict__ out8) {
    __shared__ double red[PS_T], L[PS_MAXM], om[PS_MAXM];
    __shared__ double th_s;
    const uint64_t *tail = ks + (n - M);
    const double cut = bf_order_value(ks[n - M - 1]), ecut = exp(cut);
    for (int j = threadIdx.x; j < m; j += PS_T) L[j] = (double)M * (log(-thj[j] / kj[j]) - kj[j] - 1.);
    __syncthreads();
    for (int j = threadIdx.x; j < m; j += PS_T) {
        double s = 0.;
        for (int l = 0; l < m; ++l) s += exp(L[l] - L[j]);
        om[j] = 1. / s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double th = 0.;
        for (int j = 0; j < m; ++j) th += om[j] * thj[j];
        th_s = th;
    }
    __syncthreads();
    const double th = th_s;
    double s = 0.;
    for (long i = threadIdx.x; i < M; i += PS_T) s += log1p(-th * ps_exceed(tail, i, ecut));
    s = bf_block_reduce<PS_T>(s, red, BfSum());
    if (threadIdx.x == 0) {
        const double k = s / (double)M;
        const bool flat = !(ps_exceed(tail, M - 1, ecut) > 0.);   // no spread in the tail: nothing to fit
        out8[0] = flat ? __builtin_inf() : (k * (double)M + 5.) / ((double)M + 10.);
        out8[1] = flat ? __builtin_nan("") : -k / th;
        out8[3] = cut;
        if (flat) out8[7] = (double)((int)out8[7] | 2);
    }
}

// without a fit (M < 5): khat = inf, the cut for the record
__global__ void ps_nofit_kernel(long n, long M, const uint64_t *__restrict__ ks, double *__restrict__ out8) {
    out8[0] = __builtin_inf();
    out8[1] = __builtin_nan("");
    out8[3] = bf_order_value(ks[n - M - 1]);
    out8[7] = (double)((int)out8[7] | 2);
}

// the tail's expected order statistics under the fit, back to the original positions
__global__ __launch_bounds__(PS_T) void ps_smooth_kernel(long n, long M, const int64_t *__restrict__ order, const double *__restrict__ out8,
                                                        double *__restrict__ lw) {
    const long i = (long)blockIdx.x * PS_T + threadIdx.x;
    if (i >= M || (int)out8[7] != 0) return;
    const double khat = out8[0], sigma = out8[1], ecut = exp(out8[3]);
    const double l1p = log1p(-((double)i + 0.5) / (double)M);
    const double q = khat == 0. ? -sigma * l1p : sigma * expm1(-khat * l1p) / khat;
    const double v = log(ecut + q);
    lw[order[n - M + i]] = v > 0. ? 0. : v;   // capped at the shifted maximum (order is a permutation of 0 .. n - 1; a NaN stays)
}

__global__ __launch_bounds__(PS_T) void ps_lse_kernel(long n, const double *__restrict__ lw, double *__restrict__ part) {
    __shared__ double red[PS_T];
    double s1 = 0., s2 = 0.;
    for (long i = (long)blockIdx.x * PS_T + threadIdx.x; i < n; i += (long)gridDim.x * PS_T) {
        const double v = lw[i];       // <= 0 after the shift and the cap: no overflow, and the largest term is near 1
        s1 += exp(v);
        s2 += exp(2. * v);
    }
    s1 = bf_block_reduce<PS_T>(s1, red, BfSum());
    s2 = bf_block_reduce<PS_T>(s2, red, BfSum());
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s1;
        part[PS_MAXB + blockIdx.x] = s2;
    }
}

__global__ __launch_bounds__(PS_T) void ps_lse_final_kernel(long n, long M, int nb, const double *__restrict__ part, double *__restrict__ out8,
                                                           double *__restrict__ lse) {
    __shared__ double red[PS_T];
    double s1 = 0., s2 = 0.;
    for (int i = threadIdx.x; i < nb; i += PS_T) {
        s1 += part[i];
        s2 += part[PS_MAXB + i];
    }
    s1 = bf_block_reduce<PS_T>(s1, red, BfSum());
    s2 = bf_block_reduce<PS_T>(s2, red, BfSum());
    if (threadIdx.x == 0) {
        const double nan = __builtin_nan("");
        const bool bad = ((int)out8[7] & 1) != 0;
        const double l = bad ? nan : log(s1);
        *lse = l;
        out8[2] = (double)M;
        out8[4] = out8[6] + l - log((double)n);
        out8[5] = bad ? nan : s1 * s1 / s2;
        if (bad) out8[0] = out8[1] = out8[3] = out8[6] = nan;
    }
}

__global__ __launch_bounds__(PS_T) void ps_normalise_kernel(long n, const double *__restrict__ lse, double *__restrict__ lw) {
    const long i = (long)blockIdx.x * PS_T + threadIdx.x;
    if (i < n) lw[i] -= *lse;   // (a NaN lse, the flag of non-finite input, makes every weight NaN)
}

extern "C" int bfhip_psis(bfhip_ctx *ctx, long n, const double *logp, const double *logq, double *lw_out, double *out8, void *work,
                          size_t work_bytes) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || !logp || !lw_out || !out8 || !work) return bf_set_error(BFHIP_ERR_ARG, "bfhip_psis: invalid argument");
    if (n > 0x7fffffffL) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_psis: more than 2^31-1 values");
    if (work_bytes < BFHIP_PSIS_WORK_BYTES(n))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_psis: work buffer of %zu bytes, %zu needed", work_bytes, (size_t)BFHIP_PSIS_WORK_BYTES(n));
    long M = (long)ceil(3. * sqrt((double)n));
    if (n / 5 < M) M = n / 5;
    const int m = 30 + (int)floor(sqrt((double)M));
    if (m > PS_MAXM) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_psis: %d candidate thetas", m);
    uint64_t *keys = (uint64_t *)work;
    int64_t *order = (int64_t *)((char *)work + 8 * (size_t)n);
    double *part = (double *)((char *)work + 16 * (size_t)n);   // 2 PS_MAXB partial results
    double *kj = part + 2 * PS_MAXB, *thj = kj + PS_MAXM, *lse = thj + PS_MAXM;
    const int nb = ps_grid(n, PS_T);
    const unsigned ne = (unsigned)((n + PS_T - 1) / PS_T);
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(ps_ratio_kernel, dim3(nb), dim3(PS_T), 0, st, n, logp, logq, lw_out, part);
    hipLaunchKernelGGL(ps_max_kernel, dim3(1), dim3(PS_T), 0, st, nb, part, out8);
    hipLaunchKernelGGL(ps_shift_kernel, dim3(ne), dim3(PS_T), 0, st, n, out8, lw_out);
    BF_HIP_CHECK(hipGetLastError());
    if (int rc = bfhip_sort_keys(ctx, n, lw_out, keys, order)) return rc;
    if (M >= 5) {
        hipLaunchKernelGGL(ps_theta_kernel, dim3(m), dim3(PS_T), 0, st, n, M, m, keys, kj, thj);
        hipLaunchKernelGGL(ps_fit_kernel, dim3(1), dim3(PS_T), 0, st, n, M, m, keys, kj, thj, out8);
        hipLaunchKernelGGL(ps_smooth_kernel, dim3((unsigned)((M + PS_T - 1) / PS_T)), dim3(PS_T), 0, st, n, M, order, out8, lw_out);
    } else {
        hipLaunchKernelGGL(ps_nofit_kernel, dim3(1), dim3(1), 0, st, n, M, keys, out8);
    }
    hipLaunchKernelGGL(ps_lse_kernel, dim3(nb), dim3(PS_T), 0, st, n, lw_out, part);
    hipLaunchKernelGGL(ps_lse_final_kernel, dim3(1), dim3(PS_T), 0, st, n, M, nb, part, out8, lse);
    hipLaunchKernelGGL(ps_normalise_kernel, dim3(ne), dim3(PS_T), 0, st, n, lse, lw_out);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ==== the weighted table ==============================================================================================================
// columns: element e = (row, column b), b fastest; row = chain n_draw + draw.  The gather is bfhip_diag.hip's, without the split.
extern "C" int bfhip_wstat_columns(bfhip_ctx *ctx, int n_chain, long n_draw, long ldw, long ldr, const void *x, int is_f32, long since,
                                   int k0, int nb, const double *w, double *out) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n_chain < 1 || n_draw < 1 || !x || !out || since < 0 || k0 < 0 || nb < 1 || nb > WS_B || ldr < (long)k0 + nb ||
        (n_chain > 1 && ldw < 1))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_wstat_columns: invalid argument");
    const long n_el = (long)n_chain * n_draw * WS_B, nblk = (n_el + PS_T - 1) / PS_T;
    if ((long)n_chain * n_draw > 0x7fffffffL || nblk > 0x7fffffffL)
        return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_wstat_columns: more than 2^31-1 values per column");
    return bf_columns_launch(ctx, 1, n_el, n_draw, ldw, ldr, x, is_f32, since * ldr + k0, nb, BFHIP_DIAG_PLAIN, nullptr, w, out);
}

// ---- sums of the weights: sum w, sum w^2, the number of non-zero weights, a flag for a negative or non-finite one ----------------------
__global__ __launch_bounds__(PS_T) void ws_wsum_kernel(long n, const double *__restrict__ w, double *__restrict__ part) {
    __shared__ double red[PS_T];
    double s1 = 0., s2 = 0., cnt = 0., bad = 0.;
    for (long i = (long)blockIdx.x * PS_T + threadIdx.x; i < n; i += (long)gridDim.x * PS_T) {
        const double v = w[i];
        s1 += v;
        s2 += v * v;
        if (v != 0.) cnt += 1.;
        if (!(v >= 0.) || v == __builtin_inf()) bad = 1.;
    }
    s1 = bf_block_reduce<PS_T>(s1, red, BfSum());
    s2 = bf_block_reduce<PS_T>(s2, red, BfSum());
    cnt = bf_block_reduce<PS_T>(cnt, red, BfSum());   // (whole numbers below 2^31: exact)
    bad = bf_block_reduce<PS_T>(bad, red, BfMax());
    if (threadIdx.x == 0) {
        part[blockIdx.x] = s1;
        part[PS_MAXB + blockIdx.x] = s2;
        part[2 * PS_MAXB + blockIdx.x] = cnt;
        part[3 * PS_MAXB + blockIdx.x] = bad;
    }
}

__global__ __launch_bounds__(PS_T) void ws_wsum_final_kernel(int nb, const double *__restrict__ part, double *__restrict__ wsum) {
    __shared__ double red[PS_T];
    double s1 = 0., s2 = 0., cnt = 0., bad = 0.;
    for (int i = threadIdx.x; i < nb; i += PS_T) {
        s1 += part[i];
        s2 += part[PS_MAXB + i];
        cnt += part[2 * PS_MAXB + i];
        bad = fmax(bad, part[3 * PS_MAXB + i]);
    }
    s1 = bf_block_reduce<PS_T>(s1, red, BfSum());
    s2 = bf_block_reduce<PS_T>(s2, red, BfSum());
    cnt = bf_block_reduce<PS_T>(cnt, red, BfSum());
    bad = bf_block_reduce<PS_T>(bad, red, BfMax());
    if (threadIdx.x == 0) {
        wsum[0] = s1;
        wsum[1] = s2;
        wsum[2] = cnt;
        wsum[3] = bad;
    }
}

// ---- column moments: thread (slice sl, column b) walks rows sl, sl + 16 G, ...; PASS 1: sum w x, min, max; PASS 2: the centred sums -------
// Slice 0 folds the other slices' (sum, min or sum, max) onto its own, slice by slice: bf_slice_fold's order, the three in one
// loop (three calls of it keep fifteen more LDS reads in flight and take up to seven more registers)
template <int PASS>
__device__ inline void ws_fold(double &a0, double &a1, double &a2, const double *r0, const double *r1, const double *r2, int b) {
    for (int i = 1; i < WS_ROWS; ++i) {
        a0 += r0[i * WS_B + b];
        a1 = PASS == 1 ? fmin(a1, r1[i * WS_B + b]) : a1 + r1[i * WS_B + b];
        a2 = fmax(a2, r2[i * WS_B + b]);
    }
}
template <int PASS>
__global__ __launch_bounds__(PS_T) void ws_moments_kernel(long n, const double *__restrict__ series, const double *__restrict__ w,
                                                         const double *__restrict__ mean, double *__restrict__ part) {
    __shared__ double r0[PS_T], r1[PS_T], r2[PS_T];
    const int b = threadIdx.x & (WS_B - 1), sl = threadIdx.x / WS_B;
    const double mu = PASS == 2 ? mean[b] : 0.;
    double a0 = 0., a1 = PASS == 1 ? __builtin_inf() : 0., a2 = -__builtin_inf();
    for (long r = (long)blockIdx.x * WS_ROWS + sl; r < n; r += (long)gridDim.x * WS_ROWS) {
        const double wv = w[r];
        if (wv == 0.) continue;   // a row of zero weight is not read as a number: it may hold anything
        const double v = series[r * WS_B + b];
        if (PASS == 1) {
            a0 += wv * v;
            a1 = fmin(a1, v);     // (fmin / fmax pass over a NaN; the NaN shows in the sum)
            a2 = fmax(a2, v);
        } else {
            const double d = v - mu, wd2 = wv * (d * d);
            a0 += wd2;
            a1 += wv * wd2;
        }
    }
    r0[threadIdx.x] = a0;
    r1[threadIdx.x] = a1;
    r2[threadIdx.x] = a2;
    __syncthreads();
    if (sl == 0) {
        ws_fold<PASS>(a0, a1, a2, r0, r1, r2, b);
        part[(long)blockIdx.x * WS_B + b] = a0;
        part[((long)PS_MAXB + blockIdx.x) * WS_B + b] = a1;
        if (PASS == 1) part[((long)2 * PS_MAXB + blockIdx.x) * WS_B + b] = a2;
    }
}

// one workgroup: the workgroups' partial results in the same shape.  out (5, WS_B): mean, sum w d^2, sum w^2 d^2, min, max
template <int PASS>
__global__ __launch_bounds__(PS_T) void ws_moments_final_kernel(int nb, const double *__restrict__ part, double *__restrict__ out) {
    __shared__ double r0[PS_T], r1[PS_T], r2[PS_T];
    const int b = threadIdx.x & (WS_B - 1), sl = threadIdx.x / WS_B;
    double a0 = 0., a1 = PASS == 1 ? __builtin_inf() : 0., a2 = -__builtin_inf();
    for (int g = sl; g < nb; g += WS_ROWS) {
        a0 += part[(long)g * WS_B + b];
        const double p1 = part[((long)PS_MAXB + g) * WS_B + b];
        a1 = PASS == 1 ? fmin(a1, p1) : a1 + p1;
        if (PASS == 1) a2 = fmax(a2, part[((long)2 * PS_MAXB + g) * WS_B + b]);
    }
    r0[threadIdx.x] = a0;
    r1[threadIdx.x] = a1;
    r2[threadIdx.x] = a2;
    __syncthreads();
    if (sl == 0) {
        ws_fold<PASS>(a0, a1, a2, r0, r1, r2, b);
        if (PASS == 1) {
            out[b] = a0;
            out[3 * WS_B + b] = a1;
            out[4 * WS_B + b] = a2;
        } else {
            out[WS_B + b] = a0;
            out[2 * WS_B + b] = a1;
        }
    }
}

extern "C" int bfhip_wstat_moments(bfhip_ctx *ctx, long n, const double *series, const double *w, double *wsum, double *out,
                                   double *work) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || n > 0x7fffffffL || !w || !work || (series ? !out : !wsum))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_wstat_moments: invalid argument");
    hipStream_t st = ctx->stream;
    if (!series) {
        const int nb = ps_grid(n, PS_T);
        hipLaunchKernelGGL(ws_wsum_kernel, dim3(nb), dim3(PS_T), 0, st, n, w, work);
        hipLaunchKernelGGL(ws_wsum_final_kernel, dim3(1), dim3(PS_T), 0, st, nb, work, wsum);
    } else {
        const int nb = ps_grid(n, WS_ROWS);
        hipLaunchKernelGGL(ws_moments_kernel<1>, dim3(nb), dim3(PS_T), 0, st, n, series, w, (const double *)nullptr, work);
        hipLaunchKernelGGL(ws_moments_final_kernel<1>, dim3(1), dim3(PS_T), 0, st, nb, work, out);
        hipLaunchKernelGGL(ws_moments_kernel<2>, dim3(nb), dim3(PS_T), 0, st, n, series, w, out, work);
        hipLaunchKernelGGL(ws_moments_final_kernel<2>, dim3(1), dim3(PS_T), 0, st, nb, work, out);
    }
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- running sum of the permuted weights --------------------------------------------------------------------------------------------
// A workgroup's tile is WS_TILE consecutive sorted positions, WS_ITEMS per thread.  v[e] <- the thread's own running sum; returns
// the sum of the threads in front of it (a Hillis-Steele scan of the 256 thread sums in LDS), *total the tile's sum.
__device__ inline double ws_tile_scan(long n, long base, const uint32_t *__restrict__ order, const double *__restrict__ w, double *v,
                                      double (*buf)[PS_T], double *total) {
    double run = 0.;
    for (int e = 0; e < WS_ITEMS; ++e) {
        const long p = base + (long)threadIdx.x * WS_ITEMS + e;
        if (p < n) run += w[order[p]];   // (order[p] < n: a permutation of 0 .. n - 1)
        v[e] = run;
    }
    int src = 0;
    buf[0][threadIdx.x] = run;
    __syncthreads();
    for (int o = 1; o < PS_T; o <<= 1) {
        const double a = buf[src][threadIdx.x];
        buf[src ^ 1][threadIdx.x] = (int)threadIdx.x >= o ? buf[src][threadIdx.x - o] + a : a;
        src ^= 1;
        __syncthreads();
    }
    const double before = threadIdx.x ? buf[src][threadIdx.x - 1] : 0.;
    *total = buf[src][PS_T - 1];
    __syncthreads();   // (the buffers are free again)
    return before;
}

__global__ __launch_bounds__(PS_T) void ws_cum_sums_kernel(long n, const uint32_t *__restrict__ order, const double *__restrict__ w,
                                                          double *__restrict__ tsum) {
    __shared__ double buf[2][PS_T];
    double v[WS_ITEMS], total;
    ws_tile_scan(n, (long)blockIdx.x * WS_TILE, order, w, v, buf, &total);
    if (threadIdx.x == 0) tsum[blockIdx.x] = total;
}

// one workgroup: tile sums -> the sum of the tiles in front of each, PS_T tiles at a time with the carry of the chunks before
__global__ __launch_bounds__(PS_T) void ws_cum_offsets_kernel(long n_tile, double *__restrict__ tsum) {
    __shared__ double buf[2][PS_T];
    double carry = 0.;
    for (long t0 = 0; t0 < n_tile; t0 += PS_T) {
        const long i = t0 + threadIdx.x;
        int src = 0;
        buf[0][threadIdx.x] = i < n_tile ? tsum[i] : 0.;
        __syncthreads();
        for (int o = 1; o < PS_T; o <<= 1) {
            const double a = buf[src][threadIdx.x];
            buf[src ^ 1][threadIdx.x] = (int)threadIdx.x >= o ? buf[src][threadIdx.x - o] + a : a;
            src ^= 1;
            __syncthreads();
        }
        if (i < n_tile) tsum[i] = carry + (threadIdx.x ? buf[src][threadIdx.x - 1] : 0.);
        carry += buf[src][PS_T - 1];
        __syncthreads();
    }
}

__global__ __launch_bounds__(PS_T) void ws_cum_write_kernel(long n, const uint32_t *__restrict__ order, const double *__restrict__ w,
                                                           const double *__restrict__ toff, double *__restrict__ cum) {
    __shared__ double buf[2][PS_T];
    double v[WS_ITEMS], total;
    const long base = (long)blockIdx.x * WS_TILE;
    const double before = toff[blockIdx.x] + ws_tile_scan(n, base, order, w, v, buf, &total);
    for (int e = 0; e < WS_ITEMS; ++e) {
        const long p = base + (long)threadIdx.x * WS_ITEMS + e;
        if (p < n) cum[p] = before + v[e];
    }
}

extern "C" int bfhip_wstat_cumweights(bfhip_ctx *ctx, long n, const uint32_t *order, const double *w, double *cum, double *work) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || n > 0x7fffffffL || !order || !w || !cum || !work)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_wstat_cumweights: invalid argument");
    const long n_tile = (n + WS_TILE - 1) / WS_TILE;   // <= 2^20: a grid dimension
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(ws_cum_sums_kernel, dim3((unsigned)n_tile), dim3(PS_T), 0, st, n, order, w, work);
    hipLaunchKernelGGL(ws_cum_offsets_kernel, dim3(1), dim3(PS_T), 0, st, n_tile, work);
    hipLaunchKernelGGL(ws_cum_write_kernel, dim3((unsigned)n_tile), dim3(PS_T), 0, st, n, order, w, work, cum);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ---- weighted quantiles: a thread per probability -------------------------------------------------------------------------------------
// The sample is the first n_pos = wsum[2] sorted positions (the rows of zero weight were masked and sorted last).
// pos_k = (mid_k - mid_0) / (mid_last - mid_0) with mid_k = cum[k] - w_(k) / 2; the last k with pos_k <= q by bisection.
__device__ inline double ws_pos(long k, const uint32_t *order, const double *w, const double *cum, double m0, double den) {
    return ((cum[k] - 0.5 * w[order[k]]) - m0) / den;
}

__global__ void ws_quantiles_kernel(long n, const uint64_t *__restrict__ ks, const uint32_t *__restrict__ order, const double *__restrict__ w,
                                    const double *__restrict__ cum, const double *__restrict__ wsum, int nq, const double *__restrict__ probs,
                                    int b, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    double val = __builtin_nan("");
    const double cnt = wsum[2];
    const long np = cnt >= 1. && cnt <= (double)n ? (long)cnt : 0;
    if (np == 1) val = bf_order_value(ks[0]);
    else if (np > 1) {
        const double q = probs[i];
        const double m0 = cum[0] - 0.5 * w[order[0]], den = (cum[np - 1] - 0.5 * w[order[np - 1]]) - m0;
        if (den > 0.) {
            long lo = 0, hi = np - 1;   // pos_lo <= q throughout (pos_0 = 0)
            while (lo < hi) {
                const long mid = (lo + hi + 1) >> 1;
                if (ws_pos(mid, order, w, cum, m0, den) <= q) lo = mid;
                else hi = mid - 1;
            }
            const double a = bf_order_value(ks[lo]);
            if (lo == np - 1) val = a;
            else {
                const double c = bf_order_value(ks[lo + 1]), pk = ws_pos(lo, order, w, cum, m0, den);
                const double t = (q - pk) / (ws_pos(lo + 1, order, w, cum, m0, den) - pk), d = c - a;
                val = t >= 0.5 ? c - d * (1. - t) : a + d * t;
            }
        }
    }
    out[(long)i * WS_B + b] = val;
}

extern "C" int bfhip_wstat_quantiles(bfhip_ctx *ctx, long n, const uint64_t *keys_sorted, const uint32_t *order, const double *w,
                                     const double *cum, const double *wsum, int nq, const double *probs, int b, double *out) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || n > 0x7fffffffL || !keys_sorted || !order || !w || !cum || !wsum || nq < 1 || !probs || b < 0 || b >= WS_B || !out)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_wstat_quantiles: invalid argument");
    hipLaunchKernelGGL(ws_quantiles_kernel, dim3((unsigned)((nq + 63) / 64)), dim3(64), 0, ctx->stream, n, keys_sorted, order, w, cum, wsum,
                       nq, probs, b, out);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ==== pointwise PSIS-LOO and WAIC of a batch of columns ==============================================================================
#include "bfhip_ploo.h"
#include "bfhip_rw.h"
#include "bfhip_lgo.h"
#include "bfhip_pscale.h"
