// bfhip_acor.hip -- the chains' integrated autocorrelation time (utils/acor.py:79-145: emcee's estimator with Sokal's automatic
// window, bayesfast.utils.integrated_time) as two data-parallel reductions over walkers and time.  The window search runs on the
// host over the per-lag sums, block by block (bayesfast_amd/utils/acor.py: integrated_time_sharded).
//
//   bfhip_acor_moments   mean and 1 / a_wk(0) of every (walker w, dimension k) series, a_wk(0) = sum_s y(s)^2, y = x - mean:
//                        two passes over time (no one-pass variance)
//   bfhip_acor_lag_sums  S(t, k) = sum_w a_wk(t) / a_wk(0) for the lags t0 .. t0 + n_lag - 1, a_wk(t) = sum_s y(s) y(s + t)
//                        (the linear autocovariance the zero-padded FFT of the host port gives)
//
// The lag pass: a workgroup takes a group of walkers, 16 series (a tile of td dimensions of 16 / td walkers) and 64 lags.  It stages
// each chunk of 256 centred time steps, with a halo of 64 (and, beyond lag 0, the chunk of the lagged series), in LDS; a lane owns
// one series and 16 consecutive lags, keeps a rotating window of 16 lagged values in registers and does 16 FP64 FMAs per two LDS
// reads.  The four waves take a quarter of every chunk each.  Every sum has a fixed order (time in order within a wave's quarters,
// walkers in order, then waves, walker slots and walker groups in order), set by the shape alone: the result is bitwise
// repeatable and the same whichever lag block computes a lag.  No float atomics, 64-bit offsets throughout.
#include <cmath>
#include "bfhip_block.h"

#define AC_SLOTS 16                       // series per workgroup
#define AC_R 16                           // lags per lane
#define AC_LAGS 64                        // lags per workgroup: 4 lane groups of AC_R
#define AC_CT 256                         // time steps per staged chunk
#define AC_WAVES 4                        // waves per workgroup; each takes AC_CT / AC_WAVES steps of every chunk
#define AC_TH (64 * AC_WAVES)
#define AC_SB (AC_CT + AC_LAGS + 1)       // odd strides: the 16 series of a wave fall in distinct LDS banks
#define AC_SA (AC_CT + 1)
#define AC_MAXG 256                       // walker groups (partial sums in the caller's work buffer)

// walkers per group and the group count: functions of n_w alone, so that the order of the walker sum is set by the shape
static inline void ac_groups(int n_w, int *wpg, int *n_g) {
    *wpg = (n_w + AC_MAXG - 1) / AC_MAXG;
    *n_g = (n_w + *wpg - 1) / *wpg;
}
// dimensions per lag-pass workgroup: the smallest power of two >= n_d, at most AC_SLOTS (log2)
static inline int ac_log_td(int n_d) {
    int l = 0;
    while ((1 << l) < n_d && (1 << l) < AC_SLOTS) ++l;
    return l;
}

// ---- moments: 16 series (flattened walker-major (w, k) indices) x 16 time slices per workgroup ----------------------------------
__global__ __launch_bounds__(256) void bf_acor_moments_kernel(int n_w, long n_t, int n_d, long ldw, const double *__restrict__ x,
                                                             double *__restrict__ mean, double *__restrict__ inv) {
    __shared__ double red[256];
    const int q = threadIdx.x & 15, sl = threadIdx.x >> 4;
    const long id = (long)blockIdx.x * 16 + q;
    const bool ok = id < (long)n_w * n_d;
    const double *xs = x + (ok ? (id / n_d) * ldw + id % n_d : 0);
    double sm = 0.;
    if (ok)
        for (long s = sl; s < n_t; s += 16) sm += xs[s * n_d];
    red[threadIdx.x] = sm;
    __syncthreads();
    const double m = bf_slice_fold(0., 0, red, q, BfSum()) / (double)n_t;   // (every thread, from a literal 0)
    __syncthreads();
    double sq = 0.;
    if (ok)
        for (long s = sl; s < n_t; s += 16) {
            const double d = xs[s * n_d] - m;
            sq = fma(d, d, sq);
        }
    red[threadIdx.x] = sq;
    __syncthreads();
    if (sl == 0 && ok) {
        const double a0 = bf_slice_fold(0., 0, red, q, BfSum());
        mean[id] = m;
        inv[id] = 1. / a0;   // a constant series: 1 / 0 = inf, and its lag sums 0 * inf = NaN, as the host port's 0 / 0
    }
}

// ---- lag sums: grid (walker groups, dimension tiles, lag tiles of AC_LAGS) -> part[g][t - t0][k] ---------------------------------
// LDS: B[AC_SLOTS][AC_SB] = y(s0 + tb + i), zero beyond the series, tb the workgroup's first lag; A[AC_SLOTS][AC_SA] = y(s0 + i)
// (A is B itself when tb = 0).  Lane (j = lane / 16, p = lane % 16): series slot p, lags tb + 16 j .. tb + 16 j + 15.
__global__ __launch_bounds__(AC_TH) void bf_acor_lag_kernel(int n_w, long n_t, int n_d, long ldw, const double *__restrict__ x,
                                                           const double *__restrict__ mean, const double *__restrict__ inv, long t0,
                                                           int n_lag, int ltd, int wpg, double *__restrict__ part) {
    extern __shared__ double lds[];
    const int td = 1 << ltd, ws_n = AC_SLOTS >> ltd;
    const int g = blockIdx.x, k0 = blockIdx.y * td, l0 = blockIdx.z * AC_LAGS;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, p = lane & 15, j = lane >> 4;
    const long tb = t0 + l0;
    const long n_eff = n_t - tb;   // steps s with a nonzero product at some lag of this workgroup
    double *B = lds, *A = (tb == 0) ? lds : lds + AC_SLOTS * AC_SB;
    const int sa = (tb == 0) ? AC_SB : AC_SA;
    const int w_begin = g * wpg, w_end = min(w_begin + wpg, n_w);
    const int my_k = k0 + (p & (td - 1));
    double tot[AC_R];
#pragma unroll
    for (int r = 0; r < AC_R; ++r) tot[r] = 0.;
    for (int w0 = w_begin; n_eff > 0 && w0 < w_end; w0 += ws_n) {
        double acc[AC_R];
#pragma unroll
        for (int r = 0; r < AC_R; ++r) acc[r] = 0.;
        for (long s0 = 0; s0 < n_eff; s0 += AC_CT) {
            __syncthreads();   // the previous chunk's readers are done
            for (int e = tid; e < AC_SLOTS * (AC_CT + AC_LAGS); e += AC_TH) {
                const int q = e & (AC_SLOTS - 1), i = e / AC_SLOTS;
                const int wq = w0 + (q >> ltd), kq = k0 + (q & (td - 1));
                const long s = s0 + tb + i;
                double v = 0.;
                if (wq < w_end && kq < n_d && s < n_t) v = x[(long)wq * ldw + s * n_d + kq] - mean[(long)wq * n_d + kq];
                B[q * AC_SB + i] = v;
            }
            if (tb != 0)
                for (int e = tid; e < AC_SLOTS * AC_CT; e += AC_TH) {
                    const int q = e & (AC_SLOTS - 1), i = e / AC_SLOTS;
                    const int wq = w0 + (q >> ltd), kq = k0 + (q & (td - 1));
                    const long s = s0 + i;
                    double v = 0.;
                    if (wq < w_end && kq < n_d && s < n_t) v = x[(long)wq * ldw + s * n_d + kq] - mean[(long)wq * n_d + kq];
                    A[q * AC_SA + i] = v;
                }
            __syncthreads();
            const int sq = wave * (AC_CT / AC_WAVES);
            const long left = n_eff - s0 - sq;
            if (left > 0) {   // (wave-uniform)
                // steps beyond n_eff multiply lagged values past the series' end, which are staged as 0
                const int n_s = (int)((left < AC_CT / AC_WAVES ? left : AC_CT / AC_WAVES) + AC_R - 1) / AC_R * AC_R;
                const double *Ap = A + p * sa + sq;
                const double *Bp = B + p * AC_SB + sq + j * AC_R;
                double win[AC_R];   // win[(u + r) % AC_R] = lagged value for lag r at step s + u
#pragma unroll
                for (int r = 0; r < AC_R; ++r) win[r] = Bp[r];
                for (int s = 0; s < n_s; s += AC_R) {
#pragma unroll
                    for (int u = 0; u < AC_R; ++u) {
                        const double a = Ap[s + u];
#pragma unroll
                        for (int r = 0; r < AC_R; ++r) acc[r] = fma(a, win[(u + r) % AC_R], acc[r]);
                        win[u] = Bp[s + u + AC_R];   // (index < AC_CT + AC_LAGS: the halo)
                    }
                }
            }
        }
        const int my_w = w0 + (p >> ltd);
        if (my_w < w_end && my_k < n_d) {
            const double iv = inv[(long)my_w * n_d + my_k];
#pragma unroll
            for (int r = 0; r < AC_R; ++r) tot[r] = fma(acc[r], iv, tot[r]);
        }
    }
    // fixed-order combination: walker slots in order, each over the four waves in order
    __syncthreads();
    double *red = lds;   // [r][wave][lane]: AC_R * AC_TH <= AC_SLOTS * AC_SB doubles
#pragma unroll
    for (int r = 0; r < AC_R; ++r) red[(r * AC_WAVES + wave) * 64 + lane] = tot[r];
    __syncthreads();
    for (int o = tid; o < AC_LAGS * td; o += AC_TH) {
        const int kk = o & (td - 1), lag = o >> ltd, jj = lag / AC_R, r = lag % AC_R;
        double sm = 0.;
        for (int ws = 0; ws < ws_n; ++ws) {
            const int ln = jj * 16 + (ws << ltd) + kk;
            for (int wv = 0; wv < AC_WAVES; ++wv) sm += red[(r * AC_WAVES + wv) * 64 + ln];
        }
        const long t = l0 + lag;
        // a lag >= n_t has no terms: 0, also where the tile's earlier lags are live and sm is 0 * inf or 0 * NaN (a constant or a
        // non-finite series), as in a tile wholly beyond the series
        if (t < n_lag && k0 + kk < n_d) part[((long)g * n_lag + t) * n_d + k0 + kk] = (tb + lag < n_t) ? sm : 0.;
    }
}

// out[i] = sum_g part[g][i], g in order
__global__ __launch_bounds__(256) void bf_acor_reduce_kernel(int n_g, long n, const double *__restrict__ part, double *__restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.;
    for (int g = 0; g < n_g; ++g) s += part[(long)g * n + i];
    out[i] = s;
}

static bool ac_shape_ok(int n_w, long n_t, int n_d, long ldw, const double *x) {
    return n_w >= 1 && n_t >= 1 && n_d >= 1 && x && ldw >= n_t * (long)n_d && (long)n_w * n_d < (1L << 35);
}

extern "C" int bfhip_acor_moments(bfhip_ctx *ctx, int n_w, long n_t, int n_d, long ldw, const double *x, double *mean, double *inv) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || !ac_shape_ok(n_w, n_t, n_d, ldw, x) || !mean || !inv)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_acor_moments: invalid argument");
    const long nb = ((long)n_w * n_d + 15) / 16;
    if (nb > 0x7fffffffL) return bf_set_error(BFHIP_ERR_ARG, "bfhip_acor_moments: too many series");
    hipLaunchKernelGGL(bf_acor_moments_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, n_w, n_t, n_d, ldw, x, mean, inv);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

extern "C" int bfhip_acor_lag_sums(bfhip_ctx *ctx, int n_w, long n_t, int n_d, long ldw, const double *x, const double *mean,
                                   const double *inv, long t0, int n_lag, double *work, double *out) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || !ac_shape_ok(n_w, n_t, n_d, ldw, x) || !mean || !inv || t0 < 0 || n_lag < 1 || !work || !out)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_acor_lag_sums: invalid argument");
    const int ltd = ac_log_td(n_d);
    const long n_tiles_d = ((long)n_d + (1 << ltd) - 1) >> ltd, n_tiles_l = ((long)n_lag + AC_LAGS - 1) / AC_LAGS;
    if (n_tiles_d > 65535 || n_tiles_l > 65535) return bf_set_error(BFHIP_ERR_ARG, "bfhip_acor_lag_sums: n_d or n_lag too large");
    int wpg, n_g;
    ac_groups(n_w, &wpg, &n_g);
    // the A buffer is needed unless the launch's only lag tile starts at lag 0
    const size_t lds = (size_t)AC_SLOTS * (AC_SB + ((t0 == 0 && n_tiles_l == 1) ? 0 : AC_SA)) * sizeof(double);
    if (int rc = bf_set_lds(bf_acor_lag_kernel, lds)) return rc;
    const long n_out = (long)n_lag * n_d;
    hipLaunchKernelGGL(bf_acor_lag_kernel, dim3(n_g, (unsigned)n_tiles_d, (unsigned)n_tiles_l), dim3(AC_TH), lds, ctx->stream, n_w, n_t,
                       n_d, ldw, x, mean, inv, t0, n_lag, ltd, wpg, work);
    hipLaunchKernelGGL(bf_acor_reduce_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, ctx->stream, n_g, n_out, work, out);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
