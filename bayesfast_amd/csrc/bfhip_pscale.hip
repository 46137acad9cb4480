// bfhip_pscale.hip -- the distance between two weighted ECDFs of one parameter, for a batch of 16 columns of weights at once
// (bayesfast_amd/utils/power_scale.py has the definitions; bfhip_rw_weights, which writes such columns, is csrc/bfhip_pscale.h):
//
//   bfhip_pscale_cjs   J = sum h [P log2(P / M) + Q log2(Q / M)], bound = sum h (P + Q), cjs = sqrt(J / bound), ks = max |P - Q|
//
// over the sorted positions of the parameter (bfhip_diag_sort's keys and permutation), P and Q the running sums of the base weights w
// and of a column of u.  A multi-column gather-scan over the permutation: a workgroup's tile is PSC_TILE consecutive sorted positions,
// thread (slice sl, column b) walks the PSC_RUN consecutive positions of its slice, so that the sixteen lanes of a slice read the 128
// contiguous bytes of one row of u together and a wave four such rows -- the indexed-row gather with small rows.  Seventeen running
// sums: w (every lane of a slice carries it, they read the same address) and the sixteen columns of u - w, the numerator of
// t = (Q - P) / (P + Q) -- scanned as such, since Q - P of two scans cancels.
//
//   psc_sums_kernel     per tile and slice the 17 sums; slice 0 folds the slices in order into the tile's sums
//   psc_offsets_kernel  ONE workgroup: the tiles' sums -> the sum of the tiles in front of each (16 slices of consecutive tiles: a
//                       slice's total, the slices in front folded in order, then the running sum written back)
//   psc_terms_kernel    every position forms P, t and h (decoded from the keys) and adds its terms; per tile J, bound and ks
//   psc_finish_kernel   ONE workgroup: the tiles' partial results, slice sl the tiles sl, sl + 16, ..., the slices folded in order
//
// No workgroup waits on another, nothing is atomic, every order is set by n alone and lane b sees column b alone: a column's figures
// are the same bits in any slot of any batch.  Bound by the two gathers of n rows of u (128 bytes) with w and the keys.
#include "bfhip_block.h"

#define PSC_T 256
#define PSC_B BFHIP_DIAG_BATCH
#define PSC_TILE BFHIP_PSCALE_TILE
#define PSC_RUN (PSC_TILE / BF_SLICES)       // consecutive sorted positions per thread
#define PSC_TS 32                            // doubles per tile of the tile sums: 16 columns of u - w, w, then the offset of w
#define PSC_SS (BF_SLICES * (PSC_B + 1))     // ... of the slice sums: slice i, column c at i * 17 + c, w at c = 16
#define PSC_PS (3 * PSC_B)                   // ... of the partial results: J, bound, ks
static_assert(PSC_B == 16 && PSC_T == PSC_B * BF_SLICES, "a workgroup is 16 slices x 16 columns");
static_assert(PSC_TS + PSC_SS + PSC_PS == BFHIP_PSCALE_TILE_WORK, "the work buffer's doubles per tile");

struct PscWork {
    double *tsum, *ssum, *part;
};
static PscWork psc_work(double *work, long n_tile) {
    return {work, work + (size_t)n_tile * PSC_TS, work + (size_t)n_tile * (PSC_TS + PSC_SS)};
}

__device__ inline long psc_npos(long n, const double *wsum) {
    const double cnt = wsum[2];
    return cnt >= 1. && cnt <= (double)n ? (long)cnt : 0;
}

// (1 - t) log1p(-t) + (1 + t) log1p(t) = sum_k t^(2k) / (k (2k - 1)): nine terms below |t| = 1/8 (the tenth is below 4e-19 of the first)
__device__ inline double psc_f(double t) {
    if (fabs(t) < 0.125) {
        const double s = t * t;
        double v = 1. / 153.;
        v = v * s + 1. / 120.;
        v = v * s + 1. / 91.;
        v = v * s + 1. / 66.;
        v = v * s + 1. / 45.;
        v = v * s + 1. / 28.;
        v = v * s + 1. / 15.;
        v = v * s + 1. / 6.;
        v = v * s + 1.;
        return v * s;
    }
    const double a = 1. - t, b = 1. + t;
    return (a == 0. ? 0. : a * log1p(-t)) + (b == 0. ? 0. : b * log1p(t));   // 0 log 0 = 0; a NaN stays one
}

// the row of sorted position p and its weights; positions beyond the sample weigh nothing (every load is in bounds whatever p is)
__device__ inline void psc_load(long n, long np, long p, const uint32_t *__restrict__ order, const double *__restrict__ w,
                                const double *__restrict__ u, long ld_u, int b, bool col_on, double &wv, double &dv) {
    const long pc = p < n ? p : n - 1;
    long row = order[pc];
    row = row < n ? row : n - 1;   // (a permutation of 0 .. n - 1: nothing is read through an index that is no row)
    const double wr = w[row], ur = u[row * ld_u + (col_on ? b : 0)];
    const bool on = p < np;
    wv = on ? wr : 0.;
    dv = on && col_on ? ur - wr : 0.;
}

__global__ __launch_bounds__(PSC_T) void psc_sums_kernel(long n, const uint32_t *__restrict__ order, const double *__restrict__ wsum,
                                                        const double *__restrict__ w, const double *__restrict__ u, long ld_u, int nb,
                                                        double *__restrict__ tsum, double *__restrict__ ssum) {
    __shared__ double rd[PSC_T], rw[BF_SLICES];
    const int b = threadIdx.x & (PSC_B - 1), sl = threadIdx.x / PSC_B;
    const long np = psc_npos(n, wsum), p0 = (long)blockIdx.x * PSC_TILE + (long)sl * PSC_RUN;
    double sw = 0., sd = 0.;
    if (p0 < np) {
#pragma unroll 4
        for (int e = 0; e < PSC_RUN; ++e) {
            double wv, dv;
            psc_load(n, np, p0 + e, order, w, u, ld_u, b, b < nb, wv, dv);
            sw += wv;
            sd += dv;
        }
    }
    double *ss = ssum + (size_t)blockIdx.x * PSC_SS + sl * (PSC_B + 1);
    ss[b] = sd;
    if (b == 0) ss[PSC_B] = rw[sl] = sw;
    rd[threadIdx.x] = sd;
    __syncthreads();
    if (sl != 0) return;
    tsum[(size_t)blockIdx.x * PSC_TS + b] = bf_slice_fold(sd, 1, rd, b, BfSum());
    if (b == 0) {
        for (int i = 1; i < BF_SLICES; ++i) sw += rw[i];
        tsum[(size_t)blockIdx.x * PSC_TS + PSC_B] = sw;
    }
}

__global__ __launch_bounds__(PSC_T) void psc_offsets_kernel(long n_tile, double *__restrict__ tsum) {
    __shared__ double rd[PSC_T], rw[BF_SLICES];
    const int b = threadIdx.x & (PSC_B - 1), sl = threadIdx.x / PSC_B;
    const long per = (n_tile + BF_SLICES - 1) / BF_SLICES, t0 = sl * per, t1 = t0 + per < n_tile ? t0 + per : n_tile;
    double sd = 0., sw = 0.;
    for (long t = t0; t < t1; ++t) {
        sd += tsum[(size_t)t * PSC_TS + b];
        sw += tsum[(size_t)t * PSC_TS + PSC_B];
    }
    rd[threadIdx.x] = sd;
    if (b == 0) rw[sl] = sw;
    __syncthreads();
    sd = sw = 0.;
    for (int i = 0; i < sl; ++i) {   // the slices in front, in order
        sd += rd[i * PSC_B + b];
        sw += rw[i];
    }
    for (long t = t0; t < t1; ++t) {   // (a lane writes what it alone reads: the w offsets go to a slot of their own)
        const double vd = tsum[(size_t)t * PSC_TS + b], vw = tsum[(size_t)t * PSC_TS + PSC_B];
        tsum[(size_t)t * PSC_TS + b] = sd;
        if (b == 0) tsum[(size_t)t * PSC_TS + PSC_B + 1] = sw;
        sd += vd;
        sw += vw;
    }
}

__global__ __launch_bounds__(PSC_T) void psc_terms_kernel(long n, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ order,
                                                         const double *__restrict__ wsum, const double *__restrict__ w,
                                                         const double *__restrict__ u, long ld_u, int nb, const double *__restrict__ tsum,
                                                         const double *__restrict__ ssum, double *__restrict__ part) {
    __shared__ double rj[PSC_T], rb[PSC_T], rk[PSC_T];
    const int b = threadIdx.x & (PSC_B - 1), sl = threadIdx.x / PSC_B;
    const long np = psc_npos(n, wsum), p0 = (long)blockIdx.x * PSC_TILE + (long)sl * PSC_RUN;
    double accj = 0., accb = 0., acck = 0.;
    if (p0 + 1 < np) {   // (the last position of the sample closes no bin)
        double P = tsum[(size_t)blockIdx.x * PSC_TS + PSC_B + 1], D = tsum[(size_t)blockIdx.x * PSC_TS + b];
        const double *ss = ssum + (size_t)blockIdx.x * PSC_SS;
        for (int i = 0; i < sl; ++i) {
            P += ss[i * (PSC_B + 1) + PSC_B];
            D += ss[i * (PSC_B + 1) + b];
        }
#pragma unroll 4
        for (int e = 0; e < PSC_RUN; ++e) {
            const long p = p0 + e;
            double wv, dv;
            psc_load(n, np, p, order, w, u, ld_u, b, b < nb, wv, dv);
            const long pa = p < n ? p : n - 1, pb = p + 1 < n ? p + 1 : n - 1;
            const double h = bf_order_value(keys[pb]) - bf_order_value(keys[pa]);
            P += wv;
            D += dv;
            if (p + 1 < np) {
                const double S = P + (P + D);   // P + Q
                double t = D / S;
                if (t > 1.) t = 1.;             // (Q a rounding below 0; a NaN passes)
                if (t < -1.) t = -1.;
                accb += h * S;
                accj += h * ((0.5 * S) * psc_f(t));
                if (h > 0.) acck = fmax(acck, fabs(D));
            }
        }
    }
    rj[threadIdx.x] = accj;
    rb[threadIdx.x] = accb;
    rk[threadIdx.x] = acck;
    __syncthreads();
    if (sl != 0) return;
    double *pt = part + (size_t)blockIdx.x * PSC_PS;
    pt[b] = bf_slice_fold(accj, 1, rj, b, BfSum());
    pt[PSC_B + b] = bf_slice_fold(accb, 1, rb, b, BfSum());
    pt[2 * PSC_B + b] = bf_slice_fold(acck, 1, rk, b, BfMax());
}

__global__ __launch_bounds__(PSC_T) void psc_finish_kernel(long n, long n_tile, const uint64_t *__restrict__ keys, const double *__restrict__ wsum,
                                                          int nb, const double *__restrict__ part, double *__restrict__ out) {
    __shared__ double rj[PSC_T], rb[PSC_T], rk[PSC_T];
    const int b = threadIdx.x & (PSC_B - 1), sl = threadIdx.x / PSC_B;
    double accj = 0., accb = 0., acck = 0.;
    for (long t = sl; t < n_tile; t += BF_SLICES) {
        const double *pt = part + (size_t)t * PSC_PS;
        accj += pt[b];
        accb += pt[PSC_B + b];
        acck = fmax(acck, pt[2 * PSC_B + b]);
    }
    rj[threadIdx.x] = accj;
    rb[threadIdx.x] = accb;
    rk[threadIdx.x] = acck;
    __syncthreads();
    if (sl != 0 || b >= nb) return;
    const double J = bf_slice_fold(accj, 1, rj, b, BfSum()) * 1.4426950408889634074;   // / ln 2
    const double bound = bf_slice_fold(accb, 1, rb, b, BfSum());
    const double ks = bf_slice_fold(acck, 1, rk, b, BfMax());
    const long np = psc_npos(n, wsum);
    int flags = 0;
    if (np >= 1) {
        const double lo = bf_order_value(keys[0]), hi = bf_order_value(keys[np - 1]);
        if (!(fabs(lo) < __builtin_inf()) || !(fabs(hi) < __builtin_inf())) flags |= 1;
    }
    if (!(flags & 1) && bound == 0.) flags |= 2;
    const double nan = __builtin_nan("");
    out[BFHIP_CJS_J * PSC_B + b] = (flags & 1) ? nan : J;
    out[BFHIP_CJS_BOUND * PSC_B + b] = (flags & 1) ? nan : bound;
    out[BFHIP_CJS_CJS * PSC_B + b] = flags ? nan : sqrt(J / bound);
    out[BFHIP_CJS_KS * PSC_B + b] = flags || J != J ? nan : ks;
    out[BFHIP_CJS_FLAGS * PSC_B + b] = (double)flags;
}

extern "C" int bfhip_pscale_cjs(bfhip_ctx *ctx, long n, const uint64_t *keys_sorted, const uint32_t *order, const double *wsum,
                                const double *w, const double *u, long ld_u, int nb, double *out, double *work) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n < 1 || !keys_sorted || !order || !wsum || !w || !u || nb < 1 || nb > PSC_B || ld_u < nb || !out || !work)
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_pscale_cjs: invalid argument");
    if (n > 0x7fffffffL) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_pscale_cjs: more than 2^31-1 rows");
    const long n_tile = (n + PSC_TILE - 1) / PSC_TILE;   // <= 2^20: a grid dimension
    const PscWork pw = psc_work(work, n_tile);
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(psc_sums_kernel, dim3((unsigned)n_tile), dim3(PSC_T), 0, st, n, order, wsum, w, u, ld_u, nb, pw.tsum, pw.ssum);
    hipLaunchKernelGGL(psc_offsets_kernel, dim3(1), dim3(PSC_T), 0, st, n_tile, pw.tsum);
    hipLaunchKernelGGL(psc_terms_kernel, dim3((unsigned)n_tile), dim3(PSC_T), 0, st, n, keys_sorted, order, wsum, w, u, ld_u, nb,
                       (const double *)pw.tsum, (const double *)pw.ssum, pw.part);
    hipLaunchKernelGGL(psc_finish_kernel, dim3(1), dim3(PSC_T), 0, st, n, n_tile, keys_sorted, wsum, nb, (const double *)pw.part, out);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
