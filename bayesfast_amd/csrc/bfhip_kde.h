// bfhip_kde.h -- the pairwise sum of the multivariate kernel density estimate (bfhip_kde_logsum):
//     out[i] = log sum_j exp(logw[j] - |zq_i - z_j|^2 / 2)
// for m whitened queries against n whitened data rows, a true log-sum-exp in float64.
//
//   kd_rows_kernel     c_j = logw_j - |z_j|^2 / 2 per data row (-inf: the row is no part of the sample; NaN: the row or its
//                      weight is not usable, which poisons every output)
//   kd_tile_kernel     workgroup (p, b): data part p against the 64 queries of block b, one 16-query tile per wave.  The
//                      exponent of pair (i, j) is c_j + zq_i . z_j - |zq_i|^2 / 2; the dot products of a 16 x 16 tile are
//                      NS k-steps of v_mfma_f64_16x16x4_f64 with the queries as rows (A) and the data rows as columns (B),
//                      both read as pldh_gram_tile reads G: lane l of k-step s holds [l & 15][4 s + (l >> 4)].
//   kd_merge_kernel    the parts' (maximum, scaled sum) pairs of a query, merged in increasing p.
//
// The log-sum-exp RESCALES A RUNNING MAXIMUM: a lane owns rows 4 r + (l >> 4), r < 4, of column l & 15 of every tile and keeps,
// per row, the largest exponent M it has met and S = sum exp(t - M).  A new term costs ONE exponential either way
// (e = exp(-|t - M|), then S = S e + 1 or S = S + e), which is what the alternative -- a first pass for the smallest energy --
// also pays per pair, on top of a second round of dot products.  The sixteen columns' pairs are merged once, after the lane's
// stream, by a butterfly over l & 15 whose result is read from column 0.
//
// Partition: kd_plan(n) cuts the data rows into P <= KD_PMAX parts of R rows, R a multiple of 16 -- a function of n alone, so
// one query (the density at zero) still gives P workgroups, and every sum (a lane's stream within a part, the butterfly, the
// merge over p) has an order fixed by (n, d).  A query's result depends on its row and the data only: the same bits alone, in
// any batch, at any offset.  No atomics.
#pragma once
#include "bfhip_common.h"
#include <math.h>

#define KD_T 256            // threads of a tile workgroup: four waves, one query tile each
#define KD_QB 64            // queries of a workgroup
#define KD_MINROWS 256      // data rows of a part, at least
#define KD_PMAX 256         // parts, at most
#define KD_MCHUNK 8192      // queries of one launch (the partials of a launch: KD_PMAX x KD_MCHUNK pairs)

typedef double kd_d4 __attribute__((ext_vector_type(4)));

struct KdPlan { int P; long R; };   // part p holds rows [p R, min(n, (p + 1) R))
static inline KdPlan kd_plan(long n) {
    long P = (n + KD_MINROWS - 1) / KD_MINROWS;
    if (P > KD_PMAX) P = KD_PMAX;
    long R = (n + P - 1) / P;
    R = (R + 15) / 16 * 16;
    return {(int)((n + R - 1) / R), R};
}

// the k-step classes the tile kernel is compiled for: the smallest that holds ceil(d / 4) (zero k-steps change no bit)
static inline int kd_steps(int d) {
    const int ns = (d + 3) / 4;
    const int cls[] = {1, 2, 4, 8, 12, 16, 24, 32};
    for (int c : cls)
        if (ns <= c) return c;
    return 32;
}
// row stride of a staged tile in doubles: = 2 mod 32, so that the 32 lanes of one LDS pass (16 rows x 2 columns) meet 32 banks
__host__ __device__ constexpr int kd_ld(int NS) { return (4 * NS + 29) / 32 * 32 + 2; }

struct KdWork {
    double *c;         // n
    double2 *part;     // P x min(m, KD_MCHUNK)
    size_t bytes;
};
static KdWork kd_work(void *work, long n, long m) {
    char *p = (char *)work;
    KdWork w;
    auto take = [&](size_t bytes) { char *q = p; p += (bytes + 255) / 256 * 256; return (void *)q; };
    w.c = (double *)take(sizeof(double) * (size_t)n);
    w.part = (double2 *)take(sizeof(double2) * (size_t)kd_plan(n).P * (size_t)(m < KD_MCHUNK ? m : KD_MCHUNK));
    w.bytes = (size_t)(p - (char *)work);
    return w;
}

__global__ __launch_bounds__(KD_T) void kd_rows_kernel(int d, long n, const double *__restrict__ z, long ldz,
                                                      const double *__restrict__ logw, double *__restrict__ c) {
    const long j = (long)blockIdx.x * KD_T + threadIdx.x;
    if (j >= n) return;
    const double lw = logw ? logw[j] : 0.;
    double v;
    if (lw == -INFINITY) v = -INFINITY;
    else if (!(lw < INFINITY)) v = NAN;     // NaN or +inf
    else {
        const double *r = z + (size_t)j * ldz;
        double s = 0.;
        for (int k = 0; k < d; ++k) s = fma(r[k], r[k], s);
        v = s < INFINITY ? lw - 0.5 * s : NAN;   // a NaN or an infinity in the row
    }
    c[j] = v;
}

// one more term t for the pair (M, S)
__device__ inline void kd_add(double &M, double &S, double t) {
    const double e = t == -INFINITY ? 0. : exp(-fabs(t - M));
    if (t > M) {
        S = fma(S, e, 1.);
        M = t;
    } else
        S += e;       // a NaN term lands here and stays
}
// (M, S) += (M2, S2)
__device__ inline void kd_join(double &M, double &S, double M2, double S2) {
    const double Mn = M2 > M ? M2 : M;
    const double e1 = M == -INFINITY ? 0. : exp(M - Mn), e2 = M2 == -INFINITY ? 0. : exp(M2 - Mn);
    S = S * e1 + S2 * e2;
    M = Mn;
}

template <int NS>
__global__ __launch_bounds__(KD_T) void kd_tile_kernel(int d, long n, const double *__restrict__ z, long ldz, const double *__restrict__ c,
                                                      long m, const double *__restrict__ zq, long ldq, long q0, long mc, int exclude_self,
                                                      long R, double2 *__restrict__ part) {
    constexpr int LD = kd_ld(NS), DP = 4 * NS, NL = (16 * DP + KD_T - 1) / KD_T;
    __shared__ double zs[2][16 * LD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ci = lane & 15, kr = lane >> 4;
    const long lo = (long)blockIdx.x * R, hi = lo + R < n ? lo + R : n;
    const long qt = q0 + (long)blockIdx.y * KD_QB + 16 * wv;      // the wave's first query

    // the wave's queries: A[i = ci][k = kr] of k-step s, and |zq_i|^2 / 2 of the lane's four result rows
    double a[NS];
    {
        const long i = qt + ci;
        const double *r = zq + (size_t)(i < m ? i : 0) * ldq;
#pragma unroll
        for (int s = 0; s < NS; ++s) a[s] = (i < m && 4 * s + kr < d) ? r[4 * s + kr] : 0.;
    }
    double qh[4];
    {
        double s2 = 0.;
#pragma unroll
        for (int s = 0; s < NS; ++s) s2 = fma(a[s], a[s], s2);
        const double p0 = __shfl(s2, ci, 64), p1 = __shfl(s2, ci + 16, 64), p2 = __shfl(s2, ci + 32, 64), p3 = __shfl(s2, ci + 48, 64);
        const double h = 0.5 * ((p0 + p1) + (p2 + p3));          // row ci, in every lane of that row
#pragma unroll
        for (int r = 0; r < 4; ++r) qh[r] = __shfl(h, 4 * r + kr, 64);
    }

    // staging: element e = tid + KD_T k of the 16 x DP tile; rows past the part, rows of weight -inf and columns past d are zero
    double pre[NL];
    auto fetch = [&](long j0) {
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            const int e = tid + KD_T * k, row = e / DP, col = e % DP;
            const long j = j0 + row;
            double v = 0.;
            if (e < 16 * DP && j < hi && col < d && c[j] != -INFINITY) v = z[(size_t)j * ldz + col];
            pre[k] = v;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int k = 0; k < NL; ++k) {
            const int e = tid + KD_T * k;
            if (e < 16 * DP) zs[buf][(e / DP) * LD + e % DP] = pre[k];
        }
    };

    double M[4], S[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { M[r] = -INFINITY; S[r] = 0.; }

    fetch(lo);
    stage(0);
    __syncthreads();
    int buf = 0;
    for (long j0 = lo; j0 < hi; j0 += 16, buf ^= 1) {
        const bool more = j0 + 16 < hi;
        if (more) fetch(j0 + 16);
        const long j = j0 + ci;
        const double cj = j < hi ? c[j] : -INFINITY;
        kd_d4 acc = {0., 0., 0., 0.};
        const double *bp = &zs[buf][ci * LD + kr];
#pragma unroll
        for (int s = 0; s < NS; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], bp[4 * s], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            double t = cj + acc[r];
            if (exclude_self && qt + 4 * r + kr == j) t = -INFINITY;
            kd_add(M[r], S[r], t);
        }
        if (more) stage(buf ^ 1);
        __syncthreads();
    }

    // the sixteen columns of a row, then the query's norm
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
        for (int k = 1; k < 16; k <<= 1) {
            const double M2 = __shfl_xor(M[r], k, 64), S2 = __shfl_xor(S[r], k, 64);
            kd_join(M[r], S[r], M2, S2);
        }
        const long i = qt + 4 * r + kr;
        if (ci == 0 && i < m && i < q0 + mc) part[(size_t)blockIdx.x * mc + (i - q0)] = make_double2(M[r] - qh[r], S[r]);
    }
}

__global__ __launch_bounds__(KD_T) void kd_merge_kernel(int P, long mc, const double2 *__restrict__ part, double *__restrict__ out) {
    const long i = (long)blockIdx.x * KD_T + threadIdx.x;
    if (i >= mc) return;
    double Mt = -INFINITY;
    for (int p = 0; p < P; ++p) {
        const double v = part[(size_t)p * mc + i].x;
        if (v > Mt) Mt = v;
    }
    double s = 0.;
    for (int p = 0; p < P; ++p) {
        const double2 v = part[(size_t)p * mc + i];
        s += v.y * (v.x == -INFINITY ? 0. : exp(v.x - Mt));     // a NaN maximum or sum stays NaN
    }
    out[i] = Mt + log(s);
}
