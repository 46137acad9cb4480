// bfhip_kde.h -- the pairwise sum of the multivariate kernel density estimate (bfhip_kde_logsum):
//     out[i] = log sum_j exp(logw[j] - |zq_i - z_j|^2 / 2)
// for m whitened queries against n whitened data rows, a true log-sum-exp in float64.  The second half of the file is
// bfhip_kde_wmean, the kernel-weighted means of a per-row matrix v over the same pairs (its own comment is there).
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

// ---- kernel-weighted means (bfhip_kde_wmean) ------------------------------------------------------------------------------------------
//     mean[i][c] = sum_j p_ij v[j][c],   p_ij = exp(t_ij) / sum_j' exp(t_ij'),   t_ij = c_j + zq_i . z_j - |zq_i|^2 / 2,
// and the log-sum-exp of the t_ij beside it, in ONE pass over the pairs: the second product of an attention kernel.
//
//   kd_wm_tile_kernel   workgroup (p, b) as kd_tile_kernel, but the energy tile is taken TRANSPOSED: the staged data rows are the
//                       A operand and the wave's 16 queries (in registers) the B operand of v_mfma_f64_16x16x4_f64, the LDS read
//                       address unchanged.  Lane l then holds t[data 4 r + (l >> 4)][query l & 15] in acc[r], and after the
//                       exponential p[r] IS the A operand (row l & 15 = query, k = l >> 4 = data row within k-step r) of k-step r
//                       of the second product P (16 queries x 16 data) . V (16 data x 16 columns): P never leaves its registers.
//                       V's tile is staged in LDS beside z's (row stride = 16 mod 32 doubles); with v == z the z tile is the V
//                       tile.  The result tile o[cb][r] holds [query 4 r + (l >> 4)][column 16 cb + (l & 15)].
//   kd_wm_merge_kernel  a wave per query: the largest of the parts' maxima, the parts' factors exp(M_p - M) once (in LDS), then
//                       the denominator and every column's numerator summed in increasing p.
//
// Running maximum, per query: a tile's maximum for query l & 15 is the lane's four terms joined over the four l >> 4 groups
// (two xor shuffles), so M is the same number in the four lanes of a query.  Where it rises, S and the numerators of that query
// are scaled by f = exp(M_old - M_new); the numerators of query 4 r + (l >> 4) live in other lanes than its M, so f is fetched by
// one shuffle per r.  f is exactly 1 where M did not move, so the whole step is skipped when no lane of the wave moved.
//
// The denominator is NOT a column of ones in V: S = S f + ((p0 + p1) + (p2 + p3)) in the lane that owns the four terms needs no
// shuffle for its rescaling and no seventeenth column (a whole extra column block at k = 16, 32, 64, 128); the four l >> 4
// groups' sums are joined once after the part, (S0 + S1) + (S2 + S3).
//
// Partials: (M - |zq|^2 / 2, S, k numerators) per (part, query), k + 2 doubles.  The queries of a launch shrink from KD_MCHUNK
// until P x chunk x (k + 2) doubles fit KD_WM_BUDGET (a multiple of 64, at least 64: at most 64 x 256 x 130 x 8 = 17 MB); the
// chunk decides which launch a query belongs to and nothing else.  Every order of summation is fixed by (n, d, k).  No atomics.
#define KD_WM_BUDGET ((size_t)1 << 26)     // bytes of partials of one launch

// row stride of a staged V tile in doubles: = 16 mod 32, so that the 32 lanes of one LDS pass (2 rows x 16 columns) meet 32 banks
__host__ __device__ constexpr int kd_ldv(int CB) { return CB % 2 ? 16 * CB : 16 * CB + 16; }
// column blocks of 16: with v == z the z tile's own columns, ceil(4 NS / 16); otherwise the class that holds ceil(k / 16)
__host__ __device__ constexpr int kd_wm_same_blocks(int NS) { return (NS + 3) / 4; }
static inline int kd_wm_blocks(int k) {
    const int cb = (k + 15) / 16;
    return cb <= 1 ? 1 : cb <= 2 ? 2 : cb <= 4 ? 4 : 8;
}
static inline long kd_wm_chunk(long n, int k) {
    long mc = (long)(KD_WM_BUDGET / (sizeof(double) * (size_t)kd_plan(n).P * (size_t)(k + 2))) / KD_QB * KD_QB;
    return mc > KD_MCHUNK ? KD_MCHUNK : mc < KD_QB ? KD_QB : mc;
}
static inline size_t kd_wm_lds(int ns, int cb, bool same) {
    return sizeof(double) * (size_t)(2 * 16 * kd_ld(ns) + (same ? 0 : 2 * 16 * kd_ldv(cb)) + 2 * 16);
}

struct KdWmWork {
    double *c;         // n
    double *part;      // P x min(m, chunk) x (k + 2)
    size_t bytes;
};
static KdWmWork kd_wm_work(void *work, long n, long m, int k) {
    char *p = (char *)work;
    KdWmWork w;
    auto take = [&](size_t bytes) { char *q = p; p += (bytes + 255) / 256 * 256; return (void *)q; };
    const long mc = kd_wm_chunk(n, k);
    w.c = (double *)take(sizeof(double) * (size_t)n);
    w.part = (double *)take(sizeof(double) * (size_t)kd_plan(n).P * (size_t)(m < mc ? m : mc) * (size_t)(k + 2));
    w.bytes = (size_t)(p - (char *)work);
    return w;
}

template <int NS, int CB, bool SAME>
__global__ __launch_bounds__(KD_T) void kd_wm_tile_kernel(int d, long n, const double *z, long ldz, const double *__restrict__ c, int k,
                                                         const double *v, long ldv, long m, const double *zq, long ldq, long q0, long mc,
                                                         int exclude_self, long R, double *__restrict__ part) {
    constexpr int LD = kd_ld(NS), DP = 4 * NS, NL = (16 * DP + KD_T - 1) / KD_T, LDV = SAME ? LD : kd_ldv(CB), VP = 16 * CB;
    constexpr int NV = SAME ? 1 : CB;      // 16 x VP elements over KD_T threads
    extern __shared__ double kd_wm_lds_buf[];
    double *zs = kd_wm_lds_buf;                                  // [2][16 LD]
    double *vs = SAME ? zs : zs + 2 * 16 * LD;                   // [2][16 LDV]
    double *cs = zs + 2 * 16 * LD + (SAME ? 0 : 2 * 16 * LDV);   // [2][16]
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ci = lane & 15, kr = lane >> 4, KS = k + 2;
    const long lo = (long)blockIdx.x * R, hi = lo + R < n ? lo + R : n;
    const long qt = q0 + (long)blockIdx.y * KD_QB + 16 * wv;      // the wave's first query

    // the wave's queries: B[k = kr][j = ci] of k-step s, and |zq|^2 / 2 of query ci
    double b[NS];
    {
        const long i = qt + ci;
        const double *r = zq + (size_t)(i < m ? i : 0) * ldq;
#pragma unroll
        for (int s = 0; s < NS; ++s) b[s] = (i < m && 4 * s + kr < d) ? r[4 * s + kr] : 0.;
    }
    double qh;
    {
        double s2 = 0.;
#pragma unroll
        for (int s = 0; s < NS; ++s) s2 = fma(b[s], b[s], s2);
        const double p0 = __shfl(s2, ci, 64), p1 = __shfl(s2, ci + 16, 64), p2 = __shfl(s2, ci + 32, 64), p3 = __shfl(s2, ci + 48, 64);
        qh = 0.5 * ((p0 + p1) + (p2 + p3));
    }

    // staging as in kd_tile_kernel; V's tile has columns past k zero, and the tile's c_j go to LDS too (a lane needs four of them)
    double pre[NL], prv[NV], prc = -INFINITY;
    auto fetch = [&](long j0) {
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            const int e = tid + KD_T * q, row = e / DP, col = e % DP;
            const long j = j0 + row;
            double x = 0.;
            if (e < 16 * DP && j < hi && col < d && c[j] != -INFINITY) x = z[(size_t)j * ldz + col];
            pre[q] = x;
        }
        if (!SAME) {
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const int e = tid + KD_T * q, row = e / VP, col = e % VP;
                const long j = j0 + row;
                double x = 0.;
                if (j < hi && col < k && c[j] != -INFINITY) x = v[(size_t)j * ldv + col];
                prv[q] = x;
            }
        }
        if (tid < 16) prc = j0 + tid < hi ? c[j0 + tid] : -INFINITY;
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int q = 0; q < NL; ++q) {
            const int e = tid + KD_T * q;
            if (e < 16 * DP) zs[buf * 16 * LD + (e / DP) * LD + e % DP] = pre[q];
        }
        if (!SAME) {
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                const int e = tid + KD_T * q;
                vs[buf * 16 * LDV + (e / VP) * LDV + e % VP] = prv[q];
            }
        }
        if (tid < 16) cs[buf * 16 + tid] = prc;
    };

    double M = -INFINITY, S = 0.;
    kd_d4 o[CB];
#pragma unroll
    for (int cb = 0; cb < CB; ++cb) o[cb] = kd_d4{0., 0., 0., 0.};

    fetch(lo);
    stage(0);
    __syncthreads();
    int buf = 0;
    for (long j0 = lo; j0 < hi; j0 += 16, buf ^= 1) {
        const bool more = j0 + 16 < hi;
        if (more) fetch(j0 + 16);
        kd_d4 acc = {0., 0., 0., 0.};
        const double *ap = &zs[buf * 16 * LD + ci * LD + kr];
#pragma unroll
        for (int s = 0; s < NS; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ap[4 * s], b[s], acc, 0, 0, 0);
        double t[4], tm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            t[r] = cs[buf * 16 + 4 * r + kr] + acc[r];
            if (exclude_self && qt + ci == j0 + 4 * r + kr) t[r] = -INFINITY;
            if (t[r] > tm) tm = t[r];          // a NaN term is no maximum; it reaches S and the numerators through exp
        }
        {
            const double t1 = __shfl_xor(tm, 16, 64);
            if (t1 > tm) tm = t1;
            const double t2 = __shfl_xor(tm, 32, 64);
            if (t2 > tm) tm = t2;
        }
        if (__any(tm > M)) {
            const double Mn = tm > M ? tm : M;
            const double f = M == -INFINITY ? 0. : exp(M - Mn);      // exactly 1 where M stays
            S *= f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double fr = __shfl(f, 4 * r + kr, 64);
#pragma unroll
                for (int cb = 0; cb < CB; ++cb) o[cb][r] *= fr;
            }
            M = Mn;
        }
        double p[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) p[r] = t[r] == -INFINITY ? 0. : exp(t[r] - M);
        S += (p[0] + p[1]) + (p[2] + p[3]);
        const double *vp = &vs[buf * 16 * LDV + kr * LDV + ci];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int cb = 0; cb < CB; ++cb) o[cb] = __builtin_amdgcn_mfma_f64_16x16x4f64(p[r], vp[4 * r * LDV + 16 * cb], o[cb], 0, 0, 0);
        if (more) stage(buf ^ 1);
        __syncthreads();
    }

    // the four data groups' denominators of query ci, then the partial rows
    {
        const double s0 = __shfl(S, ci, 64), s1 = __shfl(S, ci + 16, 64), s2 = __shfl(S, ci + 32, 64), s3 = __shfl(S, ci + 48, 64);
        const long i = qt + ci;
        if (kr == 0 && i < m && i < q0 + mc) {
            double *row = part + ((size_t)blockIdx.x * mc + (i - q0)) * KS;
            row[0] = M - qh;
            row[1] = (s0 + s1) + (s2 + s3);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long i = qt + 4 * r + kr;
        if (i < m && i < q0 + mc) {
            double *row = part + ((size_t)blockIdx.x * mc + (i - q0)) * KS + 2;
#pragma unroll
            for (int cb = 0; cb < CB; ++cb)
                if (16 * cb + ci < k) row[16 * cb + ci] = o[cb][r];
        }
    }
}

__global__ __launch_bounds__(KD_T) void kd_wm_merge_kernel(int P, long mc, int k, const double *__restrict__ part, double *__restrict__ logsum,
                                                          double *__restrict__ mean, long ldo) {
    __shared__ double es[KD_T / 64][KD_PMAX];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, KS = k + 2;
    const long i = (long)blockIdx.x * (KD_T / 64) + wv;
    const bool live = i < mc;                    // the same in every lane of a wave
    const double *row = part + (size_t)(live ? i : 0) * KS;
    const size_t step = (size_t)mc * KS;
    double Mt = -INFINITY;
    for (int p = lane; p < P; p += 64) {
        const double x = row[p * step];
        if (x > Mt) Mt = x;
    }
#pragma unroll
    for (int q = 1; q < 64; q <<= 1) {
        const double x = __shfl_xor(Mt, q, 64);
        if (x > Mt) Mt = x;
    }
    for (int p = lane; p < P; p += 64) {
        const double x = row[p * step];
        es[wv][p] = x == -INFINITY ? 0. : exp(x - Mt);
    }
    __syncthreads();
    if (!live) return;
    double s = 0.;
    for (int p = 0; p < P; ++p) s = fma(es[wv][p], row[p * step + 1], s);      // a NaN sum stays NaN
    if (lane == 0 && logsum) logsum[i] = Mt + log(s);
    for (int col = lane; col < k; col += 64) {
        double a = 0.;
        for (int p = 0; p < P; ++p) a = fma(es[wv][p], row[p * step + 2 + col], a);
        mean[(size_t)i * ldo + col] = fabs(a) < INFINITY ? a / s : NAN;     // p inf is inf, 0 inf is NaN: a bad value gives NaN either way
    }
}
