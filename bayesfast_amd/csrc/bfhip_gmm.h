// bfhip_gmm.h -- one pass of expectation-maximisation for a mixture of K Gaussians over n draws (bfhip_gmm_step): with
//     t_ik = logc_k - |(x_i - mean_k) A_k|^2 / 2,   Sigma_k^-1 = A_k A_k^T,
// the log density logpdf_i = log sum_k exp(t_ik), the responsibilities r_ik = exp(t_ik - logpdf_i) and, with w_i = exp(logw_i) and the
// caller's centre c, the statistics the M step needs:
//     N_k = sum_i w_i r_ik,   S1_k = sum_i w_i r_ik (x_i - c),   S2_k = sum_i w_i r_ik (x_i - c)(x_i - c)^T,
// then sum_i w_i logpdf_i and sum_i w_i.
//
//   gm_e_kernel       a workgroup takes 64 rows, a wave one 16-row tile whose values stay in registers.  The components are looped
//                     with A_k (and mean_k) staged in LDS, row stride = 16 mod 32 doubles as kd_wm_tile_kernel's V tile, so that the
//                     two rows of a 32-lane pass meet 32 banks; at d = 128 one factor is 144 KB of the 160.  The product
//                     (x - mean_k) A_k is NS k-steps of v_mfma_f64_16x16x4_f64 per block of 16 output columns, laid out as
//                     kd_tile_kernel lays out its operands: the DIFFERENCE is the A operand (lane l of k-step s holds
//                     [row l & 15][4 s + (l >> 4)]), A_k the B operand ([4 s + (l >> 4)][column l & 15]).  The squares of a result
//                     tile are summed per lane over the column blocks and then over the sixteen columns by a butterfly, so every
//                     lane of row 4 r + (l >> 4) holds the energy.  The log-sum-exp over k rescales a running maximum
//                     (gm_add).  t_ik goes to the work buffer (written and read back by the SAME lane, k & 15); after the last
//                     component it is replaced there by w_i r_ik.  A workgroup leaves its rows' (sum w logpdf, sum w).
//   gm_moment_kernel  workgroup (part p, component k): rows are the contraction dimension, four rows per k-step.  For the tile
//                     (ta, tb) of S2 the A operand is w r (x - c) of column block ta ([column l & 15][row l >> 4]) and the B operand
//                     (x - c) of column block tb, both read from global memory as they are (16 consecutive doubles per row).  Only
//                     the upper tiles are computed: above 32 columns they are split over the four waves, which all walk every
//                     row; up to 32 columns every wave takes all (one or three) tiles of every fourth k-step and the waves are
//                     folded in LDS in increasing order.  N_k and S1_k are plain sums beside the products.
//   gm_merge_kernel   folds the parts in increasing p, mirrors the upper triangle of S2 (of a diagonal tile too: (w x_a) x_b and
//                     (w x_b) x_a round differently) and folds the row blocks' two sums.
//
// A row of weight -inf has w r = 0 exactly, and a row with w r = 0 is taken as zeros by the moment kernel whatever it holds.  A NaN or
// +inf weight, or a non-finite row of weight above -inf, has w r = NaN for every k, which reaches every entry of stats.
//
// Partition: gm_plan(n) cuts the rows into P <= GM_PMAX parts of R rows, R a multiple of 16, by n alone (kd_plan's rule with fewer
// parts: a part leaves K (1 + d + d^2) doubles).  Every sum has an order fixed by (n, d, k); no atomics.
#pragma once
#include "bfhip_common.h"
#include <math.h>

#define GM_T 256            // threads of a workgroup: four waves
#define GM_RB 64            // rows of a workgroup of the E kernel
#define GM_MINROWS 256      // rows of a part, at least
#define GM_PMAX 128         // parts, at most

typedef double gm_d4 __attribute__((ext_vector_type(4)));

struct GmPlan { int P; long R; };   // part p holds rows [p R, min(n, (p + 1) R))
static inline GmPlan gm_plan(long n) {
    long P = (n + GM_MINROWS - 1) / GM_MINROWS;
    if (P > GM_PMAX) P = GM_PMAX;
    long R = (n + P - 1) / P;
    R = (R + 15) / 16 * 16;
    return {(int)((n + R - 1) / R), R};
}
// the k-step classes the E kernel is compiled for: the smallest that holds ceil(d / 4) (zero k-steps change no bit)
static inline int gm_steps(int d) {
    const int ns = (d + 3) / 4;
    const int cls[] = {1, 2, 4, 8, 12, 16, 24, 32};
    for (int c : cls)
        if (ns <= c) return c;
    return 32;
}
// row stride of a staged factor in doubles: = 16 mod 32, so that the 32 lanes of one LDS pass (2 rows x 16 columns) meet 32 banks
__host__ __device__ constexpr int gm_ldw(int CB) { return CB % 2 ? 16 * CB : 16 * CB + 16; }
// one more term t for the pair (M, S) of a running-maximum log-sum-exp (kd_add of bfhip_kde.h)
__device__ inline void gm_add(double &M, double &S, double t) {
    const double e = t == -INFINITY ? 0. : exp(-fabs(t - M));
    if (t > M) {
        S = fma(S, e, 1.);
        M = t;
    } else
        S += e;       // a NaN term lands here and stays
}
static inline size_t gm_stat_size(int d) { return 1 + (size_t)d + (size_t)d * d; }
__host__ __device__ constexpr int gm_cols(int NS) { return (4 * NS + 15) / 16; }      // blocks of 16 output columns
static inline size_t gm_e_lds(int ns) { return sizeof(double) * (size_t)(4 * ns * gm_ldw(gm_cols(ns)) + 4 * ns + 8); }

struct GmWork {
    double *wr;        // n x k: t_ik, then w_i r_ik
    double2 *esum;     // per 64 rows: (sum w logpdf, sum w)
    double *part;      // P x k x (1 + d + d^2)
    size_t bytes;
};
static GmWork gm_work(void *work, long n, int d, int k) {
    char *p = (char *)work;
    GmWork w;
    auto take = [&](size_t bytes) { char *q = p; p += (bytes + 255) / 256 * 256; return (void *)q; };
    w.wr = (double *)take(sizeof(double) * (size_t)n * (size_t)k);
    w.esum = (double2 *)take(sizeof(double2) * (size_t)((n + GM_RB - 1) / GM_RB));
    w.part = (double *)take(sizeof(double) * (size_t)gm_plan(n).P * (size_t)k * gm_stat_size(d));
    w.bytes = (size_t)(p - (char *)work);
    return w;
}

template <int NS>
__global__ __launch_bounds__(GM_T) void gm_e_kernel(int d, int K, long n, const double *__restrict__ x, long ldx,
                                                   const double *__restrict__ logw, const double *__restrict__ mean,
                                                   const double *__restrict__ whiten, const double *__restrict__ logc,
                                                   double *__restrict__ logpdf, double *__restrict__ resp, long ldr, double *wr,
                                                   double2 *__restrict__ esum, int want_stats) {
    constexpr int DP = 4 * NS, CB = gm_cols(NS), LDW = gm_ldw(CB), WC = 16 * CB;
    extern __shared__ double gm_lds_buf[];
    double *as = gm_lds_buf;            // [DP][LDW]: A_k, zero past d
    double *ms = as + DP * LDW;         // [DP]: mean_k, zero past d
    double *ws = ms + DP;               // [8]: the waves' two sums
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, ci = lane & 15, kr = lane >> 4;
    const long i0 = (long)blockIdx.x * GM_RB + 16 * wv;      // the wave's first row

    // the wave's rows: [row ci][4 s + kr] of k-step s; a row with a NaN or an infinity is bad
    double xr[NS];
    int bad = 0;
    {
        const long i = i0 + ci;
        const double *r = x + (size_t)(i < n ? i : 0) * ldx;
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            xr[s] = (i < n && 4 * s + kr < d) ? r[4 * s + kr] : 0.;
            if (!(fabs(xr[s]) < INFINITY)) bad = 1;
        }
        bad |= __shfl_xor(bad, 16, 64);
        bad |= __shfl_xor(bad, 32, 64);
    }
    int badrow[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) badrow[r] = __shfl(bad, 4 * r + kr, 64);

    double M[4], S[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { M[r] = -INFINITY; S[r] = 0.; }

    for (int k = 0; k < K; ++k) {
        __syncthreads();      // the previous component's reads
        const double *ak = whiten + (size_t)k * d * d;
        for (int e = tid; e < DP * WC; e += GM_T) {
            const int a = e / WC, b = e % WC;
            as[a * LDW + b] = (a < d && b < d) ? ak[(size_t)a * d + b] : 0.;
        }
        if (tid < DP) ms[tid] = tid < d ? mean[(size_t)k * d + tid] : 0.;
        __syncthreads();
        double a[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) a[s] = xr[s] - ms[4 * s + kr];
        double en[4] = {0., 0., 0., 0.};
#pragma unroll
        for (int cb = 0; cb < CB; ++cb) {
            gm_d4 acc = {0., 0., 0., 0.};
            const double *bp = &as[kr * LDW + 16 * cb + ci];
#pragma unroll
            for (int s = 0; s < NS; ++s) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s], bp[4 * s * LDW], acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) en[r] = fma(acc[r], acc[r], en[r]);
        }
        const double lc = logc[k];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
#pragma unroll
            for (int q = 1; q < 16; q <<= 1) en[r] += __shfl_xor(en[r], q, 64);
            const double t = badrow[r] ? NAN : lc - 0.5 * en[r];
            gm_add(M[r], S[r], t);
            const long i = i0 + 4 * r + kr;
            if (ci == (k & 15) && i < n && (resp || want_stats)) wr[(size_t)i * K + k] = t;
        }
    }

    double sl = 0., sw = 0.;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long i = i0 + 4 * r + kr;
        if (i >= n) continue;
        const double lp = M[r] + log(S[r]);
        if (ci == 0 && logpdf) logpdf[i] = lp;
        const double lw = logw ? logw[i] : 0.;
        const bool off = lw == -INFINITY;
        const double w = off ? 0. : lw < INFINITY ? exp(lw) : NAN;      // NaN or +inf: NaN
        if (!resp && !want_stats) continue;      // the log density alone: t_ik was not kept
        for (int k = ci; k < K; k += 16) {
            const double rr = exp(wr[(size_t)i * K + k] - lp);
            if (resp) resp[(size_t)i * ldr + k] = rr;
            if (want_stats) wr[(size_t)i * K + k] = off ? 0. : w * rr;
        }
        if (!off) {
            sl = fma(w, lp, sl);
            sw += badrow[r] ? NAN : w;
        }
    }
    if (!want_stats) return;      // the same in every thread
    // rows 4 r + kr of the wave: the four kr groups, then the waves, in increasing order
    {
        const double l0 = __shfl(sl, 0, 64), l1 = __shfl(sl, 16, 64), l2 = __shfl(sl, 32, 64), l3 = __shfl(sl, 48, 64);
        const double w0 = __shfl(sw, 0, 64), w1 = __shfl(sw, 16, 64), w2 = __shfl(sw, 32, 64), w3 = __shfl(sw, 48, 64);
        if (lane == 0) {
            ws[2 * wv] = (l0 + l1) + (l2 + l3);
            ws[2 * wv + 1] = (w0 + w1) + (w2 + w3);
        }
    }
    __syncthreads();
    if (tid == 0) esum[blockIdx.x] = make_double2(((ws[0] + ws[2]) + ws[4]) + ws[6], ((ws[1] + ws[3]) + ws[5]) + ws[7]);
}

// the q-th upper tile (ta <= tb) of a CB x CB grid of tiles, row by row
__host__ __device__ constexpr int gm_tile_a(int CB, int q) {
    int ta = 0;
    while (q >= CB - ta) { q -= CB - ta; ++ta; }
    return ta;
}
__host__ __device__ constexpr int gm_tile_b(int CB, int q) {
    int ta = 0;
    while (q >= CB - ta) { q -= CB - ta; ++ta; }
    return ta + q;
}
__host__ __device__ constexpr int gm_tiles(int CB) { return CB * (CB + 1) / 2; }
__host__ __device__ constexpr bool gm_split_rows(int CB) { return CB <= 2; }
static inline size_t gm_moment_lds(int cb) { return gm_split_rows(cb) ? sizeof(double) * (size_t)(4 * gm_tiles(cb) * 256 + 4 * cb * 16 + 4) : 0; }

// acc[u] += (wc xc[ta])^T xc[tb] for the wave's tiles u = U .. NU - 1, the block numbers compile-time constants (registers, no scratch)
template <int CB, int TG, int tg, int U, int NU>
__device__ inline void gm_mac(gm_d4 (&acc)[NU], double wc, const double (&xc)[CB]) {
    if constexpr (U < NU) {
        constexpr int ta = gm_tile_a(CB, tg + TG * U), tb = gm_tile_b(CB, tg + TG * U);
        acc[U] = __builtin_amdgcn_mfma_f64_16x16x4f64(wc * xc[ta], xc[tb], acc[U], 0, 0, 0);
        gm_mac<CB, TG, tg, U + 1, NU>(acc, wc, xc);
    }
}

// one wave of the moment kernel; out is the (part, component) slot [N, S1 (d), S2 (d x d, the upper triangle written)]
template <int CB, int W>
__device__ inline void gm_moment_wave(int d, int K, int k, long lo, long hi, const double *__restrict__ x, long ldx,
                                      const double *__restrict__ centre, const double *__restrict__ wr, double *__restrict__ out,
                                      double *lds) {
    constexpr int NT = gm_tiles(CB);
    constexpr bool SR = gm_split_rows(CB);
    constexpr int RG = SR ? 4 : 1, TG = SR ? 1 : 4, rg = SR ? W : 0, tg = SR ? 0 : W;
    constexpr int NU = (NT - tg + TG - 1) / TG;      // this wave's tiles: tg, tg + TG, ...
    constexpr bool SUMS = SR || W == 0;              // this wave keeps N and S1
    const int lane = threadIdx.x & 63, ci = lane & 15, kr = lane >> 4;
    double cen[CB];
#pragma unroll
    for (int t = 0; t < CB; ++t) cen[t] = 16 * t + ci < d ? centre[16 * t + ci] : 0.;
    gm_d4 acc[NU];
#pragma unroll
    for (int u = 0; u < NU; ++u) acc[u] = gm_d4{0., 0., 0., 0.};
    double s1[CB], s0 = 0.;
#pragma unroll
    for (int t = 0; t < CB; ++t) s1[t] = 0.;

    double w, xv[CB];
    auto fetch = [&](long j0) {
        const long j = j0 + kr;
        w = j < hi ? wr[(size_t)j * K + k] : 0.;
        const bool on = w != 0.;      // a NaN is on
        const double *r = x + (size_t)(j < hi ? j : lo) * ldx;
#pragma unroll
        for (int t = 0; t < CB; ++t) xv[t] = (on && 16 * t + ci < d) ? r[16 * t + ci] - cen[t] : 0.;
    };
    if (lo + 4 * rg < hi) fetch(lo + 4 * rg);
    for (long j0 = lo + 4 * rg; j0 < hi; j0 += 4 * RG) {
        const double wc = w;
        double xc[CB];
#pragma unroll
        for (int t = 0; t < CB; ++t) xc[t] = xv[t];
        if (j0 + 4 * RG < hi) fetch(j0 + 4 * RG);
        if (SUMS) {
            s0 += wc;
#pragma unroll
            for (int t = 0; t < CB; ++t) s1[t] = fma(wc, xc[t], s1[t]);
        }
        gm_mac<CB, TG, tg, 0, NU>(acc, wc, xc);
    }

    // the four kr groups' rows of N and S1
    if (SUMS) {
        const double p0 = __shfl(s0, ci, 64), p1 = __shfl(s0, ci + 16, 64), p2 = __shfl(s0, ci + 32, 64), p3 = __shfl(s0, ci + 48, 64);
        s0 = (p0 + p1) + (p2 + p3);
#pragma unroll
        for (int t = 0; t < CB; ++t) {
            const double q0 = __shfl(s1[t], ci, 64), q1 = __shfl(s1[t], ci + 16, 64), q2 = __shfl(s1[t], ci + 32, 64),
                         q3 = __shfl(s1[t], ci + 48, 64);
            s1[t] = (q0 + q1) + (q2 + q3);
        }
    }
    if (SR) {
        // lds: [4 waves][NT][4 r][64 lanes], then [4][CB][16], then [4]
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) lds[((W * NT + u) * 4 + r) * 64 + lane] = acc[u][r];
        double *l1 = lds + 4 * NT * 256, *l0 = l1 + 4 * CB * 16;
        if (kr == 0) {
#pragma unroll
            for (int t = 0; t < CB; ++t) l1[(W * CB + t) * 16 + ci] = s1[t];
        }
        if (lane == 0) l0[W] = s0;
    } else {
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int ta = gm_tile_a(CB, tg + TG * u), tb = gm_tile_b(CB, tg + TG * u);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int a = 16 * ta + 4 * r + kr, b = 16 * tb + ci;
                if (a <= b && b < d) out[1 + d + (size_t)a * d + b] = acc[u][r];
            }
        }
        if (SUMS) {
            if (kr == 0) {
#pragma unroll
                for (int t = 0; t < CB; ++t)
                    if (16 * t + ci < d) out[1 + 16 * t + ci] = s1[t];
            }
            if (lane == 0) out[0] = s0;
        }
    }
}

template <int CB>
__global__ __launch_bounds__(GM_T) void gm_moment_kernel(int d, int K, long n, const double *__restrict__ x, long ldx,
                                                        const double *__restrict__ centre, const double *__restrict__ wr, long R,
                                                        double *__restrict__ part) {
    extern __shared__ double gm_lds_buf[];
    constexpr int NT = gm_tiles(CB);
    const int wv = threadIdx.x >> 6, k = blockIdx.y;
    const long lo = (long)blockIdx.x * R, hi = lo + R < n ? lo + R : n;
    double *out = part + ((size_t)blockIdx.x * K + k) * (1 + (size_t)d + (size_t)d * d);
    switch (wv) {
        case 0: gm_moment_wave<CB, 0>(d, K, k, lo, hi, x, ldx, centre, wr, out, gm_lds_buf); break;
        case 1: gm_moment_wave<CB, 1>(d, K, k, lo, hi, x, ldx, centre, wr, out, gm_lds_buf); break;
        case 2: gm_moment_wave<CB, 2>(d, K, k, lo, hi, x, ldx, centre, wr, out, gm_lds_buf); break;
        default: gm_moment_wave<CB, 3>(d, K, k, lo, hi, x, ldx, centre, wr, out, gm_lds_buf); break;
    }
    if (!gm_split_rows(CB)) return;
    __syncthreads();
    // the waves in increasing order
    const double *lds = gm_lds_buf, *l1 = lds + 4 * NT * 256, *l0 = l1 + 4 * CB * 16;
    for (int e = threadIdx.x; e < NT * 256; e += GM_T) {
        const double v = ((lds[e] + lds[NT * 256 + e]) + lds[2 * NT * 256 + e]) + lds[3 * NT * 256 + e];
        const int u = e / 256, r = (e / 64) & 3, lane = e & 63;
        const int a = 16 * gm_tile_a(CB, u) + 4 * r + (lane >> 4), b = 16 * gm_tile_b(CB, u) + (lane & 15);
        if (a <= b && b < d) out[1 + d + (size_t)a * d + b] = v;
    }
    for (int e = threadIdx.x; e < CB * 16; e += GM_T)
        if (e < d) out[1 + e] = ((l1[e] + l1[CB * 16 + e]) + l1[2 * CB * 16 + e]) + l1[3 * CB * 16 + e];
    if (threadIdx.x == 0) out[0] = ((l0[0] + l0[1]) + l0[2]) + l0[3];
}

// stats: N (K), S1 (K x d), S2 (K x d x d), sum w logpdf, sum w.  The last workgroup folds the row blocks' two sums.
__global__ __launch_bounds__(GM_T) void gm_merge_kernel(int d, int K, int P, long nb, const double *__restrict__ part,
                                                       const double2 *__restrict__ esum, double *__restrict__ stats) {
    const size_t SZ = 1 + (size_t)d + (size_t)d * d, total = (size_t)K * SZ;
    if (blockIdx.x == gridDim.x - 1) {
        __shared__ double2 fs[GM_T];
        double2 s = make_double2(0., 0.);
        for (long b = threadIdx.x; b < nb; b += GM_T) {
            s.x += esum[b].x;
            s.y += esum[b].y;
        }
        fs[threadIdx.x] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            double2 t = make_double2(0., 0.);
            for (int q = 0; q < GM_T; ++q) {
                t.x += fs[q].x;
                t.y += fs[q].y;
            }
            stats[total] = t.x;
            stats[total + 1] = t.y;
        }
        return;
    }
    const size_t e = (size_t)blockIdx.x * GM_T + threadIdx.x;
    if (e >= total) return;
    size_t k, off;
    if (e < (size_t)K) {
        k = e;
        off = 0;
    } else if (e < (size_t)K * (1 + d)) {
        k = (e - K) / d;
        off = 1 + (e - K) % d;
    } else {
        const size_t q = e - (size_t)K * (1 + d);
        k = q / ((size_t)d * d);
        const size_t a = q % ((size_t)d * d) / d, b = q % d;
        off = 1 + d + (a < b ? a * d + b : b * d + a);
    }
    double s = 0.;
    for (int p = 0; p < P; ++p) s += part[((size_t)p * K + k) * SZ + off];
    stats[e] = s;
}
