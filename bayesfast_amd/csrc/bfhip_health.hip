// bfhip_health.hip -- did the sampler itself work: the per-chain figures behind the three warnings a NUTS / HMC user expects after a
// run (divergent transitions, transitions that hit the tree-depth limit, low E-BFMI), taken from the statistics table where
// bfhip_sampler_run left it (bayesfast_amd/utils/health.py holds the totals, the robust scores among the chains and the flags).
//
//   bfhip_health_chains  one workgroup per chain, two passes over the chain's rows [row0, row0 + n_rows) of stats, read in place:
//                        pass 1 stages tiles of HC_TH rows in LDS by coalesced reads of the contiguous block (a row is 11 doubles,
//                        so a lane reading its own row from memory would touch 11 cache lines) and takes the counts, the depth
//                        histogram, the three sums and sum (E_i - E_{i-1})^2; pass 2 takes sum (logp - mean)^2 and sum (E - mean)^2
//                        about the means of pass 1 (no one-pass variance), straight from the cache the block is still in.
//
// Thread t owns rows t, t + HC_TH, ... and adds them in that order; the HC_TH partial tuples then go through bf_block_tree.  The
// order of every sum is therefore set by n_rows alone: a chain's outputs are the same bits alone or in any launch, at any chain
// index.  Counts are carried as doubles (exact below 2^53) so that they share the tree.  No atomics, 64-bit offsets throughout.
#include <cmath>
#include "bfhip_block.h"

#define HC_TH 256                                   // threads per workgroup = rows per staged tile
#define HC_NB (BFHIP_MAX_TREEDEPTH + 1)             // bins of the depth histogram
#define HC_K1 11                                    // pass 1's tuple
#define HC_K2 2                                     // pass 2's tuple

// the columns of the two layouts
struct HcCols { int depth, size, accept, accepted, step, diverging; };
__device__ inline HcCols hc_cols(int sampler) {
    if (sampler == 0) return {BFHIP_NS_TREE_DEPTH, BFHIP_NS_TREE_SIZE, BFHIP_NS_MEAN_TREE_ACCEPT, -1, BFHIP_NS_STEP_SIZE, BFHIP_NS_DIVERGING};
    return {-1, BFHIP_HS_N_INT_STEP, BFHIP_HS_ACCEPT_STAT, BFHIP_HS_ACCEPTED, BFHIP_HS_STEP_SIZE, BFHIP_HS_DIVERGING};
}
// a table entry that holds a count: its integer part, 0 for anything that is none (negative, NaN, 2^52 or more)
__device__ inline double hc_count(double v) { return (v > 0. && v < 4503599627370496.) ? floor(v) : 0.; }

struct HcMerge1 {   // sums, but the largest tree
    __device__ void operator()(double *a, const double *b) const {
#pragma unroll
        for (int k = 0; k < HC_K1; ++k) a[k] = (k == 3) ? fmax(a[k], b[k]) : a[k] + b[k];
    }
};
struct HcMerge2 {
    __device__ void operator()(double *a, const double *b) const {
        a[0] += b[0];
        a[1] += b[1];
    }
};

__global__ __launch_bounds__(HC_TH) void bf_health_chains_kernel(long n_rows, long ldc, const double *__restrict__ stats, int sampler,
                                                                 int max_treedepth, long long *__restrict__ out_i,
                                                                 double *__restrict__ out_f) {
    __shared__ double buf[HC_TH * BFHIP_STAT_STRIDE];   // a tile of rows; afterwards the trees' slots (HC_K1 HC_TH <= its size)
    __shared__ int hist[HC_NB * HC_TH];                 // hist[b * HC_TH + t]: thread t's own count of depth b
    __shared__ long long hpart[16 * 16];
    static_assert(HC_K1 * HC_TH <= HC_TH * BFHIP_STAT_STRIDE, "the slots fit the tile");
    static_assert(HC_NB <= 16, "16 bins of 16 parts");
    const int t = threadIdx.x;
    const long c = blockIdx.x;
    const double *base = stats + c * ldc;
    const HcCols col = hc_cols(sampler);
    const bool nuts = sampler == 0;
#pragma unroll
    for (int b = 0; b < HC_NB; ++b) hist[b * HC_TH + t] = 0;
    // v: 0 n_divergent, 1 n_max_treedepth, 2 n_leapfrog, 3 max_tree_size, 4 n_accepted, 5 n_nonfinite, 6 sum accept, 7 sum logp,
    //    8 sum E, 9 sum (E_i - E_{i-1})^2, 10 n_moved
    double v[HC_K1];
#pragma unroll
    for (int k = 0; k < HC_K1; ++k) v[k] = 0.;
    for (long s0 = 0; s0 < n_rows; s0 += HC_TH) {
        const long left = n_rows - s0;
        const int nr = (int)(left < HC_TH ? left : HC_TH);
        __syncthreads();   // the previous tile's readers are done
        const double *src = base + s0 * BFHIP_STAT_STRIDE;
        for (int e = t; e < nr * BFHIP_STAT_STRIDE; e += HC_TH) buf[e] = src[e];
        __syncthreads();
        if (t < nr) {
            const double *row = buf + t * BFHIP_STAT_STRIDE;   // (an odd stride in doubles: the lanes of a half wave fall in distinct banks)
            const double lp = row[BFHIP_NS_LOGP], en = row[BFHIP_NS_ENERGY];
            const double sz = hc_count(row[col.size]);
            v[0] += (row[col.diverging] != 0.) ? 1. : 0.;
            v[2] += sz;
            v[3] = fmax(v[3], sz);
            v[5] += (isfinite(lp) && isfinite(en)) ? 0. : 1.;
            v[6] += row[col.accept];
            v[7] += lp;
            v[8] += en;
            if (nuts) {
                const double dp = row[col.depth];
                v[1] += (dp >= (double)max_treedepth) ? 1. : 0.;
                const int b = (dp >= 0. && dp <= (double)BFHIP_MAX_TREEDEPTH) ? (int)dp : BFHIP_MAX_TREEDEPTH;   // (NaN: the last bin)
                hist[b * HC_TH + t] += 1;
            } else {
                v[4] += (row[col.accepted] != 0.) ? 1. : 0.;
            }
            if (s0 + t > 0) {
                const double *before = ((t > 0) ? row : src) - BFHIP_STAT_STRIDE;   // (the row before a tile's first: from memory)
                const double de = en - before[BFHIP_NS_ENERGY];
                v[9] = fma(de, de, v[9]);
                v[10] += (lp != before[BFHIP_NS_LOGP]) ? 1. : 0.;
            }
        }
    }
    bf_block_tree<HC_TH, HC_K1>(v, buf, HcMerge1());
    const double n = (double)n_rows;
    const double m_lp = v[7] / n, m_en = v[8] / n;
    double q[HC_K2] = {0., 0.};
    for (long s = t; s < n_rows; s += HC_TH) {
        const double *row = base + s * BFHIP_STAT_STRIDE;
        const double a = row[BFHIP_NS_LOGP] - m_lp, b = row[BFHIP_NS_ENERGY] - m_en;
        q[0] = fma(a, a, q[0]);
        q[1] = fma(b, b, q[1]);
    }
    bf_block_tree<HC_TH, HC_K2>(q, buf, HcMerge2());
    // the histogram: 16 parts of 16 threads' counts per bin, then the parts (integers: any order is exact)
    {
        const int b = t >> 4, p = t & 15;
        long long sm = 0;
        if (b < HC_NB)
            for (int i = 0; i < 16; ++i) sm += hist[b * HC_TH + p * 16 + i];
        hpart[t] = sm;
    }
    __syncthreads();
    long long *oi = out_i + c * BFHIP_HEALTH_I_N;
    if (t < HC_NB) {
        long long sm = 0;
        for (int p = 0; p < 16; ++p) sm += hpart[t * 16 + p];
        oi[BFHIP_HEALTH_I_DEPTH_HIST + t] = sm;
    }
    if (t == 0) {
        oi[BFHIP_HEALTH_I_N_DIVERGENT] = (long long)v[0];
        oi[BFHIP_HEALTH_I_N_MAX_TREEDEPTH] = (long long)v[1];
        oi[BFHIP_HEALTH_I_N_LEAPFROG] = (long long)v[2];
        oi[BFHIP_HEALTH_I_MAX_TREE_SIZE] = (long long)v[3];
        oi[BFHIP_HEALTH_I_N_ACCEPTED] = (long long)v[4];
        oi[BFHIP_HEALTH_I_N_NONFINITE] = (long long)v[5];
        oi[BFHIP_HEALTH_I_N_MOVED] = (long long)v[10];
        const bool bad = v[5] != 0.;   // a non-finite logp or energy: the chain's moments are NaN, whatever inf - inf would give
        double *of = out_f + c * BFHIP_HEALTH_F_N;
        of[BFHIP_HEALTH_F_MEAN_ACCEPT] = v[6] / n;
        of[BFHIP_HEALTH_F_LOGP_MEAN] = bad ? NAN : m_lp;
        of[BFHIP_HEALTH_F_LOGP_VAR] = bad ? NAN : q[0] / (n - 1.);
        of[BFHIP_HEALTH_F_ENERGY_MEAN] = bad ? NAN : m_en;
        of[BFHIP_HEALTH_F_ENERGY_VAR] = bad ? NAN : q[1] / (n - 1.);
        // a constant energy (no difference at all): NaN, the 0 / 0 it stands for, whatever the mean's rounding left in q[1]
        of[BFHIP_HEALTH_F_BFMI] = (bad || v[9] == 0.) ? NAN : v[9] / q[1];
        of[BFHIP_HEALTH_F_STEP_SIZE] = base[(n_rows - 1) * BFHIP_STAT_STRIDE + col.step];
    }
}

extern "C" int bfhip_health_chains(bfhip_ctx *ctx, int n_chain, long n_rows, long ldc, const double *stats, int sampler, int max_treedepth,
                                   long long *out_i, double *out_f) {
    BfDeviceGuard dev_guard(ctx);
    if (!ctx || n_chain < 1 || n_rows < 2 || n_rows > (1L << 38) || !stats || !out_i || !out_f || (sampler != 0 && sampler != 1) ||
        max_treedepth < 1 || max_treedepth > BFHIP_MAX_TREEDEPTH || (n_chain > 1 && ldc < n_rows * BFHIP_STAT_STRIDE))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_health_chains: invalid argument");
    hipLaunchKernelGGL(bf_health_chains_kernel, dim3((unsigned)n_chain), dim3(HC_TH), 0, ctx->stream, n_rows, ldc, stats, sampler,
                       max_treedepth, out_i, out_f);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
