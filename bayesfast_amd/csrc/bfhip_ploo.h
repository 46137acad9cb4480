// bfhip_ploo.h -- pointwise PSIS-LOO and WAIC of a batch of 16 columns of pointwise log likelihoods (bayesfast_amd/utils/data_loo.py has
// the definitions); included at the end of bfhip_psis.hip, whose generalised-Pareto fit (ps_theta_kernel, ps_fit_kernel) it runs on
// each column's tail.  A column holds ell_s, or z_s with ell_s = c - z_s^2 / 2; lb are the base log weights (NULL: -log n each).
//
//   bfhip_ploo_moments   max r, lpd, sum w ell, sum w (ell - mean)^2, sum w^2, flags            two passes over the batch
//   bfhip_ploo_tail      the M + 1 largest pairs (key of r - max r, row) of every column, ascending
//   bfhip_ploo_finish    the fit per column, the smoothed tail, the sums behind elpd_loo, ess_loo and pit    one pass over the batch
//
// The select.  PSIS needs the M + 1 <= 3 sqrt(n) + 2 largest ratios of a column in the order of a stable ascending sort, that is the
// rows whose pair (key, row) is not below the pair at sorted position n - M - 1 (the cut).  A most-significant-digit radix select
// finds the cut's key: eight passes over the batch, each a histogram of one byte of the keys that share the bytes chosen so far (a
// thread counts runs of equal digits in registers, a workgroup adds them into LDS, then into 16 x 256 global counters; the counts
// are integers, so the atomics do not disturb the result), each followed by one small kernel that walks the 256 counters from the
// top.  A ninth pass appends the rows above the cut's key to the column's candidate list and counts, per workgroup, the rows EQUAL
// to it; a workgroup owns a contiguous range of rows, so these counts, walked from the last workgroup down, and a second walk
// inside the one range that holds it, give the cut's row.  Rows equal to the cut's key and behind its row join the candidates in a
// tenth pass, which ends at once in every workgroup unless some column has ties across its cut.  The M candidates of a column come
// in no fixed order; two stable segmented radix sorts (rocPRIM), by row and then by key, put them in the order of the pairs.
// Nothing sorts a column: beyond the ten reads of the batch the work is O(M log M) per column, in global memory.
#pragma once
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#define PL_B BFHIP_DIAG_BATCH
#define PL_BINS 256
#define PL_HPAD (PL_BINS + 1)     // a column's LDS counters start one bank after its neighbour's
#define PL_MAXG 4096              // workgroups of a select pass, each on a contiguous range of rows
#define PL_MINROWS 256            // rows of such a range, at least
#define PL_NPART 7                // partial results per column of the moment passes
static_assert(PL_B == 16 && PS_T == PL_B * BF_SLICES, "a workgroup is 16 row slices x 16 columns");
static_assert(PL_MAXG % PS_T == 0, "bfhip_ploo_tail's locate kernel walks the workgroups' counts in 256 groups");

// rows of the out block (BFHIP_PLOO_NOUT, 16)
enum { PL_LPD = 0, PL_SWE, PL_WAIC, PL_ELPD, PL_KHAT, PL_SIGMA, PL_M, PL_CUT, PL_ESS, PL_PIT, PL_MAXR, PL_FLAGS, PL_SW2, PL_MAXB, PL_MAXT,
       PL_SPARE };
static_assert(PL_SPARE + 1 == BFHIP_PLOO_NOUT, "the out block's rows");

struct PlCols {   // a batch: element (row, column b) at s[row * ld + b]
    long n;
    const double *s;
    long ld;
    int nb, mode;
    const double *c, *lb;
};

// Every kernel of the select, and the finish's test of a row against the cut pair, must see the same bits of a row's shifted ratio:
// its three operations are kept from being contracted, which the compiler would decide kernel by kernel.
__device__ inline double pl_ell(const PlCols &a, long row, int b) {
#pragma clang fp contract(off)
    const double v = a.s[row * a.ld + b];
    const double h = 0.5 * (v * v);
    return a.mode == BFHIP_PLOO_Z ? a.c[b] - h : v;
}
// the log ratio that removes the point, less the column's largest: (lb - ell) - mx; a row of zero weight has -inf, whatever it holds
__device__ inline double pl_shifted(double lb, double ell, double mx) {
#pragma clang fp contract(off)
    const double r = lb == -__builtin_inf() ? lb : lb - ell;
    return r - mx;
}
__device__ inline uint64_t pl_key(const PlCols &a, long row, int b, double mx) {
    return bf_order_key(pl_shifted(a.lb ? a.lb[row] : 0., pl_ell(a, row, b), mx));
}
__device__ inline double pl_phi(double z) { return 0.5 * erfc(-z * 0.70710678118654752440); }

// ==== moments ========================================================================================================================
// thread (slice sl, column b) walks rows sl, sl + 16 G, ...; slice 0 folds the slices in order (bf_slice_fold), one workgroup the workgroups
template <int PASS>
__device__ inline void pl_fold(double *v, double (*red)[PS_T], int b, int sl) {   // slice 0 leaves with the column's values in v
    constexpr int K = PASS == 1 ? PL_NPART : 2;
    for (int k = 0; k < K; ++k) red[k][threadIdx.x] = v[k];
    __syncthreads();
    if (sl != 0) return;
    for (int k = 0; k < K; ++k)   // PASS 1: three maxima, then two sums and two counts (whole numbers)
        v[k] = (PASS == 2 || k >= 3) ? bf_slice_fold(v[k], 1, red[k], b, BfSum()) : bf_slice_fold(v[k], 1, red[k], b, BfMax());
}

template <int PASS>
__device__ inline void pl_start(double *v) {
    for (int k = 0; k < PL_NPART; ++k) v[k] = PASS == 1 && k < 3 ? -__builtin_inf() : 0.;
}

// PASS 1: max r, max (lb + ell), max lb, sum w ell, sum w^2, rows with a non-finite ell, rows of non-zero weight
// PASS 2: sum exp(lb + ell - max), sum w (ell - mean)^2
template <int PASS>
__global__ __launch_bounds__(PS_T) void pl_moments_kernel(PlCols a, const double *__restrict__ out, double *__restrict__ part) {
    __shared__ double red[PL_NPART][PS_T];
    const int b = threadIdx.x & (PL_B - 1), sl = threadIdx.x / PL_B;
    const double lb0 = -log((double)a.n), w0 = 1. / (double)a.n;
    double v[PL_NPART];
    pl_start<PASS>(v);
    if (b < a.nb) {
        const double mt = PASS == 2 ? out[PL_MAXT * PL_B + b] : 0., mean = PASS == 2 ? out[PL_SWE * PL_B + b] : 0.;
        for (long r = (long)blockIdx.x * BF_SLICES + sl; r < a.n; r += (long)gridDim.x * BF_SLICES) {
            const double lb = a.lb ? a.lb[r] : lb0;
            if (lb == -__builtin_inf()) continue;   // not part of the sample: the row is not read as a number
            const double ell = pl_ell(a, r, b), w = a.lb ? exp(lb) : w0;
            if (PASS == 1) {
                v[0] = fmax(v[0], (a.lb ? lb : 0.) - ell);
                v[1] = fmax(v[1], lb + ell);
                v[2] = fmax(v[2], lb);
                v[3] += w * ell;
                v[4] += w * w;
                if (!(fabs(ell) < __builtin_inf())) v[5] += 1.;
                v[6] += 1.;
            } else {
                const double d = ell - mean;
                v[0] += exp(lb + ell - mt);
                v[1] += w * (d * d);
            }
        }
    }
    pl_fold<PASS>(v, red, b, sl);
    if (sl == 0)
        for (int k = 0; k < (PASS == 1 ? PL_NPART : 2); ++k) part[((long)k * PS_MAXB + blockIdx.x) * PL_B + b] = v[k];
}

template <int PASS>
__global__ __launch_bounds__(PS_T) void pl_moments_final_kernel(int nblk, const double *__restrict__ part, double *__restrict__ out) {
    __shared__ double red[PL_NPART][PS_T];
    constexpr int K = PASS == 1 ? PL_NPART : 2;
    const int b = threadIdx.x & (PL_B - 1), sl = threadIdx.x / PL_B;
    double v[PL_NPART];
    pl_start<PASS>(v);
    for (int g = sl; g < nblk; g += BF_SLICES)
        for (int k = 0; k < K; ++k) {
            const double p = part[((long)k * PS_MAXB + g) * PL_B + b];
            v[k] = (PASS == 2 || k >= 3) ? v[k] + p : fmax(v[k], p);
        }
    pl_fold<PASS>(v, red, b, sl);
    if (sl != 0) return;
    if (PASS == 1) {
        out[PL_MAXR * PL_B + b] = v[0];
        out[PL_MAXT * PL_B + b] = v[1];
        out[PL_MAXB * PL_B + b] = v[2];
        out[PL_SWE * PL_B + b] = v[3];
        out[PL_SW2 * PL_B + b] = v[4];
        out[PL_FLAGS * PL_B + b] = (v[5] != 0. ? 1. : 0.) + (v[6] == 0. ? 4. : 0.);
        out[PL_SPARE * PL_B + b] = 0.;
    } else {
        out[PL_LPD * PL_B + b] = out[PL_MAXT * PL_B + b] + log(v[0]);
        out[PL_WAIC * PL_B + b] = v[1];
    }
}

static inline long pl_tail_size(long n) {
    long M = (long)ceil(3. * sqrt((double)n));
    return n / 5 < M ? n / 5 : M;
}

static int pl_check(const char *who, bfhip_ctx *ctx, long n, const double *series, long ld, int nb, int mode, const double *c) {
    if (!ctx || n < 1 || !series || nb < 1 || nb > PL_B || ld < nb || (mode != BFHIP_PLOO_ELL && mode != BFHIP_PLOO_Z) ||
        (mode == BFHIP_PLOO_Z && !c))
        return bf_set_error(BFHIP_ERR_ARG, "%s: invalid argument", who);
    if (n > 0x7fffffffL) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "%s: more than 2^31-1 rows", who);
    return 0;
}

// ---- the work buffer: the moment passes' partial results and everything the select and the finish keep ------------------------------
struct PlWork {
    double *part;        // PL_NPART PS_MAXB 16
    uint32_t *hist;      // 16 x 256
    uint64_t *prefix;    // 16: the bytes of the cut's key chosen so far
    uint32_t *krem;      // 16: rows of the current prefix that come behind the cut
    uint32_t *gcount;    // 16: candidates appended
    uint32_t *idxc;      // 16: the cut's row
    uint32_t *eqcnt;     // PL_MAXG x 16
    double *out8;        // 16 x 8: ps_fit_kernel's results
    double *kj, *thj;    // 16 x PS_MAXM each
    uint64_t *ck[2];     // 16 (M + 1) candidate keys, twice
    uint32_t *ci[2];     // ... and rows
    double *sm;          // 16 (M + 1) smoothed tail values
    size_t bytes;
};
static PlWork pl_work(void *work, long n) {
    const size_t L = (size_t)PL_B * (size_t)(pl_tail_size(n) + 1);
    char *p = (char *)work;
    PlWork w;
    auto take = [&](size_t bytes) { char *q = p; p += (bytes + 255) / 256 * 256; return (void *)q; };
    w.part = (double *)take(sizeof(double) * PL_NPART * PS_MAXB * PL_B);
    w.hist = (uint32_t *)take(4 * PL_B * PL_BINS);
    w.prefix = (uint64_t *)take(8 * PL_B);
    w.krem = (uint32_t *)take(4 * PL_B);
    w.gcount = (uint32_t *)take(4 * PL_B);
    w.idxc = (uint32_t *)take(4 * PL_B);
    w.eqcnt = (uint32_t *)take(4 * (size_t)PL_MAXG * PL_B);
    w.out8 = (double *)take(8 * PL_B * 8);
    w.kj = (double *)take(8 * PL_B * PS_MAXM);
    w.thj = (double *)take(8 * PL_B * PS_MAXM);
    for (int i = 0; i < 2; ++i) w.ck[i] = (uint64_t *)take(8 * L);
    for (int i = 0; i < 2; ++i) w.ci[i] = (uint32_t *)take(4 * L);
    w.sm = (double *)take(8 * L);
    w.bytes = (size_t)(p - (char *)work);
    return w;
}

extern "C" size_t bfhip_ploo_work_bytes(long n) { return n < 1 || n > 0x7fffffffL ? 0 : pl_work(nullptr, n).bytes; }

extern "C" int bfhip_ploo_moments(bfhip_ctx *ctx, long n, const double *series, long ld, int nb, int mode, const double *c, const double *lb,
                                  double *out, void *work, size_t work_bytes) {
    BfDeviceGuard dev_guard(ctx);
    if (int rc = pl_check("bfhip_ploo_moments", ctx, n, series, ld, nb, mode, c)) return rc;
    if (!out || !work || work_bytes < bfhip_ploo_work_bytes(n)) return bf_set_error(BFHIP_ERR_ARG, "bfhip_ploo_moments: invalid argument");
    const PlWork w = pl_work(work, n);
    const PlCols a = {n, series, ld, nb, mode, c, lb};
    const int g = ps_grid(n, BF_SLICES);
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(pl_moments_kernel<1>, dim3(g), dim3(PS_T), 0, st, a, (const double *)out, w.part);
    hipLaunchKernelGGL(pl_moments_final_kernel<1>, dim3(1), dim3(PS_T), 0, st, g, w.part, out);
    hipLaunchKernelGGL(pl_moments_kernel<2>, dim3(g), dim3(PS_T), 0, st, a, (const double *)out, w.part);
    hipLaunchKernelGGL(pl_moments_final_kernel<2>, dim3(1), dim3(PS_T), 0, st, g, w.part, out);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}

// ==== the select =====================================================================================================================
struct PlGrid { int G; long R; };   // G workgroups, workgroup g on rows [g R, min(n, (g + 1) R)), R a multiple of 16
static inline PlGrid pl_grid(long n) {
    long G = (n + PL_MINROWS - 1) / PL_MINROWS;
    if (G > PL_MAXG) G = PL_MAXG;
    long R = (n + G - 1) / G;
    R = (R + BF_SLICES - 1) / BF_SLICES * BF_SLICES;
    return {(int)((n + R - 1) / R), R};
}

__global__ __launch_bounds__(PS_T) void pl_select_init_kernel(long M, uint32_t *hist, uint64_t *prefix, uint32_t *krem, uint32_t *gcount) {
    for (int i = threadIdx.x; i < PL_B * PL_BINS; i += PS_T) hist[i] = 0;
    if (threadIdx.x < PL_B) {
        prefix[threadIdx.x] = 0;
        krem[threadIdx.x] = (uint32_t)M;   // the cut has M pairs behind it
        gcount[threadIdx.x] = 0;
    }
}

// byte `pass` (0: the most significant) of the keys whose bytes above it equal the column's prefix
__global__ __launch_bounds__(PS_T) void pl_hist_kernel(PlCols a, long R, int pass, const double *__restrict__ out,
                                                      const uint64_t *__restrict__ prefix, uint32_t *__restrict__ hist) {
    __shared__ uint32_t h[PL_B * PL_HPAD];
    const int b = threadIdx.x & (PL_B - 1), sl = threadIdx.x / PL_B;
    for (int i = threadIdx.x; i < PL_B * PL_HPAD; i += PS_T) h[i] = 0;
    __syncthreads();
    if (b < a.nb) {
        const double mx = out[PL_MAXR * PL_B + b];
        const uint64_t pre = prefix[b];
        const int shift = 56 - 8 * pass;
        const long lo = (long)blockIdx.x * R, hi = lo + R < a.n ? lo + R : a.n;
        int last = 0;
        uint32_t run = 0;
        for (long r = lo + sl; r < hi; r += BF_SLICES) {
            const uint64_t key = pl_key(a, r, b, mx);
            if (pass > 0 && (key >> (shift + 8)) != pre) continue;
            const int d = (int)((key >> shift) & (PL_BINS - 1));
            if (d != last) {
                if (run) atomicAdd(&h[b * PL_HPAD + last], run);
                last = d;
                run = 0;
            }
            ++run;
        }
        if (run) atomicAdd(&h[b * PL_HPAD + last], run);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PL_B * PL_BINS; i += PS_T) {
        const uint32_t v = h[(i / PL_BINS) * PL_HPAD + (i & (PL_BINS - 1))];
        if (v) atomicAdd(&hist[i], v);
    }
}

// the byte that holds the cut: from the top, the first counter that the remaining rank falls into
__global__ __launch_bounds__(PS_T) void pl_pick_kernel(int nb, uint32_t *hist, uint64_t *prefix, uint32_t *krem) {
    const int b = threadIdx.x;
    if (b < nb) {
        uint32_t k = krem[b];
        int d = PL_BINS - 1;
        for (; d > 0; --d) {
            const uint32_t cnt = hist[b * PL_BINS + d];
            if (k < cnt) break;
            k -= cnt;
        }
        prefix[b] = (prefix[b] << 8) | (uint64_t)d;
        krem[b] = k;   // (after the last byte: rows with the cut's key behind the cut)
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PL_B * PL_BINS; i += PS_T) hist[i] = 0;
}

// EQUAL 0: append the rows above the cut's key, count the rows equal to it per workgroup.  1: append the rows equal to it behind the
// cut's row (nothing to do unless a column has ties across its cut)
template <int EQUAL>
__global__ __launch_bounds__(PS_T) void pl_compact_kernel(PlCols a, long R, long M, const double *__restrict__ out,
                                                         const uint64_t *__restrict__ prefix, const uint32_t *__restrict__ krem,
                                                         const uint32_t *__restrict__ idxc, uint32_t *__restrict__ gcount,
                                                         uint32_t *__restrict__ eqcnt, uint64_t *__restrict__ ck, uint32_t *__restrict__ ci) {
    __shared__ uint32_t eq[PL_B];
    const int b = threadIdx.x & (PL_B - 1), sl = threadIdx.x / PL_B;
    if (threadIdx.x < PL_B) eq[threadIdx.x] = 0;
    __syncthreads();
    if (b < a.nb && (EQUAL == 0 || krem[b] != 0)) {
        const double mx = out[PL_MAXR * PL_B + b];
        const uint64_t kc = prefix[b];
        const uint32_t ic = EQUAL ? idxc[b] : 0;
        const long lo = (long)blockIdx.x * R, hi = lo + R < a.n ? lo + R : a.n;
        uint32_t n_eq = 0;
        for (long r = lo + sl; r < hi; r += BF_SLICES) {
            const uint64_t key = pl_key(a, r, b, mx);
            if (EQUAL == 0 && key == kc) ++n_eq;
            if (EQUAL ? (key == kc && (uint32_t)r > ic) : key > kc) {
                const uint32_t pos = atomicAdd(&gcount[b], 1u);
                if ((long)pos < M) {   // (always: M pairs lie behind the cut)
                    ck[(long)b * (M + 1) + 1 + pos] = key;
                    ci[(long)b * (M + 1) + 1 + pos] = (uint32_t)r;
                }
            }
        }
        if (EQUAL == 0 && n_eq) atomicAdd(&eq[b], n_eq);
    }
    if (EQUAL == 0) {
        __syncthreads();
        if (threadIdx.x < PL_B) eqcnt[(long)blockIdx.x * PL_B + threadIdx.x] = eq[threadIdx.x];
    }
}

// workgroup b: the cut's row.  krem[b] rows with the cut's key come behind it; the workgroups' counts from the last one down give its
// range of rows, the counts of 256 pieces of that range its piece, a walk down the piece the row.
__global__ __launch_bounds__(PS_T) void pl_locate_kernel(PlCols a, int G, long R, long M, const double *__restrict__ out,
                                                        const uint64_t *__restrict__ prefix, const uint32_t *__restrict__ krem,
                                                        const uint32_t *__restrict__ eqcnt, uint32_t *__restrict__ idxc,
                                                        uint64_t *__restrict__ tail_keys, uint32_t *__restrict__ tail_idx) {
    __shared__ uint32_t cnt[PS_T];
    __shared__ long s_lo, s_hi;
    __shared__ uint32_t s_k;
    const int b = blockIdx.x, t = threadIdx.x;
    const double mx = out[PL_MAXR * PL_B + b];
    const uint64_t kc = prefix[b];
    const int per = (G + PS_T - 1) / PS_T;
    uint32_t c = 0;
    for (int g = t * per; g < (t + 1) * per && g < G; ++g) c += eqcnt[(long)g * PL_B + b];
    cnt[t] = c;
    __syncthreads();
    if (t == 0) {
        uint32_t k = krem[b];
        int q = PS_T - 1;
        for (; q > 0; --q) {
            if (k < cnt[q]) break;
            k -= cnt[q];
        }
        int g = (q + 1) * per - 1 < G - 1 ? (q + 1) * per - 1 : G - 1;
        for (; g > q * per; --g) {
            const uint32_t e = eqcnt[(long)g * PL_B + b];
            if (k < e) break;
            k -= e;
        }
        if (g < 0) g = 0;
        s_lo = (long)g * R;
        s_hi = s_lo + R < a.n ? s_lo + R : a.n;
        s_k = k;
    }
    __syncthreads();
    const long lo = s_lo, hi = s_hi, step = (hi - lo + PS_T - 1) / PS_T;
    const long p0 = lo + t * step, p1 = p0 + step < hi ? p0 + step : hi;
    c = 0;
    for (long r = p0; r < p1; ++r) c += pl_key(a, r, b, mx) == kc ? 1u : 0u;
    __syncthreads();
    cnt[t] = c;
    __syncthreads();
    if (t == 0) {
        uint32_t k = s_k;
        int q = PS_T - 1;
        for (; q > 0; --q) {
            if (k < cnt[q]) break;
            k -= cnt[q];
        }
        const long q0 = lo + q * step, q1 = q0 + step < hi ? q0 + step : hi;
        long row = q0 < a.n ? q0 : a.n - 1;
        for (long r = q1 - 1; r >= q0; --r)
            if (pl_key(a, r, b, mx) == kc) {
                if (k == 0) {
                    row = r;
                    break;
                }
                --k;
            }
        idxc[b] = (uint32_t)row;
        tail_keys[(long)b * (M + 1)] = kc;
        tail_idx[(long)b * (M + 1)] = (uint32_t)row;
    }
}

struct PlSegment {   // the candidates of column i: positions 1 .. M of its row of M + 1
    unsigned len, off;
    __host__ __device__ unsigned operator()(unsigned i) const { return i * len + off; }
};

extern "C" int bfhip_ploo_tail(bfhip_ctx *ctx, long n, const double *series, long ld, int nb, int mode, const double *c, const double *lb,
                               const double *out, uint64_t *tail_keys, uint32_t *tail_idx, void *work, size_t work_bytes) {
    BfDeviceGuard dev_guard(ctx);
    if (int rc = pl_check("bfhip_ploo_tail", ctx, n, series, ld, nb, mode, c)) return rc;
    if (!out || !tail_keys || !tail_idx || !work || work_bytes < bfhip_ploo_work_bytes(n))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_ploo_tail: invalid argument");
    const long M = pl_tail_size(n);
    const PlWork w = pl_work(work, n);
    const PlCols a = {n, series, ld, nb, mode, c, lb};
    const PlGrid gr = pl_grid(n);
    hipStream_t st = ctx->stream;
    // the two sorts' temporary storage, in the context's workspace (grown before the first launch: growing waits for the stream)
    const unsigned L = (unsigned)(M + 1);
    auto seg0 = rocprim::make_transform_iterator(rocprim::counting_iterator<unsigned>(0), PlSegment{L, 1});
    auto seg1 = rocprim::make_transform_iterator(rocprim::counting_iterator<unsigned>(0), PlSegment{L, L});
    int bits = 1;
    while (bits < 32 && ((long)1 << bits) < n) ++bits;
    size_t tmp_i = 0, tmp_k = 0;
    if (M > 1) {
        hipError_t e = rocprim::segmented_radix_sort_pairs(nullptr, tmp_i, w.ci[0], w.ci[1], w.ck[0], w.ck[1], (unsigned)(L * nb), (unsigned)nb,
                                                           seg0, seg1, 0, (unsigned)bits, st);
        if (e == hipSuccess)
            e = rocprim::segmented_radix_sort_pairs(nullptr, tmp_k, w.ck[1], tail_keys, w.ci[1], tail_idx, (unsigned)(L * nb), (unsigned)nb, seg0,
                                                    seg1, 0, 64, st);
        if (e != hipSuccess) return bf_set_error(BFHIP_ERR_HIP, "rocprim::segmented_radix_sort_pairs (size query): %s", hipGetErrorString(e));
        if (int rc = bf_grow(ctx, &ctx->scratch, &ctx->scratch_bytes, tmp_i > tmp_k ? tmp_i : tmp_k)) return rc;
    }
    hipLaunchKernelGGL(pl_select_init_kernel, dim3(1), dim3(PS_T), 0, st, M, w.hist, w.prefix, w.krem, w.gcount);
    for (int pass = 0; pass < 8; ++pass) {
        hipLaunchKernelGGL(pl_hist_kernel, dim3(gr.G), dim3(PS_T), 0, st, a, gr.R, pass, out, (const uint64_t *)w.prefix, w.hist);
        hipLaunchKernelGGL(pl_pick_kernel, dim3(1), dim3(PS_T), 0, st, nb, w.hist, w.prefix, w.krem);
    }
    // with M > 1 the candidates go through the sorts; a single one is in place at once
    uint64_t *ck = M > 1 ? w.ck[0] : tail_keys;
    uint32_t *ci = M > 1 ? w.ci[0] : tail_idx;
    hipLaunchKernelGGL(pl_compact_kernel<0>, dim3(gr.G), dim3(PS_T), 0, st, a, gr.R, M, out, (const uint64_t *)w.prefix,
                       (const uint32_t *)w.krem, (const uint32_t *)w.idxc, w.gcount, w.eqcnt, ck, ci);
    hipLaunchKernelGGL(pl_locate_kernel, dim3(nb), dim3(PS_T), 0, st, a, gr.G, gr.R, M, out, (const uint64_t *)w.prefix,
                       (const uint32_t *)w.krem, (const uint32_t *)w.eqcnt, w.idxc, tail_keys, tail_idx);
    hipLaunchKernelGGL(pl_compact_kernel<1>, dim3(gr.G), dim3(PS_T), 0, st, a, gr.R, M, out, (const uint64_t *)w.prefix,
                       (const uint32_t *)w.krem, (const uint32_t *)w.idxc, w.gcount, w.eqcnt, ck, ci);
    BF_HIP_CHECK(hipGetLastError());
    if (M > 1) {
        hipError_t e = rocprim::segmented_radix_sort_pairs(ctx->scratch, tmp_i, w.ci[0], w.ci[1], w.ck[0], w.ck[1], (unsigned)(L * nb),
                                                           (unsigned)nb, seg0, seg1, 0, (unsigned)bits, st);
        if (e == hipSuccess)
            e = rocprim::segmented_radix_sort_pairs(ctx->scratch, tmp_k, w.ck[1], tail_keys, w.ci[1], tail_idx, (unsigned)(L * nb),
                                                    (unsigned)nb, seg0, seg1, 0, 64, st);
        if (e != hipSuccess) return bf_set_error(BFHIP_ERR_HIP, "rocprim::segmented_radix_sort_pairs: %s", hipGetErrorString(e));
    }
    return 0;
}

// ==== finish =========================================================================================================================
__global__ void pl_fit_init_kernel(double *out8) { out8[threadIdx.x] = 0.; }

// sm[b][i]: what tail position i (tail_keys[b][1 + i]) weighs -- the fit's expected order statistic, capped at 0, or its own value
// where nothing is smoothed
__global__ __launch_bounds__(PS_T) void pl_smooth_kernel(long M, const uint64_t *__restrict__ tail_keys, const double *__restrict__ out8s,
                                                        double *__restrict__ sm) {
    const long i = (long)blockIdx.x * PS_T + threadIdx.x;
    const int b = blockIdx.y;
    if (i >= M) return;
    const double *out8 = out8s + 8 * b;
    double v = bf_order_value(tail_keys[(long)b * (M + 1) + 1 + i]);
    if ((int)out8[7] == 0) {
        const double khat = out8[0], sigma = out8[1], ecut = exp(out8[3]);
        const double l1p = log1p(-((double)i + 0.5) / (double)M);
        const double q = khat == 0. ? -sigma * l1p : sigma * expm1(-khat * l1p) / khat;
        v = log(ecut + q);
        v = v > 0. ? 0. : v;
    }
    sm[(long)b * (M + 1) + i] = v;
}

// the rows not above the cut pair, each with its own ratio: sum e, sum e^2, sum exp(lb - max lb), sum e Phi(z), e = exp(r - max r)
__global__ __launch_bounds__(PS_T) void pl_body_kernel(PlCols a, long M, const double *__restrict__ out, const uint64_t *__restrict__ tail_keys,
                                                      const uint32_t *__restrict__ tail_idx, double *__restrict__ part) {
    __shared__ double red[4][PS_T];
    const int b = threadIdx.x & (PL_B - 1), sl = threadIdx.x / PL_B;
    const double lb0 = -log((double)a.n);
    double v[4] = {0., 0., 0., 0.};
    if (b < a.nb) {
        const double mx = out[PL_MAXR * PL_B + b], mb = out[PL_MAXB * PL_B + b];
        const uint64_t kc = tail_keys[(long)b * (M + 1)];   // the cut pair
        const uint32_t ic = tail_idx[(long)b * (M + 1)];
        for (long r = (long)blockIdx.x * BF_SLICES + sl; r < a.n; r += (long)gridDim.x * BF_SLICES) {
            const double lb = a.lb ? a.lb[r] : lb0;
            if (lb == -__builtin_inf()) continue;
            const double rs = pl_shifted(a.lb ? lb : 0., pl_ell(a, r, b), mx);
            const uint64_t key = bf_order_key(rs);
            if (key > kc || (key == kc && (uint32_t)r > ic)) continue;   // a tail row: it comes with its smoothed value
            const double e = exp(rs);
            v[0] += e;
            v[1] += e * e;
            v[2] += a.lb ? exp(lb - mb) : 1.;   // exp(rs + ell), less the shift the finish adds back: without weights r = -ell
            if (a.mode == BFHIP_PLOO_Z) v[3] += e * pl_phi(a.s[r * a.ld + b]);
        }
    }
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = v[k];
    __syncthreads();
    if (sl == 0)
        for (int k = 0; k < 4; ++k) part[((long)k * PS_MAXB + blockIdx.x) * PL_B + b] = bf_slice_fold(v[k], 1, red[k], b, BfSum());
}

// workgroup b: the workgroups' body sums, the M tail rows fetched by index, the column's figures
__global__ __launch_bounds__(PS_T) void pl_finish_kernel(PlCols a, long M, int nblk, const double *__restrict__ part,
                                                        const uint32_t *__restrict__ tail_idx, const double *__restrict__ sm,
                                                        const double *__restrict__ out8s, double *__restrict__ out) {
    __shared__ double red[PS_T];
    const int b = blockIdx.x;
    const double lb0 = -log((double)a.n);
    const double mx = out[PL_MAXR * PL_B + b], mb = a.lb ? out[PL_MAXB * PL_B + b] : 0., shift = mb - mx;
    double body[4], tail[4] = {0., 0., 0., 0.};
    for (int k = 0; k < 4; ++k) {
        double s = 0.;
        for (int g = threadIdx.x; g < nblk; g += PS_T) s += part[((long)k * PS_MAXB + g) * PL_B + b];
        body[k] = bf_block_reduce<PS_T>(s, red, BfSum());
    }
    for (long i = threadIdx.x; i < M; i += PS_T) {
        const double v = sm[(long)b * (M + 1) + i], e = exp(v);
        const long row = tail_idx[(long)b * (M + 1) + 1 + i];
        tail[0] += e;
        tail[1] += e * e;
        if (row >= a.n) continue;   // (the caller's array: nothing is read through an index that is no row)
        const double lb = a.lb ? a.lb[row] : lb0;
        if (lb == -__builtin_inf()) continue;   // a row of zero weight in the tail (fewer than M + 1 rows have any): in the normalisation only
        tail[2] += exp(v + pl_ell(a, row, b) - shift);
        if (a.mode == BFHIP_PLOO_Z) tail[3] += e * pl_phi(a.s[row * a.ld + b]);
    }
    for (int k = 0; k < 4; ++k) tail[k] = bf_block_reduce<PS_T>(tail[k], red, BfSum());
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
    out[PL_PIT * PL_B + b] = bad || a.mode != BFHIP_PLOO_Z ? nan : (body[3] + tail[3]) / s1;
    out[PL_FLAGS * PL_B + b] = (double)flags;
    if (bad) out[PL_LPD * PL_B + b] = out[PL_SWE * PL_B + b] = out[PL_WAIC * PL_B + b] = out[PL_MAXR * PL_B + b] = nan;
}

// the fit per column (w.out8) and the smoothed tail values (w.sm): bfhip_ploo_finish and bfhip_rw_finish (bfhip_rw.h) launch the same
static void pl_fit_and_smooth(hipStream_t st, const PlWork &w, int nb, long M, int m, const uint64_t *tail_keys) {
    hipLaunchKernelGGL(pl_fit_init_kernel, dim3(1), dim3(PL_B * 8), 0, st, w.out8);
    for (int b = 0; b < nb; ++b) {   // the fit of bfhip_psis on an ascending key array of length M + 1: its n is M + 1
        const uint64_t *ks = tail_keys + (long)b * (M + 1);
        double *kj = w.kj + (long)b * PS_MAXM, *thj = w.thj + (long)b * PS_MAXM, *out8 = w.out8 + 8 * b;
        if (M >= 5) {
            hipLaunchKernelGGL(ps_theta_kernel, dim3(m), dim3(PS_T), 0, st, M + 1, M, m, ks, kj, thj);
            hipLaunchKernelGGL(ps_fit_kernel, dim3(1), dim3(PS_T), 0, st, M + 1, M, m, ks, (const double *)kj, (const double *)thj, out8);
        } else {
            hipLaunchKernelGGL(ps_nofit_kernel, dim3(1), dim3(1), 0, st, M + 1, M, ks, out8);
        }
    }
    if (M > 0)
        hipLaunchKernelGGL(pl_smooth_kernel, dim3((unsigned)((M + PS_T - 1) / PS_T), nb), dim3(PS_T), 0, st, M, tail_keys,
                           (const double *)w.out8, w.sm);
}

extern "C" int bfhip_ploo_finish(bfhip_ctx *ctx, long n, const double *series, long ld, int nb, int mode, const double *c, const double *lb,
                                 const uint64_t *tail_keys, const uint32_t *tail_idx, double *out, void *work, size_t work_bytes) {
    BfDeviceGuard dev_guard(ctx);
    if (int rc = pl_check("bfhip_ploo_finish", ctx, n, series, ld, nb, mode, c)) return rc;
    if (!out || !tail_keys || !tail_idx || !work || work_bytes < bfhip_ploo_work_bytes(n))
        return bf_set_error(BFHIP_ERR_ARG, "bfhip_ploo_finish: invalid argument");
    const long M = pl_tail_size(n);
    const int m = 30 + (int)floor(sqrt((double)M));
    if (m > PS_MAXM) return bf_set_error(BFHIP_ERR_UNSUPPORTED, "bfhip_ploo_finish: %d candidate thetas", m);
    const PlWork w = pl_work(work, n);
    const PlCols a = {n, series, ld, nb, mode, c, lb};
    hipStream_t st = ctx->stream;
    pl_fit_and_smooth(st, w, nb, M, m, tail_keys);
    const int g = ps_grid(n, BF_SLICES);
    hipLaunchKernelGGL(pl_body_kernel, dim3(g), dim3(PS_T), 0, st, a, M, (const double *)out, tail_keys, tail_idx, w.part);
    hipLaunchKernelGGL(pl_finish_kernel, dim3(nb), dim3(PS_T), 0, st, a, M, g, (const double *)w.part, tail_idx, (const double *)w.sm,
                       (const double *)w.out8, out);
    BF_HIP_CHECK(hipGetLastError());
    return 0;
}
